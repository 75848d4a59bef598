"""The chunk seams of the engine's host code (csrc/engine_launch.h, csrc/aes_schedule.h) at PARAM_TOY: the smallest shape that crosses each,
the launches it must come to, and the inputs that are distinct on both sides of a seam.  A helper module like wire_formats.py: no test,
no fixture, no call into the engine.  test_gpu_chunk_seams.py asserts every count below from the context's profile counters, so a chunk
constant that changes turns a seam test red instead of into a one-chunk test.

  MAX_CHUNK_BITS = 32,768 bits per launch of the data movers and per WoPBS chunk; 64 GLWEs of N = 512 bits; 23 AES-128 keys of 1,408 bits
  2 GiB of CMUX-tree workspace per WoPBS chunk of inputs wider than 9 bits
  8,192 workgroups x 16 polynomials per pass of forward_fourier_kernel
  256 blocks per pass of add_bcast_kernel at the toy set (16,384 / 64 workgroups in y)
"""
import numpy as np

import wire_formats as wf

N = 512
MAX_CHUNK_BITS = 32768
CHUNK_GLWES = MAX_CHUNK_BITS // N                    # 64

# A. data movement: 65 full GLWEs and one bit, so the second launch starts at GLWE 64 and its last workgroup holds one bit of four
M_BITS = 65 * N + 1                                  # 33,281
M_GLWES = 66
M_LAUNCHES = 2
FIRST_INDICES = {"carry into the high nonce word": (1 << 32) - MAX_CHUNK_BITS - 2,      # the second launch starts at 2^32 - 2
                 "wrap of the 64-bit index": (1 << 64) - MAX_CHUNK_BITS - 1}              # the second launch starts at 2^64 - 1

# B. many AES-128 keys
KEY_BITS_PACKED = 11 * 128                           # 1,408 bits of round keys per key
KEYS_PER_CHUNK = MAX_CHUNK_BITS // KEY_BITS_PACKED   # 23
N_KEYS_PACK = 29                                     # 23 + 6; and 144 middle bytes x 29 = 4,176 bytes = 33,408 bits: the seam inside key 28
MID_BYTES = 9 * 16
N_KEYS_EXPAND = 1025                                 # 4 bytes per key and step: 4,096 bytes per chunk, key 1,024 the first of chunk 2
EXPAND_WOPBS = 40 + 10                               # 40 refreshed words and 10 SubWord per AES-128 key expansion

# C. WoPBS
PER_INPUT_BITS = 9
PER_INPUT_CHUNK = MAX_CHUNK_BITS // PER_INPUT_BITS   # 3,640 inputs
PER_INPUT_N = PER_INPUT_CHUNK + 1
PER_INPUT_LUTS = 509                                 # a prime below 512: a_i = i mod 509, so a_i != a_(i - 3640)
TREE_BITS, TREE_LUTS = 16, 4
TREE_CHUNK = (2 << 30) // (TREE_LUTS * TREE_BITS * (1 << (TREE_BITS - 9)) * 2 * N * 8)      # 32 inputs: 2^26 bytes each at k = 1
TREE_N = TREE_CHUNK + 1

# D. K4: 8,192 workgroups x 16 polynomials, then a ragged second pass
FOURIER_FIRST_PASS = 8192 * 16
FOURIER_TAIL = 17
FOURIER_DISTINCT = 1024

# E. linear layers and schedules
BLOCKS = 257                                         # 32,896 bits a step; block 256 is the second pass of add_bcast_kernel
WINDOW = 200
PUBLIC_BLOCKS = 300                                  # pools of 4,800 bytes = 38,400 bits


def chunks(total: int, chunk: int) -> int:
    return -(-total // chunk)


def random_words(seed: int, shape):
    return np.random.default_rng(seed).integers(0, 1 << 64, shape, dtype=np.uint64)


def edge_glwes_at_the_seam(width: int, fields: int, seed: int = 0x5EA3):
    """66 uniform GLWEs with wire_formats.edge_word_list at the first and the last fields of GLWEs 63, 64 and 65 -- the last GLWE of chunk 1
    and the first two of chunk 2 -- in an order rotated GLWE by GLWE"""
    glwe = random_words(seed + width, (M_GLWES, fields))
    words = wf.edge_word_list(width)
    n = len(words)
    for g in (CHUNK_GLWES - 1, CHUNK_GLWES, CHUNK_GLWES + 1):
        rot = [words[(i + g) % n] for i in range(n)]
        glwe[g, :n] = rot
        glwe[g, fields - n:] = rot
    return glwe


def per_input_adds(n: int = PER_INPUT_N):
    a = np.arange(n) % PER_INPUT_LUTS
    assert (a[PER_INPUT_CHUNK:] != a[:n - PER_INPUT_CHUNK]).all()
    return a


def tree_values():
    """33 inputs of 16 bits: 0, 2^16 - 1, 2^15, a pair on both sides of every tree bit 9..15, random ones; inputs 31 and 32 (the last of
    chunk 1, the first of chunk 2) differ in every tree bit"""
    rng = np.random.default_rng(0x7EE)
    vals = [0, (1 << 16) - 1, 1 << 15]
    for t in range(9, 16):
        r = int(rng.integers(0, 1 << 16)) & ~(1 << t)
        vals += [r, r | (1 << t)]
    vals += [int(v) for v in rng.integers(0, 1 << 16, TREE_N - len(vals) - 2)]
    vals += [0x2A5C, 0x2A5C ^ 0xFE00]
    assert len(vals) == TREE_N and len(set(vals)) == TREE_N
    return vals


TREE_FUNCTIONS = (lambda v: (v * 37 + 5) & 0xFFFF, lambda v: (v ^ (v >> 3) ^ 0x5555) & 0xFFFF, lambda v: (v * v + 1) & 0xFFFF,
                  lambda v: (0xFFFF - v) & 0xFFFF)


def bits_of(values, width: int):
    return np.array([[(int(v) >> j) & 1 for j in range(width)] for v in values], dtype=np.uint8)


def value_of(bits) -> int:
    return int(sum(int(b) << j for j, b in enumerate(bits)))


def fourier_inputs():
    """(the 1,041 distinct polynomials, the polynomial every one of the 131,089 rows holds): 1,024 random ones tiled over the first pass,
    17 fresh ones behind them, three of them constant 0, 2^64 - 1 and 2^63"""
    distinct = random_words(0xF4, (FOURIER_DISTINCT + FOURIER_TAIL, N))
    distinct[FOURIER_DISTINCT + 3] = 0
    distinct[FOURIER_DISTINCT + 8] = (1 << 64) - 1
    distinct[FOURIER_DISTINCT + 16] = 1 << 63
    which = np.concatenate([np.arange(FOURIER_FIRST_PASS) % FOURIER_DISTINCT, FOURIER_DISTINCT + np.arange(FOURIER_TAIL)])
    return distinct, which


def window_launches(n_blocks: int, steps: int, window: int):
    """(blind-rotation launches, key-switch launches) of `steps` WoPBS over n_blocks blocks cut into windows: the stream of steps x n
    block-rounds in (step, block) order, a launch of two segments where a window straddles two steps"""
    total, k2, k1 = steps * n_blocks, 0, 0
    for i0 in range(0, total, window):
        length, b0 = min(window, total - i0), i0 % n_blocks
        k2 += 1
        k1 += 1 if n_blocks - b0 >= length else 2
    return k2, k1


def public_pool_round_1(blocks) -> int:
    """distinct (position, byte value) pairs of the blocks: the pool of round 1, at most 16 x 256 whatever the batch"""
    return len({(p, (int(b) >> (8 * (15 - p))) & 0xFF) for b in blocks for p in range(16)})
