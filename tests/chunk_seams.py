"""The chunk seams of the engine's host code (csrc/engine_launch.h, csrc/aes_schedule.h) at PARAM_TOY: the smallest shape that crosses each,
the launches it must come to, and the inputs that are distinct on both sides of a seam.  A helper module like wire_formats.py: no test,
no fixture, no call into the engine.  test_gpu_chunk_seams.py asserts every count below from the context's profile counters, so a chunk
constant that changes turns a seam test red instead of into a one-chunk test.

  MAX_CHUNK_BITS = 32,768 bits per launch of the data movers and per WoPBS chunk; 64 GLWEs of N = 512 bits; 23 AES-128 keys of 1,408 bits
  2 GiB of CMUX-tree workspace per WoPBS chunk of inputs wider than 9 bits
  8,192 workgroups x 16 polynomials per pass of forward_fourier_kernel
  256 blocks per pass of add_bcast_kernel at the toy set (16,384 / 64 workgroups in y)

and of the later modes (test_gpu_chunk_seams_modes.py, pinned without a GPU by test_chunk_seams_modes_cpu.py):

  256 blocks or slots per pass of xts_whiten_kernel and mac_link_kernel: the same 16,384 / 64 (SLOTS_PER_PASS)
  2^20 workgroups = 8,192 tweak blocks per pass of bit_rows_kernel<XtsRows> (TWEAK_ROWS_PER_PASS)
  128 inputs per chunk of the 16-bit tag WoPBS of a CCM call: 2^24 bytes of CMUX tree each (TAG_TREE_CHUNK); 256 messages per chunk of
  its 8-bit one (TAG_BYTE_CHUNK)

and of the calls that came after those (test_gpu_chunk_seams_calls.py, pinned without a GPU by test_chunk_seams_calls_cpu.py; part G):

  257 keys, streams or wrapped keys: one block behind the 4,096 bytes of a byte WoPBS chunk and the 256 slots of a link's grid pass, in
  the CMAC subkey derivation, the CMAC chain with its tag check, and the key unwrap
  65,536 workgroups per launch of gate_kernel (GATE_MAX_GRID), 8 instances a workgroup at k = 1; MAX_CHUNK_BITS gates per circuit
  bootstrap of a gate call
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


# F. the later modes: XTS, CCM and the keyed public calls ---------------------------------------------------------------------------------
BIG1_TOY = 513                                       # k N + 1 words of an LWE ciphertext at PARAM_TOY
CHUNK_BYTES = MAX_CHUNK_BITS // 8                    # 4,096 bytes per chunk of a byte WoPBS: 256 blocks


def slots_per_pass(big1: int) -> int:
    """blocks (xts_whiten_kernel) or slots (mac_link_kernel) per grid pass: gridDim.y is capped at 16,384 / gx, gx the workgroups of 256
    lanes over the 128 big1 words of a block, at most 64"""
    return 16384 // min(64, -(-128 * big1 // 256))


SLOTS_PER_PASS = slots_per_pass(BIG1_TOY)            # 256
TWEAK_ROWS_PER_PASS = (1 << 20) // 128               # 8,192 tweak blocks: one workgroup per row of kN + 1 words, 2^20 workgroups
TAG_TREE_CHUNK = (2 << 30) // (1 * 16 * (1 << 7) * 2 * N * 8)       # 128 inputs: one LUT, 16 bits, 2^7 GLWEs of 8 KB per output bit at k = 1
TAG_BYTE_CHUNK = MAX_CHUNK_BITS // 8 // 16           # 256 messages: 16 bytes of tag difference each

# 1. fheaes_xts_whiten alone and 2. fheaes_mac_link alone: one block or slot behind the pass
WHITEN_BLOCKS, WHITEN_TWEAKS = SLOTS_PER_PASS + 1, 5
LINK_SLOTS, LINK_ENC = SLOTS_PER_PASS + 1, SLOTS_PER_PASS + 3
MAC_NONE = 0xFFFFFFFF

# 3. fheaes_xts_tweaks: 68 units of 122 offsets are 8,296 tweak blocks = 1,061,888 rows; 67 units stay below 2^20
TWEAK_UNITS, TWEAK_OFFSETS = 68, 122
TWEAK_BLOCKS = TWEAK_UNITS * TWEAK_OFFSETS
TWEAK_SEAM = divmod(TWEAK_ROWS_PER_PASS, TWEAK_OFFSETS)     # (unit 67, offset 18): the first tweak block of the second pass

# 4. XTS-AES decryption: blocks 121 .. 486 of four units of 122 blocks
XTS_SEGMENT = 120
XTS_BPU, XTS_FIRST, XTS_BLOCKS = 122, 121, 366
XTS_SECTORS = (0x0123456789, 7, (1 << 64) - 2, 1 << 100)
XTS_ALONE = (0, 1, 255, 256, 365)

# 5. CCM: 257 messages under 3 keys; position -> (AAD bytes, payload bytes, tag bytes) of the long ones, the rest (0, 0, 8)
CCM_MESSAGES, CCM_KEYS = 257, 3
CCM_LONG = {0: (3, 16, 4), 127: (40, 40, 16), 128: (14, 21, 8), 255: (20, 16, 16), 256: (30, 5, 10)}
CCM_BAD = sorted({1, 127, 129, 255, 256} | set(range(37, CCM_MESSAGES, 37)))   # and every 37th: position 0 is valid, position 256 is not
CCM_BAD_CIPHERTEXT = 256                             # a ciphertext bit there; a bit of the last compared tag byte at the others
MAC_STREAMS = 257
MAC_LENGTHS = {0: 3, 255: 0, 256: 3}                 # the rest chain one block
MAC_ALONE = (0, 1, 255, 256)

# 6. keyed public calls: PUBLIC_BLOCKS blocks under 3 keys
PUBLIC_KEYS, PUBLIC_SEED = 3, 0xE1E
PUBLIC_ALONE = (0, 255, 256, PUBLIC_BLOCKS - 1)


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


# ---- F. the later modes ------------------------------------------------------------------------------------------------------------------
def wopbs_chunks(n_inputs: int, bits: int, n_luts: int, k1: int) -> int:
    """the chunks wopbs_dev cuts n_inputs into: MAX_CHUNK_BITS // bits inputs each, and above 9 bits no more inputs than keep the CMUX tree
    (n_luts x bits x 2^(bits - 9) GLWEs of k1 N words per input) within 2 GiB; k1 = k + 1"""
    chunk = max(1, MAX_CHUNK_BITS // bits)
    if bits > 9:
        chunk = max(1, min(chunk, (2 << 30) // (n_luts * bits * (1 << (bits - 9)) * k1 * N * 8)))
    return chunks(n_inputs, chunk) if n_inputs else 0


def byte_wopbs(n_bytes: int):
    """(launches, units) of the key switch of one byte WoPBS over n_bytes bytes: chunks of 4,096 bytes, a unit per bit"""
    return wopbs_chunks(n_bytes, 8, 1, 2), 8 * n_bytes


def whiten_table(n: int = WHITEN_BLOCKS, rows: int = WHITEN_TWEAKS):
    """tweak_of_block: (7 b + 3) mod 5, not monotone; block 256 takes a row that block 0 and block 255 do not"""
    tab = [(7 * b + 3) % rows for b in range(n)]
    assert tab[SLOTS_PER_PASS] not in (tab[0], tab[SLOTS_PER_PASS - 1]) and set(tab) == set(range(rows))
    return tab


def link_tables(n: int = LINK_SLOTS, n_enc: int = LINK_ENC):
    """(src_block, enc_bytes) of the link over 257 slots: slot 256 reads block 0 and slot 0 block 258, slot 255 has no block; enc_bytes
    cycles through 0, 1, 15 and 16, with 5 at slot 256"""
    src = [(5 * s + 2) % n_enc for s in range(n)]
    src[SLOTS_PER_PASS], src[0], src[SLOTS_PER_PASS - 1] = 0, n_enc - 1, MAC_NONE
    eb = [(0, 1, 15, 16)[s % 4] for s in range(n)]
    eb[SLOTS_PER_PASS] = 5
    return src, eb


def xts_segment_rows(bpu: int = XTS_BPU, first_block: int = XTS_FIRST, n_blocks: int = XTS_BLOCKS):
    """(touched units, tweak rows of every segment) of an XTS call by the segment rule: per unit and segment the offsets of the call's
    blocks there, and offset 120 -- the next segment's anchor -- where the unit's last block lies in a later segment"""
    blocks = range(first_block, first_block + n_blocks)
    units = sorted({g // bpu for g in blocks})
    rows = []
    for u in units:
        mine = [g % bpu for g in blocks if g // bpu == u]
        for s in range(max(mine) // XTS_SEGMENT + 1):
            if s == len(rows):
                rows.append(0)
            rows[s] += len({j % XTS_SEGMENT for j in mine if j // XTS_SEGMENT == s}) + (1 if max(mine) // XTS_SEGMENT > s else 0)
    return len(units), rows


def xts_keyswitch(public_plan, bpu: int = XTS_BPU, first_block: int = XTS_FIRST, n_blocks: int = XTS_BLOCKS, nr: int = 10):
    """{part: (launches, units)} of the key switch of an XTS call round by round (AES_WINDOW_OFF).  public rounds: one WoPBS per round
    over the pool of the tweak blocks (public_plan: the pool sizes, aes_public_plan of those blocks); refresh: the anchors of segment 0,
    then one identity WoPBS per segment over its rows; cipher: nr WoPBS over the call's blocks"""
    units, rows = xts_segment_rows(bpu, first_block, n_blocks)
    parts = {"public_rounds": [byte_wopbs(n) for n in public_plan],
             "refresh": [byte_wopbs(16 * units)] + [byte_wopbs(16 * r) for r in rows],
             "cipher": [byte_wopbs(16 * n_blocks)] * nr}
    return {name: (sum(l for l, _ in v), sum(u for _, u in v)) for name, v in parts.items()}


def total(parts):
    """(launches, units) summed over the parts of xts_keyswitch / ccm_keyswitch"""
    return sum(l for l, _ in parts.values()), sum(u for _, u in parts.values())


def ccm_shape(i: int):
    """(key index, AAD bytes, payload bytes, tag bytes) of message i: the key changes across 128 and across 256"""
    return ((i * 2 + i // 128) % CCM_KEYS,) + CCM_LONG.get(i, (0, 0, 8))


def ccm_stream_blocks():
    """(chain length, payload blocks) of every message: the AAD with its 2-byte length in whole blocks, then the payload blocks"""
    out = []
    for i in range(CCM_MESSAGES):
        _, aad, payload, _ = ccm_shape(i)
        out.append(((2 + aad + 15) // 16 * (aad > 0) + (payload + 15) // 16, (payload + 15) // 16))
    return [a for a, _ in out], [b for _, b in out]


def live_prefixes(lengths):
    """n_active of a chain: the streams longer than i, for every step i"""
    return [sum(1 for v in lengths if v > i) for i in range(max(lengths, default=0))]


def chain_keyswitch(n_active, nr: int = 10):
    """(launches, units) of the cipher passes of a chain round by round: nr WoPBS over the live prefix of every step"""
    parts = [byte_wopbs(16 * a) for a in n_active for _ in range(nr)]
    return sum(l for l, _ in parts), sum(u for _, u in parts)


def ccm_keyswitch(public_plan, n_active, n: int = CCM_MESSAGES, nr: int = 10):
    """{part: (launches, units)} of the key switch of a CCM call round by round: the public rounds over their pools, the chain, the 8-bit
    tag WoPBS over 16 n bytes and the 16-bit one over n inputs"""
    pub = [byte_wopbs(v) for v in public_plan]
    return {"public_rounds": (sum(l for l, _ in pub), sum(u for _, u in pub)), "chain": chain_keyswitch(n_active, nr),
            "tag_bytes": byte_wopbs(16 * n), "tag_tree": (wopbs_chunks(n, 16, 1, 2), 16 * n)}


def mac_lengths():
    return [MAC_LENGTHS.get(s, 1) for s in range(MAC_STREAMS)]


def public_keyed_blocks():
    """(blocks, key of every block, data blocks) of the keyed public calls: random, and the same for both directions"""
    rng = np.random.default_rng(PUBLIC_SEED)
    blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(PUBLIC_BLOCKS)]
    data = [int.from_bytes(rng.bytes(16), "big") for _ in range(PUBLIC_BLOCKS)]
    return blocks, [int(k) for k in rng.integers(0, PUBLIC_KEYS, PUBLIC_BLOCKS)], data


# ---- G. the later calls: CMAC, key unwrap and the gate -------------------------------------------------------------------------------------
# (test_gpu_chunk_seams_calls.py, pinned without a GPU by test_chunk_seams_calls_cpu.py.)  The rules restated:
#   a byte WoPBS takes CHUNK_BYTES = 4,096 bytes a chunk: 256 blocks, so 257 keys or streams put one block behind the seam
#   mac_link_kernel and kw_link_kernel take SLOTS_PER_PASS = 256 slots or keys a grid pass; bit_rows_kernel<CmacRows> one workgroup per output row
#   gate_kernel takes GATE_MAX_GRID = 65,536 workgroups a launch, GATE_R = 8 instances a workgroup at k = 1, and a bootstrapped gate call
#   MAX_CHUNK_BITS gates a chunk, whose GGSWs lie at g mod MAX_CHUNK_BITS of one workspace
GATE_MAX_GRID = 65536
GATE_R = 8                                           # instances per workgroup at PARAM_TOY (k = 1); 3 at k = 4
CALL_ALONE = (0, 1, 255, 256)                        # the streams and wrapped keys that also run alone

# A. CMAC subkeys of 257 keys, the SP 800-38B key the one behind the seam
CMAC_KEYS = 257
CMAC_VECTOR_KEY = 256
CMAC_KEYS_ALONE = (0, 127, 128, 255, 256)

# B. CMAC tags and verification: 257 streams under a store of 259 keys, two of them never named
CMAC_STORE_KEYS = 259
CMAC_UNNAMED = (5, 130)
CMAC_STREAMS = 257
CMAC_LENGTHS = {0: 48, 100: 17, 255: 0, 256: 48}     # the rest one block: 16 bytes (K1) at even streams, 1..15 bytes (K2) at odd ones
CMAC_BAD = sorted({1, 127, 129, 255, 256} | set(range(41, CMAC_STREAMS, 41)))    # position 0 verifies, 255 and 256 do not
CMAC_BAD_MESSAGE = 256                               # a message bit there; a bit of the last compared tag byte at the others

# C. key unwrap: 257 wrapped AES-128 keys (n = 2 semiblocks) under 3 KEKs, RFC 3394 4.1 at key 256 under KEK 0
KW_KEYS, KW_KEKS, KW_SEMIBLOCKS = 257, 3, 2
KW_VECTOR_KEY = 256
KW_BAD = sorted({1, 127, 129, 255} | set(range(37, KW_KEYS, 37)))     # keys 0 and 256 are valid, key 255 is not
KW_WRONG_KEK = 128                                   # a valid blob named under another KEK than the one that wrapped it

# D. gate_kernel behind GATE_MAX_GRID: gate 0 ends in workgroup 65,536, the first of the second launch, with 3 instances
GATE_GRID_RUNS = [GATE_R * GATE_MAX_GRID + 3, 0, 9, 1]
GATE_ROW_PERIOD = 7                                  # the rows of test_gpu_gate._inputs, coprime to GATE_R: every phase in a workgroup

# E. both gate seams in one bootstrapped call: 32,769 gates, chunk 1 of 65,537 workgroups, chunk 2 of gate 32,768 alone with two
GATE_BOOT_GATES = MAX_CHUNK_BITS + 1
GATE_BOOT_HEAD = GATE_R * (MAX_CHUNK_BITS + 3)       # gate 0: 32,771 workgroups
GATE_BOOT_TAIL = (1, 1, 0, 9)                        # gates 32,765 .. 32,768


def gate_table(runs, R: int = GATE_R, chunk: int = 0):
    """(first instance, gate, instances) of every workgroup: a run cut into workgroups of up to R instances, a run of 0 none; chunk > 0:
    the gate as its place in the chunk's workspace"""
    out, first = [], 0
    for g, run in enumerate(runs):
        out += [(first + i, g % chunk if chunk else g, min(R, run - i)) for i in range(0, run, R)]
        first += run
    return out


def gate_workgroups(runs, R: int = GATE_R) -> int:
    return sum(-(-int(r) // R) for r in runs)


def gate_launches(runs, R: int = GATE_R, chunk: int = 0):
    """the kernel launches of every launch_gate of a call: one launch_gate for all runs, or (chunk > 0) one per chunk of gates"""
    runs = list(runs)
    parts = [runs] if not chunk else [runs[g0:g0 + chunk] for g0 in range(0, len(runs), chunk)]
    return [chunks(gate_workgroups(part, R), GATE_MAX_GRID) for part in parts]


def gate_boot_runs(head: int = GATE_BOOT_HEAD):
    """the runs of E: gate 0 `head` instances, gate 32,767 none, gate 32,768 nine, every other gate one"""
    runs = [1] * GATE_BOOT_GATES
    runs[0] = head
    runs[-4:] = GATE_BOOT_TAIL
    return runs


def gate_packed_runs():
    """the runs of E in the GLWE form: one GLWE a gate, none under gate 32,767, two under gate 32,768"""
    runs = [1] * GATE_BOOT_GATES
    runs[-2:] = [0, 2]
    return runs


def cmac_key_of_stream(s: int) -> int:
    """a permutation of the 257 named keys of the store of 259 (257 is prime): the keys are not in stream order"""
    named = [k for k in range(CMAC_STORE_KEYS) if k not in CMAC_UNNAMED]
    return named[(100 * s + 7) % len(named)]


def cmac_message_bytes(s: int) -> int:
    return CMAC_LENGTHS.get(s, 16 if s % 2 == 0 else 1 + s % 15)


def cmac_tag_bytes(s: int) -> int:
    return 4 + s % 13


def cmac_chain_blocks():
    return [max(1, -(-cmac_message_bytes(s) // 16)) for s in range(CMAC_STREAMS)]


def cmac_keyswitch(public_plan, n_derived: int, n_active, n_verified: int = 0, nr: int = 10):
    """{part: (launches, units)} of the key switch of a CMAC call round by round.  With n_derived keys whose subkeys the call derives: the
    public rounds over their pools (public_plan: aes_public_plan_keyed of one zero block per key), the identity WoPBS over the 16 bytes
    of every L and the one over the 32 bytes of every raw K1 | K2.  The chain over its live prefixes.  With n_verified tags: the 8-bit tag
    WoPBS over 16 bytes a stream and the 16-bit one over one input a stream"""
    parts = {"chain": chain_keyswitch(n_active, nr)}
    if n_derived:
        pub = [byte_wopbs(v) for v in public_plan]
        parts["public_rounds"] = (sum(l for l, _ in pub), sum(u for _, u in pub))
        parts["refresh_l"], parts["refresh_k"] = byte_wopbs(16 * n_derived), byte_wopbs(32 * n_derived)
    if n_verified:
        parts["tag_bytes"], parts["tag_tree"] = byte_wopbs(16 * n_verified), (wopbs_chunks(n_verified, 16, 1, 2), 16 * n_verified)
    return parts


def kw_kek_of_key():
    """(j + 1) mod 3: the KEK of key j is not that of key j - 128; key 256 takes KEK 0, which keys 0 and 255 do not"""
    return [(j + 1) % KW_KEKS for j in range(KW_KEYS - 1)] + [0]


def kw_keyswitch(n_keys: int = KW_KEYS, n: int = KW_SEMIBLOCKS, nr: int = 10, window: int = 0):
    """{part: (launches, units)} of the key switch of a key unwrap: 6 n passes of the equivalent inverse cipher over all keys (round by
    round, or window > 0: in windows of that many blocks), the identity WoPBS over the 8 n payload bytes of every key, the two tag WoPBS"""
    if window:
        cipher = (6 * n * window_launches(n_keys, nr, min(window, n_keys))[1], 6 * n * nr * 128 * n_keys)
    else:
        cipher = (6 * n * nr * byte_wopbs(16 * n_keys)[0], 6 * n * nr * byte_wopbs(16 * n_keys)[1])
    return {"cipher": cipher, "refresh": byte_wopbs(8 * n * n_keys), "tag_bytes": byte_wopbs(16 * n_keys),
            "tag_tree": (wopbs_chunks(n_keys, 16, 1, 2), 16 * n_keys)}
