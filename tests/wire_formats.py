"""The wire formats of include/fheaes.h in plain numpy and Python integers: references for test_wire_formats_cpu.py and
test_gpu_wire_formats.py.  A helper module like edge_words.py: no test, no fixture, no call into the engine.

  mod_switch_word / read_back_word   the rounding rule v = ((x + 2^(63-w)) >> (64-w)) mod 2^w and x' = v << (64-w), on Python integers
  round_words                        the same on uint64 arrays (wrapping sum): the read-back words of a switched array
  switch_glwes / read_back_glwes     the bit-string packer: field e of a GLWE at bits [e w, (e+1) w) of ONE Python integer per GLWE, cut
                                     into little-endian 64-bit words
  noise_std / noise_bound            (1 + h) 2^(2(64-w)) / 12 and (1 + h) 2^(63-w)
  edge_glwes                         uniform GLWEs with the edge-word set written into them, and the classes the set holds

The seeded form needs no reference of its own: client.mask_words is the stream (pinned to csrc/client.c by test_seeded_keys.py), and
SeededCiphertexts.expand() is built on it.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
WIDTHS = (8, 10, 13, 16, 32)


# ---- the rounding rule ----------------------------------------------------------------------------------------------------------------
def mod_switch_word(x: int, w: int) -> int:
    return (((int(x) + (1 << (63 - w))) & M64) >> (64 - w)) & ((1 << w) - 1)


def read_back_word(v: int, w: int) -> int:
    return (int(v) << (64 - w)) & M64


def round_words(x, w: int):
    """uint64 array -> the words a switch to w bits and a read-back leave: ((x + 2^(63-w)) >> (64-w)) << (64-w), the sum wrapping"""
    if w == 64:
        return np.array(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return ((np.asarray(x, dtype=np.uint64) + np.uint64(1 << (63 - w))) >> np.uint64(64 - w)) << np.uint64(64 - w)


# ---- the bit-string packer --------------------------------------------------------------------------------------------------------------
def switch_glwes(glwe, w: int) -> np.ndarray:
    """[G][fields] 64-bit words -> [G][fields w / 64]: one Python integer per GLWE holds its bit string, field e at bits [e w, (e+1) w)"""
    glwe = np.asarray(glwe, dtype=np.uint64)
    if w == 64:
        return glwe.copy()
    fields = glwe.shape[1]
    assert fields * w % 64 == 0
    out = np.empty((glwe.shape[0], fields * w // 64), dtype=np.uint64)
    for g in range(glwe.shape[0]):
        s = 0
        for e, x in enumerate(glwe[g].tolist()):
            s |= mod_switch_word(x, w) << (e * w)
        out[g] = [(s >> (64 * i)) & M64 for i in range(out.shape[1])]
    return out


def read_back_glwes(packed, fields: int, w: int) -> np.ndarray:
    """[G][fields w / 64] -> [G][fields] words x' = v << (64-w)"""
    packed = np.asarray(packed, dtype=np.uint64)
    if w == 64:
        return packed.copy()
    out = np.empty((packed.shape[0], fields), dtype=np.uint64)
    for g in range(packed.shape[0]):
        s = sum(int(x) << (64 * i) for i, x in enumerate(packed[g].tolist()))
        out[g] = [read_back_word((s >> (e * w)) & ((1 << w) - 1), w) for e in range(fields)]
    return out


# ---- noise --------------------------------------------------------------------------------------------------------------------------------
def noise_std(h: int, w: int) -> float:
    """each of the 1 + h words of a phase (the body, the h mask words at set key bits) moves uniformly within +- 2^(63-w)"""
    return math.sqrt((1 + h) * 2.0 ** (2 * (64 - w)) / 12.0)


def noise_bound(h: int, w: int) -> int:
    return (1 + h) << (63 - w)


# ---- edge words ---------------------------------------------------------------------------------------------------------------------------
def edge_word_list(w: int):
    """0, 2^64-1, 2^63, 2^63-1 and the ties (2j+1) 2^(63-w) for j in {0, 1, 2^(w-1)-1, 2^(w-1), 2^w-1}, each also -1 and +1 (the last tie
    wraps to 0); w = 64 has no ties"""
    words = [0, M64, 1 << 63, (1 << 63) - 1]
    if w != 64:
        for j in (0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1):
            tie = (2 * j + 1) << (63 - w)
            words += [tie, (tie - 1) & M64, (tie + 1) & M64]
    return words


def straddles(e: int, w: int) -> bool:
    return (e * w) % 64 + w > 64


def edge_glwes(k: int, w: int, n_glwe: int = 3, N: int = 512, seed: int = 0xED6E):
    """(glwes [n_glwe][(k+1)N] uniform with the edge words in them, classes).  Every GLWE carries the whole word list, in an order
    rotated by one GLWE by GLWE (the last field of GLWE 0 holds the top tie + 1 and that of GLWE 2 holds 2^64 - 1: both wrap to 0), as a
    run from the first field of every polynomial on and a run up to the last field of every polynomial -- first and last field of a
    polynomial and of the GLWE -- and, for widths that do not divide 64, once more on the first fields of polynomial 0 beyond its
    first run that straddle two words.  `classes` counts, over the placed words and with the plain rules above, what the set holds."""
    fields = (k + 1) * N
    words = edge_word_list(w)
    n = len(words)
    out = np.random.default_rng(seed + 64 * k + w).integers(0, 1 << 64, (n_glwe, fields), dtype=np.uint64)
    half = 1 << (63 - w) if w != 64 else 0
    spots = [start + i for j in range(k + 1) for start in (j * N, j * N + N - n) for i in range(n)]
    if w != 64 and 64 % w:
        across = [e for e in range(n, N - n) if straddles(e, w)][:n]
        assert len(across) == n
        spots += across
    cls = {"placed": 0, "extremes": 0, "ties": 0, "tie_neighbours": 0, "wrap_to_zero": 0, "straddling": 0, "first_of_polynomial": 0,
           "last_of_polynomial": 0, "first_of_glwe": 0, "last_of_glwe": 0, "wrap_straddling": 0, "wrap_last_of_glwe": 0}
    for g in range(n_glwe):
        for i, e in enumerate(spots):
            x = words[(i + g) % n]
            out[g, e] = x
            cls["placed"] += 1
            cls["extremes"] += x in (0, M64, 1 << 63, (1 << 63) - 1)
            if w != 64:
                cls["ties"] += x % (2 * half) == half
                cls["tie_neighbours"] += (x + 1) % (2 * half) == half or (x - 1) % (2 * half) == half
                cls["wrap_to_zero"] += x + half > M64
                cls["straddling"] += straddles(e, w)
                cls["wrap_straddling"] += x + half > M64 and straddles(e, w)
                cls["wrap_last_of_glwe"] += x + half > M64 and e == fields - 1
            cls["first_of_polynomial"] += e % N == 0
            cls["last_of_polynomial"] += e % N == N - 1
            cls["first_of_glwe"] += e == 0
            cls["last_of_glwe"] += e == fields - 1
    return out, {key: int(v) for key, v in cls.items()}
