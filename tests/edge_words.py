"""Edge words: the inputs that random words and honest ciphertexts never reach, with plain references that do not call the oracle.

A helper module (no test, no fixture) shared by test_edge_words_cpu.py, which pins the oracle against the plain references below
and asserts that every generator really holds the classes it is meant to hold, and test_gpu_edge_words.py, which runs the same
sets through the HIP kernels.

Plain references (Python integers, fractions.Fraction and numpy uint64 wrapping only):
  decompose / decompose_offset   the two gadget rules, as restated in test_oracle_primitives.py
  mod_switch                     round(x / 2^54) mod 1024
  balanced_bytes                 x = sum_j kb_j 2^(8j) mod 2^64 with kb_j in [-128, 127]
  keyswitch_plain / pfpks_plain  K1 / K3 as one uint64 matrix product
  torus_round                    the canonical back-conversion on an exact rational
  blind_rotation_trivial         K2 under a noise-free BSK of a binary key s under the zero GLWE key

Every generator returns (set, classes): `classes` counts what the set contains, computed with the plain references.
"""
import dataclasses
from fractions import Fraction

import numpy as np

from tfhe_aes_amd import PARAM_OPT

M64 = (1 << 64) - 1
EXTREMES = (0, M64, 1 << 63, (1 << 63) - 1)

# the kernels of PARAM_OPT (k = 4) on an LWE dimension at which the oracle does a thousand blind rotations in a second: NOT secure
PARAM_EDGE = dataclasses.replace(PARAM_OPT, name="PARAM_EDGE", lwe_dimension=24)


# ---------------------------------------------------------------------------------------------------------------------------------
# plain references
# ---------------------------------------------------------------------------------------------------------------------------------
def decompose(x, b, level):
    """SURVEY.md Appendix A.3 (the key switches), digit list index 0 = level 1"""
    r = 64 - b * level
    st = ((x >> r) + ((x >> (r - 1)) & 1)) & ((1 << (b * level)) - 1)
    out = [0] * level
    for l in range(level - 1, -1, -1):
        d = st & ((1 << b) - 1)
        st >>= b
        carry = ((((d - 1) & M64) | st) & d) >> (b - 1)
        st += carry
        out[l] = d - (carry << b)
    return out


def decompose_offset(x, b, level):
    """canonical form v3 (the external products): closest representable, then the offset rule"""
    r = 64 - b * level
    z = (x + ((1 << (r - 1)) if r > 0 else 0)) & M64
    for l in range(level):
        z = (z + ((1 << (b - 1)) << (64 - b * (l + 1)))) & M64
    return [((z >> (64 - b * (l + 1))) & ((1 << b) - 1)) - (1 << (b - 1)) for l in range(level)]


def mod_switch(x):
    """the closest multiple of 2^54, in units of 2^54, mod 1024 (a tie rounds up; 1024 wraps to 0)"""
    return ((int(x) + (1 << 53)) // (1 << 54)) % 1024


def balanced_bytes(x):
    """kb[0..7] in [-128, 127] with sum_j kb[j] 2^(8j) = x mod 2^64: a byte of 128 or more becomes byte - 256 and carries"""
    out, carry = [], 0
    for j in range(8):
        v = ((int(x) >> (8 * j)) & 0xFF) + carry
        carry = 1 if v >= 128 else 0
        out.append(v - 256 * carry)
    assert sum(v << (8 * j) for j, v in enumerate(out)) & M64 == int(x)
    return out


def digit_planes(d):
    """a digit as low plane in [-128, 127] + 256 * high plane"""
    lo = ((d + 128) & 255) - 128
    return lo, (d - lo) >> 8


def digits_of_rows(x, b, level):
    """[m][words] uint64 -> [m][words * level] int64, digit of (word i, level l + 1) at i * level + l"""
    x = np.asarray(x, dtype=np.uint64)
    cache = {}
    out = np.empty((x.shape[0], x.shape[1] * level), dtype=np.int64)
    for r in range(x.shape[0]):
        for i, w in enumerate(x[r].tolist()):
            d = cache.get(w)
            if d is None:
                d = cache[w] = decompose(w, b, level)
            out[r, i * level:(i + 1) * level] = d
    return out


def keyswitch_plain(x, ksk, p):
    """K1: x [m][kN+1], ksk [kN][ks_level][n+1] -> [m][n+1]: out = -sum digit KSK, the input body added to column n"""
    x = np.asarray(x, dtype=np.uint64)
    key = np.asarray(ksk, dtype=np.uint64).reshape(p.big * p.ks_level, p.n + 1)
    d = digits_of_rows(x[:, :p.big], p.ks_base_log, p.ks_level).astype(np.uint64)
    out = np.uint64(0) - d @ key
    out[:, p.n] += x[:, p.big]
    return out


def pfpks_plain(x, pfpksk, p):
    """K3: x [m][kN+1], pfpksk [k+1][kN+1][pfks_level][(k+1)N] -> [m][k+1][(k+1)N]: out_z = -sum_{i < kN+1, l} digit KEY[z]"""
    x = np.asarray(x, dtype=np.uint64)
    k1 = p.k + 1
    key = np.asarray(pfpksk, dtype=np.uint64).reshape(k1, p.big1 * p.pfks_level, k1 * p.N)
    d = digits_of_rows(x, p.pfks_base_log, p.pfks_level).astype(np.uint64)
    return np.stack([np.uint64(0) - d @ key[z] for z in range(k1)], axis=1)


def torus_round(c):
    """the canonical back-conversion of the exact value c (torus units of 2^-64): w = c / 2^64; w -= rint(w); rint(w 2^64) mod 2^64,
    rint rounding ties to even (Python's round() on a Fraction does)"""
    w = Fraction(c) / (1 << 64)
    w -= round(w)
    return int(round(w * (1 << 64))) % (1 << 64)


def trivial_bsk(s, p):
    """a noise-free bootstrapping key of the binary LWE key s under the ZERO GLWE key: bsk[i][l][k][k][0] = s_i 2^(64 - 8 (l + 1)),
    every other word 0 -- [n][pbs_level][k+1][k+1][N]"""
    k1 = p.k + 1
    bsk = np.zeros((p.n, p.pbs_level, k1, k1, p.N), dtype=np.uint64)
    for l in range(p.pbs_level):
        bsk[:, l, p.k, p.k, 0] = np.asarray(s, dtype=np.uint64) << np.uint64(64 - p.pbs_base_log * (l + 1))
    return bsk


def blind_rotation_trivial(x, s, p):
    """K2 (cbs_pbs at level 1) under trivial_bsk(s): x [m][n+1] -> [m][kN+1].

    The external product by GGSW i multiplies the body by s_i and leaves the zero masks zero, so one iteration turns the accumulator
    acc into acc X^(s_i a~_i) exactly (its coefficients are +-2^48: two roundings away from any tie), and the loop ends at
    tv X^e,  e = (-b~ + sum_i s_i a~_i) mod 1024,  tv = -2^48 (1 + X + ... + X^511),  b~ = mod_switch(b + 2^62).
    Coefficient 0 of (1 + ... + X^511) X^e is +1 for e = 0, -1 for 0 < e <= 512 (X^(512 - e) X^e = X^512 = -1) and +1 for e > 512
    (X^(1024 - e) X^e = X^1024 = 1); the sample extraction takes it and the stage adds 2^48: body = 2^48 - sign 2^48, masks 0."""
    x = np.asarray(x, dtype=np.uint64)
    half = 1 << (64 - p.cbs_base_log - 1)
    out = np.zeros((x.shape[0], p.big1), dtype=np.uint64)
    s = [int(v) for v in s]
    assert len(s) == p.n and set(s) <= {0, 1}
    for r, row in enumerate(x.tolist()):
        e = (-mod_switch((row[p.n] + (1 << 62)) & M64) + sum(si * mod_switch(a) for si, a in zip(s, row[:p.n]))) % 1024
        sign = 1 if (e == 0 or e > 512) else -1
        out[r, p.big] = (half - sign * half) & M64
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# K2: small LWE rows [m][n+1]
# ---------------------------------------------------------------------------------------------------------------------------------
TIE_T = (0, 1, 2, 255, 256, 511, 512, 513, 1022, 1023)


def tie_words():
    """(2t+1) 2^53 + {-1, 0, 1} (the ties of the modulus switch and their neighbours), t 2^54 + {-1, 0, 1} (the exact values and
    theirs) for the listed t, and the four extreme words: 64 words"""
    w = []
    for t in TIE_T:
        w += [((2 * t + 1) * (1 << 53) + e) & M64 for e in (-1, 0, 1)]
        w += [(t * (1 << 54) + e) & M64 for e in (-1, 0, 1)]
    return w + list(EXTREMES)


def k2_rows(n, seed=0x2E06E):
    """the K2 edge set [rows][n+1] (no padding: the callers cycle it) and its classes"""
    rng = np.random.default_rng(seed)
    blocks = []
    # (1) every switched body value once: b~ = mod_switch(x + 2^62) = b
    a = rng.integers(0, 1 << 64, (1024, n + 1), dtype=np.uint64)
    a[:, n] = [((b << 54) - (1 << 62)) & M64 for b in range(1024)]
    blocks.append(a)
    # (2) tie words in every mask position and in the body, the body both as the word itself and as the word before the 2^62 shift
    W = tie_words()
    t = np.empty((2 * len(W), n + 1), dtype=np.uint64)
    for r in range(len(W)):
        row = [W[(r + j) % len(W)] for j in range(n + 1)]
        t[2 * r] = row
        row[n] = (row[n] - (1 << 62)) & M64
        t[2 * r + 1] = row
    blocks.append(t)
    # (3) whole rows of one mask word, under four bodies each
    bodies = [0, 1 << 63, ((1 << 53) - (1 << 62)) & M64, int(rng.integers(0, 1 << 64, dtype=np.uint64))]
    for word in (0, 1 << 63, M64, 1 << 54):
        c = np.full((len(bodies), n + 1), word, dtype=np.uint64)
        c[:, n] = bodies
        blocks.append(c)
    # (4) uniform random rows
    blocks.append(rng.integers(0, 1 << 64, (32, n + 1), dtype=np.uint64))
    x = np.ascontiguousarray(np.concatenate(blocks))
    return x, k2_classes(x)


def k2_classes(x):
    n = x.shape[1] - 1
    rows = x.tolist()
    words = {w for row in rows for w in row[:n]} | {(row[n] + (1 << 62)) & M64 for row in rows}       # what the modulus switch sees
    masks = [[mod_switch(w) for w in row[:n]] for row in rows]
    ties = 0
    for t in TIE_T:
        tie = (2 * t + 1) << 53
        if tie - 1 in words and tie in words and mod_switch(tie - 1) == t and mod_switch(tie) == (t + 1) % 1024:
            ties += 1
    return {
        "distinct_body": len({mod_switch((row[n] + (1 << 62)) & M64) for row in rows}),
        "ties_both_sides": ties,
        "tie_in_body": sum(1 for row in rows if ((row[n] + (1 << 62)) & M64) & ((1 << 54) - 1) == 1 << 53),
        "tie_in_mask": sum(1 for row in rows for w in row[:n] if w & ((1 << 54) - 1) == 1 << 53),
        "wrap_to_zero": sum(1 for w in words if w >= (1 << 64) - (1 << 53) and mod_switch(w) == 0),
        "rows_all_mask_0": sum(1 for m in masks if set(m) == {0}),
        "rows_all_mask_512": sum(1 for m in masks if set(m) == {512}),
        "rows_all_mask_1": sum(1 for m in masks if set(m) == {1}),
        "rows_all_mask_wrapped": sum(1 for row, m in zip(rows, masks) if set(m) == {0} and set(row[:n]) == {M64}),
        "extreme_words": sum(1 for e in EXTREMES if e in words),
    }


# ---------------------------------------------------------------------------------------------------------------------------------
# K1 / K3: big LWE rows [m][kN+1] and keys
# ---------------------------------------------------------------------------------------------------------------------------------
def gadget(p, stage):
    return {"K1": (p.ks_base_log, p.ks_level), "K3": (p.pfks_base_log, p.pfks_level)}[stage]


def half_digit_words(b, level):
    """words with as many digits of +B/2, and of -B/2, as the key switches' rule can produce.

    Under that rule a digit of magnitude B/2 needs the raw digit B/2 (after the carry from below), and its sign is the top bit of the
    raw digit above it: + where that bit is clear, - where it is set.  Two neighbouring levels can therefore never both hold +-B/2
    (the upper one would need the raw value B/2, top bit set, and B/2 - 1 or B/2 with the top bit clear at once), and level 1 has
    nothing above it, so it is never -B/2.  The most a word can hold is +B/2 at levels L, L-2, ... (ceil(L/2) digits) and -B/2 at
    levels L, L-2, ... above level 1 (floor(L/2) digits).  Returns (word with every other digit +B/2, its count, word with every
    other digit -B/2, its count)."""
    h, best = 1 << (b - 1), {}
    for sign in (1, -1):
        for top in (1, 2):                                        # every other level, ending at level L, starting at 1 or 2
            levels = [l for l in range(level, 0, -2) if l >= top]
            x = sum(sign * h << (64 - b * l) for l in levels) & M64
            cnt = decompose(x, b, level).count(sign * h)
            if cnt > best.get(sign, (0, 0))[1]:
                best[sign] = (x, cnt)
    return best[1][0], best[1][1], best[-1][0], best[-1][1]


def ks_words(p, stage):
    """name -> word: the edge words of a key switch's input"""
    b, level = gadget(p, stage)
    r = 64 - b * level
    plus, _, minus, _ = half_digit_words(b, level)
    w = {"half_plus": plus, "half_minus": minus, "all_ones": M64, "below_round": (1 << (r - 1)) - 1, "round_tie": 1 << (r - 1),
         "zero": 0, "top_bit": 1 << 63, "below_top": (1 << 63) - 1,
         "raw_half": sum((1 << (b - 1)) << (64 - b * (l + 1)) for l in range(level))}
    if stage == "K3":
        w["lo_m128_hi_8"] = sum(1920 << (64 - b * (l + 1)) for l in range(level))       # every digit 1920 = 8 * 256 - 128
        w["lo_127"] = sum(1919 << (64 - b * (l + 1)) for l in range(level))             # every digit 1919 = 7 * 256 + 127
    return w


def ks_inputs(p, stage, m, seed=0x15E0):
    """[m][kN+1]: one full row per edge word first (the order of ks_words), then rows that mix them per word with random words"""
    rng = np.random.default_rng(seed + (1 if stage == "K3" else 0))
    words = ks_words(p, stage)
    vals = np.array(list(words.values()), dtype=np.uint64)
    assert m > len(vals) + 2
    x = np.empty((m, p.big1), dtype=np.uint64)
    for i, v in enumerate(vals):
        x[i] = v
    mixed = m - len(vals)
    pick = rng.integers(0, len(vals) + 2, (mixed, p.big1))                   # two of the choices mean "a random word"
    rnd = rng.integers(0, 1 << 64, (mixed, p.big1), dtype=np.uint64)
    x[len(vals):] = np.where(pick < len(vals), vals[np.minimum(pick, len(vals) - 1)], rnd)
    return x, ks_input_classes(x, p, stage)


def ks_input_classes(x, p, stage):
    b, level = gadget(p, stage)
    h = 1 << (b - 1)
    words = ks_words(p, stage)
    _, n_plus, _, n_minus = half_digit_words(b, level)
    full = {name: 0 for name in words}
    mixed = 0
    for row in x.tolist():
        kinds = set(row)
        if len(kinds) == 1:
            for name, v in words.items():
                if row[0] == v:
                    full[name] += 1
        elif len(kinds & set(words.values())) >= len(words) - 1:
            mixed += 1
    c = {"full_" + name: cnt for name, cnt in full.items()}
    c["mixed_rows"] = mixed
    c["half_plus_digits"] = decompose(words["half_plus"], b, level).count(h)
    c["half_minus_digits"] = decompose(words["half_minus"], b, level).count(-h)
    c["half_plus_max"], c["half_minus_max"] = n_plus, n_minus
    c["all_ones_digits_zero"] = int(not any(decompose(M64, b, level)))
    if stage == "K3":
        c["planes_lo_m128_hi_8"] = int({digit_planes(d) for d in decompose(words["lo_m128_hi_8"], b, level)} == {(-128, 8)})
        c["planes_lo_127"] = int({digit_planes(d)[0] for d in decompose(words["lo_127"], b, level)} == {127})
    return c


KEY_M128 = 0x7F7F7F7F7F7F7F80          # every balanced byte -128: the carry runs through all eight bytes
KEY_P127 = 0x7F7F7F7F7F7F7F7F          # every balanced byte +127
KEY_ALT = 0x0080008000800080           # balanced bytes -128, 1 alternating: a carry that stops at once, four times
KEY_PATTERNS = ("m128", "p127", "ones", "top", "mixture")


def key_words(pattern, shape, seed=0x6E7):
    """a key of `shape` uint64 words: one word everywhere, or per word one of the four, KEY_ALT or a random word"""
    one = {"m128": KEY_M128, "p127": KEY_P127, "ones": M64, "top": 1 << 63}
    if pattern in one:
        return np.full(shape, one[pattern], dtype=np.uint64)
    assert pattern == "mixture"
    rng = np.random.default_rng(seed)
    table = np.array([KEY_M128, KEY_P127, M64, 1 << 63, KEY_ALT], dtype=np.uint64)
    pick = rng.integers(0, 7, shape, dtype=np.uint8)                          # 5 and 6: a random word
    out = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    np.copyto(out, table[np.minimum(pick, 4)], where=pick < 5)
    return out


def k3_accumulator_peak(x_row, key_word, p):
    """max over the eight int32 accumulators of one K3 output under a key of one word everywhere, from digits and balanced bytes:
    accumulator s sums  low plane x byte s  +  high plane x byte s-1  over all Q = (kN+1) levels rows.  Returns (peak, Q 128 128)"""
    b, level = gadget(p, "K3")
    kb = balanced_bytes(key_word)
    lo = hi = 0
    for w in x_row.tolist():
        for d in decompose(w, b, level):
            l, h = digit_planes(d)
            lo, hi = lo + l, hi + h
    peak = max(abs(lo * kb[s] + (hi * kb[s - 1] if s else 0)) for s in range(8))
    return peak, p.big1 * level * 128 * 128


# ---------------------------------------------------------------------------------------------------------------------------------
# K4: torus polynomials
# ---------------------------------------------------------------------------------------------------------------------------------
K4_WORDS = (0, 1, M64, 1 << 63, (1 << 63) - 1, (1 << 53) + 1, (1 << 54) + 2)
K4_MONOMIALS = (0, 255, 256, 511)


def k4_polys():
    """[polys][512]: polynomials of one word everywhere (2^53 + 1 and 2^54 + 2 are ties of the int64 -> f64 conversion), single
    monomials of 1, of 2^63 and of 2^64 - 1 at the first and last coefficient of either half"""
    polys = [np.full(512, w, dtype=np.uint64) for w in K4_WORDS]
    for j in K4_MONOMIALS:
        for v in (1, 1 << 63, M64):
            q = np.zeros(512, dtype=np.uint64)
            q[j] = v
            polys.append(q)
    x = np.stack(polys)
    classes = {"constant": sum(1 for q in x if len(set(q.tolist())) == 1 and int(q[0]) in K4_WORDS),
               "monomial": sum(1 for q in x if np.count_nonzero(q) == 1 and int(np.flatnonzero(q)[0]) in K4_MONOMIALS)}
    return x, classes


# ---------------------------------------------------------------------------------------------------------------------------------
# K5 / CMUX: the constant-spectrum family and the generic one
# ---------------------------------------------------------------------------------------------------------------------------------
CMUX_D = (1, -1, 3, -3, 5, -5, 8192, -8192, 12288, -12288, 16383, -16384)
CMUX_G = tuple(s * 2.0 ** e for e in (-2, -1, 0, 31, 32, 38, 39, 49, 50, 51, 52) for s in (1.0, -1.0))
CMUX_BITS = 10
CMUX_OFFSETS = {4: (0, 15), 1: (0, 6, 12, 18)}           # by k: 3 inputs x (k + 1) columns per call walk the whole list of g


def cmux_constant_family(p, n_inputs, n_luts, offset, seed=0xC0857):
    """10-bit vertical packing with lut_per_input whose result is known exactly.

    One tree level: cmux(GGSW of bit 9, P0, P1) = P0 + GGSW (x) (P1 - P0).  P1 - P0 is d 2^49 at coefficient 0 of the body: one digit d
    of the 15-bit gadget, whose transform is the constant d.  The GGSW's body row is the constant g_c in column c, so column c of the
    product has the constant spectrum d g_c (exact: g_c is a power of two), whose inverse transform is 256 d g_c at coefficient 0:
    the back-conversion is asked for exactly torus_round(d g_c).  The mask rows of the GGSW are finite random doubles against zero
    digits; the GGSWs of bits 0..8 are +0.0, so the rotation adds nothing.  Expected output: mask word 512 c = torus_round(d g_c),
    every other mask word 0, body = P0[0] + torus_round(d g_k).

    Returns (ggsw_f [n_inputs][10][1][k+1][k+1][256][2], luts [n_inputs][n_luts][10][1024], expected [n_inputs][n_luts][10][kN+1]),
    classes."""
    rng = np.random.default_rng(seed + 131 * offset + p.k)
    k1, bits = p.k + 1, CMUX_BITS
    g = np.array([[CMUX_G[(offset + i * k1 + c) % len(CMUX_G)] for c in range(k1)] for i in range(n_inputs)])
    ggsw = np.zeros((n_inputs, bits, 1, k1, k1, 256, 2), dtype=np.float64)
    ggsw[:, 9, 0, :p.k] = rng.standard_normal((n_inputs, p.k, k1, 256, 2)) * 2.0 ** 60
    ggsw[:, 9, 0, p.k, :, :, 0] = g[:, :, None]
    inst = n_luts * bits
    d = np.empty((n_inputs, inst), dtype=np.int64)
    for i in range(n_inputs):
        for q in range(inst):
            j = (q + i) % (len(CMUX_D) + 4)
            d[i, q] = CMUX_D[j] if j < len(CMUX_D) else int(rng.integers(-8192, 8192)) * 2 + 1
    luts = rng.integers(0, 1 << 64, (n_inputs, inst, 2, 512), dtype=np.uint64)
    luts[:, :, 1] = luts[:, :, 0]
    luts[:, :, 1, 0] += (d % (1 << 15)).astype(np.uint64) << np.uint64(49)
    want = np.zeros((n_inputs, inst, p.big1), dtype=np.uint64)
    cls = {"low_tie": 0, "half": 0, "hi_tie": 0, "wraps": 0, "values": 0}
    for i in range(n_inputs):
        for q in range(inst):
            for c in range(k1):
                v = Fraction(int(d[i, q])) * Fraction(float(g[i, c]))
                t = torus_round(v)
                cls["values"] += 1
                cls["low_tie"] += int(v.denominator == 2)                                                 # v is a half-integer
                red = v / (1 << 64) - round(v / (1 << 64))                                            # w after w -= rint(w)
                cls["half"] += int(abs(red) == Fraction(1, 2))
                cls["hi_tie"] += int((red * (1 << 32)).denominator == 2)
                cls["wraps"] += int(abs(v) >= 1 << 63)
                if c < p.k:
                    want[i, q, c * 512] = t
                else:
                    want[i, q, p.big] = (int(luts[i, q, 0, 0]) + t) & M64
    shape = (n_inputs, n_luts, bits)
    return (ggsw, np.ascontiguousarray(luts.reshape(shape + (1024,))), want.reshape(shape + (p.big1,))), cls


def cmux_generic_family(p, n_inputs, n_luts, bits, seed=0x6E2E):
    """random LUT words and Fourier GGSWs whose every entry is +0.0, -0.0, +-2^63 or an honest-scale value (normal 2^66).
    Returns (ggsw_f [n_inputs][bits][1][k+1][k+1][256][2], luts [n_luts][bits][W]), classes"""
    rng = np.random.default_rng(seed + 16 * bits + p.k)
    k1, W = p.k + 1, max(512, 1 << bits)
    shape = (n_inputs, bits, 1, k1, k1, 256, 2)
    pick = rng.integers(0, 8, shape)
    table = np.array([0.0, -0.0, 2.0 ** 63, -(2.0 ** 63)])
    ggsw = np.where(pick < 4, table[np.minimum(pick, 3)], rng.standard_normal(shape) * 2.0 ** 66)
    luts = rng.integers(0, 1 << 64, (n_luts, bits, W), dtype=np.uint64)
    bitsview = np.ascontiguousarray(ggsw).view(np.uint64)
    cls = {"plus_zero": int((bitsview == 0).sum()), "minus_zero": int((bitsview == 1 << 63).sum()),
           "two_63": int((np.abs(ggsw) == 2.0 ** 63).sum()), "finite": int(np.isfinite(ggsw).all())}
    return (np.ascontiguousarray(ggsw), luts), cls
