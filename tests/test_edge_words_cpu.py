"""The edge sets of edge_words.py on the CPU: every generator holds the classes it is meant to hold, and the oracle agrees with the
plain references on them -- so that test_gpu_edge_words.py can take the oracle as the reference for the HIP kernels on these words.

No oracle output is stored: the GPU tests compare against the oracle live."""
import numpy as np
import pytest

import edge_words as ew
from edge_words import PARAM_EDGE
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_TOY


# ---- the conditions: what each set contains, computed with the plain references -------------------------------------------------
def test_k2_edge_rows_hold_their_classes():
    x, c = ew.k2_rows(PARAM_EDGE.n)
    assert x.shape[1] == PARAM_EDGE.n + 1 == PARAM_TOY.n + 1
    assert c["distinct_body"] == 1024
    assert c["ties_both_sides"] == len(ew.TIE_T) and c["tie_in_body"] >= len(ew.TIE_T) and c["tie_in_mask"] >= len(ew.TIE_T) * PARAM_EDGE.n
    assert c["wrap_to_zero"] >= 3                      # (2 * 1023 + 1) 2^53, the word after it, 2^64 - 1
    assert c["rows_all_mask_0"] >= 2 and c["rows_all_mask_wrapped"] >= 1 and c["rows_all_mask_512"] >= 1 and c["rows_all_mask_1"] >= 1
    assert c["extreme_words"] == 4
    assert ew.mod_switch((1 << 64) - (1 << 53)) == 0 and ew.mod_switch((1 << 64) - (1 << 53) - 1) == 1023


@pytest.mark.parametrize("stage", ["K1", "K3"])
@pytest.mark.parametrize("p", [PARAM_TOY, PARAM_EDGE], ids=lambda p: p.name)
def test_key_switch_inputs_hold_their_classes(p, stage):
    b, level = ew.gadget(p, stage)
    x, c = ew.ks_inputs(p, stage, 20)
    for name in ew.ks_words(p, stage):
        assert c["full_" + name] >= 1, name
    assert c["mixed_rows"] >= 1 and c["all_ones_digits_zero"] == 1
    # digits of +-B/2: as many as the rule can produce (edge_words.half_digit_words says why no word has them at every level)
    assert c["half_plus_digits"] == c["half_plus_max"] == (level + 1) // 2
    assert c["half_minus_digits"] == c["half_minus_max"] == level // 2
    if stage == "K3":
        assert c["planes_lo_m128_hi_8"] == 1 and c["planes_lo_127"] == 1
        row = x[list(ew.ks_words(p, stage)).index("lo_m128_hi_8")]
        peak, bound = ew.k3_accumulator_peak(row, ew.KEY_M128, p)
        assert 0.9 * bound <= peak <= bound < 1 << 31              # the int32 bound of kern_keyswitch.h, reached
        assert ew.balanced_bytes(ew.KEY_M128) == [-128] * 8 and ew.balanced_bytes(ew.KEY_P127) == [127] * 8
        assert ew.balanced_bytes(ew.M64) == [-1, 0, 0, 0, 0, 0, 0, 0] and ew.balanced_bytes(ew.KEY_ALT) == [-128, 1] * 4


def test_no_word_has_neighbouring_half_digits():
    """the reason the key-switch rows hold +-B/2 at every other level only: exhaustive at base 2^2 x 6 levels (all 2^12 digit strings
    with every continuation below), sampled around every candidate at base 2^12 x 3 levels"""
    for top in range(1 << 12):
        for low in (0, 1 << 51, (1 << 52) - 1):
            d = ew.decompose((top << 52) | low, 2, 6)
            assert all(not (abs(d[l]) == 2 and abs(d[l + 1]) == 2) for l in range(5)) and d[0] != -2
    rng = np.random.default_rng(12)
    for a in (2047, 2048, 2049):
        for b_ in (2047, 2048, 2049):
            for c_ in (2047, 2048, 2049):
                for low in (0, 1 << 27, (1 << 28) - 1, int(rng.integers(0, 1 << 28))):
                    d = ew.decompose((a << 52) | (b_ << 40) | (c_ << 28) | low, 12, 3)
                    assert all(not (abs(d[l]) == 2048 and abs(d[l + 1]) == 2048) for l in range(2)) and d[0] != -2048


def test_k4_and_cmux_sets_hold_their_classes():
    x, c = ew.k4_polys()
    assert c == {"constant": len(ew.K4_WORDS), "monomial": 3 * len(ew.K4_MONOMIALS)} and x.shape == (19, 512)
    for p, offsets in ((PARAM_EDGE, ew.CMUX_OFFSETS[4]), (PARAM_TOY, ew.CMUX_OFFSETS[1])):
        total = {}
        for off in offsets:
            _, cls = ew.cmux_constant_family(p, 3, 2, off)
            for k, v in cls.items():
                total[k] = total.get(k, 0) + v
        assert total["low_tie"] >= 8 and total["half"] >= 4 and total["hi_tie"] >= 4 and total["wraps"] >= 8, (p.name, total)
    for bits in (1, 9, 11):
        _, cls = ew.cmux_generic_family(PARAM_EDGE, 3, 2, bits)
        assert cls["finite"] == 1 and min(cls["plus_zero"], cls["minus_zero"], cls["two_63"]) > 0


def test_torus_round_is_the_canonical_rounding():
    assert ew.torus_round(0) == 0 and ew.torus_round(-1) == ew.M64 and ew.torus_round(1 << 64) == 0
    assert ew.torus_round(ew.Fraction(1, 2)) == 0 and ew.torus_round(ew.Fraction(3, 2)) == 2 and ew.torus_round(ew.Fraction(-1, 2)) == 0
    assert ew.torus_round(ew.Fraction(-3, 2)) == ew.M64 - 1 and ew.torus_round(ew.Fraction(5, 2)) == 2
    assert ew.torus_round(1 << 63) == ew.torus_round(-(1 << 63)) == ew.torus_round(3 << 63) == 1 << 63       # w = +-1/2: r = +-2^63 wraps


# ---- key switches: oracle == plain uint64 matrix product -------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ew.KEY_PATTERNS)
def test_key_switches_toy_oracle_against_the_plain_product(pattern):
    p = PARAM_TOY
    ksk = ew.key_words(pattern, (p.big, p.ks_level, p.n + 1))
    pf = ew.key_words(pattern, (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8)
    bsk = np.zeros(p.bsk_words, dtype=np.uint64)
    o = orc.Oracle(p, ksk, bsk, pf)
    x1, _ = ew.ks_inputs(p, "K1", 16)
    x3, _ = ew.ks_inputs(p, "K3", 16)
    assert np.array_equal(o.keyswitch(x1), ew.keyswitch_plain(x1, ksk, p))
    assert np.array_equal(o.pfpks(x3), ew.pfpks_plain(x3, pf, p))


def test_key_switches_k4_oracle_against_the_plain_product():
    """k = 4, the mixture keys, 2 mixed rows (the PFPKSK has 630 MB whatever n is: one array)"""
    p = PARAM_EDGE
    ksk = ew.key_words("mixture", (p.big, p.ks_level, p.n + 1))
    pf = ew.key_words("mixture", (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8)
    o = orc.Oracle(p, ksk, np.zeros(p.bsk_words, dtype=np.uint64), pf)
    x1 = ew.ks_inputs(p, "K1", 16)[0][-2:]
    x3 = ew.ks_inputs(p, "K3", 16)[0][-2:]
    assert np.array_equal(o.keyswitch(x1), ew.keyswitch_plain(x1, ksk, p))
    assert np.array_equal(o.pfpks(x3), ew.pfpks_plain(x3, pf, p))


# ---- blind rotation under the trivial BSK: oracle == closed form ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ones", "random"])
def test_blind_rotation_trivial_bsk_oracle_against_the_closed_form(which):
    p = PARAM_EDGE
    s = np.ones(p.n, dtype=np.uint64) if which == "ones" else trivial_key(p)
    assert which == "ones" or 0 < int(s.sum()) < p.n
    x, _ = ew.k2_rows(p.n)
    o = orc.Oracle(p, np.zeros(1, dtype=np.uint64), ew.trivial_bsk(s, p), np.zeros(1, dtype=np.uint64))
    got, want = o.cbs_pbs(x), ew.blind_rotation_trivial(x, s, p)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:16]
    assert set(np.unique(want[:, p.big]).tolist()) == {0, 1 << 49}            # both signs occur


def trivial_key(p):
    return np.random.default_rng(0x5EC).integers(0, 2, p.n, dtype=np.uint64)


# ---- vertical packing ------------------------------------------------------------------------------------------------------------
def vp_oracle(p, ggsw_f, luts, per_input):
    """the oracle on a whole call: ggsw_f [n_inputs][bits]..., luts [n_sets][n_luts][bits][W] -> [n_inputs][n_luts][bits][kN+1]"""
    bits = ggsw_f.shape[1]
    return np.stack([orc.vertical_packing(p, ggsw_f[i], bits, luts[i if per_input else 0]) for i in range(ggsw_f.shape[0])])


@pytest.mark.parametrize("p", [PARAM_EDGE, PARAM_TOY], ids=lambda p: p.name)
def test_vertical_packing_constant_spectrum_oracle_against_exact_rounding(p):
    for off in ew.CMUX_OFFSETS[p.k]:
        (ggsw_f, luts, want), _ = ew.cmux_constant_family(p, 3, 2, off)
        got = vp_oracle(p, ggsw_f, luts, True)
        assert np.array_equal(got, want), (off, np.argwhere(got != want)[:8])


@pytest.mark.parametrize("bits", [1, 9, 11])
def test_vertical_packing_generic_oracle_is_deterministic(bits):
    p = PARAM_EDGE
    (ggsw_f, luts), _ = ew.cmux_generic_family(p, 3, 2, bits)
    a = vp_oracle(p, ggsw_f, luts[None], False)
    b = vp_oracle(p, ggsw_f.copy(), luts[None].copy(), False)
    assert a.shape == (3, 2, bits, p.big1) and np.array_equal(a, b) and len(np.unique(a)) > a.size // 2
