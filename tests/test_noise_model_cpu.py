"""The noise budget (tests/noise_model.py) against the CPU oracle: every stage of a WoPBS at PARAM_TOY, K1 and one external product
per gadget at PARAM_OPT, the checker itself, and the model's closed values.  The oracle had never been held to a derived noise value:
the parity tests compare the kernels with it word for word, so a flaw the two share shows only here and in test_gpu_noise.py.

Every case measures an error as a signed integer (a phase against the phase or the message it should carry) and hands it to
noise_model.assert_noise with the variance the model derives and the number of ciphertexts whose errors do not share a mask.  Nothing
here is fitted: the bands are sampling bounds, and the model's one measured input is the f64 transform's error against the exact
schoolbook product."""
import math

import numpy as np
import pytest

import edge_words as ew
import noise_model as nm
from gpu_support import oc, tc  # noqa: F401  (clients with the kits' keys and an encryption sequence of their own)
from oracle import oracle as orc
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.server import gen_lut

# what test_gpu_noise.py uses: name -> independent ciphertexts.  The doubling condition is asserted on every one of them.
GPU_CASES = {
    "K1": 4096, "K2 opt": 2100, "K2 toy": 300, "K3": 64, "sweep toy": 256 * 8, "sweep opt": 256, "wide 10": 32 * 10, "wide 12": 32 * 12,
    "AES output": 128, "key expansion toy": 208 * 8, "key expansion opt": 208, "equivalent inverse toy": 256 * 8, "equivalent inverse opt": 256,
    # PARAM_OPT, where the outputs of one input share its GGSWs: 64 inputs, or 64 bytes of 4 blocks under 4 keys
    "wide 10 opt": 64, "wide 12 opt": 64, "wide 16 opt": 64, "tag LUT row 0 opt": 64, "CMAC output opt": 64, "tag difference opt": 64,
}


@pytest.fixture(scope="module")
def tm(toy):
    return nm.NoiseModel.of_client(toy.client)


@pytest.fixture(scope="module")
def om(opt):
    return nm.NoiseModel.of_client(opt.client)


# ---- the model's inputs -------------------------------------------------------------------------------------------------------------------
def test_digit_moments_come_from_the_plain_references():
    mean, second = nm.digit_moments("signed", 2, 6)
    assert len(second) == 6 and all(1.2 < v < 1.55 for v in second) and max(second) - min(second) > 0.1   # about 1.3, and not one value
    assert abs(sum(second) / 6 - 4 / 12) > 0.9                                 # B^2 / 12 = 0.33 would be four times too small
    assert abs(mean[0] - 0.4) < 0.01 and all(abs(v) < 1e-9 for v in mean[1:])
    for rule, b, L in (("signed", 12, 3), ("offset", 8, 5), ("offset", 15, 1)):
        mean, second = nm.digit_moments(rule, b, L)
        for m1, m2 in zip(mean, second):
            assert abs(m2 / (4.0 ** b / 12) - 1) < 0.02 and abs(m1) < 0.02 * 2.0 ** b
    assert nm.digit_moments("offset", 15, 1)[0][0] == -0.5                       # the offset rule's digits are uniform in [-B/2, B/2)


def test_offset_digits_is_the_plain_reference():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(0, 1 << 64, 300, dtype=np.uint64), np.array(ew.EXTREMES, dtype=np.uint64)])
    for b, L in ((8, 5), (15, 1)):
        d = nm.offset_digits(x, b, L)
        assert all(list(d[:, i]) == ew.decompose_offset(int(x[i]), b, L) for i in range(x.size))


def test_transform_error_is_the_measured_input():
    v8, v15 = nm.fft_variance(8), nm.fft_variance(15)
    assert 43.2 < math.log2(v8) < 43.6 and 57.2 < math.log2(v15) < 57.6          # std 2^21.7 and 2^28.7 per coefficient
    assert abs(math.log2(v15 / v8) - 14) < 0.3                                   # proportional to the digits: seven more bits of them


def test_a_chain_of_products_loses_more_than_its_products():
    """the external product accumulates (k+1) L products in the Fourier domain in one fma chain per point and transforms back once: the
    running sum is rounded at every step, so the error grows faster than the number of products -- and it is weaker at the lowest
    frequencies, which a binary key polynomial (mean 1/2) weighs most"""
    for k, b, L, lo, hi in ((1, 8, 5, 1.12, 1.24), (4, 8, 5, 1.30, 1.45), (1, 15, 1, 1.0, 1.06), (4, 15, 1, 1.03, 1.12)):
        v, a = nm.fft_chain_variance(k, b, L)
        ratio = v / ((k + 1) * L * nm.fft_variance(b))
        print("k = %d, B = 2^%d, %d levels: v_chain = %.3f (k+1) L v_fft, a = %.3f" % (k, b, L, ratio, a))
        assert lo < ratio < hi and 0.65 < a < 0.9


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def test_max_sigmas():
    assert nm.max_sigmas(64) == 8 and nm.max_sigmas(1 << 15) == 8 and nm.max_sigmas(1 << 20) == 8.5
    for n in (1 << 15, 1 << 20):
        assert n * math.erfc(nm.max_sigmas(n) / math.sqrt(2)) < 2.0 ** -30


def test_every_gpu_case_rejects_a_doubled_variance():
    for name, n in GPU_CASES.items():
        assert 1 + nm.band(n) < 2, name
        assert nm.rejects_doubling(n), name
    assert not nm.rejects_doubling(50)


def test_outputs_that_share_their_ggsws_count_once_where_that_matters(tm, om):
    assert tm.wopbs_independent(256, 8) == GPU_CASES["sweep toy"] and om.wopbs_independent(256, 8) == GPU_CASES["sweep opt"]
    assert tm.wopbs_independent(208, 8) == GPU_CASES["key expansion toy"] and om.wopbs_independent(208, 8) == GPU_CASES["key expansion opt"]
    assert tm.wopbs_independent(32, 12, 12) == GPU_CASES["wide 12"] and tm.wopbs_independent(32, 10, 10) == GPU_CASES["wide 10"]
    assert 7 * tm.cmux(0) / tm.wopbs_mean(8) < 0.05 and 0.55 < 7 * om.cmux(0) / om.wopbs_mean(8) < 0.7
    for width in (10, 12, 16):
        assert om.wopbs_independent(64, width, width) == GPU_CASES["wide %d opt" % width]
    assert om.wopbs_independent(64, 1, 16) == GPU_CASES["tag LUT row 0 opt"]
    assert om.wopbs_independent(64, 8) == GPU_CASES["CMAC output opt"] == GPU_CASES["tag difference opt"]


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_checker_accepts_one_sigma_and_rejects_one_and_a_half(name):
    n = GPU_CASES[name]
    rng = np.random.default_rng(n)
    sigma = 2.0 ** 40
    z = rng.normal(0.0, 1.0, n)
    nm.assert_noise(np.rint(z * sigma), sigma * sigma, n, name)                  # a Gaussian sample as drawn
    z /= math.sqrt(np.mean(z * z))                                               # then one of exactly unit mean square, scaled
    nm.assert_noise(np.rint(z * sigma), sigma * sigma, n, name)
    with pytest.raises(AssertionError):
        nm.assert_noise(np.rint(1.5 * z * sigma), sigma * sigma, n, name)          # 2.25 times the variance
    with pytest.raises(AssertionError):
        nm.assert_noise(np.rint(math.sqrt(2.0) * z * sigma), sigma * sigma, n, name)   # twice the variance: the doubling condition
    if nm.band(n) < 1 - 1 / 2.25:                                                # a model that overstates by 1.5 sigma fails as well,
        with pytest.raises(AssertionError):                                      # where the band's lower edge is above 0.44
            nm.assert_noise(np.rint(z * sigma / 1.5), sigma * sigma, n, name)


def test_checker_weighs_each_sample_and_bounds_the_worst():
    rng = np.random.default_rng(11)
    var = np.where(np.arange(4096) % 2 == 0, 1.0, 100.0) * 2.0 ** 60
    e = rng.normal(0.0, 1.0, 4096) * np.sqrt(var)
    nm.assert_noise(e, var, 4096, "two classes")
    flat = rng.normal(0.0, 1.0, 4096) * math.sqrt(var.mean())
    nm.assert_noise(flat, var.mean(), 4096, "one class")
    with pytest.raises(AssertionError):
        nm.assert_noise(flat, var, 4096, "one class held to two: the same mean square, but not sample by sample")
    e[7] = 9.0 * math.sqrt(var[7])
    with pytest.raises(AssertionError):
        nm.assert_noise(e, var, 4096, "one sample at nine sigma")
    # a term left out on purpose widens the upper side only
    z = rng.normal(0.0, 1.0, 4096) * 2.0 ** 30
    nm.assert_noise(1.12 * z, 2.0 ** 60, 4096, "left out", left_out=0.3 * 2.0 ** 60)
    with pytest.raises(AssertionError):
        nm.assert_noise(1.12 * z, 2.0 ** 60, 4096, "not left out")
    with pytest.raises(AssertionError):
        nm.assert_noise(z / 1.12, 2.0 ** 60, 4096, "the lower side stays", left_out=0.3 * 2.0 ** 60)


# ---- closed values: a change to the model shows in review ---------------------------------------------------------------------------------
TOY_LOG2 = {"k1": 54.22, "modswitch": 54.11, "extprod0": 27.52, "extprod1": 27.63, "k2": 29.85, "pfks": 29.50, "k3_carried": 30.56,
            "cmux0": 48.24, "cmux1": 51.23, "wopbs8": 52.15, "aes_out": 52.65, "wopbs16": 52.70, "wopbs16_x0": 50.19}
OPT_LOG2 = {"k1": 56.20, "modswitch": 56.41, "extprod0": 29.17, "extprod1": 29.22, "k2": 33.89, "pfks": 29.01, "k3_carried": 33.90,
            "cmux0": 52.11, "cmux1": 52.66, "wopbs8": 53.84, "aes_out": 54.34, "wopbs16": 54.39, "wopbs16_x0": 54.06}


def test_closed_values_param_toy(tm):
    got = tm.log2_sigmas()
    print({k: round(v, 2) for k, v in got.items()})
    assert (tm.h_small, tm.h_polys) == (13, (259,))
    for name, want in TOY_LOG2.items():
        assert want - 0.1 < got[name] < want + 0.1, (name, got[name])
    assert 135 < tm.decision_margin() < 148


def test_closed_values_param_opt(om):
    got = om.log2_sigmas()
    print({k: round(v, 2) for k, v in got.items()}, om.h_small, om.h_polys, om.decision_margin())
    for name, want in OPT_LOG2.items():
        assert want - 0.1 < got[name] < want + 0.1, (name, got[name])
    # the f64 transform leads K2 at PARAM_OPT: its term is more than a hundred times the key noise
    transform = om.extprod_transform_term("pbs")
    assert transform / (om.extprod(0) - transform) > 100
    # a five-term sum (MixColumns and the round key), K1 and the modulus switch in front of K2's decision
    assert (om.h_small, om.h_polys) == (338, (263, 246, 248, 259))
    assert 33 < om.decision_margin() < 36
    # a gate's circuit bootstrap decides on `valid`, a 16-bit output: 15 CMUXes' worth of noise per term still leaves 32.7 sigma
    assert 32 < om.decision_margin(5, 16) < 33.5 < om.decision_margin(5, 12) < 34.2


# ---- PARAM_TOY through the oracle, stage by stage -----------------------------------------------------------------------------------------
def _fresh(client, m, seed):
    bits = np.random.default_rng(seed).integers(0, 2, m).astype(np.uint8)
    return bits, client.encrypt_bits(bits)


def _k1_error(kit, x):
    c = kit.client
    _, ph_in = c.decrypt_bits(x, return_phase=True)
    return nm.signed(c.phase_small(kit.oracle.keyswitch(x)) - ph_in)


def test_k1_toy(toy, tm, tc):
    _, x = _fresh(tc, 4096, 0xA1)
    nm.assert_noise(_k1_error(toy, x), tm.k1(), 4096, "K1 toy")


def test_k1_param_opt(opt, om, oc):
    _, x = _fresh(oc, 512, 0xA2)
    nm.assert_noise(_k1_error(opt, x), om.k1(), 512, "K1 opt")


def test_modulus_switch_toy(toy, tm):
    c = toy.client
    rng = np.random.default_rng(0xA3)
    small, _ = nm.small_lwe(c.lwe_sk, rng.integers(0, 2, 2048), 1.0, rng)
    switched = np.array([[orc.mod_switch(int(w)) for w in row] for row in small[:64]], dtype=np.uint64)
    fast = ((small + np.uint64(1 << 53)) >> np.uint64(54)) & np.uint64(1023)
    assert np.array_equal(fast[:64], switched)                                   # the oracle's switch is what the numpy line does
    err = nm.signed(c.phase_small(fast << np.uint64(54)) - c.phase_small(small))
    nm.assert_noise(err, tm.modswitch(), 2048, "modulus switch toy")
    assert abs(err.astype(np.float64).mean()) < 5 * math.sqrt(tm.modswitch() / 2048)   # and it is not biased


def _extprod_error(kit, i, gadget, count, seed):
    """[count][N]: the phase of GGSW_i (x) Lambda minus s_i times the phase of Lambda, Lambda uniform; the cbs gadget (one level) reads
    the first level of the BSK's GGSW, whose rows carry s_i 2^56 instead of s_i 2^49: exact only for s_i = 0, which is what is asked"""
    c, p = kit.client, kit.params
    b, L = (p.pbs_base_log, p.pbs_level) if gadget == "pbs" else (p.cbs_base_log, p.cbs_level)
    s = int(c.lwe_sk[i])
    assert gadget == "pbs" or s == 0
    ggsw = kit.keys.bsk.reshape(p.n, p.pbs_level, (p.k + 1) ** 2 * p.N)[i, :L]
    rng = np.random.default_rng(seed)
    lam = rng.integers(0, 1 << 64, (count, (p.k + 1) * p.N), dtype=np.uint64)
    out = np.stack([orc.external_product_add(p, L, b, ggsw, lam[t], np.zeros_like(lam[t])) for t in range(count)])
    return nm.signed(c.glwe_phase(out) - c.glwe_phase(lam) * np.uint64(s))


@pytest.mark.parametrize("which", ["toy", "opt"])
def test_one_external_product_per_gadget(which, request):
    kit = request.getfixturevalue(which)
    model = request.getfixturevalue("tm" if which == "toy" else "om")
    sk = kit.client.lwe_sk
    zero, one = int(np.flatnonzero(sk == 0)[0]), int(np.flatnonzero(sk == 1)[0])
    count = 128 if which == "toy" else 64
    nm.assert_noise(_extprod_error(kit, zero, "pbs", count, 1), model.extprod(0, "pbs"), count, which + " external product, s_i = 0")
    nm.assert_noise(_extprod_error(kit, one, "pbs", count, 2), model.extprod(1, "pbs"), count, which + " external product, s_i = 1")
    nm.assert_noise(_extprod_error(kit, zero, "cbs", count, 3), model.extprod(0, "cbs"), count, which + " external product, CMUX gadget")


@pytest.mark.parametrize("which", ["toy", "opt"])
def test_transform_error_in_the_phase(which, request):
    """The f64 transform's error where it matters: one external product against the same product computed exactly (schoolbook, digits
    from the plain rule) with real BSK rows, seen through the secret key.  The mask columns' errors are multiplied by the key
    polynomials, so the phase carries about (1 + 7/8 h_big) v_chain (NoiseModel.extprod derives the factor) -- std 2^27.4 at PARAM_TOY and
    2^29.2 at PARAM_OPT per external product, not the 2^21.7 of one coefficient of one product."""
    kit = request.getfixturevalue(which)
    model = request.getfixturevalue("tm" if which == "toy" else "om")
    c, p = kit.client, kit.params
    k1, L, b = p.k + 1, p.pbs_level, p.pbs_base_log
    count = 128 if which == "toy" else 64
    rng = np.random.default_rng(0xF7)
    errs = []
    for t in range(count):
        i = int(rng.integers(0, p.n))
        rows = kit.keys.bsk.reshape(p.n, L, k1, k1, p.N)[i]
        lam = rng.integers(0, 1 << 64, (k1, p.N), dtype=np.uint64)
        got = orc.external_product_add(p, L, b, rows, lam, np.zeros_like(lam)).reshape(k1, p.N)
        d = nm.offset_digits(lam, b, L)                                          # [L][k1][N]
        exact = np.zeros((k1, p.N), dtype=np.uint64)
        with np.errstate(over="ignore"):
            for l in range(L):
                for r in range(k1):
                    for col in range(k1):
                        exact[col] += orc.negacyclic_mul_exact(d[l, r], rows[l, r, col])
        errs.append(nm.signed(c.glwe_phase((got - exact).reshape(-1))))
    nm.assert_noise(np.stack(errs), model.extprod_transform_term("pbs"), count, which + " transform error in the phase")


@pytest.fixture(scope="module")
def k2_toy(toy, tm):
    """512 honest small-key inputs (K1's and the modulus switch's noise from the model) through the oracle's K2"""
    c = toy.client
    rng = np.random.default_rng(0xA4)
    bits = rng.integers(0, 2, 512).astype(np.uint8)
    small, _ = nm.small_lwe(c.lwe_sk, bits, tm.k1() + tm.modswitch(), rng)
    return bits, toy.oracle.cbs_pbs(small)


def test_k2_toy(toy, tm, k2_toy):
    bits, out = k2_toy
    _, ph = toy.client.decrypt_bits(out, return_phase=True)
    err = nm.signed(ph - (bits.astype(np.uint64) << np.uint64(64 - toy.params.cbs_base_log)))
    nm.assert_noise(err, tm.k2(), 512, "K2 toy")


def test_k3_toy(toy, tm, k2_toy):
    bits, out = k2_toy
    m = 256
    e_k0, e_k, e_set, e_clear = nm.k3_errors(toy.client, toy.oracle.pfpks(out[:m]), bits[:m])
    k = toy.params.k
    nm.assert_noise(e_k0, tm.k3(k, 1), m, "K3 toy row k, coefficient 0")
    nm.assert_noise(e_k, tm.k3(k, 0), m, "K3 toy row k, other coefficients")
    nm.assert_noise(e_set, tm.k3(0, 1), m, "K3 toy rows j < k, key bit 1")
    nm.assert_noise(e_clear, tm.k3(0, 0), m, "K3 toy rows j < k, key bit 0")
    # and the row means the CMUX term is built from
    assert abs(tm.k3(0) - (tm.pfks() + tm.h_polys[0] / 512 * tm.k3_carried())) < 1e-6 * tm.k3(0)


SWEEPS = {
    "sbox": (orc.LUTSET_SBOX, [lambda x: aes_clear.SBOX[x]]),
    "inv sbox": (orc.LUTSET_INV_SBOX, [lambda x: aes_clear.INV_SBOX[x]]),
    "many_sbox": (orc.LUTSET_ENC_ROUND, [lambda x, m=m: aes_clear.gf_mul(aes_clear.SBOX[x], m) for m in (1, 2, 3)]),
    "many_sbox inv": (orc.LUTSET_DEC_MUL, [lambda x, m=m: aes_clear.gf_mul(x, m) for m in (9, 11, 13, 14)]),
}


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_wopbs_sweep_toy(toy, tm, tc, name):
    """all 256 byte values through the oracle's LUT sets: the table, and the noise as a function of the input's bits"""
    which, fs = SWEEPS[name]
    x = tc.encrypt_bytes(np.arange(256))
    err, vals = nm.wopbs_error(toy.client, toy.oracle.wopbs_batch(x, orc.build_lutset(which)))
    assert vals.tolist() == [[f(v) for f in fs] for v in range(256)]
    nm.assert_noise(err, tm.wopbs(8, np.arange(256))[:, None, None], tm.wopbs_independent(256, 8), "WoPBS toy, " + name, left_out=tm.wopbs_left_out())


@pytest.mark.parametrize("width", [10, 12])
def test_wide_inputs_toy(toy, tm, tc, width):
    rng = np.random.default_rng(width)
    table = rng.integers(0, 1 << width, 1 << width)
    vals = rng.integers(0, 1 << width, 32)
    vals[:2] = (0, (1 << width) - 1)
    bits = ((vals[:, None] >> np.arange(width)) & 1).astype(np.uint8)
    lut = gen_lut(2, 1, 512, width, lambda v: int(table[v]))
    err, got = nm.wopbs_error(toy.client, toy.oracle.wopbs_batch(tc.encrypt_bits(bits), np.stack([lut])))
    assert got[:, 0].tolist() == table[vals].tolist()
    nm.assert_noise(err, tm.wopbs(width, vals)[:, None, None], 32 * width, "WoPBS toy, %d bits" % width, left_out=tm.wopbs_left_out())


def test_aes_output_toy(toy, tm, tc):
    """one block through the oracle's key expansion and encryption: every output word is a fresh S-Box output plus a round-key word"""
    c, O = tc, toy.oracle
    pt = 0x3243F6A8885A308D313198A2E0370734
    out = O.aes_encrypt(O.aes_key_expansion(c.encrypt_u128(c.key)), c.encrypt_u128(pt))
    want = aes_clear.aes128_encrypt_block(c.key, pt)
    assert c.decrypt_u128(out) == want
    err, _ = nm.wopbs_error(c, out[None])
    nm.assert_noise(err, nm.aes_output_variance(tm, c.key, [want]), 128, "AES output toy", left_out=2 * tm.wopbs_left_out())


def test_tag_difference_toy(toy, tm, tc):
    """X + S0 + trivial(tag) of a tag check through the oracle: two cipher outputs under one key share the last round key's ciphertexts,
    whose error the sum carries twice (noise_model.tag_difference_variance).  Four keys, two blocks each: 512 independent words at
    PARAM_TOY, enough for the band to refuse the two aes_output_variance sums alone, which count that word once each."""
    c, O = tc, toy.oracle
    errs, var, two_sums = [], [], []
    for i in range(4):
        key = bytes(np.random.default_rng(0xCC70 + i).integers(0, 256, 16, dtype=np.uint8).tolist())
        rk = O.aes_key_expansion(c.encrypt_aes_key(key))
        b1, b2 = 0x1111 * (i + 1), 0x0123456789ABCDEF << (8 * i)
        x, s0 = aes_clear.aes_encrypt_block(key, b1), aes_clear.aes_encrypt_block(key, b2)
        diff = O.aes_encrypt(rk, c.encrypt_u128(b1)) + O.aes_encrypt(rk, c.encrypt_u128(b2)) + c.trivial_bytes(list((x ^ s0).to_bytes(16, "big")))
        e, vals = nm.wopbs_error(c, diff[None])
        assert not vals.any()
        v, t = nm.tag_difference_variance(tm, key, x, s0)
        errs.append(e[0]); var.append(v); two_sums.append(t)
    err = np.stack(errs)
    nm.assert_noise(err, np.stack(var), 512, "tag difference toy", left_out=6 * tm.wopbs_left_out())
    with pytest.raises(AssertionError):
        nm.assert_noise(err, np.stack(two_sums), 512, "tag difference toy, the round key counted once per output", left_out=4 * tm.wopbs_left_out())
