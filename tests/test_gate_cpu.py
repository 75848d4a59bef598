"""The gate without a GPU: the numpy model of its two ends (tests/gate_model.py: embed, extract), the whole composition at PARAM_TOY
through the oracle -- circuit bootstrap of an encrypted 0 and an encrypted 1, one external product -- held to the variance the model
derives, the launch plan, and the refusals that need no device."""
import ctypes
import math

import numpy as np
import pytest

import gate_model as gm
import noise_model as nm
from aes_model import ref_unpack
from gpu_support import tc  # noqa: F401
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native


@pytest.fixture(scope="module")
def tm(toy):
    return nm.NoiseModel.of_client(toy.client)


@pytest.fixture(scope="module")
def om(opt):
    return nm.NoiseModel.of_client(opt.client)


# ---- the reference model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [PARAM_TOY, PARAM_OPT], ids=lambda p: p.name)
def test_embed_is_the_inverse_of_the_extraction_at_coefficient_0(p):
    rng = np.random.default_rng(0x6A7E)
    x = rng.integers(0, 1 << 64, (5, p.big1), dtype=np.uint64)
    x[1] = 0
    x[2] = (1 << 64) - 1
    x[3] = 1 << 63
    g = gm.embed(x, p.k, p.N)
    assert g.shape == (5, p.k + 1, p.N)
    assert np.array_equal(gm.extract(g), x)
    # the index rule Server.unpack documents, at i = 0: body glwe[kN], mask word pN + c = glwe[pN + (-c mod N)], negated when c > 0
    for r in range(5):
        assert np.array_equal(ref_unpack(g[r].reshape(1, -1), 1, p)[0], x[r])
    # the body polynomial is the body at coefficient 0 and nothing else; a mask polynomial is its words reversed and negated
    assert np.array_equal(g[:, p.k, 0], x[:, p.big]) and not g[:, p.k, 1:].any()
    assert np.array_equal(g[0, 0, 0], x[0, 0]) and int(g[0, 0, 1]) == (-int(x[0, p.N - 1])) % (1 << 64)
    assert int(g[0, p.k - 1, p.N - 1]) == (-int(x[0, (p.k - 1) * p.N + 1])) % (1 << 64)
    # extract of any GLWE is unpack at i = 0, and embed(extract(g)) keeps the mask polynomials
    glwe = rng.integers(0, 1 << 64, (2, p.k + 1, p.N), dtype=np.uint64)
    assert np.array_equal(gm.extract(glwe), ref_unpack(glwe.reshape(2, -1), p.N + 1, p)[[0, p.N]])
    assert np.array_equal(gm.embed(gm.extract(glwe), p.k, p.N)[:, :p.k], glwe[:, :p.k])


# ---- end to end at PARAM_TOY through the oracle -------------------------------------------------------------------------------------------
GATES_PER_VALUE, BITS_PER_GATE = 64, 4


def test_gate_through_the_oracle_decrypts_to_valid_times_bit_within_the_derived_variance(toy, tm, tc):  # noqa: F811
    p = toy.params
    valid = np.array([0, 1] * GATES_PER_VALUE, dtype=np.uint8)
    ggsw = toy.oracle.circuit_bootstrap(toy.oracle.keyswitch(tc.encrypt_bits(valid)))           # [gates][1][k+1][(k+1)N]
    bits = np.tile(np.array([0, 1, 1, 0], dtype=np.uint8), (valid.size, 1))                       # all four combinations, twice per gate
    ct = tc.encrypt_bits(bits)                                                                    # [gates][4][kN+1]
    out = np.stack([gm.gate_reference(p, ggsw[g], ct[g], 0) for g in range(valid.size)])
    got, ph_out = tc.decrypt_bits(out, return_phase=True)
    assert np.array_equal(got, bits * valid[:, None])
    _, ph_in = tc.decrypt_bits(ct, return_phase=True)
    err = nm.signed(ph_out - ph_in * valid[:, None].astype(np.uint64))                            # against valid * phase(in): what the gate adds
    for v in (0, 1):
        digits, rounding, transform = gm.gate_terms(tm, v)
        assert (rounding == 0) == (v == 0) and transform < 1e-6 * (digits + rounding)
        n = gm.gate_independent(tm, v, GATES_PER_VALUE, BITS_PER_GATE)
        assert nm.rejects_doubling(n)
        nm.assert_noise(err[valid == v], gm.gate_variance(tm, v), n, "gate of %d through the oracle, toy" % v)
    # the GLWE form: N bits per product; every coefficient of the phase is held to the GLWE form's variance
    # (one GLWE per gate: the coefficients of a GLWE share its mask, so the GLWEs are what counts as independent)
    glwe = np.random.default_rng(0x61).integers(0, 1 << 64, (valid.size, (p.k + 1) * p.N), dtype=np.uint64)
    prod = np.stack([gm.gate_reference(p, ggsw[g], glwe[g:g + 1], 1)[0] for g in range(valid.size)])
    e = nm.signed(tc.glwe_phase(prod) - tc.glwe_phase(glwe) * valid[:, None].astype(np.uint64))
    for v in (0, 1):
        nm.assert_noise(e[valid == v], gm.gate_variance(tm, v, lwe_form=False), GATES_PER_VALUE, "gate of %d on GLWEs through the oracle, toy" % v)


def test_a_gate_is_one_cmux_iteration_and_keeps_the_level(tm, om):
    """what backs "a gated ciphertext keeps the level of its input" (include/fheaes.h): the GLWE form's variance IS
    NoiseModel.cmux term for term, the LWE form's is below it, and a WoPBS output carries seven such iterations"""
    for m in (tm, om):
        for v in (0, 1):
            assert math.isclose(gm.gate_variance(m, v, lwe_form=False), m.cmux(v), rel_tol=1e-12)
            assert gm.gate_variance(m, v, lwe_form=True) <= m.cmux(v)
        r = gm.level_ratio(m)
        print(m.p.name, {k: round(x, 4) for k, x in r.items()}, {"gate1": round(0.5 * math.log2(gm.gate_variance(m, 1)), 2),
                                                                "gate0": round(0.5 * math.log2(gm.gate_variance(m, 0)), 2)})
        assert r["gate / cmux(1)"] <= 1.0 and r["gate / wopbs"] <= 2.0 / 7.0 + 1e-9
    # closed values (log2 sigma), so that a change of the model shows in review
    for m, g1, g0 in ((tm, 51.23, 48.05), (om, 52.66, 52.11)):
        assert abs(0.5 * math.log2(gm.gate_variance(m, 1)) - g1) < 0.1 and abs(0.5 * math.log2(gm.gate_variance(m, 0)) - g0) < 0.1


# ---- the launch plan and the refusals that need no device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,R", [(4, 3), (1, 8)])
def test_gate_plan(k, R):
    plan = lambda runs: _native.gate_plan(runs, k)
    assert plan([1]) == {"workgroups": 1, "instances_per_workgroup": R}
    assert plan([R])["workgroups"] == 1
    assert plan([R + 1])["workgroups"] == 2
    assert plan([0, 2 * R - 1, 1])["workgroups"] == 3                     # a gate of 0 has no workgroup; workgroups never mix gates
    assert plan([])["workgroups"] == 0 and plan([0, 0])["workgroups"] == 0
    assert plan([16384 // 64] * 64)["workgroups"] == 64 * -(-256 // R)    # 64 messages of 32 bytes
    with pytest.raises(_native.FheAesError):
        _native.gate_plan([1], 2)
    lib = _native.load_library()
    w, per = ctypes.c_uint64(), ctypes.c_uint32()
    assert lib.fheaes_gate_plan(None, 1, k, ctypes.byref(w), ctypes.byref(per)) == -1
    assert lib.fheaes_gate_plan(None, 0, k, None, ctypes.byref(per)) == -1


def test_gate_calls_reject_a_null_context():
    lib = _native.load_library()
    runs = (ctypes.c_uint64 * 1)(1)
    buf = np.zeros(8, dtype=np.uint64)
    ptr = buf.ctypes.data
    assert lib.fheaes_gate_ggsw(None, ptr, 1, runs, ptr, 1, 0, ptr, _native.HOST) == -1
    assert lib.fheaes_gate_bits(None, ptr, 1, runs, ptr, 1, ptr, _native.HOST) == -1
    assert lib.fheaes_gate_packed(None, ptr, 1, runs, ptr, 1, ptr, _native.HOST) == -1
    assert lib.fheaes_gate_ggsw(None, None, 0, None, None, 0, 0, None, _native.HOST) == -1
