"""The equivalent inverse cipher on the MI355X (fheaes_aes_decryption_round_keys + fheaes_aes_decrypt_equivalent, FIPS-197 section
5.3.5): word for word against aes_model.AesModel (the CPU oracle's WoPBS with composed LUTs, numpy wrapping sums),
decrypting to the plaintext at the toy set and at PARAM_OPT, within the noise guard, with the host / device / multi-context paths agreeing."""

import numpy as np
import pytest

from aes_model import AesModel, noise
from aes_vectors import FIPS_C1_CT, FIPS_C1_KEY, FIPS_C1_PT
from conftest import sha
from gpu_support import dev, host, oc, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF


@pytest.fixture(scope="module")
def toy_case(toy, tc):
    """(round keys of the kit's AES key from the oracle, the model, the model's decryption round keys)"""
    w = toy.oracle.aes_key_expansion(tc.encrypt_u128(tc.key))
    model = AesModel(toy.oracle)
    return w, model, model.dec_round_keys(w)


def test_toy_decryption_round_keys_word_exact(toy, toy_server, toy_case, tc):
    w, _, dw_want = toy_case
    dw = toy_server.aes_decryption_round_keys(w)
    assert np.array_equal(dw, dw_want)
    assert np.array_equal(tc.decrypt_bytes(dw),
                          np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(tc.key)), dtype=np.uint8))


def test_toy_three_blocks_word_exact(toy, toy_server, toy_case, tc):
    c, key = tc, tc.key
    _, model, dw = toy_case
    pts = [IV, 0, (1 << 128) - 1]
    st = np.stack([c.encrypt_u128(aes_clear.aes128_encrypt_block(key, v)) for v in pts])
    got = toy_server.aes_decrypt_equivalent(dw, st.copy())
    assert np.array_equal(got, model.decrypt_equivalent(dw, st))
    assert [c.decrypt_u128(got[i]) for i in range(3)] == pts


def test_toy_host_and_device_memspace_agree(toy, toy_server, toy_case, tc):
    c = tc
    w, _, _ = toy_case
    st = np.stack([c.encrypt_u128(aes_clear.aes128_encrypt_block(c.key, IV + i)) for i in range(2)])
    dw = toy_server.aes_decryption_round_keys(w)
    want = toy_server.aes_decrypt_equivalent(dw, st.copy())
    d_w = dev(w)                                                     # kept alive: the device calls are only enqueued
    d_dw = toy_server.aes_decryption_round_keys(d_w)
    d_st = dev(st)
    toy_server.aes_decrypt_equivalent(d_dw, d_st)
    toy_server.synchronize()
    assert np.array_equal(host(d_dw), dw)
    assert np.array_equal(host(d_st), want)
    with pytest.raises(ValueError):
        toy_server.aes_decrypt_equivalent(dw, d_st)                  # mixed memory spaces are refused


def test_toy_fips197_c1_known_answer(toy, toy_server, tc):
    c = tc
    rk = toy_server.aes_key_expansion(c.encrypt_u128(FIPS_C1_KEY))
    dw = toy_server.aes_decryption_round_keys(rk)
    assert np.array_equal(c.decrypt_bytes(dw), np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(FIPS_C1_KEY)), dtype=np.uint8))
    assert c.decrypt_u128(toy_server.aes_decrypt_equivalent(dw, c.encrypt_u128(FIPS_C1_CT))) == FIPS_C1_PT


def test_noise_guard_of_the_conversion_and_the_rounds(toy, toy_case, tc):
    """a fresh context: the key conversion sums 4 WoPBS outputs (InvMixColumns, no key) and refreshes them; a round of the equivalent
    inverse cipher then sums 4 WoPBS outputs + 1 refreshed key = 5, the limit (MaxNoiseLevel::new(5), client.rs:92)"""
    w, _, _ = toy_case
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        dw = srv.aes_decryption_round_keys(w)
        assert srv.engine.noise_level_seen() == (4, 5)
        srv.aes_decrypt_equivalent(dw, tc.encrypt_u128(1))
        assert srv.engine.noise_level_seen() == (5, 5)
    finally:
        srv.engine.close()


def test_errors_before_keys_null_pointers_and_in_place_conversion(toy, toy_case, tc):
    w, _, _ = toy_case
    p = toy.params
    fresh = _native.Engine(p, device=0)
    try:
        for call in (lambda: fresh.aes_decryption_round_keys(w, np.empty_like(w)),
                     lambda: fresh.aes_decrypt_equivalent(w, tc.encrypt_u128(0), 1)):
            with pytest.raises(_native.FheAesError) as e:
                call()
            assert e.value.code == -2                                # FHEAES_ERR_NOKEYS
    finally:
        fresh.close()
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    wp = w.ctypes.data
    out = np.empty_like(w)
    st = tc.encrypt_u128(0)
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_aes_decryption_round_keys(h, None, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_decryption_round_keys(h, wp, None, ms) == -1
        assert lib.fheaes_aes_decrypt_equivalent(h, None, st.ctypes.data, 1, ms) == -1
        assert lib.fheaes_aes_decrypt_equivalent(h, wp, None, 1, ms) == -1
    assert lib.fheaes_aes_decryption_round_keys(h, wp, wp, _native.HOST) == -1               # identical buffers: not in place
    assert b"overlap" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_decryption_round_keys(h, wp, wp + 8 * 16 * 8 * p.big1, _native.HOST) == -1     # overlapping ones
    d_w = dev(w)
    assert lib.fheaes_aes_decryption_round_keys(h, d_w.data_ptr(), d_w.data_ptr(), _native.DEVICE) == -1
    with pytest.raises(_native.FheAesError) as e:
        eng.aes_decryption_round_keys(w, w)
    assert e.value.code == -1


def test_toy_server_group_matches_one_context(toy, toy_server, toy_case, tc):
    c = tc
    w, _, _ = toy_case
    st = np.stack([c.encrypt_u128(aes_clear.aes128_encrypt_block(c.key, IV + i)) for i in range(4)])
    dw = toy_server.aes_decryption_round_keys(w)
    want = toy_server.aes_decrypt_equivalent(dw, st.copy())
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        dw_g = group.aes_decryption_round_keys(w)
        assert np.array_equal(dw_g, dw)
        got = group.aes_decrypt_equivalent(dw_g, st.copy())
        assert np.array_equal(got, want)
        assert [c.decrypt_u128(got[i]) for i in range(4)] == [IV + i for i in range(4)]
    finally:
        for s in group.servers:
            s.engine.close()


def test_param_opt_one_block_word_exact(opt, opt_server, oc):
    """key conversion + one block at the reference's parameter set against the model (~450 byte WoPBS on the oracle)"""
    c = oc
    key, pt = c.key, 0x3243F6A8885A308D313198A2E0370734
    w = opt_server.aes_key_expansion(c.encrypt_u128(key))
    model = AesModel(opt.oracle)
    dw = opt_server.aes_decryption_round_keys(w)
    assert np.array_equal(dw, model.dec_round_keys(w))
    st = c.encrypt_u128(aes_clear.aes128_encrypt_block(key, pt))
    got = opt_server.aes_decrypt_equivalent(dw, st.copy())
    assert np.array_equal(got, model.decrypt_equivalent(dw, st))
    assert c.decrypt_u128(got) == pt


def test_param_opt_32_block_shard_on_device(opt, opt_server, oc):
    """BASELINE configs[4] shard size: 32 blocks on resident tensors through both decryptions -- every block decrypts to its plaintext,
    the equivalent inverse cipher's outputs and round keys stay within the noise of one fresh WoPBS output, and a second launch gives
    the same words"""
    c = oc
    key = c.key
    n = 32
    d_rk = dev(opt_server.aes_key_expansion(c.encrypt_u128(key)))
    d_dw = opt_server.aes_decryption_round_keys(d_rk)
    pts = [(IV + 0x9E3779B97F4A7C15 * i) & ((1 << 128) - 1) for i in range(n)]
    states = np.stack([c.encrypt_u128(aes_clear.aes128_encrypt_block(key, v)) for v in pts])
    d_ref, d_eq = dev(states), dev(states)
    opt_server.aes_decrypt(d_rk, d_ref)
    opt_server.aes_decrypt_equivalent(d_dw, d_eq)
    opt_server.synchronize()
    ref, eq = host(d_ref), host(d_eq)
    got_ref, got_eq = c.decrypt_bytes(ref), c.decrypt_bytes(eq)
    want = np.array([[(v >> (8 * (15 - b))) & 0xFF for b in range(16)] for v in pts], dtype=np.uint8)
    wrong = [i for i in range(n) if not np.array_equal(got_eq[i], want[i])]
    assert not wrong, "blocks wrong after aes_decrypt_equivalent: %s" % wrong
    assert np.array_equal(got_eq, got_ref)
    # output noise: one fresh WoPBS output + one round key, as test_128_ctr_blocks_param_opt bounds it
    err = noise(c, eq)
    assert np.abs(err).max() < 1 << 59, "max |noise| = 2^%.1f" % np.log2(float(np.abs(err).max()))
    assert np.abs(err).std() < 1 << 56
    # dw[1..9] went through an identity WoPBS: the noise of one fresh WoPBS output, like the refreshed words of the key
    # expansion (server.rs:150); summed and not refreshed they would carry four (twice the standard deviation)
    dw, rk = host(d_dw), host(d_rk)
    assert np.array_equal(dw[0], rk[0]) and np.array_equal(dw[10], rk[10])
    e_dw, e_rk = noise(c, dw[1:10]), noise(c, rk[1:11])
    assert np.abs(e_dw).max() < 1 << 59
    ratio = float(np.abs(e_dw).std()) / float(np.abs(e_rk).std())
    assert 0.7 < ratio < 1.4, "noise std of dw[1..9] / fresh round keys = %.2f" % ratio
    # determinism: a second launch from the same input
    d_eq2 = dev(states)
    opt_server.aes_decrypt_equivalent(d_dw, d_eq2)
    opt_server.synchronize()
    assert sha(host(d_eq2)) == sha(eq)
