"""AES-192 and AES-256 on the MI355X (the five fheaes_aes_*_bits entry points, FIPS-197 with Nk = 6 / 8 and Nr = 12 / 14): word for word
against aes_model.AesModel (the CPU oracle's WoPBS, numpy wrapping sums; pinned to the oracle's own AES-128 in
test_aes_key_sizes_cpu.py), the FIPS-197 appendix C vectors end to end, the 128-bit case against the entry points that have no key-size argument, errors,
the noise guard, several contexts, and 32 resident blocks per key size at PARAM_OPT."""

import numpy as np
import pytest

from aes_model import AesModel, noise
from aes_vectors import A2_KEY, A3_KEY, FIPS_C, FIPS_C_PT, MASK128, NR, block_bytes, key_words
from conftest import sha
from gpu_support import dev, host, oc, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
OPT_KEYS = {192: A2_KEY, 256: A3_KEY}                   # keys of the PARAM_OPT tests: the NIST SP 800-38A ones (F.1.3, F.1.5)


@pytest.fixture(scope="module")
def toy_model(toy):
    return AesModel(toy.oracle)


@pytest.fixture(scope="module")
def toy_cases(toy_model, tc):
    """per key size: (the AES key, its encryption, the model's round keys, the model's decryption round keys)"""
    out = {}
    for bits in (192, 256):
        key = FIPS_C[bits][0]
        ek = tc.encrypt_aes_key(key)
        w = toy_model.key_expansion(ek)
        out[bits] = (key, ek, w, toy_model.dec_round_keys(w))
    return out


# ---- PARAM_TOY, word for word against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [192, 256])
def test_toy_key_expansion_word_exact(toy, toy_server, toy_cases, tc, bits):
    key, ek, w, _ = toy_cases[bits]
    got = toy_server.aes_key_expansion(ek)
    assert got.shape == (NR[bits] + 1, 16, 8, toy.params.big1)
    assert np.array_equal(got, w)
    assert np.array_equal(tc.decrypt_bytes(got), key_words(aes_clear.expand_key(key)))


@pytest.mark.parametrize("bits", [192, 256])
def test_toy_three_blocks_word_exact(toy, toy_server, toy_model, toy_cases, tc, bits):
    key, _, w, dw = toy_cases[bits]
    pts = [IV, 0, MASK128]
    cts = [aes_clear.aes_encrypt_block(key, v) for v in pts]
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    enc = toy_server.aes_encrypt(w, st.copy())
    assert np.array_equal(enc, toy_model.encrypt(w, st))
    assert [tc.decrypt_u128(enc[i]) for i in range(3)] == cts
    dec = toy_server.aes_decrypt(w, enc.copy())
    assert np.array_equal(dec, toy_model.decrypt(w, enc))
    assert [tc.decrypt_u128(dec[i]) for i in range(3)] == pts
    got_dw = toy_server.aes_decryption_round_keys(w)
    assert np.array_equal(got_dw, dw)
    assert np.array_equal(tc.decrypt_bytes(got_dw), key_words(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))))
    eq = toy_server.aes_decrypt_equivalent(dw, enc.copy())
    assert np.array_equal(eq, toy_model.decrypt_equivalent(dw, enc))
    assert [tc.decrypt_u128(eq[i]) for i in range(3)] == pts


@pytest.mark.parametrize("bits", [192, 256])
def test_toy_fips197_appendix_c_through_server(toy, toy_server, tc, bits):
    key, ct = FIPS_C[bits]
    rk = toy_server.aes_key_expansion(tc.encrypt_aes_key(key))
    assert np.array_equal(tc.decrypt_bytes(rk), key_words(aes_clear.expand_key(key)))
    enc = toy_server.aes_encrypt(rk, tc.encrypt_u128(FIPS_C_PT))
    assert tc.decrypt_u128(enc) == ct
    assert tc.decrypt_u128(toy_server.aes_decrypt(rk, enc.copy())) == FIPS_C_PT
    dw = toy_server.aes_decryption_round_keys(rk)
    assert tc.decrypt_u128(toy_server.aes_decrypt_equivalent(dw, enc.copy())) == FIPS_C_PT
    assert tc.decrypt_u128(toy_server.aes_decryption(rk, enc.copy())) == FIPS_C_PT        # the README spelling forwards the same way


@pytest.mark.parametrize("bits", [192, 256])
def test_toy_host_arrays_and_resident_tensors_agree(toy, toy_server, toy_cases, tc, bits):
    _, ek, _, _ = toy_cases[bits]
    st = np.stack([tc.encrypt_u128(IV + i) for i in range(2)])
    rk = toy_server.aes_key_expansion(ek)
    enc = toy_server.aes_encrypt(rk, st.copy())
    dec = toy_server.aes_decrypt(rk, enc.copy())
    dw = toy_server.aes_decryption_round_keys(rk)
    eq = toy_server.aes_decrypt_equivalent(dw, enc.copy())
    d_ek = dev(ek)                                                   # kept alive: the device calls are only enqueued
    d_rk = toy_server.aes_key_expansion(d_ek)
    d_enc = dev(st)
    toy_server.aes_encrypt(d_rk, d_enc)
    toy_server.synchronize()
    d_dec = dev(host(d_enc))
    toy_server.aes_decrypt(d_rk, d_dec)
    d_dw = toy_server.aes_decryption_round_keys(d_rk)
    d_eq = dev(host(d_enc))
    toy_server.aes_decrypt_equivalent(d_dw, d_eq)
    toy_server.synchronize()
    assert tuple(d_rk.shape) == rk.shape and tuple(d_dw.shape) == dw.shape
    assert np.array_equal(host(d_rk), rk)
    assert np.array_equal(host(d_enc), enc)
    assert np.array_equal(host(d_dec), dec)
    assert np.array_equal(host(d_dw), dw)
    assert np.array_equal(host(d_eq), eq)
    with pytest.raises(ValueError):
        toy_server.aes_encrypt(rk, d_eq)                             # mixed memory spaces are refused


# ---- key_bits = 128: the same words as the entry points without the argument ------------------------------------------------------------
def test_bits_entry_points_at_128_give_the_words_of_the_old_ones(toy, tc):
    eng = toy.engine()
    shape = (11, 16, 8, toy.params.big1)
    ek = tc.encrypt_u128(tc.key)
    rk_old, rk_new = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
    eng.aes_key_expansion(ek, rk_old)
    eng.aes_key_expansion_bits(ek, 128, rk_new)
    assert np.array_equal(rk_new, rk_old)
    assert np.array_equal(tc.decrypt_bytes(rk_old), key_words(aes_clear.expand_key(tc.key)))
    st = np.stack([tc.encrypt_u128(IV + i) for i in range(2)])
    enc_old, enc_new = st.copy(), st.copy()
    eng.aes_encrypt(rk_old, enc_old, 2)
    eng.aes_encrypt_bits(rk_old, 128, enc_new, 2)
    assert np.array_equal(enc_new, enc_old)
    dec_old, dec_new = enc_old.copy(), enc_old.copy()
    eng.aes_decrypt(rk_old, dec_old, 2)
    eng.aes_decrypt_bits(rk_old, 128, dec_new, 2)
    assert np.array_equal(dec_new, dec_old)
    dw_old, dw_new = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
    eng.aes_decryption_round_keys(rk_old, dw_old)
    eng.aes_decryption_round_keys_bits(rk_old, 128, dw_new)
    assert np.array_equal(dw_new, dw_old)
    eq_old, eq_new = enc_old.copy(), enc_old.copy()
    eng.aes_decrypt_equivalent(dw_old, eq_old, 2)
    eng.aes_decrypt_equivalent_bits(dw_old, 128, eq_new, 2)
    assert np.array_equal(eq_new, eq_old)
    assert [tc.decrypt_u128(eq_old[i]) for i in range(2)] == [IV, IV + 1]
    # ... and on resident tensors
    d_rk, d_a, d_b = dev(rk_old), dev(st), dev(st)
    eng.aes_encrypt(d_rk, d_a, 2)
    eng.aes_encrypt_bits(d_rk, 128, d_b, 2)
    eng.synchronize()
    assert np.array_equal(host(d_a), enc_old) and np.array_equal(host(d_b), enc_old)


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
def test_errors_key_bits_missing_keys_overlap_and_shapes(toy, toy_server, toy_cases, tc):
    p = toy.params
    _, ek, w, dw = toy_cases[256]
    st = tc.encrypt_u128(0)
    out = np.empty_like(w)
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    for ms in (_native.HOST, _native.DEVICE):
        for rc in (lib.fheaes_aes_key_expansion_bits(h, ek.ctypes.data, 100, out.ctypes.data, ms),
                   lib.fheaes_aes_encrypt_bits(h, w.ctypes.data, 100, st.ctypes.data, 1, ms),
                   lib.fheaes_aes_decrypt_bits(h, w.ctypes.data, 100, st.ctypes.data, 1, ms),
                   lib.fheaes_aes_decryption_round_keys_bits(h, w.ctypes.data, 100, out.ctypes.data, ms),
                   lib.fheaes_aes_decrypt_equivalent_bits(h, dw.ctypes.data, 100, st.ctypes.data, 1, ms)):
            assert rc == -1
            assert b"key_bits" in lib.fheaes_last_error(h)
        assert lib.fheaes_aes_key_expansion_bits(h, None, 256, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_key_expansion_bits(h, ek.ctypes.data, 256, None, ms) == -1
        assert lib.fheaes_aes_encrypt_bits(h, None, 256, st.ctypes.data, 1, ms) == -1
        assert lib.fheaes_aes_decrypt_bits(h, w.ctypes.data, 256, None, 1, ms) == -1
        assert lib.fheaes_aes_decryption_round_keys_bits(h, w.ctypes.data, 256, None, ms) == -1
        assert lib.fheaes_aes_decrypt_equivalent_bits(h, None, 256, st.ctypes.data, 1, ms) == -1
    with pytest.raises(_native.FheAesError) as e:
        eng.aes_encrypt_bits(w, 100, st.copy(), 1)
    assert e.value.code == -1 and "key_bits" in str(e.value)
    # a context without keys
    fresh = _native.Engine(p, device=0)
    try:
        for call in (lambda: fresh.aes_key_expansion_bits(ek, 256, np.empty_like(w)),
                     lambda: fresh.aes_encrypt_bits(w, 256, st.copy(), 1),
                     lambda: fresh.aes_decrypt_bits(w, 256, st.copy(), 1),
                     lambda: fresh.aes_decryption_round_keys_bits(w, 256, np.empty_like(w)),
                     lambda: fresh.aes_decrypt_equivalent_bits(dw, 256, st.copy(), 1)):
            with pytest.raises(_native.FheAesError) as e:
                call()
            assert e.value.code == -2                                # FHEAES_ERR_NOKEYS
    finally:
        fresh.close()
    # the conversion is not in place: identical buffers, and buffers that overlap only when all 15 round keys are counted
    rkw = 16 * 8 * p.big1                                            # words of one round key
    both = np.zeros(27 * rkw, dtype=np.uint64)
    both[:15 * rkw] = w.reshape(-1)
    a = both.ctypes.data
    assert lib.fheaes_aes_decryption_round_keys_bits(h, a, 256, a, _native.HOST) == -1
    assert b"overlap" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_decryption_round_keys_bits(h, a, 256, a + 12 * rkw * 8, _native.HOST) == -1
    assert b"overlap" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_decryption_round_keys_bits(h, a + 12 * rkw * 8, 256, a, _native.HOST) == -1
    d_w = dev(w)
    assert lib.fheaes_aes_decryption_round_keys_bits(h, d_w.data_ptr(), 256, d_w.data_ptr(), _native.DEVICE) == -1
    assert np.array_equal(both[:15 * rkw], w.reshape(-1))            # nothing was written
    # shapes that are no AES key size never reach the library
    bad = np.zeros((12, 16, 8, p.big1), dtype=np.uint64)
    for call in (lambda: toy_server.aes_encrypt(bad, st.copy()), lambda: toy_server.aes_decrypt(bad, st.copy()),
                 lambda: toy_server.aes_decryption_round_keys(bad), lambda: toy_server.aes_decrypt_equivalent(bad, st.copy()),
                 lambda: toy_server.aes_key_expansion(np.zeros((20, 8, p.big1), dtype=np.uint64)),
                 lambda: toy_server.aes_encrypt(w.reshape(15 * 16, 8, p.big1), st.copy())):
        with pytest.raises(ValueError):
            call()


def test_noise_guard_of_the_256_bit_schedules(toy, toy_cases, tc):
    """a fresh context: every sum of the key expansion has two nominal terms; a round sums 4 WoPBS outputs + 1 round key = 5, the limit"""
    _, ek, _, _ = toy_cases[256]
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        rk = srv.aes_key_expansion(ek)
        assert srv.engine.noise_level_seen() == (2, 5)
        srv.aes_encrypt(rk, tc.encrypt_u128(1))
        assert srv.engine.noise_level_seen() == (5, 5)
    finally:
        srv.engine.close()
    srv = Server(toy.keys, device=0)
    try:
        dw = srv.aes_decryption_round_keys(rk)
        assert srv.engine.noise_level_seen() == (4, 5)
        srv.aes_decrypt_equivalent(dw, tc.encrypt_u128(1))
        assert srv.engine.noise_level_seen() == (5, 5)
    finally:
        srv.engine.close()


def test_toy_server_group_matches_one_context_at_256_bits(toy, toy_server, toy_cases, tc):
    key, ek, w, _ = toy_cases[256]
    pts = [IV + i for i in range(4)]
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    want_enc = toy_server.aes_encrypt(w, st.copy())
    dw = toy_server.aes_decryption_round_keys(w)
    want_eq = toy_server.aes_decrypt_equivalent(dw, want_enc.copy())
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        assert np.array_equal(group.aes_key_expansion(ek), w)
        enc = group.aes_encrypt(w, st.copy())
        assert np.array_equal(enc, want_enc)
        dw_g = group.aes_decryption_round_keys(w)
        assert np.array_equal(dw_g, dw)
        eq = group.aes_decrypt_equivalent(dw_g, enc.copy())
        assert np.array_equal(eq, want_eq)
        assert np.array_equal(group.aes_decrypt(w, enc.copy()), toy_server.aes_decrypt(w, enc.copy()))
        assert [tc.decrypt_u128(enc[i]) for i in range(4)] == [aes_clear.aes_encrypt_block(key, v) for v in pts]
        assert [tc.decrypt_u128(eq[i]) for i in range(4)] == pts
    finally:
        for s in group.servers:
            s.engine.close()


# ---- PARAM_OPT ---------------------------------------------------------------------------------------------------------------------------
def test_param_opt_aes256_key_expansion_and_one_block_word_exact(opt, opt_server, oc):
    """at the reference's parameter set against the model: 65 four-byte and 14 sixteen-byte WoPBS calls on the oracle (484 byte WoPBS)"""
    key, pt = OPT_KEYS[256], 0x3243F6A8885A308D313198A2E0370734
    ek = oc.encrypt_aes_key(key)
    model = AesModel(opt.oracle)
    w = opt_server.aes_key_expansion(ek)
    assert np.array_equal(w, model.key_expansion(ek))
    assert np.array_equal(oc.decrypt_bytes(w), key_words(aes_clear.expand_key(key)))
    st = oc.encrypt_u128(pt)
    got = opt_server.aes_encrypt(w, st.copy())
    assert np.array_equal(got, model.encrypt(w, st))
    assert oc.decrypt_u128(got) == aes_clear.aes_encrypt_block(key, pt)


@pytest.mark.parametrize("bits", [192, 256])
def test_param_opt_32_blocks_on_device(opt, opt_server, oc, bits):
    """32 blocks on resident tensors: aes_encrypt, then aes_decrypt_equivalent on its output, and 4 of the blocks through aes_decrypt.
    Every block decrypts to the FIPS-197 ciphertext, then to its plaintext; the outputs carry the noise of one fresh WoPBS output plus
    one round key (the last round does not depend on Nr: the bounds of test_gpu_aes_eqinv.py); a second launch gives the same words."""
    c, key, n = oc, OPT_KEYS[bits], 32
    d_ek = dev(c.encrypt_aes_key(key))
    d_rk = opt_server.aes_key_expansion(d_ek)
    d_dw = opt_server.aes_decryption_round_keys(d_rk)
    pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
    cts = [aes_clear.aes_encrypt_block(key, v) for v in pts]
    states = np.stack([c.encrypt_u128(v) for v in pts])
    d_enc = dev(states)
    opt_server.aes_encrypt(d_rk, d_enc)
    opt_server.synchronize()
    assert tuple(d_rk.shape) == (NR[bits] + 1, 16, 8, opt.params.big1)
    assert np.array_equal(c.decrypt_bytes(host(d_rk)), key_words(aes_clear.expand_key(key)))
    enc = host(d_enc)
    got = c.decrypt_bytes(enc)
    want = block_bytes(cts)
    wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not wrong, "blocks wrong after aes_encrypt: %s" % wrong
    d_eq, d_ref = dev(enc), dev(enc[:4])
    opt_server.aes_decrypt_equivalent(d_dw, d_eq)
    opt_server.aes_decrypt(d_rk, d_ref)
    opt_server.synchronize()
    eq, ref = host(d_eq), host(d_ref)
    got = c.decrypt_bytes(eq)
    want = block_bytes(pts)
    wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not wrong, "blocks wrong after aes_decrypt_equivalent: %s" % wrong
    assert np.array_equal(c.decrypt_bytes(ref), want[:4])
    for name, words in (("aes_encrypt", enc), ("aes_decrypt_equivalent", eq), ("aes_decrypt", ref)):
        err = np.abs(noise(c, words))
        print("AES-%d %s: max |noise| = 2^%.2f, std = 2^%.2f" % (bits, name, np.log2(float(err.max())), np.log2(float(err.std()))))
        assert err.max() < 1 << 59, "%s: max |noise| = 2^%.1f" % (name, np.log2(float(err.max())))
        assert err.std() < 1 << 56, "%s: std = 2^%.1f" % (name, np.log2(float(err.std())))
    # determinism: a second launch from the same inputs
    d_enc2, d_eq2 = dev(states), dev(enc)
    opt_server.aes_encrypt(d_rk, d_enc2)
    opt_server.aes_decrypt_equivalent(d_dw, d_eq2)
    opt_server.synchronize()
    assert sha(host(d_enc2)) == sha(enc)
    assert sha(host(d_eq2)) == sha(eq)
