"""AES-192 and AES-256 (FIPS-197 with Nk = 6 / 8 key words, Nr = 12 / 14 rounds) without a GPU: the clear-domain cipher against the
vectors of FIPS-197 appendices A and C and of SP 800-38A (aes_vectors.py), the five `_bits` entry points of the library, and the
word-exact model the GPU tests compare against (aes_model.AesModel): at 128 bits it has to reproduce the oracle's own key expansion,
encryption and decryption word for word, which pins its conventions before it is trusted for the other two key sizes."""
import ctypes

import numpy as np
import pytest

from aes_model import AesModel
from aes_vectors import A2_KEY, A3_KEY, FIPS_C, FIPS_C_PT, NR, SP800_PT, key_words, own_client
from tfhe_aes_amd import _native, aes_clear

BITS_FUNCS = ("fheaes_aes_key_expansion_bits", "fheaes_aes_encrypt_bits", "fheaes_aes_decrypt_bits",
              "fheaes_aes_decryption_round_keys_bits", "fheaes_aes_decrypt_equivalent_bits")


# ---- 1. aes_clear against FIPS-197 and SP 800-38A -----------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_clear_fips197_appendix_c(bits):
    key, ct = FIPS_C[bits]
    w = aes_clear.expand_key(key)
    assert len(w) == NR[bits] + 1 and all(len(r) == 16 for r in w)
    assert aes_clear.aes_encrypt_block(key, FIPS_C_PT) == ct
    assert aes_clear.aes_decrypt_block(key, ct) == FIPS_C_PT
    dw = aes_clear.inv_mix_columns_round_keys(w)
    assert len(dw) == len(w) and dw[0] == w[0] and dw[-1] == w[-1]
    assert aes_clear.aes_decrypt_block_equivalent(dw, ct) == FIPS_C_PT


def test_clear_key_expansion_fips197_appendix_a():
    w = aes_clear.expand_key(A2_KEY)
    assert len(w) == 13 and bytes(w[0] + w[1][:8]) == A2_KEY
    assert bytes(w[12][12:]).hex() == "01002202"                    # w[51]
    w = aes_clear.expand_key(A3_KEY)
    assert len(w) == 15 and bytes(w[0] + w[1]) == A3_KEY
    assert bytes(w[14][12:]).hex() == "706c631e"                    # w[59]


def test_clear_sp800_38a_ecb_first_blocks():
    assert aes_clear.aes_encrypt_block(A2_KEY, SP800_PT) == 0xBD334F1D6E45F25FF712A214571FA5CC
    assert aes_clear.aes_encrypt_block(A3_KEY, SP800_PT) == 0xF3EED1BDB5D2A03C064B5A7E3DB181F8


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_clear_both_decryptions_invert_encryption(bits):
    rng = np.random.default_rng(0xAE5 + bits)
    for _ in range(20):
        key, pt = rng.bytes(bits // 8), int.from_bytes(rng.bytes(16), "big")
        ct = aes_clear.aes_encrypt_block(key, pt)
        assert ct != pt
        assert aes_clear.aes_decrypt_block(key, ct) == pt
        assert aes_clear.aes_decrypt_block_equivalent(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key)), ct) == pt
        if bits == 128:                                             # the int-key functions other files use: same cipher
            k = int.from_bytes(key, "big")
            assert aes_clear.expand_key(k) == aes_clear.expand_key(key)
            assert aes_clear.aes128_encrypt_block(k, pt) == ct
            assert aes_clear.aes128_decrypt_block(k, ct) == pt


def test_clear_refuses_other_key_lengths():
    for n in (0, 15, 20, 33):
        with pytest.raises(ValueError):
            aes_clear.expand_key(bytes(n))


# ---- 2. the library ------------------------------------------------------------------------------------------------------------
def test_library_exports_the_key_size_entry_points():
    lib = _native.load_library()
    for name in BITS_FUNCS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


def test_key_size_entry_points_reject_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        for bits in (128, 192, 256, 100):
            assert lib.fheaes_aes_key_expansion_bits(None, buf, bits, buf, ms) == -1
            assert lib.fheaes_aes_key_expansion_bits(None, None, bits, None, ms) == -1
            assert lib.fheaes_aes_decryption_round_keys_bits(None, buf, bits, buf, ms) == -1
            assert lib.fheaes_aes_decryption_round_keys_bits(None, None, bits, None, ms) == -1
            for fn in (lib.fheaes_aes_encrypt_bits, lib.fheaes_aes_decrypt_bits, lib.fheaes_aes_decrypt_equivalent_bits):
                assert fn(None, buf, bits, buf, 1, ms) == -1
                assert fn(None, None, bits, None, 0, ms) == -1


def test_client_encrypts_an_aes_key_of_each_size(toy):
    c = own_client(toy)
    for bits in (128, 192, 256):
        key = FIPS_C[bits][0]
        ct = c.encrypt_aes_key(key)
        assert ct.shape == (bits // 8, 8, toy.params.big1)
        assert bytes(c.decrypt_bytes(ct)) == key
    with pytest.raises(ValueError):
        c.encrypt_aes_key(bytes(20))


def test_round_keys_of_each_size_round_trip_through_a_file(toy, tmp_path):
    from tfhe_aes_amd.client import load_ciphertexts, save_ciphertexts

    p = toy.params
    rng = np.random.default_rng(5)
    for n in (11, 13, 15):
        rk = rng.integers(0, 1 << 63, size=(n, 16, 8, p.big1), dtype=np.uint64)
        save_ciphertexts(tmp_path / "rk.npz", p, "round_keys", rk)
        assert np.array_equal(load_ciphertexts(tmp_path / "rk.npz", p, "round_keys"), rk)
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "bad.npz", p, "round_keys", rk[:12])


# ---- 3. the model at PARAM_TOY ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(toy):
    return AesModel(toy.oracle)


def test_model_at_128_bits_is_the_oracle_word_for_word(toy, model):
    c = own_client(toy)
    key, _ = FIPS_C[128]
    ek = c.encrypt_aes_key(key)
    w = toy.oracle.aes_key_expansion(ek)
    assert np.array_equal(model.key_expansion(ek), w)
    st = np.stack([c.encrypt_u128(FIPS_C_PT), c.encrypt_u128(0xDEADBEEF)])
    for i in range(2):
        enc = toy.oracle.aes_encrypt(w, st[i])
        assert np.array_equal(model.encrypt(w, st[i]), enc)
        assert np.array_equal(model.decrypt(w, enc), toy.oracle.aes_decrypt(w, enc))
    assert np.array_equal(model.encrypt(w, st)[1], model.encrypt(w, st[1]))          # a batch is its blocks


@pytest.mark.parametrize("bits", [192, 256])
def test_model_at_param_toy_fips197_appendix_c(toy, model, bits):
    c = own_client(toy)
    key, ct = FIPS_C[bits]
    w = model.key_expansion(c.encrypt_aes_key(key))
    want_w = aes_clear.expand_key(key)
    assert w.shape == (NR[bits] + 1, 16, 8, toy.params.big1)
    assert np.array_equal(c.decrypt_bytes(w), key_words(want_w))
    enc = model.encrypt(w, c.encrypt_u128(FIPS_C_PT))
    assert c.decrypt_u128(enc) == ct
    assert c.decrypt_u128(model.decrypt(w, enc)) == FIPS_C_PT
    dw = model.dec_round_keys(w)
    assert np.array_equal(c.decrypt_bytes(dw), key_words(aes_clear.inv_mix_columns_round_keys(want_w)))
    assert np.array_equal(dw[0], w[0]) and np.array_equal(dw[-1], w[-1])
    assert c.decrypt_u128(model.decrypt_equivalent(dw, enc)) == FIPS_C_PT
