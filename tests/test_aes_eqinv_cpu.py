"""The equivalent inverse cipher (FIPS-197 section 5.3.5, Fig. 15) without a GPU: the clear-domain counterpart decrypts like the
ordinary inverse cipher, the library exports the two entry points and refuses a NULL context, and the word-exact model the GPU tests
compare against (aes_model.AesModel: dec_round_keys, decrypt_equivalent) decrypts to the plaintext at PARAM_TOY."""
import ctypes

import numpy as np

from aes_model import AesModel
from aes_vectors import FIPS_C1_CT, FIPS_C1_KEY, FIPS_C1_PT, own_client
from tfhe_aes_amd import _native, aes_clear


def test_clear_equivalent_inverse_cipher_fips197_c1_and_random_blocks():
    dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(FIPS_C1_KEY))
    assert aes_clear.aes128_decrypt_block_equivalent(dw, FIPS_C1_CT) == FIPS_C1_PT
    assert aes_clear.aes128_decrypt_block(FIPS_C1_KEY, FIPS_C1_CT) == FIPS_C1_PT
    rng = np.random.default_rng(0x535)
    for _ in range(20):
        key, ct = int.from_bytes(rng.bytes(16), "big"), int.from_bytes(rng.bytes(16), "big")
        dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))
        assert aes_clear.aes128_decrypt_block_equivalent(dw, ct) == aes_clear.aes128_decrypt_block(key, ct)


def test_clear_decryption_round_keys_keep_the_outer_keys():
    w = aes_clear.expand_key(FIPS_C1_KEY)
    dw = aes_clear.inv_mix_columns_round_keys(w)
    assert len(dw) == 11 and dw[0] == w[0] and dw[10] == w[10]
    # FIPS-197 C.1, EQUIVALENT INVERSE CIPHER: round[ 1].ik_sch = dw[9], round[ 9].ik_sch = dw[1]
    assert bytes(dw[9]).hex() == "13aa29be9c8faff6f770f58000f7bf03"
    assert bytes(dw[1]).hex() == "8c56dff0825dd3f9805ad3fc8659d7fd"


def test_library_exports_the_equivalent_inverse_cipher():
    lib = _native.load_library()
    assert hasattr(lib, "fheaes_aes_decryption_round_keys") and hasattr(lib, "fheaes_aes_decrypt_equivalent")
    assert b" 0.4 " in lib.fheaes_version()


def test_equivalent_inverse_cipher_rejects_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_aes_decryption_round_keys(None, buf, buf, ms) == -1
        assert lib.fheaes_aes_decryption_round_keys(None, None, None, ms) == -1
        assert lib.fheaes_aes_decrypt_equivalent(None, buf, buf, 1, ms) == -1
        assert lib.fheaes_aes_decrypt_equivalent(None, None, None, 0, ms) == -1


def test_model_decrypts_at_param_toy(toy):
    """key conversion + two blocks through the model: the decryption round keys decrypt to InvMixColumns(w), the blocks to plaintext"""
    c = own_client(toy)
    key = FIPS_C1_KEY
    w = toy.oracle.aes_key_expansion(c.encrypt_u128(key))
    model = AesModel(toy.oracle)
    dw = model.dec_round_keys(w)
    want_dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))
    assert np.array_equal(c.decrypt_bytes(dw), np.array(want_dw, dtype=np.uint8))
    cts = [FIPS_C1_CT, aes_clear.aes128_encrypt_block(key, 0xDEADBEEF)]
    out = model.decrypt_equivalent(dw, np.stack([c.encrypt_u128(v) for v in cts]))
    assert c.decrypt_u128(out[0]) == FIPS_C1_PT
    assert c.decrypt_u128(out[1]) == 0xDEADBEEF
