"""The equivalent inverse cipher (FIPS-197 section 5.3.5, Fig. 15) without a GPU: the clear-domain counterpart decrypts like the
ordinary inverse cipher, the library exports the two entry points and refuses a NULL context, and the word-exact model the GPU tests
compare against (tests/test_gpu_aes_eqinv.py) decrypts to the plaintext at PARAM_TOY.

The model is written here from FIPS-197 rather than from csrc/aes_schedule.h: the oracle's WoPBS with LUTs built by server.gen_lut from the
aes_clear tables, and numpy uint64 wrapping sums for the linear layers (InvShiftRows, InvMixColumns, AddRoundKey)."""
import ctypes

import numpy as np

from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import Client

FIPS_C1_KEY = 0x000102030405060708090A0B0C0D0E0F
FIPS_C1_PT = 0x00112233445566778899AABBCCDDEEFF
FIPS_C1_CT = 0x69C4E0D86A7B0430D8CDB78070B4C55A

# InvMixColumns, FIPS-197 eq. (5.10): out[r] = sum_j INV_MC[r][j] * in[j] within one column
INV_MC = ((0x0E, 0x0B, 0x0D, 0x09), (0x09, 0x0E, 0x0B, 0x0D), (0x0D, 0x09, 0x0E, 0x0B), (0x0B, 0x0D, 0x09, 0x0E))
MULS = (0x09, 0x0B, 0x0D, 0x0E)                  # the order of the 4-LUT sets


def own_client(kit):
    """a Client with the kit's secret key but its own encryption counter: the session client's sequence of encryptions, which the
    other test files run on, stays as it was"""
    return Client(1, kit.client.iv, kit.client.key, params=kit.params, seed=kit.client.test_seed)


def _luts(fs):
    from tfhe_aes_amd.server import gen_lut

    return np.stack([gen_lut(2, 1, 512, 8, f) for f in fs])


class EqInvModel:
    """word-exact model of fheaes_aes_decryption_round_keys + fheaes_aes_decrypt_equivalent on the CPU oracle"""

    def __init__(self, oracle):
        self.O = oracle
        self.big1 = oracle.params.big1
        self.mul = _luts([lambda x, m=m: aes_clear.gf_mul(x, m) for m in MULS])
        self.mul_inv_s = _luts([lambda x, m=m: aes_clear.gf_mul(aes_clear.INV_SBOX[x], m) for m in MULS])
        self.inv_s = _luts([lambda x: aes_clear.INV_SBOX[x]])
        self.identity = _luts([lambda x: x])

    def _wopbs(self, st, luts):
        """[B][16][8][kN+1] -> [B][16][L][8][kN+1]"""
        b = st.shape[0]
        return self.O.wopbs_batch(np.ascontiguousarray(st).reshape(b * 16, 8, self.big1), luts).reshape(b, 16, len(luts), 8, self.big1)

    @staticmethod
    def _inv_mix(y, shift):
        """y [B][16][4][8][kN+1] (the four multiples of every byte) -> InvMixColumns(InvShiftRows^shift(state)), as wrapping sums"""
        out = np.zeros((y.shape[0], 16) + y.shape[3:], dtype=np.uint64)
        for c in range(4):
            for r in range(4):
                for j in range(4):
                    src = 4 * ((c - j) % 4 if shift else c) + j          # InvShiftRows: row j of column c comes from column c - j
                    out[:, 4 * c + r] += y[:, src, MULS.index(INV_MC[r][j])]
        return out

    def dec_round_keys(self, w):
        w = np.ascontiguousarray(w, dtype=np.uint64)
        mix = self._inv_mix(self._wopbs(w[1:10], self.mul), shift=False)
        fresh = self._wopbs(mix, self.identity)[:, :, 0]
        return np.concatenate([w[:1], fresh, w[10:]])

    def decrypt(self, dw, state):
        st = np.ascontiguousarray(state, dtype=np.uint64)
        single = st.ndim == 3
        st = (st[None] if single else st) + dw[10]
        for rnd in range(9, 0, -1):
            st = self._inv_mix(self._wopbs(st, self.mul_inv_s), shift=True) + dw[rnd]
        y = self._wopbs(st, self.inv_s)[:, :, 0]
        out = np.empty_like(st)
        for c in range(4):
            for r in range(4):
                out[:, 4 * c + r] = y[:, 4 * ((c - r) % 4) + r] + dw[0][4 * c + r]
        return out[0] if single else out


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
    model = EqInvModel(toy.oracle)
    dw = model.dec_round_keys(w)
    want_dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))
    assert np.array_equal(c.decrypt_bytes(dw), np.array(want_dw, dtype=np.uint8))
    cts = [FIPS_C1_CT, aes_clear.aes128_encrypt_block(key, 0xDEADBEEF)]
    out = model.decrypt(dw, np.stack([c.encrypt_u128(v) for v in cts]))
    assert c.decrypt_u128(out[0]) == FIPS_C1_PT
    assert c.decrypt_u128(out[1]) == 0xDEADBEEF
