"""AES-192 and AES-256 (FIPS-197 with Nk = 6 / 8 key words, Nr = 12 / 14 rounds) without a GPU: the clear-domain cipher against the
vectors of FIPS-197 appendices A and C and of SP 800-38A, the five `_bits` entry points of the library, and the word-exact model the GPU
tests compare against (tests/test_gpu_aes_key_sizes.py).

The CPU oracle has AES-128 schedules only, so the model is written here from FIPS-197 rather than from csrc/aes_schedule.h: the oracle's WoPBS
with LUTs built by server.gen_lut from the aes_clear tables, and numpy uint64 wrapping sums for the linear layers (RotWord, Rcon,
ShiftRows, MixColumns, AddRoundKey and their inverses).  At 128 bits it has to reproduce the oracle's own key expansion, encryption and
decryption word for word; that pins its conventions before it is trusted for the other two key sizes."""
import ctypes

import numpy as np
import pytest

from test_aes_eqinv_cpu import own_client
from tfhe_aes_amd import _native, aes_clear

# FIPS-197 appendix C.1 / C.2 / C.3: key 00 01 02 .., one plaintext
FIPS_C_PT = 0x00112233445566778899AABBCCDDEEFF
FIPS_C = {128: (bytes(range(16)), 0x69C4E0D86A7B0430D8CDB78070B4C55A),
          192: (bytes(range(24)), 0xDDA97CA4864CDFE06EAF70A0EC0D7191),
          256: (bytes(range(32)), 0x8EA2B7CA516745BFEAFC49904B496089)}
# FIPS-197 appendix A.2 / A.3 (key expansion; the last word) and SP 800-38A F.1.3 / F.1.5 (ECB, first block) with the same keys
A2_KEY = bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b")
A3_KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
SP800_PT = 0x6BC1BEE22E409F96E93D7E117393172A

NR = {128: 10, 192: 12, 256: 14}
BITS_FUNCS = ("fheaes_aes_key_expansion_bits", "fheaes_aes_encrypt_bits", "fheaes_aes_decrypt_bits",
              "fheaes_aes_decryption_round_keys_bits", "fheaes_aes_decrypt_equivalent_bits")

# MixColumns, FIPS-197 eq. (5.6), and InvMixColumns, eq. (5.10): out[r] = sum_j M[r][j] * in[j] within one column
MC = ((2, 3, 1, 1), (1, 2, 3, 1), (1, 1, 2, 3), (3, 1, 1, 2))
INV_MC = ((0x0E, 0x0B, 0x0D, 0x09), (0x09, 0x0E, 0x0B, 0x0D), (0x0D, 0x09, 0x0E, 0x0B), (0x0B, 0x0D, 0x09, 0x0E))
ENC_MULS = (1, 2, 3)                             # the order of the 3-LUT set {S, 2S, 3S}
DEC_MULS = (0x09, 0x0B, 0x0D, 0x0E)              # the order of the 4-LUT sets


def _luts(fs):
    from tfhe_aes_amd.server import gen_lut

    return np.stack([gen_lut(2, 1, 512, 8, f) for f in fs])


def key_words(rk):
    """round keys as lists of 16 ints -> what the client decrypts from [Nr+1][16][8][kN+1]"""
    return np.array(rk, dtype=np.uint8)


class AesModel:
    """word-exact model of the five AES operations for Nk = 4 / 6 / 8 on the CPU oracle's WoPBS"""

    def __init__(self, oracle):
        S, IS, mul = aes_clear.SBOX, aes_clear.INV_SBOX, aes_clear.gf_mul
        self.O = oracle
        self.big1 = oracle.params.big1
        self.enc_round = _luts([lambda x, m=m: mul(S[x], m) for m in ENC_MULS])
        self.sbox = _luts([lambda x: S[x]])
        self.inv_sbox = _luts([lambda x: IS[x]])
        self.dec_mul = _luts([lambda x, m=m: mul(x, m) for m in DEC_MULS])
        self.dec_eq_round = _luts([lambda x, m=m: mul(IS[x], m) for m in DEC_MULS])
        self.identity = _luts([lambda x: x])

    # ---- building blocks ----
    def _wopbs(self, st, luts):
        """[B][16][8][kN+1] -> [B][16][L][8][kN+1]"""
        b = st.shape[0]
        return self.O.wopbs_batch(np.ascontiguousarray(st).reshape(b * 16, 8, self.big1), luts).reshape(b, 16, len(luts), 8, self.big1)

    def _word(self, word, luts):
        """one key word [4][8][kN+1] through a one-LUT WoPBS"""
        return self.O.wopbs_batch(np.ascontiguousarray(word), luts)[:, 0]

    @staticmethod
    def _shift(y, inverse):
        """ShiftRows (row r of column c comes from column c + r) or its inverse (from column c - r) on [B][16][...]"""
        out = np.empty_like(y)
        for c in range(4):
            for r in range(4):
                out[:, 4 * c + r] = y[:, 4 * ((c - r if inverse else c + r) % 4) + r]
        return out

    @staticmethod
    def _mix(y, matrix, muls, shift):
        """y [B][16][L][8][kN+1] (the multiples of every byte) -> (Inv)MixColumns of the state, shift = +1: after ShiftRows, -1: after
        InvShiftRows, 0: in place; wrapping sums"""
        out = np.zeros((y.shape[0], 16) + y.shape[3:], dtype=np.uint64)
        for c in range(4):
            for r in range(4):
                for j in range(4):
                    out[:, 4 * c + r] += y[:, 4 * ((c + shift * j) % 4) + j, muls.index(matrix[r][j])]
        return out

    # ---- FIPS-197 section 5.2 under the reference's rule (server.rs:107-155): every new word refreshed by an identity WoPBS ----
    def key_expansion(self, key):
        key = np.ascontiguousarray(key, dtype=np.uint64)
        nk = key.shape[0] // 4
        nr = nk + 6
        w = [key[4 * i:4 * i + 4] for i in range(nk)]
        for i in range(nk, 4 * (nr + 1)):
            t = w[i - 1]
            if i % nk == 0:
                t = self._word(np.roll(t, -1, axis=0), self.sbox)                          # RotWord, SubWord
                rcon = np.uint64(aes_clear.RCON[i // nk - 1])                              # Rcon: a trivial ciphertext, bodies only
                t[0, :, -1] += ((rcon >> np.arange(8, dtype=np.uint64)) & np.uint64(1)) << np.uint64(63)
            elif nk > 6 and i % nk == 4:
                t = self._word(t, self.sbox)
            w.append(self._word(w[i - nk] + t, self.identity))
        return np.stack(w).reshape(nr + 1, 16, 8, self.big1)

    # ---- FIPS-197 Fig. 5 with Server::aes_encrypt's schedule ----
    def encrypt(self, rk, state):
        st = np.ascontiguousarray(state, dtype=np.uint64)
        single = st.ndim == 3
        nr = rk.shape[0] - 1
        st = (st[None] if single else st) + rk[0]
        for rnd in range(1, nr):
            st = self._mix(self._wopbs(st, self.enc_round), MC, ENC_MULS, +1) + rk[rnd]
        st = self._shift(self._wopbs(st, self.sbox)[:, :, 0], inverse=False) + rk[nr]
        return st[0] if single else st

    # ---- FIPS-197 Fig. 12 with Server::aes_decrypt's schedule: two WoPBS per round ----
    def decrypt(self, rk, state):
        st = np.ascontiguousarray(state, dtype=np.uint64)
        single = st.ndim == 3
        nr = rk.shape[0] - 1
        st = (st[None] if single else st) + rk[nr]
        for rnd in range(nr - 1, 0, -1):
            st = self._shift(self._wopbs(st, self.inv_sbox)[:, :, 0], inverse=True) + rk[rnd]
            st = self._mix(self._wopbs(st, self.dec_mul), INV_MC, DEC_MULS, 0)
        st = self._shift(self._wopbs(st, self.inv_sbox)[:, :, 0], inverse=True) + rk[0]
        return st[0] if single else st

    # ---- FIPS-197 Fig. 15: the equivalent inverse cipher ----
    def dec_round_keys(self, w):
        w = np.ascontiguousarray(w, dtype=np.uint64)
        nr = w.shape[0] - 1
        mix = self._mix(self._wopbs(w[1:nr], self.dec_mul), INV_MC, DEC_MULS, 0)
        return np.concatenate([w[:1], self._wopbs(mix, self.identity)[:, :, 0], w[nr:]])

    def decrypt_equivalent(self, dw, state):
        st = np.ascontiguousarray(state, dtype=np.uint64)
        single = st.ndim == 3
        nr = dw.shape[0] - 1
        st = (st[None] if single else st) + dw[nr]
        for rnd in range(nr - 1, 0, -1):
            st = self._mix(self._wopbs(st, self.dec_eq_round), INV_MC, DEC_MULS, -1) + dw[rnd]
        st = self._shift(self._wopbs(st, self.inv_sbox)[:, :, 0], inverse=True) + dw[0]
        return st[0] if single else st


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
