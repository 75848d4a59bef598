"""The public-ciphertext modes without a GPU: aes_clear's CBC / CFB-128 / GCM-keystream functions against SP 800-38A F.2 / F.3 and
SP 800-38D test case 3, the 32-bit counter, the sharing rule of the decryption direction (fheaes_aes_decrypt_public_plan_keyed) against
the rule restated in public_modes.rule_dec, and the shared schedule itself (public_modes.shared_decrypt: one WoPBS per distinct S-Box
input on the CPU oracle) against AesModel.decrypt_equivalent on trivial ciphertexts of the same blocks, word for word."""
import ctypes

import numpy as np
import pytest

from aes_model import AesModel
from aes_vectors import BASE, F1_PT, MASK128, NR, counters, own_client
from public_modes import (CBC, CFB128, GCM_CT_FIRST, GCM_CT_LAST, GCM_EK_J0, GCM_IV, GCM_J0, GCM_KEY, GCM_PT, IV, cbc_ct, cfb128_encrypt, inc32, rule_dec,
                          shared_decrypt)
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes
from tfhe_aes_amd.server import cbc_stream_blocks, ctr_stream_blocks, gcm_ctr_args

NEW_EXPORTS = ("fheaes_aes_decrypt_public_bits", "fheaes_aes_decrypt_public_keyed", "fheaes_aes_decrypt_public_keyed_packed",
               "fheaes_aes_cbc_decrypt_bits", "fheaes_aes_decrypt_public_plan_keyed", "fheaes_aes_ctr32_bits")


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


def test_new_entry_points_reject_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    kob = (ctypes.c_uint32 * 1)()
    for ms in (_native.HOST, _native.DEVICE):
        for bits in (128, 192, 256, 100):
            assert lib.fheaes_aes_decrypt_public_bits(None, buf, bits, buf, None, 1, buf, ms) == -1
            assert lib.fheaes_aes_cbc_decrypt_bits(None, buf, bits, buf, buf, 1, buf, ms) == -1
            assert lib.fheaes_aes_ctr32_bits(None, buf, bits, buf, 0, None, 1, buf, ms) == -1
            assert lib.fheaes_aes_decrypt_public_keyed(None, buf, bits, 1, kob, buf, None, 1, buf, ms) == -1
            assert lib.fheaes_aes_decrypt_public_keyed_packed(None, buf, bits, 1, kob, buf, None, 1, buf, ms) == -1


# ---- 2. the clear modes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_cbc_decrypt_sp800_38a_f2(bits):
    key, first, last = CBC[bits]
    ct = cbc_ct(bits)
    assert ct[0] == first and ct[3] == last
    assert aes_clear.cbc_decrypt(key, IV, ct) == F1_PT
    assert aes_clear.cbc_decrypt(key, ct[1], ct[2:]) == F1_PT[2:]              # the previous ciphertext block continues the stream
    assert aes_clear.cbc_decrypt(key, IV, []) == []


def test_cfb128_decrypt_sp800_38a_f3_14():
    key, first, last = CFB128
    ct = cfb128_encrypt(key, IV, F1_PT)
    assert ct[0] == first and ct[3] == last
    assert aes_clear.cfb128_decrypt(key, IV, ct) == F1_PT
    assert aes_clear.cfb128_decrypt(key, ct[0], ct[1:]) == F1_PT[1:]


def test_gcm_keystream_sp800_38d_test_case_3():
    ks = aes_clear.gcm_keystream(GCM_KEY, GCM_IV, 0, 4)
    ct = [k ^ p for k, p in zip(ks, GCM_PT)]
    assert ct[0] == GCM_CT_FIRST and ct[3] == GCM_CT_LAST
    assert aes_clear.aes_encrypt_block(GCM_KEY, GCM_J0) == GCM_EK_J0
    assert ks == [aes_clear.aes_encrypt_block(GCM_KEY, GCM_J0 + 1 + i) for i in range(4)]
    assert aes_clear.gcm_keystream(GCM_KEY, GCM_IV, 2, 2) == ks[2:]            # first_block continues the stream
    assert aes_clear.ctr_keystream(GCM_KEY, GCM_J0, 1, 4, counter_bits=32) == ks
    for bad in (bytes(8), bytes(16)):
        with pytest.raises(ValueError):
            aes_clear.gcm_keystream(GCM_KEY, bad, 0, 1)


def test_the_32_bit_counter_wraps_and_leaves_the_upper_96_bits():
    icb = (BASE >> 32 << 32) | 0xFFFFFFFE
    want = [icb, icb + 1, icb - 0xFFFFFFFE, icb - 0xFFFFFFFD]                   # ..FFFFFFFE, ..FFFFFFFF, ..00000000, ..00000001
    assert [aes_clear.counter_block(icb, i, 32) for i in range(4)] == want == [inc32(icb, i) for i in range(4)]
    assert all(w >> 32 == icb >> 32 for w in want)
    assert aes_clear.ctr_keystream(CBC[128][0], icb, 0, 4, counter_bits=32) == [aes_clear.aes_encrypt_block(CBC[128][0], w) for w in want]
    assert aes_clear.ctr_keystream(CBC[128][0], icb, 0, 4) == [aes_clear.aes_encrypt_block(CBC[128][0], icb + i) for i in range(4)]
    assert aes_clear.ctr_keystream(CBC[128][0], icb - 3, 3, 4, counter_bits=32) == aes_clear.ctr_keystream(CBC[128][0], icb, 0, 4, counter_bits=32)
    assert ctr_stream_blocks([(0, icb, 0, 4, None)], 32)[1] == want
    assert ctr_stream_blocks([(0, icb, 0, 4, None)])[1] == counters(icb, 4)
    for bad in (64, 0, 96, None):
        with pytest.raises(ValueError):
            aes_clear.ctr_keystream(CBC[128][0], icb, 0, 1, counter_bits=bad)
        with pytest.raises(ValueError):
            ctr_stream_blocks([(0, icb, 0, 1, None)], bad)


def test_stream_helpers_build_the_chaining_blocks():
    ct = cbc_ct(128)
    kob, blocks, chain = cbc_stream_blocks([(2, IV, ct), (0, ct[0].to_bytes(16, "big"), b"".join(c.to_bytes(16, "big") for c in ct[1:])), (1, 5, [])])
    assert kob == [2] * 4 + [0] * 3
    assert _native.u128_pairs(blocks).tolist() == _native.u128_pairs(ct + ct[1:]).tolist()
    assert _native.u128_pairs(chain).tolist() == _native.u128_pairs([IV] + ct[:3] + ct[:3]).tolist()[:7]
    assert gcm_ctr_args(GCM_IV, None, 3) == (GCM_J0, 3, None)
    assert gcm_ctr_args(GCM_IV, bytes(32), None)[1] == 2
    for bad_iv in (bytes(8), bytes(16), GCM_J0):
        with pytest.raises(ValueError, match="GHASH"):
            gcm_ctr_args(bad_iv, None, 1)
    with pytest.raises(ValueError):
        gcm_ctr_args(GCM_IV, bytes(31), None)
    with pytest.raises(ValueError):
        gcm_ctr_args(GCM_IV, None, 1, first_block=-1)
    with pytest.raises(ValueError):
        cbc_stream_blocks([(0, IV, bytes(17))])


# ---- 3. the plan ---------------------------------------------------------------------------------------------------------------------------
_C = cbc_ct(128)
PLAN_TABLE = [
    (_C, (64, 64, 64)),
    ([_C[0], _C[1], _C[0], _C[1]], (32, 32, 32)),
    (counters(BASE, 7), (22, 40, 112)),
    ([0x11111111111111111111111111111111, 0x11111111111111111111111111111122], (17, 20, 32)),
]


@pytest.mark.parametrize("row", range(len(PLAN_TABLE)))
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_plan_gives_the_expected_rows_and_the_restated_rule(bits, row):
    blocks, (r1, r2, later) = PLAN_TABLE[row]
    plan = _native.aes_decrypt_public_plan(blocks, bits)
    assert plan == [r1, r2] + [later] * (NR[bits] - 2)
    assert plan == rule_dec(blocks, NR[bits])[0]
    assert plan == _native.aes_decrypt_public_plan_keyed(blocks, [0] * len(blocks), 3, bits)      # every key 0: the single-key plan
    assert plan == _native.aes_decrypt_public_plan([b.to_bytes(16, "big") for b in blocks], bits)


def test_plan_never_shares_between_keys():
    blocks = counters(BASE, 7)
    one = _native.aes_decrypt_public_plan(blocks)
    kob = [0] * 7 + [1] * 7
    two = _native.aes_decrypt_public_plan_keyed(blocks + blocks, kob, 2)
    assert two == [2 * x for x in one] == rule_dec(blocks + blocks, 10, kob)[0]
    assert _native.aes_decrypt_public_plan_keyed(blocks + blocks, [1] * 14, 2) == one                # the same key: everything shared
    mixed = [0, 1, 0, 1, 1, 0, 0]
    assert _native.aes_decrypt_public_plan_keyed(blocks, mixed, 2, 192) == rule_dec(blocks, 12, mixed)[0]


def test_plan_of_random_blocks_and_of_no_blocks():
    rng = np.random.default_rng(0xCBC)
    blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(40)]
    distinct = len({(p, v) for b in blocks for p, v in enumerate(u128_to_bytes(b))})
    assert _native.aes_decrypt_public_plan(blocks, 256) == rule_dec(blocks, 14)[0] == [distinct] + [16 * 40] * 13
    assert _native.aes_decrypt_public_plan([], 192) == [0] * 12
    wrap = counters(MASK128 - 1, 4)
    assert _native.aes_decrypt_public_plan(wrap) == rule_dec(wrap, 10)[0]


def test_plan_rejects_bad_arguments():
    lib = _native.load_library()
    blocks = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    kob = (ctypes.c_uint32 * 2)(0, 1)
    out = (ctypes.c_uint64 * 14)()
    fn = lib.fheaes_aes_decrypt_public_plan_keyed
    assert fn(blocks, kob, 2, 2, 128, out) == 0
    assert fn(blocks, None, 2, 1, 128, out) == 0                                # NULL: every block under key 0
    for bits in (100, 0, 64, 129):
        assert fn(blocks, kob, 2, 2, bits, out) == -1
    assert fn(None, kob, 2, 2, 128, out) == -1
    assert fn(blocks, kob, 2, 2, 128, None) == -1
    assert fn(blocks, kob, 2, 1, 128, out) == -1                                # key index 1 with one key
    assert fn(blocks, kob, 2, 0, 128, out) == -1
    assert fn(blocks, kob, 2, 65537, 128, out) == -1
    with pytest.raises(_native.FheAesError):
        _native.aes_decrypt_public_plan([1, 2], 100)
    with pytest.raises(_native.FheAesError):
        _native.aes_decrypt_public_plan_keyed([1, 2], [0, 2], 2)
    with pytest.raises(ValueError):
        _native.aes_decrypt_public_plan([1 << 128])
    with pytest.raises(ValueError):
        _native.aes_decrypt_public_plan_keyed([1, 2], [0], 1)


# ---- 4. the shared schedule on the CPU oracle ---------------------------------------------------------------------------------------------
def test_shared_schedule_is_the_models_equivalent_inverse_cipher_on_trivial_bytes(toy):
    """three blocks, two of them equal: the pools of the restated rule through the oracle's WoPBS give the words of
    AesModel.decrypt_equivalent on the trivial state, in sum(plan) evaluations; with the chaining blocks added they decrypt to the CBC
    plaintext"""
    c = own_client(toy)
    model = AesModel(toy.oracle)
    key = CBC[128][0]
    dw = model.dec_round_keys(toy.oracle.aes_key_expansion(c.encrypt_aes_key(key)))
    ct = cbc_ct(128)
    blocks = [ct[0], ct[1], ct[0]]
    chain = [IV, ct[0], ct[1]]
    trivial = c.trivial_bytes([u128_to_bytes(b) for b in blocks])
    t_chain = c.trivial_bytes([u128_to_bytes(b) for b in chain])
    got, evaluated = shared_decrypt(model, dw, trivial, blocks)
    plan = _native.aes_decrypt_public_plan(blocks)
    assert evaluated == sum(plan) == 320 < 16 * 3 * 10
    want = model.decrypt_equivalent(dw, trivial)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    for i, b in enumerate(blocks):
        assert c.decrypt_u128(got[i]) == aes_clear.aes_decrypt_block(key, b)
    with_data, _ = shared_decrypt(model, dw, trivial, blocks, data=t_chain)
    assert np.array_equal(with_data, want + t_chain)
    assert [c.decrypt_u128(with_data[i]) for i in range(2)] == F1_PT[:2]
    assert c.decrypt_u128(with_data[2]) == aes_clear.aes_decrypt_block(key, ct[0]) ^ ct[1]
