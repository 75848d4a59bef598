"""Many AES keys under one FHE key, without a GPU: the seven new entry points are declared, exported and bound; the keyed sharing rule
(fheaes_aes_public_plan_keyed) against a restatement written here -- aes_model.rule() with the key in the round-1 id --
and against the counts of DESIGN.md section 7; the argument errors that need no context; aes_clear.ctr_streams against SP 800-38A F.5."""
import ctypes

import numpy as np
import pytest

from aes_model import SOURCES, TABLE, rule
from aes_vectors import BASE, F1_PT, F5, F5_CTR, MASK128, NR, counters
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes
from tfhe_aes_amd.server import ctr_stream_blocks

NEW = ("fheaes_aes_key_expansion_batch", "fheaes_aes_decryption_round_keys_batch", "fheaes_aes_encrypt_keyed", "fheaes_aes_decrypt_keyed",
       "fheaes_aes_decrypt_equivalent_keyed", "fheaes_aes_public_keyed", "fheaes_aes_public_plan_keyed")


def rule_keyed(blocks, keys, nr):
    """rule() with the round-1 id (key, p, byte): distinct ids per round"""
    ids = [[(k, p, v) for p, v in enumerate(u128_to_bytes(b))] for b, k in zip(blocks, keys)]
    counts = []
    for _ in range(nr):
        number = {}
        ids = [[number.setdefault(i, len(number)) for i in blk] for blk in ids]       # equal tuples are one id
        counts.append(len(number))
        ids = [[(p,) + tuple(blk[s] for s in SOURCES[p]) for p in range(16)] for blk in ids]
    return counts


def grouped(n_keys, per_key, start=BASE):
    """n_keys x per_key counters from `start`, key by key: (blocks, keys)"""
    return counters(start, per_key) * n_keys, [k for k in range(n_keys) for _ in range(per_key)]


# case -> (blocks, keys, n_keys, key_bits, (round 1, round 2, each later round, sum))
KEYED = {
    "one key x 128": (counters(BASE, 128), [0] * 128, 1, 128, (143, 524, 2048, 17051)),
    "2 keys x 64, grouped": grouped(2, 64) + (2, 128, (158, 536, 2048, 17078)),
    "2 keys x 64, interleaved": ([BASE + i // 2 for i in range(128)], [i % 2 for i in range(128)], 2, 128, (158, 536, 2048, 17078)),
    "8 keys x 16": grouped(8, 16) + (8, 128, (248, 608, 2048, 17240)),
    "8 keys x 16, AES-256": grouped(8, 16) + (8, 256, (248, 608, 2048, 25432)),
    "32 keys x 4": grouped(32, 4) + (32, 128, (608, 896, 2048, 17888)),
    "128 keys x BASE": ([BASE] * 128, list(range(128)), 128, 128, (2048, 2048, 2048, 20480)),
    "two blocks under two keys": ([BASE, BASE + 1] * 2, [0, 0, 1, 1], 2, 128, (34, 40, 64, 586)),
    "the same four under one key": ([BASE, BASE + 1] * 2, [0, 0, 0, 0], 2, 128, (17, 20, 32, 293)),
    "a third copy of BASE under each key": ([BASE, BASE + 1, BASE] * 2, [0, 0, 0, 1, 1, 1], 2, 128, (34, 40, 64, 586)),
    "unused keys": ([BASE, BASE + 1] * 2, [1, 1, 5, 5], 7, 128, (34, 40, 64, 586)),
}


def test_header_library_and_bindings_have_the_new_entry_points():
    lib = _native.load_library()
    header = _native.header_symbols()
    for name in NEW:
        assert name in header, name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    for method in ("aes_key_expansion_batch", "aes_decryption_round_keys_batch", "aes_encrypt_keyed", "aes_decrypt_keyed", "aes_decrypt_equivalent_keyed",
                   "aes_public_keyed"):
        assert callable(getattr(_native.Engine, method))
    assert callable(_native.aes_public_plan_keyed)


@pytest.mark.parametrize("case", list(KEYED))
def test_keyed_plan_is_the_restated_rule_and_the_documented_counts(case):
    blocks, keys, n_keys, bits, (r1, r2, later, total) = KEYED[case]
    plan = _native.aes_public_plan_keyed(blocks, keys, n_keys, bits)
    assert plan == rule_keyed(blocks, keys, NR[bits])
    assert plan == [r1, r2] + [later] * (NR[bits] - 2)
    assert sum(plan) == total


def test_128_keys_share_nothing_and_one_key_shares_what_the_single_key_plan_shares():
    blocks, keys, n_keys, bits, _ = KEYED["128 keys x BASE"]
    assert _native.aes_public_plan_keyed(blocks, keys, n_keys, bits) == [16 * 128] * 10
    assert _native.aes_public_plan_keyed(blocks, [0] * 128, n_keys, bits) == _native.aes_public_plan([BASE]) == [16] * 10


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_all_zero_keys_give_the_single_key_plan(row):
    blocks, bits, _ = TABLE[row]
    want = _native.aes_public_plan(blocks, bits)
    assert want == rule(blocks, NR[bits])[0]
    for n_keys in (1, 3, 65536):
        assert _native.aes_public_plan_keyed(blocks, [0] * len(blocks), n_keys, bits) == want
    # the same blocks under any ONE key: the key is part of every id, so nothing changes
    assert _native.aes_public_plan_keyed(blocks, [2] * len(blocks), 3, bits) == want


def test_keyed_plan_of_random_blocks_and_keys_is_the_restated_rule():
    rng = np.random.default_rng(0x3E7)
    for bits in (128, 192, 256):
        blocks = [BASE + int(v) for v in rng.integers(0, 12, size=40)]
        keys = [int(k) for k in rng.integers(0, 5, size=40)]
        assert _native.aes_public_plan_keyed(blocks, keys, 5, bits) == rule_keyed(blocks, keys, NR[bits])
    assert _native.aes_public_plan_keyed([], [], 4, 192) == [0] * 12


def test_keyed_plan_rejects_bad_arguments():
    lib = _native.load_library()
    blocks = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    keys = (ctypes.c_uint32 * 2)(0, 1)
    out = (ctypes.c_uint64 * 14)()
    plan = lib.fheaes_aes_public_plan_keyed
    assert plan(blocks, keys, 2, 2, 128, out) == 0
    assert plan(blocks, keys, 2, 1, 128, out) == -1                      # key index 1 with one key
    assert plan(blocks, keys, 2, 0, 128, out) == -1                      # n_keys = 0
    assert plan(blocks, keys, 2, 65536, 128, out) == 0                   # the documented bound
    assert plan(blocks, keys, 2, 65537, 128, out) == -1
    for bits in (100, 0, 64, 129):
        assert plan(blocks, keys, 2, 2, bits, out) == -1
    assert plan(None, keys, 2, 2, 128, out) == -1
    assert plan(blocks, None, 2, 2, 128, out) == -1
    assert plan(blocks, keys, 2, 2, 128, None) == -1
    with pytest.raises(_native.FheAesError):
        _native.aes_public_plan_keyed([1, 2], [0, 2], 2)
    with pytest.raises(_native.FheAesError):
        _native.aes_public_plan_keyed([1, 2], [0, 1], 2, 100)
    with pytest.raises(ValueError):
        _native.aes_public_plan_keyed([1, 2], [0], 2)
    with pytest.raises(ValueError):
        _native.aes_public_plan_keyed([1], [-1], 2)


def test_new_context_entry_points_reject_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    keys = (ctypes.c_uint32 * 1)(0)
    for ms in (_native.HOST, _native.DEVICE):
        for bits in (128, 192, 256, 100):
            assert lib.fheaes_aes_key_expansion_batch(None, buf, bits, 1, buf, ms) == -1
            assert lib.fheaes_aes_decryption_round_keys_batch(None, buf, bits, 1, buf, ms) == -1
            assert lib.fheaes_aes_encrypt_keyed(None, buf, bits, 1, keys, buf, 1, ms) == -1
            assert lib.fheaes_aes_decrypt_keyed(None, buf, bits, 1, keys, buf, 1, ms) == -1
            assert lib.fheaes_aes_decrypt_equivalent_keyed(None, buf, bits, 1, keys, buf, 1, ms) == -1
            assert lib.fheaes_aes_public_keyed(None, buf, bits, 1, keys, buf, None, 1, buf, ms) == -1


# ---- the clear streams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_ctr_streams_sp800_38a_f5(bits):
    key, first, last = F5[bits]
    other = bytes(reversed(key))
    streams = [(0, F5_CTR, 0, 4, F1_PT),                                     # F.5.1 / F.5.3 / F.5.5 itself
               (1, F5_CTR, 0, 2, None),                                      # the same counters under another key: its keystream
               (0, F5_CTR - 1, 3, 2, F1_PT[2:])]                             # blocks 2..3 of the first stream again, iv and first_block shifted
    out = aes_clear.ctr_streams([key, other], streams)
    assert len(out) == 8
    assert out[0] == first and out[3] == last
    assert out[4:6] == aes_clear.ctr_keystream(other, F5_CTR, 0, 2) != aes_clear.ctr_keystream(key, F5_CTR, 0, 2)
    assert out[6:8] == out[2:4]
    assert aes_clear.ctr_streams([key], []) == []


def test_ctr_stream_blocks_builds_the_counters_of_aes_ctr():
    kob, blocks, data = ctr_stream_blocks([(2, MASK128 - 1, 0, 3, None), (0, (BASE | 0xFE).to_bytes(16, "big"), 1, 2, [5, 6]), (1, 7, 0, 0, None)])
    assert kob == [2, 2, 2, 0, 0]
    assert blocks == [MASK128 - 1, MASK128, 0, BASE | 0xFF, BASE + 0x100]
    assert data == [0, 0, 0, 5, 6]
    assert ctr_stream_blocks([(0, 1, 0, 2, None)])[2] is None
    for bad in ([(0, 1 << 128, 0, 1, None)], [(0, 1, -1, 1, None)], [(0, 1, 0, 2, [1])]):
        with pytest.raises(ValueError):
            ctr_stream_blocks(bad)
