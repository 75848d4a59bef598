"""Public blocks and CTR with a public nonce, without a GPU: the sharing rule (fheaes_aes_public_plan) against the table of DESIGN.md
section 7 and against a restatement of the rule (aes_model.rule), aes_clear.ctr_keystream against SP 800-38A F.5, and the shared schedule
itself (aes_model.shared_encrypt) -- one WoPBS per distinct S-Box input, written with the CPU oracle's WoPBS and numpy wrapping sums -- against the oracle's own
aes_encrypt on trivial ciphertexts of the same blocks, word for word.  That last test pins the two facts the GPU path rests on: the
rule is exact (equal ids have word-equal inputs), and a trivial ciphertext is a legal input."""
import ctypes

import numpy as np
import pytest

from aes_model import TABLE, AesModel, rule, shared_encrypt
from aes_vectors import BASE, F1_KEY, F1_PT, F5, F5_CTR, MASK128, NR, counters, own_client
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_public_entry_points():
    lib = _native.load_library()
    for name in ("fheaes_aes_encrypt_public_bits", "fheaes_aes_ctr_bits", "fheaes_aes_public_plan"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_plan_gives_the_rows_of_the_table(row):
    blocks, bits, (r1, r2, later, total) = TABLE[row]
    plan = _native.aes_public_plan(blocks, bits)
    assert plan == [r1, r2] + [later] * (NR[bits] - 2)
    assert sum(plan) == total
    assert plan == rule(blocks, NR[bits])[0]


def test_plan_of_random_blocks_shares_nothing():
    """64 seeded random blocks, 16 n in every round.  Independent random bytes cannot give that in round 1 (64 draws from 256 values
    at each position collide: by the rule they ARE shared), so every position draws its 64 bytes without replacement; the independent
    draw is checked next to it against the restated rule: it shares in round 1 only."""
    rng = np.random.default_rng(0xC7A)
    cols = np.stack([rng.permutation(256)[:64] for _ in range(16)], axis=1)                      # [64][16]: no two blocks agree in a byte
    blocks = [int.from_bytes(bytes(int(v) for v in row), "big") for row in cols]
    assert len({(p, v) for b in blocks for p, v in enumerate(u128_to_bytes(b))}) == 16 * 64
    for bits in (128, 192, 256):
        assert _native.aes_public_plan(blocks, bits) == [16 * 64] * NR[bits]
        assert rule(blocks, NR[bits])[0] == [16 * 64] * NR[bits]
    iid = [int.from_bytes(rng.bytes(16), "big") for _ in range(64)]
    distinct = len({(p, v) for b in iid for p, v in enumerate(u128_to_bytes(b))})
    assert distinct < 16 * 64
    assert _native.aes_public_plan(iid) == rule(iid, 10)[0] == [distinct] + [16 * 64] * 9


def test_plan_takes_bytes_and_ints_alike_and_wraps_nothing():
    blocks = counters(MASK128 - 1, 4)                                    # ..FE, ..FF, 0, 1
    assert _native.aes_public_plan([b.to_bytes(16, "big") for b in blocks]) == _native.aes_public_plan(blocks) == rule(blocks, 10)[0]
    assert _native.aes_public_plan([], 192) == [0] * 12


def test_plan_rejects_bad_key_bits_and_null_pointers():
    lib = _native.load_library()
    blocks = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    out = (ctypes.c_uint64 * 14)()
    assert lib.fheaes_aes_public_plan(blocks, 2, 128, out) == 0
    for bits in (100, 0, 64, 129):
        assert lib.fheaes_aes_public_plan(blocks, 2, bits, out) == -1
    assert lib.fheaes_aes_public_plan(None, 2, 128, out) == -1
    assert lib.fheaes_aes_public_plan(blocks, 2, 128, None) == -1
    with pytest.raises(_native.FheAesError):
        _native.aes_public_plan([1, 2], 100)
    with pytest.raises(ValueError):
        _native.aes_public_plan([1 << 128])
    with pytest.raises(ValueError):
        _native.aes_public_plan([bytes(15)])


def test_public_entry_points_reject_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        for bits in (128, 192, 256, 100):
            assert lib.fheaes_aes_encrypt_public_bits(None, buf, bits, buf, 1, buf, ms) == -1
            assert lib.fheaes_aes_ctr_bits(None, buf, bits, buf, 0, None, 1, buf, ms) == -1


# ---- 2. the clear keystream ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_ctr_keystream_sp800_38a_f5(bits):
    key, first, last = F5[bits]
    ks = aes_clear.ctr_keystream(key, F5_CTR, 0, 4)
    ct = [k ^ p for k, p in zip(ks, F1_PT)]
    assert ct[0] == first and ct[3] == last
    assert ks == [aes_clear.aes_encrypt_block(key, F5_CTR + i) for i in range(4)]
    assert aes_clear.ctr_keystream(key, F5_CTR, 2, 2) == ks[2:]               # first_block continues the stream
    assert aes_clear.ctr_keystream(key, F5_CTR - 5, 5, 4) == ks


def test_ctr_keystream_wraps_mod_2_128():
    ks = aes_clear.ctr_keystream(F1_KEY, MASK128 - 1, 0, 4)
    assert ks == [aes_clear.aes_encrypt_block(F1_KEY, v) for v in (MASK128 - 1, MASK128, 0, 1)]
    assert aes_clear.ctr_keystream(F1_KEY, MASK128, 1, 1) == [aes_clear.aes_encrypt_block(F1_KEY, 0)]
    assert aes_clear.ctr_keystream(F1_KEY, 0, 0, 0) == []


# ---- 3. the shared schedule on the CPU oracle ------------------------------------------------------------------------------------------
def test_trivial_bytes_are_mask_zero_body_bit(toy):
    c = own_client(toy)
    t = c.trivial_bytes([[0x00, 0xA5], [0xFF, 0x01]])
    assert t.shape == (2, 2, 8, toy.params.big1) and t.dtype == np.uint64
    assert not t[..., :-1].any()
    assert np.array_equal(t[..., -1] >> np.uint64(63), [[[0] * 8, [1, 0, 1, 0, 0, 1, 0, 1]], [[1] * 8, [1, 0, 0, 0, 0, 0, 0, 0]]])
    assert not (t[..., -1] & np.uint64((1 << 63) - 1)).any()
    assert np.array_equal(c.decrypt_bytes(t), [[0x00, 0xA5], [0xFF, 0x01]])


def test_shared_schedule_is_the_oracles_aes_encrypt_on_trivial_bytes(toy):
    c = own_client(toy)
    model = AesModel(toy.oracle)
    rk = toy.oracle.aes_key_expansion(c.encrypt_u128(c.key))
    blocks = counters(BASE | 0xFE, 3)                                        # ..FE, ..FF, then the low byte wraps into the next
    trivial = c.trivial_bytes([u128_to_bytes(b) for b in blocks])
    got, evaluated = shared_encrypt(model, rk, trivial, blocks)
    assert evaluated == sum(_native.aes_public_plan(blocks)) < 16 * 3 * 10
    for i, b in enumerate(blocks):
        want = toy.oracle.aes_encrypt(rk, trivial[i])
        assert np.array_equal(got[i], want), "block %d differs in %d words" % (i, int((got[i] != want).sum()))
        assert c.decrypt_u128(got[i]) == aes_clear.aes_encrypt_block(c.key, b)
