"""The public-ciphertext modes on the MI355X: public blocks through the equivalent inverse cipher (fheaes_aes_decrypt_public_*), CBC and
CFB-128 decryption, and CTR with the 32-bit counter of GCM.  The reference of every word is an entry point the parent already has --
Server.aes_decrypt_equivalent / aes_encrypt_public on Client.trivial_bytes of the same blocks -- so every comparison is array_equal;
plaintexts are SP 800-38A F.2 / F.3 and SP 800-38D test case 3 (public_modes.py)."""
from fractions import Fraction

import numpy as np
import pytest

import chunk_seams as cs
from aes_vectors import BASE, F1_PT, MASK128, NR, block_bytes, counters
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from public_modes import CBC, CFB128, GCM_IV, GCM_J0, GCM_KEY, GCM_PT, IV, cbc_ct, cfb128_encrypt, inc32, rule_dec
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

BITS = [128, 192, 256]
CASES = {
    "cbc4": None,                                                         # the F.2.x ciphertext blocks of the key size
    "pairs": None,                                                        # C0, C1, C0, C1: duplicates stay shared through every round
    "consecutive7": counters(BASE, 7),
    "single": [0x3243F6A8885A308D313198A2E0370734],
}


def _blocks(case, bits):
    ct = cbc_ct(bits)
    return {"cbc4": ct, "pairs": [ct[0], ct[1], ct[0], ct[1]]}.get(case) or CASES[case]


def _trivial(c, blocks):
    return c.trivial_bytes([u128_to_bytes(b) for b in blocks])


def _bytes(blocks):
    return b"".join(b.to_bytes(16, "big") for b in blocks)


@pytest.fixture(scope="module")
def toy_keys(toy_server, tc):
    """round keys and decryption round keys of the three SP 800-38A keys, expanded and converted on the GPU"""
    rk = {bits: toy_server.aes_key_expansion(tc.encrypt_aes_key(CBC[bits][0])) for bits in BITS}
    return {bits: (rk[bits], toy_server.aes_decryption_round_keys(rk[bits])) for bits in BITS}


@pytest.fixture(scope="module")
def three_keys(toy_server, tc):
    """three AES-128 keys: round keys, decryption round keys, their packed store and what unpacking it gives"""
    rng = np.random.default_rng(0xCBC3)
    keys = [CBC[128][0], rng.bytes(16), rng.bytes(16)]
    rk = toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in keys]))
    dw = toy_server.aes_decryption_round_keys_many(rk)
    pdw = toy_server.pack_round_keys(dw)
    return dict(keys=keys, rk=rk, dw=dw, pdw=pdw, udw=toy_server.unpack_round_keys(pdw))


# ---- word equality, the inverse direction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("bits", BITS)
def test_toy_public_blocks_are_aes_decrypt_equivalent_on_trivial_bytes(toy, toy_server, toy_keys, tc, bits, case):
    blocks, dw = _blocks(case, bits), toy_keys[bits][1]
    got = toy_server.aes_decrypt_public(dw, blocks)
    assert got.shape == (len(blocks), 16, 8, toy.params.big1) and got.dtype == np.uint64
    want = toy_server.aes_decrypt_equivalent(dw, _trivial(tc, blocks))
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    key = CBC[bits][0]
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes([aes_clear.aes_decrypt_block(key, b) for b in blocks]))
    assert np.array_equal(toy_server.aes_decrypt_public(dw, [b.to_bytes(16, "big") for b in blocks]), got)
    data = [(F1_PT[i % 4] + i) & MASK128 for i in range(len(blocks))]
    with_data = toy_server.aes_decrypt_public(dw, blocks, data=_bytes(data))
    assert np.array_equal(with_data, want + _trivial(tc, data))


# ---- word equality, the modes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_toy_cbc_is_public_decryption_plus_the_chaining_blocks(toy, toy_server, toy_keys, tc, bits):
    dw, ct = toy_keys[bits][1], cbc_ct(bits)
    got = toy_server.aes_cbc_decrypt(dw, IV, ct)
    assert np.array_equal(got, toy_server.aes_decrypt_public(dw, ct, data=[IV] + ct[:3]))
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(F1_PT))
    # the previous ciphertext block continues the stream; iv as bytes, the ciphertext as one bytes object
    tail = toy_server.aes_cbc_decrypt(dw, ct[1].to_bytes(16, "big"), _bytes(ct[2:]))
    assert np.array_equal(tail, got[2:])


def test_toy_cfb_is_public_encryption_of_the_shifted_ciphertext(toy, toy_server, toy_keys, tc):
    key, first, last = CFB128
    rk = toy_keys[128][0]
    ct = cfb128_encrypt(key, IV, F1_PT)
    assert ct[0] == first and ct[3] == last
    got = toy_server.aes_cfb_decrypt(rk, IV, _bytes(ct))
    assert np.array_equal(got, toy_server.aes_encrypt_public_keyed(rk[None], [0] * 4, [IV] + ct[:3], data=ct))
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(F1_PT))
    assert np.array_equal(toy_server.aes_cfb_decrypt(rk, ct[0], ct[1:]), got[1:])


@pytest.mark.parametrize("bits", BITS)
def test_toy_ctr32_is_public_encryption_of_the_inc32_counter_blocks(toy, toy_server, toy_keys, tc, bits):
    key, rk = CBC[bits][0], toy_keys[bits][0]
    icb = (BASE >> 32 << 32) | 0xFFFFFFFD                                    # the counter wraps mod 2^32 inside the batch
    blocks = [inc32(icb, i) for i in range(5)]
    assert blocks[3] == icb >> 32 << 32 and counters(icb, 5)[3] == blocks[3] + (1 << 32)
    stream = toy_server.aes_ctr(rk, icb, 0, 5, counter_bits=32)
    assert np.array_equal(stream, toy_server.aes_encrypt_public(rk, blocks))
    assert not np.array_equal(stream[3], toy_server.aes_ctr(rk, icb, 0, 5)[3])                   # the 128-bit counter carries on
    data = F1_PT + [MASK128]
    ct = toy_server.aes_ctr(rk, icb, 0, 5, data=data, counter_bits=32)
    assert np.array_equal(ct, stream + _trivial(tc, data))
    want = [k ^ d for k, d in zip(aes_clear.ctr_keystream(key, icb, 0, 5, counter_bits=32), data)]
    assert np.array_equal(tc.decrypt_bytes(ct), block_bytes(want))
    # first_block continues the stream, across the wrap
    assert np.array_equal(toy_server.aes_ctr(rk, icb.to_bytes(16, "big"), 2, 3, data=_bytes(data[2:]), counter_bits=32), ct[2:])
    assert np.array_equal(toy_server.aes_ctr(rk, inc32(icb, -7), 7, 5, counter_bits=32), stream)
    assert np.array_equal(toy_server.aes_ctr_streams(rk[None], [(0, icb, 0, 2, None), (0, icb, 2, 3, None)], counter_bits=32), stream)


def test_toy_gcm_ctr_sp800_38d_test_case_3(toy, toy_server, tc):
    rk = toy_server.aes_key_expansion(tc.encrypt_aes_key(GCM_KEY))
    ct = [k ^ p for k, p in zip(aes_clear.gcm_keystream(GCM_KEY, GCM_IV, 0, 4), GCM_PT)]
    got = toy_server.aes_gcm_ctr(rk, GCM_IV, data=_bytes(ct))                # decryption: the ciphertext is the data
    want = toy_server.aes_encrypt_public(rk, [GCM_J0 + 1 + i for i in range(4)]) + _trivial(tc, ct)
    assert np.array_equal(got, want)
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(GCM_PT))
    assert np.array_equal(toy_server.aes_gcm_ctr(rk, GCM_IV, data=ct[2:], first_block=2), got[2:])
    ks = toy_server.aes_gcm_ctr(rk, GCM_IV, n_blocks=2)
    assert np.array_equal(tc.decrypt_bytes(ks), block_bytes(aes_clear.gcm_keystream(GCM_KEY, GCM_IV, 0, 2)))


# ---- variants ---------------------------------------------------------------------------------------------------------------------------------
def _streams():
    """(key index, iv, ciphertext): F.2.2 under key 0, two random blocks under key 2, the first three of F.2.2 again under key 1"""
    cts = [cbc_ct(128), [int.from_bytes(np.random.default_rng(7 + i).bytes(16), "big") for i in range(2)], cbc_ct(128)[:3]]
    return [(0, IV, cts[0]), (2, IV + 1, cts[1]), (1, IV, cts[2])]


def test_toy_cbc_streams_over_three_keys_are_the_single_key_calls(toy, toy_server, three_keys, tc):
    k = three_keys
    streams = _streams()
    got = toy_server.aes_cbc_streams(k["dw"], streams)
    want = np.concatenate([toy_server.aes_cbc_decrypt(k["dw"][key], iv, ct) for key, iv, ct in streams])
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    clear = sum((aes_clear.cbc_decrypt(k["keys"][key], iv, ct) for key, iv, ct in streams), [])
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(clear))
    assert clear[:4] == F1_PT
    kob = sum(([key] * len(ct) for key, _, ct in streams), [])
    blocks = sum((ct for _, _, ct in streams), [])
    plan = _native.aes_decrypt_public_plan_keyed(blocks, kob, 3)
    assert plan == rule_dec(blocks, 10, kob)[0] and plan[1:] == [16 * 9] * 9     # the two F.2.2 streams share nothing: other keys
    keyed = toy_server.aes_decrypt_public_keyed(k["dw"], kob, blocks)
    ref = _trivial(tc, blocks)
    toy_server.aes_decrypt_equivalent_keyed(k["dw"], kob, ref)
    assert np.array_equal(keyed, ref)


def test_toy_packed_round_keys_give_the_words_of_the_unpacked_store(toy, toy_server, three_keys, tc):
    k = three_keys
    streams = _streams()
    got = toy_server.aes_cbc_streams(k["pdw"], streams)
    assert np.array_equal(got, toy_server.aes_cbc_streams(k["udw"], streams))
    clear = sum((aes_clear.cbc_decrypt(k["keys"][key], iv, ct) for key, iv, ct in streams), [])
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(clear))
    one = toy_server.aes_cbc_decrypt(k["pdw"][1], IV, streams[2][2])
    assert np.array_equal(one, toy_server.aes_cbc_decrypt(k["udw"][1], IV, streams[2][2]))
    assert np.array_equal(toy_server.aes_decrypt_public(k["pdw"][0], cbc_ct(128)), toy_server.aes_decrypt_public(k["udw"][0], cbc_ct(128)))
    prk = toy_server.pack_round_keys(k["rk"][0])
    ct = cfb128_encrypt(k["keys"][0], IV, F1_PT)
    cfb = toy_server.aes_cfb_decrypt(prk, IV, ct)
    assert np.array_equal(cfb, toy_server.aes_cfb_decrypt(toy_server.unpack_round_keys(prk)[0], IV, ct))
    assert np.array_equal(tc.decrypt_bytes(cfb), block_bytes(F1_PT))
    icb = GCM_J0 | 0xFFFFFFFF
    assert np.array_equal(toy_server.aes_ctr(prk, icb, 0, 3, counter_bits=32),
                          toy_server.aes_ctr(toy_server.unpack_round_keys(prk)[0], icb, 0, 3, counter_bits=32))


def test_toy_host_arrays_and_resident_tensors_agree(toy, toy_server, toy_keys, three_keys, tc):
    rk, dw = toy_keys[192]
    ct = cbc_ct(192)
    icb = BASE | 0xFFFFFFFE
    want = (toy_server.aes_cbc_decrypt(dw, IV, ct), toy_server.aes_decrypt_public(dw, ct[:3]), toy_server.aes_cfb_decrypt(rk, IV, ct),
            toy_server.aes_ctr(rk, icb, 1, 4, data=F1_PT, counter_bits=32), toy_server.aes_cbc_streams(three_keys["dw"], _streams()),
            toy_server.aes_cbc_streams(three_keys["pdw"], _streams()))
    d_rk, d_dw, d_dw3 = dev(rk), dev(dw), dev(three_keys["dw"])
    d_pdw = toy_server.pack_round_keys(d_dw3)
    got = (toy_server.aes_cbc_decrypt(d_dw, IV, ct), toy_server.aes_decrypt_public(d_dw, ct[:3]), toy_server.aes_cfb_decrypt(d_rk, IV, ct),
           toy_server.aes_ctr(d_rk, icb, 1, 4, data=F1_PT, counter_bits=32), toy_server.aes_cbc_streams(d_dw3, _streams()),
           toy_server.aes_cbc_streams(d_pdw, _streams()))
    toy_server.synchronize()
    for g, w in zip(got, want):
        assert g.is_cuda and tuple(g.shape) == w.shape
        assert np.array_equal(host(g), w)


def test_toy_server_group_shards_inside_the_message(toy, toy_server, toy_keys, three_keys, tc):
    rk, dw = toy_keys[128]
    ct = cbc_ct(128) + cbc_ct(128)[:1]                                        # 5 blocks on 2 contexts: the boundary is inside the message
    cfb = cfb128_encrypt(CBC[128][0], IV, F1_PT + F1_PT[:1])
    icb = BASE | 0xFFFFFFFE
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        assert np.array_equal(group.aes_cbc_decrypt(dw, IV, ct), toy_server.aes_cbc_decrypt(dw, IV, ct))
        assert np.array_equal(group.aes_decrypt_public(dw, ct, data=F1_PT + [7]), toy_server.aes_decrypt_public(dw, ct, data=F1_PT + [7]))
        assert np.array_equal(group.aes_cfb_decrypt(rk, IV, cfb), toy_server.aes_cfb_decrypt(rk, IV, cfb))
        assert np.array_equal(group.aes_ctr(rk, icb, 0, 5, data=F1_PT + [7], counter_bits=32),
                              toy_server.aes_ctr(rk, icb, 0, 5, data=F1_PT + [7], counter_bits=32))
        assert np.array_equal(group.aes_gcm_ctr(rk, GCM_IV, n_blocks=5, first_block=3), toy_server.aes_gcm_ctr(rk, GCM_IV, n_blocks=5, first_block=3))
        streams = _streams()                                        # 4 + 2 + 3 blocks: the boundary is inside the first stream
        assert np.array_equal(group.aes_cbc_streams(three_keys["dw"], streams), toy_server.aes_cbc_streams(three_keys["dw"], streams))
        assert np.array_equal(group.aes_cbc_streams(three_keys["pdw"], streams), toy_server.aes_cbc_streams(three_keys["pdw"], streams))
    finally:
        for s in group.servers:
            s.engine.close()
    assert np.array_equal(tc.decrypt_bytes(toy_server.aes_cbc_decrypt(dw, IV, ct)), block_bytes(F1_PT + [aes_clear.aes_decrypt_block(CBC[128][0], ct[0]) ^ ct[3]]))


# ---- work done and noise ------------------------------------------------------------------------------------------------------------------------
def test_toy_work_done_is_the_plan_and_the_noise_level_is_five(toy, tc):
    """the blind-rotation units of a call against those of aes_decrypt_equivalent on as many blocks are sum(plan) / (16 n Nr), exactly"""
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        for bits, case in ((128, "consecutive7"), (256, "pairs"), (192, "cbc4"), (128, "pairs")):
            blocks = _blocks(case, bits)
            dw = srv.aes_decryption_round_keys(srv.aes_key_expansion(tc.encrypt_aes_key(CBC[bits][0])))
            n, plan = len(blocks), _native.aes_decrypt_public_plan(blocks, bits)
            srv.engine.profile_enable(True)
            srv.engine.profile_reset()
            srv.aes_decrypt_equivalent(dw, _trivial(tc, blocks))
            full = srv.engine.profile_read()["blind_rotate"]["units"]
            srv.engine.profile_reset()
            if case == "cbc4":
                srv.aes_cbc_decrypt(dw, IV, blocks)
            else:
                srv.aes_decrypt_public(dw, blocks)
            shared = srv.engine.profile_read()["blind_rotate"]["units"]
            srv.engine.profile_enable(False)
            assert full > 0 and shared > 0
            assert Fraction(shared, full) == Fraction(sum(plan), 16 * n * NR[bits]), (bits, plan, shared, full)
    finally:
        srv.engine.close()
    srv = Server(toy.keys, device=0)
    try:
        srv.aes_cbc_decrypt(dw, IV, cbc_ct(128)[:3])
        assert srv.engine.noise_level_seen() == (5, 5)                        # 4 WoPBS outputs + 1 round key, as aes_decrypt_equivalent
    finally:
        srv.engine.close()


# ---- the chunk seam -------------------------------------------------------------------------------------------------------------------------------
def test_public_decryption_with_pools_above_one_chunk(toy, tc):
    """300 random blocks share nothing from round 2 on: pools of 4,800 bytes, 38,400 bits, two chunks per WoPBS, FOUR outputs per pool
    entry in the workspace and an indexed gather of four terms over more than 4,096 pool entries (test_gpu_chunk_seams.py has the
    encryption direction with three).  The round keys are encrypted byte by byte from the clear ones, as there."""
    p, n = toy.params, cs.PUBLIC_BLOCKS
    rng = np.random.default_rng(0xE14)
    key = rng.bytes(16)
    blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    chain = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    clear_dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))
    dw = tc.encrypt_bytes(np.array(clear_dw, dtype=np.uint8).reshape(-1)).reshape(11, 16, 8, -1)
    plan = _native.aes_decrypt_public_plan(blocks)
    first = cs.public_pool_round_1(blocks)
    assert plan == [first] + [16 * n] * 9 and first <= 4096
    srv = Server(toy.keys, device=0)
    try:
        d_dw = dev(dw)
        buf, rows = guarded(n * 128, p.big1)
        srv.engine.profile_reset()
        srv.aes_decrypt_public(d_dw, blocks, data=chain, out=rows.view(n, 16, 8, p.big1))
        srv.synchronize()
        prof = srv.engine.profile_read()
        for stage in ("keyswitch", "blind_rotate"):                          # one chunk for the pool of round 1, two for every later one
            assert (prof[stage]["launches"], prof[stage]["units"]) == (1 + 2 * 9, 8 * sum(plan)), "%s: %r" % (stage, prof[stage])
        assert prof["linear"]["launches"] == 11
        got = host(rows).reshape(n, 16, 8, p.big1)
        assert guards_intact(buf)
        for b in (0, 255, 256, n - 1):
            want = srv.aes_decrypt_public(dw, [blocks[b]], data=[chain[b]])[0]
            assert np.array_equal(got[b], want), "block %d: %d words differ" % (b, int((got[b] != want).sum()))
        assert [tc.decrypt_u128(got[b]) for b in range(n)] == [aes_clear.aes_decrypt_block(key, v) ^ d for v, d in zip(blocks, chain)]
    finally:
        srv.engine.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(toy, toy_server, toy_keys, three_keys, tc):
    p = toy.params
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    rk, dw = toy_keys[256]
    d_rk, d_dw, d_dw3 = dev(rk), dev(dw), dev(three_keys["dw"])
    d_pdw = toy_server.pack_round_keys(d_dw3)
    toy_server.synchronize()
    buf, rows = guarded(2 * 128, p.big1)
    out = rows.view(2, 16, 8, p.big1)
    pairs = _native.u128_pairs([1, 2])
    bp = pairs.ctypes.data_as(_native._u64p)
    kob = np.array([0, 3], dtype=np.uint32)
    kp = kob.ctypes.data_as(_native._u32p)
    D = _native.DEVICE
    # bad key_bits
    assert lib.fheaes_aes_decrypt_public_bits(h, d_dw.data_ptr(), 100, bp, None, 2, out.data_ptr(), D) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_cbc_decrypt_bits(h, d_dw.data_ptr(), 100, bp, bp, 2, out.data_ptr(), D) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_ctr32_bits(h, d_rk.data_ptr(), 100, bp, 0, None, 2, out.data_ptr(), D) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_decrypt_public_keyed(h, d_dw3.data_ptr(), 100, 3, kp, bp, None, 2, out.data_ptr(), D) == -1
    # a key index >= n_keys, n_keys out of range
    assert lib.fheaes_aes_decrypt_public_keyed(h, d_dw3.data_ptr(), 128, 3, kp, bp, None, 2, out.data_ptr(), D) == -1 and b"key_of_block" in lib.fheaes_last_error(h)
    assert lib.fheaes_aes_decrypt_public_keyed_packed(h, d_pdw.data.data_ptr(), 128, 3, kp, bp, None, 2, out.data_ptr(), D) == -1
    assert lib.fheaes_aes_decrypt_public_keyed(h, d_dw3.data_ptr(), 128, 0, kp, bp, None, 2, out.data_ptr(), D) == -1
    assert lib.fheaes_aes_decrypt_public_keyed(h, d_dw3.data_ptr(), 128, 65537, kp, bp, None, 2, out.data_ptr(), D) == -1
    # null pointers; n_blocks = 0 is fine and writes nothing
    assert lib.fheaes_aes_decrypt_public_bits(h, None, 256, bp, None, 2, out.data_ptr(), D) == -1
    assert lib.fheaes_aes_decrypt_public_bits(h, d_dw.data_ptr(), 256, None, None, 2, out.data_ptr(), D) == -1
    assert lib.fheaes_aes_cbc_decrypt_bits(h, d_dw.data_ptr(), 256, None, bp, 2, out.data_ptr(), D) == -1
    assert lib.fheaes_aes_cbc_decrypt_bits(h, d_dw.data_ptr(), 256, bp, bp, 2, None, D) == -1
    assert lib.fheaes_aes_decrypt_public_bits(h, d_dw.data_ptr(), 256, bp, None, 0, out.data_ptr(), D) == 0
    assert lib.fheaes_aes_cbc_decrypt_bits(h, d_dw.data_ptr(), 256, bp, bp, 0, out.data_ptr(), D) == 0
    assert lib.fheaes_aes_ctr32_bits(h, d_rk.data_ptr(), 256, bp, 0, None, 0, out.data_ptr(), D) == 0
    # what never reaches the library
    for call in (lambda: toy_server.aes_ctr(d_rk, 1, 0, 2, out=out, counter_bits=64),
                 lambda: toy_server.aes_ctr_streams(d_rk[None], [(0, 1, 0, 2, None)], out=out, counter_bits=64),
                 lambda: toy_server.aes_gcm_ctr(d_rk, bytes(8), n_blocks=2, out=out),
                 lambda: toy_server.aes_gcm_ctr(d_rk, bytes(16), n_blocks=2, out=out),
                 lambda: toy_server.aes_gcm_ctr(d_rk, GCM_IV, data=bytes(31), out=out),
                 lambda: toy_server.aes_gcm_ctr(d_rk, GCM_IV, data=bytes(48), n_blocks=2, out=out),
                 lambda: toy_server.aes_decrypt_public(d_dw, [1, 2], data=[1], out=out),
                 lambda: toy_server.aes_decrypt_public(d_dw, [1, 2], data=bytes(31), out=out),
                 lambda: toy_server.aes_cbc_decrypt(d_dw, IV, bytes(31), out=out),
                 lambda: toy_server.aes_cbc_decrypt(d_dw, 1 << 128, [1, 2], out=out),
                 lambda: toy_server.aes_cfb_decrypt(d_rk, IV, bytes(33), out=out),
                 lambda: toy_server.aes_decrypt_public_keyed(d_dw3, [0], [1, 2], out=out),
                 lambda: toy_server.aes_decrypt_public(d_dw3, [1, 2], out=out),
                 lambda: toy_server.aes_cbc_decrypt(d_dw, IV, [1, 2, 3], out=out)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="GHASH"):
        toy_server.aes_gcm_ctr(d_rk, bytes(8), n_blocks=2, out=out)
    with pytest.raises(_native.FheAesError) as e:
        toy_server.aes_decrypt_public_keyed(d_dw3, [0, 3], [1, 2], out=out)
    assert e.value.code == -1
    with pytest.raises(_native.FheAesError) as e:
        toy_server.aes_cbc_streams(d_dw3, [(0, IV, [1]), (3, IV, [2])], out=out)
    assert e.value.code == -1
    toy_server.synchronize()
    assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
    assert toy_server.aes_decrypt_public(dw, []).shape == (0, 16, 8, p.big1)
    assert toy_server.aes_cbc_decrypt(dw, IV, b"").shape == (0, 16, 8, p.big1)
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_cbc_decrypt_bits(dw, 256, IV, [1], np.empty((1, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


# ---- PARAM_OPT --------------------------------------------------------------------------------------------------------------------------------------
def test_param_opt_cbc_f22_and_gcm_test_case_3_end_to_end(opt, opt_server, opt_rk128, oc):
    """SP 800-38A F.2.2: the resident round keys of the F.1 key converted on the GPU, aes_cbc_decrypt of the four NIST ciphertext blocks, the
    client decrypts the NIST plaintext.  SP 800-38D test case 3: its key expanded on the GPU, the first two ciphertext blocks through
    aes_gcm_ctr."""
    d_dw = opt_server.aes_decryption_round_keys(opt_rk128)
    ct = cbc_ct(128)
    assert ct[0] == CBC[128][1] and ct[3] == CBC[128][2]
    d_pt = opt_server.aes_cbc_decrypt(d_dw, IV, ct)
    d_gk = opt_server.aes_key_expansion(dev(oc.encrypt_aes_key(GCM_KEY)))
    gct = [k ^ p for k, p in zip(aes_clear.gcm_keystream(GCM_KEY, GCM_IV, 0, 2), GCM_PT)]
    assert gct[0] == 0x42831EC2217774244B7221B784D0D49C
    d_gpt = opt_server.aes_gcm_ctr(d_gk, GCM_IV, data=gct)
    opt_server.synchronize()
    assert np.array_equal(oc.decrypt_bytes(host(d_pt)), block_bytes(F1_PT))
    assert np.array_equal(oc.decrypt_bytes(host(d_gpt)), block_bytes(GCM_PT[:2]))
