"""Many AES keys under one FHE key on the MI355X: the batched key expansion and round-key conversion, the keyed cipher calls, the keyed
public / CTR call and aes_ctr_streams.  The single-key entry points are the reference, key by key, so every comparison is array_equal
on the uint64 words; the clear AES of tfhe_aes_amd.aes_clear says that those words are also right."""
import numpy as np
import pytest

from aes_vectors import BASE, F1_PT, MASK128, NR, block_bytes, key_words, own_client
from gpu_support import dev, host, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

KOB = [0, 2, 1, 0, 2]                                   # 5 blocks over 3 keys
PTS = [BASE, 0, MASK128, 0x3243F6A8885A308D313198A2E0370734, BASE + 1]


def aes_keys(bits, n=3):
    """n distinct clear AES keys of `bits` bits"""
    rng = np.random.default_rng(0xA5 + bits)
    return [rng.bytes(bits // 8) for _ in range(n)]


@pytest.fixture(scope="module")
def toy_keys(toy_server, tc):
    """per key size: (clear keys, their encryptions [3][4 Nk][8][kN+1], the single-key expansions stacked, the single-key conversions stacked)"""
    out = {}
    for bits in (128, 192, 256):
        keys = aes_keys(bits)
        ek = np.stack([tc.encrypt_aes_key(k) for k in keys])
        rk = np.stack([toy_server.aes_key_expansion(ek[i]) for i in range(3)])
        dw = np.stack([toy_server.aes_decryption_round_keys(rk[i]) for i in range(3)])
        out[bits] = (keys, ek, rk, dw)
    return out


# ---- the two per-key calls -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_key_expansion_of_three_keys_is_three_single_expansions(toy, toy_server, toy_keys, tc, bits):
    keys, ek, rk, _ = toy_keys[bits]
    got = toy_server.aes_key_expansion_many(ek)
    assert got.shape == (3, NR[bits] + 1, 16, 8, toy.params.big1) and got.dtype == np.uint64
    for i in range(3):
        assert np.array_equal(got[i], rk[i]), "key %d: %d words differ" % (i, int((got[i] != rk[i]).sum()))
        assert np.array_equal(tc.decrypt_bytes(got[i]), key_words(aes_clear.expand_key(keys[i])))
    one = toy_server.aes_key_expansion_many(ek[1:2])
    assert one.shape == (1,) + rk[1].shape and np.array_equal(one[0], rk[1])


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_round_key_conversion_of_three_keys_is_three_single_conversions(toy, toy_server, toy_keys, tc, bits):
    keys, _, rk, dw = toy_keys[bits]
    got = toy_server.aes_decryption_round_keys_many(rk)
    assert got.shape == rk.shape
    for i in range(3):
        assert np.array_equal(got[i], dw[i]), "key %d: %d words differ" % (i, int((got[i] != dw[i]).sum()))
        assert np.array_equal(tc.decrypt_bytes(got[i]), key_words(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(keys[i]))))
    assert np.array_equal(toy_server.aes_decryption_round_keys_many(rk[2:3])[0], dw[2])


# ---- the keyed cipher calls ------------------------------------------------------------------------------------------------------------
def _per_key(single, sets, kob, state):
    """the single-key call on exactly the blocks of each key, put back in place"""
    want = np.empty_like(state)
    for j in sorted(set(kob)):
        idx = [b for b, k in enumerate(kob) if k == j]
        want[idx] = single(sets[j], np.ascontiguousarray(state[idx]))
    return want


@pytest.mark.parametrize("kob", [KOB, [1] * 5], ids=["three keys", "two keys unused"])
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_keyed_cipher_calls_are_the_single_key_calls_per_key(toy, toy_server, toy_keys, tc, bits, kob):
    keys, _, rk, dw = toy_keys[bits]
    st = np.stack([tc.encrypt_u128(v) for v in PTS])
    enc = toy_server.aes_encrypt_keyed(rk, kob, st.copy())
    want = _per_key(toy_server.aes_encrypt, rk, kob, st)
    assert np.array_equal(enc, want), "%d words differ" % int((enc != want).sum())
    assert [tc.decrypt_u128(enc[b]) for b in range(5)] == [aes_clear.aes_encrypt_block(keys[k], v) for k, v in zip(kob, PTS)]
    dec = toy_server.aes_decrypt_keyed(rk, kob, enc.copy())
    assert np.array_equal(dec, _per_key(toy_server.aes_decrypt, rk, kob, enc))
    assert [tc.decrypt_u128(dec[b]) for b in range(5)] == PTS
    eq = toy_server.aes_decrypt_equivalent_keyed(dw, kob, enc.copy())
    assert np.array_equal(eq, _per_key(toy_server.aes_decrypt_equivalent, dw, kob, enc))
    assert [tc.decrypt_u128(eq[b]) for b in range(5)] == PTS


# ---- public blocks / CTR ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kob,blocks", [([0, 0, 1, 1], [BASE, BASE + 1, BASE, BASE + 1]), ([0, 1, 1, 0], [BASE, BASE, BASE + 1, BASE + 1])],
                         ids=["grouped", "interleaved"])
def test_toy_public_keyed_is_aes_encrypt_public_per_key_and_does_the_planned_work(toy, tc, toy_keys, kob, blocks):
    keys, _, rk, _ = toy_keys[128]
    srv = Server(toy.keys, device=0)                                          # a context of its own: the profile counters are its
    try:
        srv.engine.profile_enable(True)
        srv.engine.profile_reset()
        got = srv.aes_encrypt_public_keyed(rk, kob, blocks)
        units = srv.engine.profile_read()["blind_rotate"]["units"]
        srv.engine.profile_enable(False)
        plan = _native.aes_public_plan_keyed(blocks, kob, 3, 128)
        assert plan == [34, 40] + [64] * 8
        assert units == 8 * sum(plan)
        want = np.empty_like(got)
        for j in (0, 1):
            idx = [b for b, k in enumerate(kob) if k == j]
            want[idx] = srv.aes_encrypt_public(rk[j], [blocks[b] for b in idx])
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        assert np.array_equal(tc.decrypt_bytes(got), block_bytes([aes_clear.aes_encrypt_block(keys[k], v) for k, v in zip(kob, blocks)]))
    finally:
        srv.engine.close()


STREAMS = [(0, BASE, 0, 3, None),                                             # two streams under key 0 with different IVs,
           (0, BASE ^ (0xA5 << 64), 1, 2, F1_PT[:2]),                         # one of them with data
           (2, BASE | 0xFE, 0, 3, None)]                                      # ..FE ..FF, then the low counter byte wraps


@pytest.mark.parametrize("bits", [128, 256])
def test_toy_ctr_streams_are_aes_ctr_per_stream(toy, toy_server, toy_keys, tc, bits):
    keys, _, rk, _ = toy_keys[bits]
    got = toy_server.aes_ctr_streams(rk, STREAMS)
    assert got.shape == (8, 16, 8, toy.params.big1)
    at = 0
    for k, iv, first, n, data in STREAMS:
        want = toy_server.aes_ctr(rk[k], iv, first, n, data=data)
        assert np.array_equal(got[at:at + n], want), "stream at block %d: %d words differ" % (at, int((got[at:at + n] != want).sum()))
        at += n
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(aes_clear.ctr_streams(keys, STREAMS)))


# ---- memory spaces ----------------------------------------------------------------------------------------------------------------------
def test_toy_host_arrays_and_resident_tensors_agree(toy, toy_server, toy_keys, tc):
    _, ek, rk, _ = toy_keys[192]
    st = np.stack([tc.encrypt_u128(v) for v in PTS])
    enc = toy_server.aes_encrypt_keyed(rk, KOB, st.copy())
    ctr = toy_server.aes_ctr_streams(rk, STREAMS)
    d_ek = dev(ek)                                                            # kept alive: the device calls are only enqueued
    d_rk = toy_server.aes_key_expansion_many(d_ek)
    d_enc = dev(st)
    toy_server.aes_encrypt_keyed(d_rk, KOB, d_enc)
    d_ctr = toy_server.aes_ctr_streams(d_rk, STREAMS)
    toy_server.synchronize()
    assert d_rk.is_cuda and tuple(d_rk.shape) == rk.shape
    assert np.array_equal(host(d_rk), rk)
    assert np.array_equal(host(d_enc), enc)
    assert np.array_equal(host(d_ctr), ctr)
    with pytest.raises(ValueError):
        toy_server.aes_encrypt_keyed(rk, KOB, d_enc)                          # mixed memory spaces are refused


# ---- several contexts -------------------------------------------------------------------------------------------------------------------
def test_toy_server_group_shards_blocks_and_keys(toy, toy_server, toy_keys, tc):
    _, ek, rk, _ = toy_keys[128]
    st = np.stack([tc.encrypt_u128(v) for v in PTS[:4]])
    kob = [0, 1, 1, 0]
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        assert np.array_equal(group.aes_encrypt_keyed(rk[:2], kob, st.copy()), toy_server.aes_encrypt_keyed(rk[:2], kob, st.copy()))
        assert np.array_equal(group.aes_key_expansion_many(ek[:2]), rk[:2])
    finally:
        for s in group.servers:
            s.engine.close()


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_working(toy, toy_server, toy_keys, tc):
    p = toy.params
    _, ek, rk, dw = toy_keys[128]
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    st = np.stack([tc.encrypt_u128(v) for v in PTS[:2]])
    before = st.copy()
    u32 = lambda *v: (np.array(v, dtype=np.uint32).ctypes.data_as(_native._u32p))
    blocks = _native.u128_pairs([1, 2]).ctypes.data_as(_native._u64p)
    out = np.empty((3,) + rk.shape[1:], dtype=np.uint64)
    for ms in (_native.HOST, _native.DEVICE):
        for fn in (lib.fheaes_aes_encrypt_keyed, lib.fheaes_aes_decrypt_keyed, lib.fheaes_aes_decrypt_equivalent_keyed):
            assert fn(h, rk.ctypes.data, 128, 3, u32(0, 3), st.ctypes.data, 2, ms) == -1                # key index 3 of 3 keys
            assert b"key_of_block[1] = 3" in lib.fheaes_last_error(h)
            assert fn(h, rk.ctypes.data, 128, 0, u32(0, 0), st.ctypes.data, 2, ms) == -1                # n_keys = 0
            assert b"n_keys" in lib.fheaes_last_error(h)
            assert fn(h, rk.ctypes.data, 128, 65537, u32(0, 0), st.ctypes.data, 2, ms) == -1
            assert fn(h, rk.ctypes.data, 100, 3, u32(0, 0), st.ctypes.data, 2, ms) == -1
            assert fn(h, rk.ctypes.data, 128, 3, None, st.ctypes.data, 2, ms) == -1
            assert fn(h, rk.ctypes.data, 128, 3, u32(0), st.ctypes.data, 0, ms) == 0                    # no blocks: nothing to do
        assert lib.fheaes_aes_public_keyed(h, rk.ctypes.data, 128, 3, u32(0, 3), blocks, None, 2, st.ctypes.data, ms) == -1
        assert lib.fheaes_aes_public_keyed(h, rk.ctypes.data, 128, 0, u32(0, 0), blocks, None, 2, st.ctypes.data, ms) == -1
        assert lib.fheaes_aes_public_keyed(h, rk.ctypes.data, 128, 3, u32(0), blocks, None, 0, st.ctypes.data, ms) == 0
        assert lib.fheaes_aes_key_expansion_batch(h, ek.ctypes.data, 128, 0, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_decryption_round_keys_batch(h, rk.ctypes.data, 128, 0, out.ctypes.data, ms) == -1
        # overlapping buffers: the conversion is not in place (slice 1 onward of the input as the output)
        assert lib.fheaes_aes_decryption_round_keys_batch(h, rk.ctypes.data, 128, 2, rk[1:].ctypes.data, ms) == -1
        assert b"overlap" in lib.fheaes_last_error(h)
    assert np.array_equal(st, before)
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        for call in (lambda: fresh.aes_key_expansion_batch(ek, 128, 3, out), lambda: fresh.aes_decryption_round_keys_batch(rk, 128, 3, out),
                     lambda: fresh.aes_encrypt_keyed(rk, 128, 3, [0, 1], st, 2), lambda: fresh.aes_decrypt_keyed(rk, 128, 3, [0, 1], st, 2),
                     lambda: fresh.aes_decrypt_equivalent_keyed(dw, 128, 3, [0, 1], st, 2),
                     lambda: fresh.aes_public_keyed(rk, 128, 3, [0, 1], [1, 2], None, st)):
            with pytest.raises(_native.FheAesError) as e:
                call()
            assert e.value.code == -2
    finally:
        fresh.close()
    # what never reaches the library: a round-key array that is not [n_keys][Nr+1][16][8][kN+1], one key index per block
    for call in (lambda: toy_server.aes_encrypt_keyed(rk[0], [0, 0], st), lambda: toy_server.aes_encrypt_keyed(rk[:, :10], [0, 0], st),
                 lambda: toy_server.aes_encrypt_keyed(rk, [0], st), lambda: toy_server.aes_encrypt_keyed(rk, [0, 0], st[0]),
                 lambda: toy_server.aes_key_expansion_many(ek[0]), lambda: toy_server.aes_decryption_round_keys_many(rk[0]),
                 lambda: toy_server.aes_encrypt_public_keyed(rk, [0], [1, 2]), lambda: toy_server.aes_ctr_streams(rk, [(0, 1, 0, 2, [1])])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_native.FheAesError) as e:
        toy_server.aes_encrypt_keyed(rk, [0, 3], st)
    assert e.value.code == -1
    # the context works afterwards
    got = toy_server.aes_encrypt_keyed(rk, [2, 1], st.copy())
    assert np.array_equal(got[0], toy_server.aes_encrypt(rk[2], st[0].copy())) and np.array_equal(got[1], toy_server.aes_encrypt(rk[1], st[1].copy()))


# ---- PARAM_OPT: the batches cross a kernel-form boundary -------------------------------------------------------------------------------
def test_param_opt_two_keys_three_blocks(opt):
    """2 AES-128 keys expanded in one batch (64-bit WoPBS steps against the 32-bit ones of the single call), then 3 blocks under keys
    [0, 1, 0]: 384 bits a round, the 16-form, against the per-key calls' 256 and 128 bits, the latency form -- the same words"""
    oc = own_client(opt)
    srv = Server(opt.keys, device=0, engine=opt.engine())
    keys = aes_keys(128, 2)
    ek = np.stack([oc.encrypt_aes_key(k) for k in keys])
    rk = srv.aes_key_expansion_many(ek)
    for i in range(2):
        assert np.array_equal(rk[i], srv.aes_key_expansion(ek[i])), "key %d" % i
    kob, pts = [0, 1, 0], PTS[:3]
    assert srv.engine.k2_plan(3 * 128)["form"] == 1 and srv.engine.k2_plan(2 * 128)["form"] == 0
    st = np.stack([oc.encrypt_u128(v) for v in pts])
    enc = srv.aes_encrypt_keyed(rk, kob, st.copy())
    want = _per_key(srv.aes_encrypt, rk, kob, st)
    assert np.array_equal(enc, want), "%d words differ" % int((enc != want).sum())
    assert [oc.decrypt_u128(enc[b]) for b in range(3)] == [aes_clear.aes_encrypt_block(keys[k], v) for k, v in zip(kob, pts)]
