"""Packed round keys on the MI355X: fheaes_pack_round_keys / fheaes_unpack_round_keys and the four *_keyed_packed calls.  The contract is
"no new arithmetic, only where the key word comes from differs", so every comparison is array_equal on the uint64 words against entry
points that existed before: pack / unpack for the store, the keyed calls on the unpacked store for the ciphers.  The clear AES of
tfhe_aes_amd.aes_clear says that those words are also right."""
import numpy as np
import pytest

from aes_model import noise
from aes_vectors import F5, NR, block_bytes
from gpu_support import dev, guarded, guards_intact, host, oc, opt_rk128, opt_server, settled, tc, toy_server  # noqa: F401
from packed_key_model import KOB, PTS, PUBLIC_CASES, STREAMS, aes_keys, key_glwes
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import PackedRoundKeys
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

OFF = _native.AES_WINDOW_OFF


@pytest.fixture(scope="module")
def toy_keys(toy_server, tc):
    """per key size: clear keys, round keys and decryption round keys of 3 keys, both packed, and both stores unpacked again"""
    out = {}
    for bits in (128, 192, 256):
        keys = aes_keys(bits)
        rk = toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in keys]))
        dw = toy_server.aes_decryption_round_keys_many(rk)
        prk, pdw = toy_server.pack_round_keys(rk), toy_server.pack_round_keys(dw)
        out[bits] = dict(keys=keys, rk=rk, dw=dw, prk=prk, pdw=pdw, urk=toy_server.unpack_round_keys(prk), udw=toy_server.unpack_round_keys(pdw))
    return out


# ---- 1. the store ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_store_is_pack_of_each_key_and_unpacks_to_its_extraction(toy, toy_server, toy_keys, tc, bits):
    p, k = toy.params, toy_keys[bits]
    rk, prk, urk = k["rk"], k["prk"], k["urk"]
    G, gw, m = key_glwes(p, bits), (p.k + 1) * p.N, (NR[bits] + 1) * 128
    assert isinstance(prk, PackedRoundKeys) and (prk.key_bits, prk.n_keys) == (bits, 3)
    assert prk.data.dtype == np.uint64 and prk.data.shape == (3, G, gw) and prk.nbytes == 3 * G * gw * 8
    assert G == toy_server.engine._lib.fheaes_round_keys_packed_glwes(bits)
    assert urk.shape == rk.shape
    for i in range(3):
        want = toy_server.pack(rk[i])
        assert np.array_equal(prk[i].data[0], want), "key %d: %d packed words differ" % (i, int((prk.data[i] != want).sum()))
        assert np.array_equal(urk[i], toy_server.unpack(want, rk[i].shape[:-1])), "key %d: unpacked words differ" % i
        assert np.array_equal(tc.decrypt_bytes(urk[i]), np.array(aes_clear.expand_key(k["keys"][i]), dtype=np.uint8))
    assert np.array_equal(toy_server.unpack_round_keys(prk, first=1, count=2), urk[1:])
    assert np.array_equal(toy_server.unpack_round_keys(prk[2])[0], urk[2])
    assert np.array_equal(toy_server.pack_round_keys(rk[1]).data, prk.data[1:2])       # [Nr+1]... is one key
    # resident tensors inside sentinel guard rows
    d_rk = dev(rk)
    pbuf, pmid = guarded(3 * G, gw)
    toy_server.engine.pack_round_keys(d_rk, bits, 3, pmid)
    ubuf, umid = guarded(2 * m, p.big1)
    toy_server.engine.unpack_round_keys(pmid, bits, 1, 2, umid)
    toy_server.synchronize()
    assert np.array_equal(host(pmid).reshape(3, G, gw), prk.data) and guards_intact(pbuf)
    assert np.array_equal(host(umid).reshape(urk[1:].shape), urk[1:]) and guards_intact(ubuf)


# ---- 2. the keyed cipher calls ---------------------------------------------------------------------------------------------------------------
def _three_ciphers(server, tc, k, kob, pts):
    """the three keyed calls from the packed stores against the same calls on the unpacked stores, and against clear AES"""
    n = len(pts)
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    enc = server.aes_encrypt_keyed(k["prk"], kob, st.copy())
    want = server.aes_encrypt_keyed(k["urk"], kob, st.copy())
    assert np.array_equal(enc, want), "encrypt: %d words differ" % int((enc != want).sum())
    assert [tc.decrypt_u128(enc[b]) for b in range(n)] == [aes_clear.aes_encrypt_block(k["keys"][j], v) for j, v in zip(kob, pts)]
    dec = server.aes_decrypt_keyed(k["prk"], kob, enc.copy())
    want = server.aes_decrypt_keyed(k["urk"], kob, enc.copy())
    assert np.array_equal(dec, want), "decrypt: %d words differ" % int((dec != want).sum())
    assert [tc.decrypt_u128(dec[b]) for b in range(n)] == pts
    eq = server.aes_decrypt_equivalent_keyed(k["pdw"], kob, enc.copy())
    want = server.aes_decrypt_equivalent_keyed(k["udw"], kob, enc.copy())
    assert np.array_equal(eq, want), "equivalent inverse cipher: %d words differ" % int((eq != want).sum())
    assert [tc.decrypt_u128(eq[b]) for b in range(n)] == pts


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_keyed_ciphers_from_packed_keys_are_the_calls_on_the_unpacked_store(toy_server, toy_keys, tc, bits):
    _three_ciphers(toy_server, tc, toy_keys[bits], KOB, PTS)


# ---- 3. forced windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [2, 3, OFF], ids=["window 2", "window 3", "round by round"])
def test_toy_keyed_ciphers_from_packed_keys_under_forced_windows(toy_server, toy_keys, tc, window):
    """5 blocks in windows of 2 and 3: launches whose two segments belong to different steps, each reading key_of_block from its own first block"""
    eng = toy_server.engine
    eng.aes_set_window(window)
    try:
        assert eng.aes_window(5, 10) == (0 if window == OFF else window)
        _three_ciphers(toy_server, tc, toy_keys[128], KOB, PTS)
    finally:
        eng.aes_set_window(0)


# ---- 4. public blocks / CTR ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PUBLIC_CASES))
def test_toy_public_keyed_from_packed_keys_shares_as_planned(toy, tc, toy_keys, case):
    kob, blocks = PUBLIC_CASES[case]
    k = toy_keys[128]
    srv = Server(toy.keys, device=0)                                          # a context of its own: the profile counters are its
    try:
        srv.engine.profile_enable(True)
        srv.engine.profile_reset()
        got = srv.aes_encrypt_public_keyed(k["prk"], kob, blocks)
        prof = srv.engine.profile_read()
        srv.engine.profile_enable(False)
        plan = _native.aes_public_plan_keyed(blocks, kob, 3, 128)
        assert plan == [34, 40] + [64] * 8 and prof["blind_rotate"]["units"] == 8 * sum(plan)
        assert prof["linear"]["launches"] == 11                               # the pool of round 1 and one indexed layer per round
        want = srv.aes_encrypt_public_keyed(k["urk"], kob, blocks)
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        assert np.array_equal(tc.decrypt_bytes(got), block_bytes([aes_clear.aes_encrypt_block(k["keys"][j], v) for j, v in zip(kob, blocks)]))
    finally:
        srv.engine.close()


@pytest.mark.parametrize("bits", [128, 256])
def test_toy_ctr_streams_from_packed_keys(toy, toy_server, toy_keys, tc, bits):
    k = toy_keys[bits]
    got = toy_server.aes_ctr_streams(k["prk"], STREAMS)
    assert got.shape == (8, 16, 8, toy.params.big1)
    want = toy_server.aes_ctr_streams(k["urk"], STREAMS)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes(aes_clear.ctr_streams(k["keys"], STREAMS)))


# ---- 5. the single-key methods ----------------------------------------------------------------------------------------------------------------
def test_toy_single_key_methods_take_a_one_key_store(toy_server, toy_keys, tc):
    k = toy_keys[192]
    one, done, rk, dw = k["prk"][2], k["pdw"][2], k["urk"][2], k["udw"][2]
    st = np.stack([tc.encrypt_u128(v) for v in PTS[:2]])
    enc = toy_server.aes_encrypt(one, st.copy())
    assert np.array_equal(enc, toy_server.aes_encrypt(rk, st.copy()))
    assert np.array_equal(toy_server.aes_encrypt(one, st[0].copy()), enc[0])                            # one state [16][8][kN+1]
    assert np.array_equal(toy_server.aes_decrypt(one, enc.copy()), toy_server.aes_decrypt(rk, enc.copy()))
    assert np.array_equal(toy_server.aes_decrypt_equivalent(done, enc.copy()), toy_server.aes_decrypt_equivalent(dw, enc.copy()))
    assert np.array_equal(toy_server.aes_encrypt_public(one, PTS[:3]), toy_server.aes_encrypt_public(rk, PTS[:3]))
    _, iv, first, n, data = STREAMS[1]
    ctr = toy_server.aes_ctr(one, iv, first, n, data=data)
    assert np.array_equal(ctr, toy_server.aes_ctr(rk, iv, first, n, data=data))
    assert [tc.decrypt_u128(b) for b in ctr] == [ks ^ d for ks, d in zip(aes_clear.ctr_keystream(k["keys"][2], iv, first, n), data)]
    with pytest.raises(ValueError):
        toy_server.aes_encrypt(k["prk"], st.copy())                                                     # three keys: which one?


# ---- 6. argument rules -------------------------------------------------------------------------------------------------------------------------
def test_argument_rules_leave_the_context_working(toy, toy_server, toy_keys, tc):
    p, k = toy.params, toy_keys[128]
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    rk, prk = k["rk"], k["prk"].data
    sw, store_words = 128 * p.big1, prk.size
    st = np.stack([tc.encrypt_u128(v) for v in PTS[:2]])
    before = st.copy()
    u32 = lambda *v: (np.array(v, dtype=np.uint32).ctypes.data_as(_native._u32p))
    blocks = _native.u128_pairs([1, 2]).ctypes.data_as(_native._u64p)
    ciphers = (lib.fheaes_aes_encrypt_keyed_packed, lib.fheaes_aes_decrypt_keyed_packed, lib.fheaes_aes_decrypt_equivalent_keyed_packed)
    both = np.zeros(store_words + 2 * sw, dtype=np.uint64)                    # a store with a state behind it, to overlap them in
    base = both.ctypes.data
    for ms in (_native.HOST, _native.DEVICE):
        for fn in ciphers:
            assert fn(h, base, 128, 3, u32(0, 1), base + 8 * (store_words - 1), 2, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
            assert fn(h, base + 8 * sw, 128, 3, u32(0, 1), base, 2, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
            assert fn(h, prk.ctypes.data, 128, 3, u32(0, 3), st.ctypes.data, 2, ms) == -1               # key index 3 of 3 keys
            assert b"key_of_block[1] = 3" in lib.fheaes_last_error(h)
            assert fn(h, prk.ctypes.data, 100, 3, u32(0, 0), st.ctypes.data, 2, ms) == -1 and b"key_bits" in lib.fheaes_last_error(h)
            assert fn(h, prk.ctypes.data, 128, 0, u32(0, 0), st.ctypes.data, 2, ms) == -1
            assert fn(h, prk.ctypes.data, 128, 3, None, st.ctypes.data, 2, ms) == -1
            assert fn(h, prk.ctypes.data, 128, 3, u32(0), st.ctypes.data, 0, ms) == 0                   # no blocks: nothing to do
        pub = lib.fheaes_aes_public_keyed_packed
        assert pub(h, base, 128, 3, u32(0, 1), blocks, None, 2, base + 8 * (store_words - 1), ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert pub(h, prk.ctypes.data, 128, 3, u32(0, 3), blocks, None, 2, st.ctypes.data, ms) == -1
        assert pub(h, prk.ctypes.data, 200, 3, u32(0, 0), blocks, None, 2, st.ctypes.data, ms) == -1
        assert pub(h, prk.ctypes.data, 128, 3, u32(0), blocks, None, 0, st.ctypes.data, ms) == 0
        # the store itself: overlap, key size, key count
        assert lib.fheaes_pack_round_keys(h, base, 128, 1, base + 8 * 100, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_unpack_round_keys(h, base, 128, 0, 1, base + 8 * 100, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_pack_round_keys(h, rk.ctypes.data, 160, 3, both.ctypes.data, ms) == -1
        assert lib.fheaes_unpack_round_keys(h, prk.ctypes.data, 160, 0, 3, both.ctypes.data, ms) == -1
        assert lib.fheaes_pack_round_keys(h, rk.ctypes.data, 128, 0, both.ctypes.data, ms) == -1
        assert lib.fheaes_unpack_round_keys(h, prk.ctypes.data, 128, 65536, 1, both.ctypes.data, ms) == -1
        assert lib.fheaes_pack_round_keys(h, None, 128, 3, both.ctypes.data, ms) == -1
    assert np.array_equal(st, before) and not both.any()
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        out = np.empty_like(prk)
        for call in (lambda: fresh.pack_round_keys(rk, 128, 3, out), lambda: fresh.aes_encrypt_keyed_packed(prk, 128, 3, [0, 1], st, 2),
                     lambda: fresh.aes_decrypt_keyed_packed(prk, 128, 3, [0, 1], st, 2),
                     lambda: fresh.aes_decrypt_equivalent_keyed_packed(prk, 128, 3, [0, 1], st, 2),
                     lambda: fresh.aes_public_keyed(prk, 128, 3, [0, 1], [1, 2], None, st, packed=True)):
            with pytest.raises(_native.FheAesError) as e:
                call()
            assert e.value.code == -2
        back = np.empty_like(rk)                                              # unpacking needs no keys
        fresh.unpack_round_keys(prk, 128, 0, 3, back)
        assert np.array_equal(back, k["urk"])
    finally:
        fresh.close()
    # what never reaches the library
    for call in (lambda: toy_server.aes_encrypt_keyed(k["prk"], [0], st), lambda: toy_server.aes_encrypt_keyed(k["prk"], [0, 0], st[0]),
                 lambda: toy_server.unpack_round_keys(k["prk"], first=2, count=2), lambda: toy_server.unpack_round_keys(k["prk"], first=3),
                 lambda: toy_server.pack_round_keys(rk[:, :10]), lambda: toy_server.aes_encrypt_keyed(k["prk"], [0, 1], dev(st))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(_native.FheAesError) as e:
        toy_server.aes_encrypt_keyed(k["prk"], [0, 3], st)
    assert e.value.code == -1
    got = toy_server.aes_encrypt_keyed(k["prk"], [2, 1], st.copy())           # the context works afterwards
    assert np.array_equal(got, toy_server.aes_encrypt_keyed(k["urk"], [2, 1], st.copy()))


def test_toy_key_expansion_packed_in_chunks_and_resident_tensors(toy, toy_server, toy_keys, tc):
    k = toy_keys[128]
    ek = np.stack([tc.encrypt_aes_key(key) for key in k["keys"]])
    want = toy_server.pack_round_keys(toy_server.aes_key_expansion_many(ek))
    for chunk in (2, 256):                                                    # 2 + 1 keys, and all at once
        got = toy_server.aes_key_expansion_packed(ek, chunk=chunk)
        assert (got.key_bits, got.n_keys) == (128, 3) and np.array_equal(got.data, want.data)
    d_prk = toy_server.aes_key_expansion_packed(dev(ek), chunk=2)
    d_st = dev(np.stack([tc.encrypt_u128(v) for v in PTS]))
    st = host(d_st).copy()
    toy_server.aes_encrypt_keyed(d_prk, KOB, d_st)
    toy_server.synchronize()
    assert d_prk.data.is_cuda and np.array_equal(host(d_prk.data), want.data)
    assert np.array_equal(host(d_st), toy_server.aes_encrypt_keyed(want, KOB, st))


# ---- 7. / 8. PARAM_OPT: the polynomials p > 0 of the extraction, and 64-bit offsets -----------------------------------------------------------
@pytest.fixture(scope="module")
def opt_two_keys(opt, opt_server, opt_rk128, oc):
    """two AES-128 keys resident at PARAM_OPT, packed, the store unpacked again, 2 encrypted blocks, and what the keyed call on the
    unpacked store writes for them under the keys [0, 1] and [1, 0]"""
    import torch

    keys = [F5[128][0], aes_keys(128, 1)[0]]
    d_ek = dev(oc.encrypt_aes_key(keys[1]))
    d_rk2 = opt_server.aes_key_expansion(d_ek)
    opt_server.synchronize()                                                  # torch's stream stacks what the engine's stream wrote
    d_rk = settled(torch.stack([opt_rk128, d_rk2]))
    prk = opt_server.pack_round_keys(d_rk)
    urk = opt_server.unpack_round_keys(prk)
    st = np.stack([oc.encrypt_u128(v) for v in PTS[:2]])
    want = {}
    for kob in ((0, 1), (1, 0)):
        d_st = dev(st)
        opt_server.aes_encrypt_keyed(urk, list(kob), d_st)
        opt_server.synchronize()
        want[kob] = host(d_st)
    return dict(keys=keys, prk=prk, st=st, want=want)


def test_param_opt_keyed_encryption_from_packed_keys(opt, opt_server, opt_two_keys, oc):
    t = opt_two_keys
    assert t["prk"].data.is_cuda and tuple(t["prk"].data.shape) == (2, 3, 2560) and t["prk"].nbytes == 2 * 61440
    d_st = dev(t["st"])
    opt_server.aes_encrypt_keyed(t["prk"], [0, 1], d_st)
    opt_server.synchronize()
    got = host(d_st)
    assert np.array_equal(got, t["want"][0, 1]), "%d words differ" % int((got != t["want"][0, 1]).sum())
    assert [oc.decrypt_u128(got[b]) for b in range(2)] == [aes_clear.aes_encrypt_block(t["keys"][b], PTS[b]) for b in range(2)]
    err = np.abs(noise(oc, got))
    print("aes_encrypt_keyed from packed keys at PARAM_OPT: |noise| max 2^%.2f, std 2^%.2f" % (np.log2(float(err.max())), np.log2(float(err.std()))))
    assert err.max() < 1 << 59, "max |noise| = 2^%.1f" % np.log2(float(err.max()))
    assert err.std() < 1 << 56, "std = 2^%.1f" % np.log2(float(err.std()))


def test_param_opt_key_65535_of_a_full_store_needs_64_bit_offsets(opt, opt_server, opt_two_keys, oc):
    """65,536 AES-128 keys, 4.03 GB, the two packed keys tiled: key 65,535 is key 1 and starts at byte 65,535 x 61,440 = 4,026,470,400,
    where a signed 32-bit byte offset has wrapped (2^31) and an unsigned one has 268 MB left (the whole store ends 6 % short of 2^32)"""
    import torch

    t = opt_two_keys
    store = PackedRoundKeys(opt.params, 128, t["prk"].data.repeat(32768, 1, 1))
    try:
        torch.cuda.synchronize()
        assert store.n_keys == 65536 and store.nbytes == 4026531840 and 1 << 31 < 65535 * 61440 < 1 << 32
        d_st = dev(t["st"])
        opt_server.aes_encrypt_keyed(store, [65535, 0], d_st)
        opt_server.synchronize()
        got = host(d_st)
        assert np.array_equal(got, t["want"][1, 0]), "%d words differ" % int((got != t["want"][1, 0]).sum())
        assert [oc.decrypt_u128(got[b]) for b in range(2)] == [aes_clear.aes_encrypt_block(t["keys"][1 - b], PTS[b]) for b in range(2)]
    finally:
        del store
        torch.cuda.empty_cache()


# ---- 9. several contexts -----------------------------------------------------------------------------------------------------------------------
def test_toy_server_group_from_packed_keys_is_the_single_server(toy, toy_server, toy_keys, tc):
    k = toy_keys[128]
    st = np.stack([tc.encrypt_u128(v) for v in PTS])
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        assert np.array_equal(group.aes_encrypt_keyed(k["prk"], KOB, st.copy()), toy_server.aes_encrypt_keyed(k["prk"], KOB, st.copy()))
        assert np.array_equal(group.aes_ctr_streams(k["prk"], STREAMS), toy_server.aes_ctr_streams(k["prk"], STREAMS))
        assert np.array_equal(group.pack_round_keys(k["rk"]).data, k["prk"].data)
        assert np.array_equal(group.unpack_round_keys(k["prk"], 1, 1), k["urk"][1:2])
    finally:
        for s in group.servers:
            s.engine.close()
