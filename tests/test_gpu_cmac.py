"""AES-CMAC on the MI355X.  The subkey gather alone (fheaes_cmac_double) on edge words inside guard rows against numpy sums over
fheaes_cmac_subkey_row; fheaes_aes_cmac_subkeys_keyed and fheaes_aes_cmac_keyed word for word against cmac.compose_subkeys,
ccm.compose_mac and cmac.compose_verify -- entry points older than the calls, plus the gather -- so every comparison is array_equal;
subkeys, tags and validity bits from aes_clear and the SP 800-38B / RFC 4493 vectors.  The last section runs the subkeys, the tags and
the tag check once at PARAM_OPT, and holds the noise of a MAC word there to tests/noise_model.py."""
import numpy as np
import pytest

import ccm
import cmac
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, oc, opt_server, settled, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

EDGE = (0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1)
KEY_V = cmac.VECTORS[128][0]
KEYS_128 = (bytes(range(0x40, 0x50)), KEY_V, bytes(range(0xC0, 0xD0)))
_results = {}


def _u128(data):
    return int.from_bytes(data, "big")


def _dec_blocks(tc, words):
    return [bytes(b.tolist()) for b in tc.decrypt_bytes(words.reshape(-1, 16, 8, words.shape[-1]))]


# ---- the gather alone ------------------------------------------------------------------------------------------------------------------------
def _edge_l(p, n_keys, seed):
    """random L rows [n_keys][128][kN+1]: the rows the reduction terms come from (bytes 0 and 15) and a few others are constant edge
    words, and every other word of the rows between, so that the two- and three-term sums wrap"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, (n_keys, 128, p.big1), dtype=np.uint64)
    for i, v in enumerate(EDGE):
        a[:, 7 - i] = v                      # degrees 127 .. 124: what x^128 and x^129 reduce
        a[:, 120 + i] = EDGE[3 - i]          # degrees 0 .. 3
        a[:, 8 + i] = EDGE[(i + 1) % 4]
        a[:, 60 + i, ::2] = v
    return a


@pytest.mark.parametrize("n_keys", [1, 3])
def test_gather_is_the_sum(toy, n_keys):
    p = toy.params
    eng = _native.Engine(p, device=0)                                        # no keys: the gather needs none
    try:
        l = _edge_l(p, n_keys, 0xC3AC + n_keys)
        want = cmac.np_double(l)
        assert eng.noise_level_seen() == (0, 5)
        buf, rows = guarded(n_keys * 256, p.big1)
        d_out = rows.view(n_keys, 2, 128, p.big1)
        eng.cmac_double(dev(l), n_keys, d_out)
        eng.synchronize()
        got = host(d_out)
        assert guards_intact(buf)
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        assert eng.noise_level_seen() == (3, 5)                                # K2's heaviest row
        h_out = np.full((n_keys, 2, 128, p.big1), 0xA5, dtype=np.uint64)       # host arrays take the same path through staging
        eng.cmac_double(l, n_keys, h_out)
        assert np.array_equal(h_out, want)
    finally:
        eng.close()


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(toy_server, tc):
    """round keys made on the GPU: "128" three AES-128 keys, the SP 800-38B key among them; "192" and "256" the vector keys of those sizes"""
    many = lambda ks: toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in ks]))
    return {"128": many(KEYS_128), "192": many((cmac.VECTORS[192][0],)), "256": many((cmac.VECTORS[256][0],))}


def subkeys_case(which, toy_server, tc, keys):
    if ("sub", which) not in _results:
        _results["sub", which] = (toy_server.aes_cmac_subkeys(keys[which]), cmac.compose_subkeys(toy_server, tc, keys[which]))
    return _results["sub", which]


# ---- aes_cmac_subkeys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,clear_keys", [("128", KEYS_128), ("192", (cmac.VECTORS[192][0],)), ("256", (cmac.VECTORS[256][0],))])
def test_toy_subkeys_are_the_composition(toy, toy_server, tc, keys, which, clear_keys):
    got, want = subkeys_case(which, toy_server, tc, keys)
    assert got.shape == (len(clear_keys), 2, 16, 8, toy.params.big1) and got.dtype == np.uint64
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    dec = _dec_blocks(tc, got)
    assert [_u128(b) for b in dec] == [v for k in clear_keys for v in aes_clear.cmac_subkeys(k)]
    _, k1, k2, _ = cmac.VECTORS[int(which)]
    at = 2 * clear_keys.index(cmac.VECTORS[int(which)][0])
    assert dec[at:at + 2] == [k1, k2]


# ---- aes_cmac_streams ------------------------------------------------------------------------------------------------------------------------
# 0, 1, 15, 16, 17, 32 and 40 bytes: K2 alone, K1 alone, chains of 2 and 3, and in this order a sort that moves streams both ways
STREAMS = [(1, cmac.MESSAGE[:16]), (2, cmac.MESSAGE[:1]), (1, cmac.MESSAGE[:40]), (1, b""), (0, cmac.MESSAGE[:17]), (2, cmac.MESSAGE[:15]),
           (0, cmac.MESSAGE[:32])]


def streams_case(toy_server, tc, keys):
    if "mac" not in _results:
        sub, _ = subkeys_case("128", toy_server, tc, keys)
        got = toy_server.aes_cmac_streams(keys["128"], STREAMS)
        want = ccm.compose_mac(toy_server, tc, keys["128"], cmac.mac_streams(STREAMS, sub))
        _results["mac"] = (got, want)
    return _results["mac"]


def test_toy_tags_are_the_composition(toy, toy_server, tc, keys):
    got, want = streams_case(toy_server, tc, keys)
    assert got.shape == (len(STREAMS), 16, 8, toy.params.big1) and got.dtype == np.uint64
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    tags = [aes_clear.cmac(KEYS_128[k], msg) for k, msg in STREAMS]
    assert _dec_blocks(tc, got) == tags
    assert tags[0] == cmac.VECTORS[128][3][1] and tags[2] == cmac.VECTORS[128][3][2] and tags[3] == cmac.VECTORS[128][3][0]
    assert _native.aes_cmac_plan([len(m) for _, m in STREAMS]) == {"steps": 3, "chained_blocks": 11, "padded_streams": 5}


def test_toy_equivalent_paths(toy, toy_server, tc, keys):
    """packed round keys, the caller's subkeys, resident tensors inside guard rows and a ServerGroup of two contexts: the same words"""
    p = toy.params
    mac, _ = streams_case(toy_server, tc, keys)
    sub, _ = subkeys_case("128", toy_server, tc, keys)
    rk = keys["128"]
    packed = toy_server.pack_round_keys(rk)
    p_mac = toy_server.aes_cmac_streams(packed, STREAMS)
    assert np.array_equal(p_mac, toy_server.aes_cmac_streams(toy_server.unpack_round_keys(packed), STREAMS))
    assert _dec_blocks(tc, p_mac) == _dec_blocks(tc, mac)
    assert np.array_equal(toy_server.aes_cmac_subkeys(packed), toy_server.aes_cmac_subkeys(toy_server.unpack_round_keys(packed)))
    assert np.array_equal(toy_server.aes_cmac_streams(rk, STREAMS, subkeys=sub), mac)
    # a call that names one key derives that key's subkeys alone: the same words
    only1 = [st for st in STREAMS if st[0] == 1]
    assert np.array_equal(toy_server.aes_cmac_streams(rk, only1), mac[[i for i, st in enumerate(STREAMS) if st[0] == 1]])
    buf, rows = guarded(len(STREAMS) * 128, p.big1)
    d_mac = toy_server.aes_cmac_streams(dev(rk), STREAMS, subkeys=dev(sub), out=rows.view(len(STREAMS), 16, 8, p.big1))
    toy_server.synchronize()
    assert d_mac.is_cuda and guards_intact(buf) and np.array_equal(host(d_mac), mac)
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        g_mac = group.aes_cmac_streams(rk, STREAMS)
        g_sub = group.aes_cmac_subkeys(rk)
    finally:
        for s in group.servers:
            s.engine.close()
    assert np.array_equal(g_mac, mac) and np.array_equal(g_sub, sub)


# ---- aes_cmac_verify -------------------------------------------------------------------------------------------------------------------------
def test_toy_verification(toy, toy_server, tc, keys):
    """right tags of 4, 8, 12, 16 and 13 bytes verify; a flipped tag bit, a flipped message bit, a message whose length moved across a
    block boundary and the wrong key index do not; a flipped bit beyond the truncated length still verifies"""
    p = toy.params
    sub, _ = subkeys_case("128", toy_server, tc, keys)
    m17, m16, m1 = cmac.MESSAGE[:17], cmac.MESSAGE[:16], cmac.MESSAGE[:1]
    tag = lambda k, msg, t=16: aes_clear.cmac(KEYS_128[k], msg, t)
    flip = lambda data, i, bit=0x01: data[:i] + bytes([data[i] ^ bit]) + data[i + 1:]
    messages = [(0, m17, tag(0, m17, 4)), (1, m16, tag(1, m16, 8)), (2, m1, tag(2, m1, 12)), (1, b"", tag(1, b"")), (0, m16, tag(0, m16, 13)),
                (0, m17, flip(tag(0, m17, 4), 3, 0x80)),              # the last compared byte of a 4-byte tag
                (1, flip(m16, 9), tag(1, m16, 8)),                    # a message bit
                (1, m17, tag(1, m16)), (1, m16[:15], tag(1, m16)),    # one byte more and one less: across the block boundary, K1 -> K2
                (2, m16, tag(1, m16, 8))]                             # the wrong key index
    want_bits = [1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert [int(aes_clear.cmac_verify(KEYS_128[k], msg, t)) for k, msg, t in messages] == want_bits
    vbuf, vrows = guarded(len(messages), p.big1)
    d_ok = toy_server.aes_cmac_verify(dev(keys["128"]), messages, subkeys=dev(sub), valid_out=vrows)
    toy_server.synchronize()
    ok = host(d_ok)
    assert guards_intact(vbuf) and ok.shape == (len(messages), p.big1)
    assert tc.decrypt_bits(ok).tolist() == want_bits
    want = cmac.compose_verify(toy_server, tc, keys["128"], messages, sub)
    assert np.array_equal(ok, want), "%d valid words differ" % int((ok != want).sum())
    # a flipped bit beyond the truncated length: the comparison reads 8t rows, tags[s][t .. 16) of the C call are not looked at
    from tfhe_aes_amd.server import cmac_args

    eng, a = toy_server.engine, cmac_args([messages[1]])
    a["tags"][0] = list(flip(tag(1, m16), 8))
    one = np.empty((1, p.big1), dtype=np.uint64)
    eng.aes_cmac_keyed(keys["128"], 128, 3, sub, a["key_of_stream"], a["message_bytes"], a["data"], a["tags"], a["tag_bytes"], None, one)
    assert np.array_equal(one[0], ok[1]) and tc.decrypt_bits(one).tolist() == [1]
    # without the caller's subkeys, through the host path and a group: the same bits
    some = messages[:2] + messages[5:7]
    h_ok = toy_server.aes_cmac_verify(keys["128"], some)
    assert np.array_equal(h_ok, ok[[0, 1, 5, 6]])
    assert toy_server.aes_cmac_verify(keys["128"], []).shape == (0, p.big1)


# ---- noise levels ----------------------------------------------------------------------------------------------------------------------------
def test_toy_noise_levels(toy, tc):
    """The guard accepts the schedule at its limit of 5: the last link sums X (2) + the refreshed subkey (2, as every addend of a chain
    counts) + the round key.  The gather declares 3 (test_gather_is_the_sum), so K2 linked without the second refresh would be
    2 + 3 + 1 = 6 > 5.  No call of the C ABI takes a raw subkey as such -- a caller's addend always counts as 2 -- so that refusal is the
    schedule's arithmetic, asserted here on the declared figures, and not a run."""
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        rk = srv.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(KEY_V)]))
        msg = cmac.MESSAGE[:40]
        ok = srv.aes_cmac_verify(rk, [(0, msg, cmac.VECTORS[128][3][2][:8])])
        seen, limit = srv.engine.noise_level_seen()
        assert (seen, limit) == (5, 5)
    finally:
        srv.engine.close()
    assert tc.decrypt_bits(ok).tolist() == [1]
    gather = max(len(_native.cmac_subkey_row(1, i)) for i in range(128))
    assert gather == 3 and 2 + gather + 1 > limit and 2 + 2 + 1 <= limit


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_toy_errors_leave_the_outputs_untouched(toy, toy_server, tc, keys):
    p = toy.params
    eng = toy.engine()
    lib, h, D = eng._lib, eng._h, _native.DEVICE
    d_rk = dev(keys["128"])
    d_sub = dev(subkeys_case("128", toy_server, tc, keys)[0])
    buf, rows = guarded(2 * 128, p.big1)
    vbuf, vrows = guarded(2, p.big1)
    sbuf, srows = guarded(3 * 256, p.big1)
    rk, sk, o, v, so = d_rk.data_ptr(), d_sub.data_ptr(), rows.data_ptr(), vrows.data_ptr(), srows.data_ptr()
    u32 = lambda *x: np.array(x, dtype=np.uint32).ctypes.data_as(_native._u32p)
    u64 = lambda *x: np.array(x, dtype=np.uint64).ctypes.data_as(_native._u64p)
    u8 = lambda x: np.array(x, dtype=np.uint8).ctypes.data_as(_native._u8p)
    base = dict(rk=rk, bits=128, n_keys=3, sub=sk, n=2, kos=u32(0, 2), mb=u64(16, 3), data=u8([0] * 19), tags=None, tb=None, mac=o, ok=None)

    def call(**kw):
        x = dict(base, **kw)
        return lib.fheaes_aes_cmac_keyed(h, x["rk"], x["bits"], x["n_keys"], x["sub"], x["n"], x["kos"], x["mb"], x["data"], x["tags"], x["tb"], x["mac"],
                                         x["ok"], D)

    with_tags = dict(tags=u8([0] * 32), tb=u32(4, 16), ok=v)
    for name in ("rk", "kos", "mb", "data", "mac"):
        assert call(**{name: None}) == -1, name
    assert call(tags=u8([0] * 32)) == -1 and call(tb=u32(4, 16)) == -1                        # tags and tag_bytes come together
    assert call(ok=v) == -1 and b"valid_out" in lib.fheaes_last_error(h)                      # nothing to compare without tags
    assert call(**dict(with_tags, ok=None)) == -1                                             # valid_out is required with them
    assert call(bits=100) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert call(n_keys=0) == -1 and call(n_keys=65537) == -1 and b"n_keys" in lib.fheaes_last_error(h)
    assert call(n=(1 << 20) + 1) == -1 and b"n_streams" in lib.fheaes_last_error(h)
    assert call(kos=u32(0, 3)) == -1 and b"key_of_block" in lib.fheaes_last_error(h)
    assert call(mb=u64(16, (16 << 16) + 1)) == -1 and b"message_bytes" in lib.fheaes_last_error(h)
    for t in (0, 3, 17):
        assert call(**dict(with_tags, tb=u32(t, 8))) == -1 and b"tag_bytes" in lib.fheaes_last_error(h)
    assert call(mac=rk) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(mac=sk) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(**dict(with_tags, ok=o)) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(**dict(with_tags, mac=None, ok=sk)) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(n=0) == 0

    sub_call = lambda rk=rk, bits=128, n_keys=3, out=so: lib.fheaes_aes_cmac_subkeys_keyed(h, rk, bits, n_keys, out, D)
    assert sub_call(rk=None) == -1 and sub_call(out=None) == -1 and sub_call(bits=64) == -1 and sub_call(n_keys=0) == -1 and sub_call(n_keys=65537) == -1
    assert sub_call(out=rk) == -1 and b"overlap" in lib.fheaes_last_error(h)
    dbl = lambda l=sk, n_keys=3, out=so: lib.fheaes_cmac_double(h, l, n_keys, out, D)
    assert dbl(l=None) == -1 and dbl(out=None) == -1 and dbl(n_keys=65537) == -1
    assert dbl(l=so) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert dbl(n_keys=0) == 0
    for bad in (lambda: toy_server.aes_cmac_verify(d_rk, [(0, b"", bytes(3))]), lambda: toy_server.aes_cmac_streams(d_rk, [(0, b"", bytes(8))]),
                lambda: toy_server.aes_cmac_verify(d_rk, [(0, b"")]), lambda: toy_server.aes_cmac_streams(d_rk, [(0, b"")], subkeys=d_sub[:2])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_native.FheAesError):                                                  # a key index the round keys do not have
        toy_server.aes_cmac_streams(d_rk, [(3, b"")], out=rows.view(2, 16, 8, p.big1)[:1])
    toy_server.synchronize()
    assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
    assert bool((vrows == SENTINEL).all().item()) and guards_intact(vbuf)
    assert bool((srows == SENTINEL).all().item()) and guards_intact(sbuf)
    assert toy_server.aes_cmac_streams(keys["128"], []).shape == (0, 16, 8, p.big1)
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_cmac_subkeys_keyed(keys["128"], 128, 3, np.empty((3, 2, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


# ---- one call at PARAM_OPT -------------------------------------------------------------------------------------------------------------------
def _flip(data, i, bit=0x01):
    return data[:i] + bytes([data[i] ^ bit]) + data[i + 1:]


@pytest.fixture(scope="module")
def opt_keys(opt_server, oc):
    """round keys of the RFC 4493 key and of the SP 800-38B AES-256 key, and the subkeys of the first"""
    many = lambda k: opt_server.aes_key_expansion_many(np.stack([oc.encrypt_aes_key(k)]))
    rk = many(KEY_V)
    return {"128": rk, "256": many(cmac.VECTORS[256][0]), "sub": opt_server.aes_cmac_subkeys(rk)}


def test_opt_subkeys_and_tags_are_the_vectors(opt, opt_server, oc, opt_keys):
    """the subkeys against the doubling in GF(2^128); the four RFC 4493 messages (0, 16, 40 and 64 bytes: K2, K1, K2, K1, chains of 1 to
    4 steps) in one call under the AES-128 key, and the 40-byte message under the AES-256 key"""
    _, k1, k2, tags = cmac.VECTORS[128]
    l = aes_clear.aes_encrypt_block(KEY_V, 0)
    assert l == _u128(cmac.L_128)
    assert [_u128(b) for b in _dec_blocks(oc, opt_keys["sub"])] == [cmac.double(l), cmac.double(l, 2)] == [_u128(k1), _u128(k2)]
    got = opt_server.aes_cmac_streams(opt_keys["128"], [(0, cmac.MESSAGE[:n]) for n in cmac.LENGTHS], subkeys=opt_keys["sub"])
    assert got.shape == (4, 16, 8, opt.params.big1)
    assert _dec_blocks(oc, got) == list(tags)
    got256 = opt_server.aes_cmac_streams(opt_keys["256"], [(0, cmac.MESSAGE[:40])])                # its subkeys derived in the call
    assert _dec_blocks(oc, got256) == [cmac.VECTORS[256][3][2]]


def test_opt_verification(opt, opt_server, oc, opt_keys):
    """the four messages with their full tags, one tag cut to 4 bytes, and one whose last compared bit is flipped"""
    tags = cmac.VECTORS[128][3]
    messages = [(0, cmac.MESSAGE[:n], t) for n, t in zip(cmac.LENGTHS, tags)]
    messages += [(0, cmac.MESSAGE[:40], tags[2][:4]), (0, cmac.MESSAGE[:16], _flip(tags[1], 15, 0x01))]
    want_bits = [1, 1, 1, 1, 1, 0]
    assert [int(aes_clear.cmac_verify(KEY_V, msg, t)) for _, msg, t in messages] == want_bits
    ok = opt_server.aes_cmac_verify(opt_keys["128"], messages, subkeys=opt_keys["sub"])
    assert ok.shape == (6, opt.params.big1) and oc.decrypt_bits(ok).tolist() == want_bits
    want = cmac.compose_verify(opt_server, oc, opt_keys["128"], messages, opt_keys["sub"])
    assert np.array_equal(ok, want), "%d valid words differ" % int((ok != want).sum())


def test_opt_mac_output_noise(opt, opt_server, oc):
    """test_gpu_ccm.py::test_toy_mac_output_noise at PARAM_OPT: four one-block streams under four keys, 64 bytes, no round-key word
    shared.  The words of one byte share its GGSWs, whose carried errors lead at PARAM_OPT, so the bytes are counted: 64."""
    import noise_model as nm

    M = nm.NoiseModel.of_client(opt.client)
    ks = [bytes(np.random.default_rng(0xACE0 + i).integers(0, 256, 16, dtype=np.uint8).tolist()) for i in range(4)]
    rk = opt_server.aes_key_expansion_many(np.stack([oc.encrypt_aes_key(k) for k in ks]))
    blocks = [0x0123456789ABCDEF << (16 * i) for i in range(4)]
    got = opt_server.aes_cbc_mac_streams(rk, [(i, [blocks[i]]) for i in range(4)])
    want = [aes_clear.cbc_mac(ks[i], [blocks[i]]) for i in range(4)]
    err, vals = nm.wopbs_error(oc, got)
    assert [_u128(bytes(b.tolist())) for b in vals] == want
    var = np.concatenate([nm.aes_output_variance(M, ks[i], [want[i]]) for i in range(4)])
    n = M.wopbs_independent(64, 8)
    assert n == 64 and err.size == 512 and nm.rejects_doubling(n)
    nm.assert_noise(err, var, n, "CMAC output opt", left_out=2 * M.wopbs_left_out())
