"""CBC-MAC chains and AES-CCM decryption on the MI355X.  The link kernel alone (fheaes_mac_link) on edge words inside guard rows against
numpy; fheaes_aes_cbc_mac_keyed and fheaes_aes_ccm_open_keyed word for word against ccm.compose_mac / ccm.compose -- entry points older
than the two calls -- so every comparison is array_equal; plaintexts, MACs and validity bits from aes_clear and the SP 800-38C / RFC 3610
vectors.  The noise of a MAC word is held to tests/noise_model.py.  The last section runs one call at PARAM_OPT: the verdicts, the
plaintexts, the gated form, the composition word for word, and the noise of the tag difference that the first tag WoPBS decides on."""
import numpy as np
import pytest

import ccm
import noise_model as nm
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, oc, opt_server, settled, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

EDGE = (0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1)
NONE = _native.MAC_NONE
KEY_A, KEY_B = ccm.VECTORS["ex1"][0], ccm.VECTORS["rfc1"][0]
KEY_C = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
KEYS_192 = (bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"), bytes.fromhex("0123456789abcdeffedcba98765432100f1e2d3c4b5a6978"))


def _edge_blocks(p, n, seed):
    """random blocks [n][16][8][kN+1] whose first rows of bytes 0, 1, 14 and 15 are constant edge words, so that sums wrap"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, (n, 16, 8, p.big1), dtype=np.uint64)
    for i, v in enumerate(EDGE):
        a[:, 0, i] = v
        a[:, 15, 7 - i] = EDGE[3 - i]
        a[:, 1 + 13 * (i & 1), 2 + i, ::2] = v
    return a


# ---- the link kernel alone -----------------------------------------------------------------------------------------------------------------
def test_link_kernel_is_the_sum(toy, tc):
    p = toy.params
    eng = _native.Engine(p, device=0)                                        # no keys: the link needs none
    try:
        n = 5
        state, init, enc = _edge_blocks(p, n, 0xCC1), _edge_blocks(p, n, 0xCC2), _edge_blocks(p, 3, 0xCC3)
        clear = np.random.default_rng(0xCC4).integers(0, 256, (n, 16), dtype=np.uint8)
        clear[0] = 0xFF
        clear[1] = 0
        src, eb = [2, 0, NONE, 1, 2], [0, 1, 16, 15, 16]                      # enc_bytes 0, 1, 15, 16 and a slot without a block
        assert eng.noise_level_seen() == (0, 5)
        cases = [("public step", False, None, None), ("payload step", False, None, enc), ("first with init", True, init, enc),
                 ("first without init", True, None, enc), ("first, clear only", True, None, None)]
        for what, first, ini, e in cases:
            want = ccm.np_link(tc, state, first, ini, e, src, eb, clear)
            buf, rows = guarded(n * 128, p.big1)
            d_state = rows.view(n, 16, 8, p.big1)
            settled(d_state.copy_(dev(state)))
            eng.mac_link(d_state, first, None if ini is None else dev(ini), None if e is None else dev(e), src, eb, clear)
            eng.synchronize()
            got = host(d_state)
            assert guards_intact(buf), what
            assert np.array_equal(got, want), "%s: %d words differ" % (what, int((got != want).sum()))
            if what == "public step":
                assert eng.noise_level_seen() == (3, 5)                      # X (2) + the round key that follows
            if what == "payload step":
                assert eng.noise_level_seen() == (5, 5)                      # X (2) + P (2) + the round key
                h_state = state.copy()                                       # host arrays take the same path through staging
                eng.mac_link(h_state, first, None, e, src, eb, clear)
                assert np.array_equal(h_state, want)
    finally:
        eng.close()


def test_link_refusals(toy):
    p = toy.params
    eng = _native.Engine(p, device=0)
    try:
        lib, h, D = eng._lib, eng._h, _native.DEVICE
        d_enc = dev(_edge_blocks(p, 2, 1))
        buf, rows = guarded(2 * 128, p.big1)
        u32 = lambda *v: np.array(v, dtype=np.uint32).ctypes.data_as(_native._u32p)
        u8 = lambda *v: np.array(v, dtype=np.uint8).ctypes.data_as(_native._u8p)
        clear = np.zeros(32, dtype=np.uint8).ctypes.data_as(_native._u8p)
        st, e = rows.data_ptr(), d_enc.data_ptr()
        assert lib.fheaes_mac_link(h, None, 2, 0, None, e, 2, u32(0, 1), u8(16, 16), clear, D) == -1
        assert lib.fheaes_mac_link(h, st, 2, 0, None, e, 2, u32(0, 1), u8(16, 16), None, D) == -1
        assert lib.fheaes_mac_link(h, st, 2, 0, None, e, 2, None, u8(16, 16), clear, D) == -1
        assert lib.fheaes_mac_link(h, st, 2, 0, None, e, 2, u32(0, 2), u8(16, 16), clear, D) == -1 and b"src_block" in lib.fheaes_last_error(h)
        assert lib.fheaes_mac_link(h, st, 2, 0, None, e, 2, u32(0, 1), u8(16, 17), clear, D) == -1 and b"enc_bytes" in lib.fheaes_last_error(h)
        assert lib.fheaes_mac_link(h, st, 2, 0, e, None, 0, None, None, clear, D) == -1 and b"init" in lib.fheaes_last_error(h)
        assert lib.fheaes_mac_link(h, st, 2, 1, st, None, 0, None, None, clear, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_mac_link(h, st, 2, 0, None, st, 2, u32(0, 1), u8(16, 16), clear, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_mac_link(h, st, (1 << 20) + 1, 0, None, None, 0, None, None, clear, D) == -1
        assert lib.fheaes_mac_link(h, st, 0, 0, None, None, 0, None, None, clear, D) == 0
        eng.synchronize()
        assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
        assert eng.noise_level_seen() == (0, 5)
    finally:
        eng.close()


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(toy_server, tc):
    """round keys made on the GPU: "ab" the two AES-128 keys of the vectors, "c" the AES-256 key, "192" two AES-192 keys"""
    many = lambda ks: toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in ks]))
    return {"ab": many((KEY_A, KEY_B)), "c": many((KEY_C,)), "192": many(KEYS_192)}


def _u128(data):
    return int.from_bytes(data, "big")


# ---- aes_cbc_mac_streams ---------------------------------------------------------------------------------------------------------------------
MAC_BLOCKS = ([0x00112233445566778899AABBCCDDEEFF, 1 << 127, (1 << 128) - 1], [0], [0x0F0E0D0C0B0A09080706050403020100, 5])
_results = {}


def mac_case(toy_server, tc, keys):
    """three streams of 3, 1 and 2 blocks in that order under two keys: the sort moves the third in front of the second, the prefix shrinks
    3 -> 2 -> 1 and the results are scattered back"""
    if "mac" not in _results:
        streams = [(0, MAC_BLOCKS[0]), (1, MAC_BLOCKS[1]), (1, MAC_BLOCKS[2])]
        got = toy_server.aes_cbc_mac_streams(keys["192"], streams)
        want = ccm.compose_mac(toy_server, tc, keys["192"], [st + (None, None) for st in streams])
        _results["mac"] = (streams, got, want)
    return _results["mac"]


def test_toy_mac_streams_are_the_composition(toy, toy_server, tc, keys):
    streams, got, want = mac_case(toy_server, tc, keys)
    assert got.shape == (3, 16, 8, toy.params.big1) and got.dtype == np.uint64
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    macs = [aes_clear.cbc_mac(KEYS_192[k], blocks) for k, blocks in streams]
    assert [_u128(bytes(b.tolist())) for b in tc.decrypt_bytes(got)] == macs
    assert _native.aes_mac_plan([3, 1, 2])["n_active"] == [3, 2, 1]


def test_toy_mac_streams_with_init_addends_and_an_empty_stream(toy, toy_server, tc, keys):
    """a caller's init and encrypted addend (the last block with 5 real bytes), and a stream of no blocks, which keeps its init"""
    p = toy.params
    init = np.stack([tc.encrypt_u128(0x1234), tc.encrypt_u128(0x99)])
    addend = [0xA1A2A3A4A5A6A7A8A9AAABACADAEAFB0, 0xC1C2C3C4C5 << 88]
    enc = np.stack([tc.encrypt_u128(addend[0]), tc.encrypt_u128(addend[1] | 0xFFFF)])         # bytes 14, 15 of the last block are not real
    streams = [(1, [], None, None), (0, [7, 0], enc, [16, 5])]
    got = toy_server.aes_cbc_mac_streams(keys["ab"], streams, init=init)
    want = ccm.compose_mac(toy_server, tc, keys["ab"], streams, init=init)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    assert np.array_equal(got[0], init[0])
    dec = [_u128(bytes(b.tolist())) for b in tc.decrypt_bytes(got)]
    assert dec == [0x1234, aes_clear.cbc_mac(KEY_A, [7 ^ addend[0], addend[1]], init=0x99)]
    assert toy_server.aes_cbc_mac_streams(keys["ab"], []).shape == (0, 16, 8, p.big1)
    one = toy_server.aes_cbc_mac_streams(keys["ab"][0], [(0, [7 ^ addend[0] ^ 0x99])])       # one key's round keys, no table
    assert _u128(bytes(tc.decrypt_bytes(one)[0].tolist())) == aes_clear.aes_encrypt_block(KEY_A, 7 ^ addend[0] ^ 0x99)


def test_toy_mac_output_noise(toy, toy_server, tc):
    """A MAC word is a cipher output word: the last round's fresh S-Box output plus a word of the last round key
    (noise_model.aes_output_variance).  Four one-block streams under four keys: 512 words, no round-key word shared, 64 bytes of each
    kind, independent word by word at PARAM_TOY (noise_model.wopbs_independent gives the count the band is taken from)."""
    M = nm.NoiseModel.of_client(toy.client)
    ks = [bytes(np.random.default_rng(0xACE0 + i).integers(0, 256, 16, dtype=np.uint8).tolist()) for i in range(4)]
    rk = toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in ks]))
    blocks = [0x0123456789ABCDEF << (16 * i) for i in range(4)]
    got = toy_server.aes_cbc_mac_streams(rk, [(i, [blocks[i]]) for i in range(4)])
    want = [aes_clear.cbc_mac(ks[i], [blocks[i]]) for i in range(4)]
    err, vals = nm.wopbs_error(tc, got)
    assert [_u128(bytes(b.tolist())) for b in vals] == want
    var = np.concatenate([nm.aes_output_variance(M, ks[i], [want[i]]) for i in range(4)])
    n = M.wopbs_independent(64, 8)
    assert err.size == 512 and nm.rejects_doubling(n)
    nm.assert_noise(err, var, n, "CBC-MAC output toy", left_out=2 * M.wopbs_left_out())


# ---- aes_ccm_decrypt -------------------------------------------------------------------------------------------------------------------------
def _messages(name):
    if name == "vectors":                                 # examples 1 and 2 and the RFC vector in one call under their two keys
        return "ab", (KEY_A, KEY_B), [ccm.message(0, "ex1"), ccm.message(0, "ex2"), ccm.message(1, "rfc1")]
    if name == "small":                                   # AES-256: chain length 0, AAD only, payload only with a partial last block
        nonce = ccm.run(0x30, 11)
        return "c", (KEY_C,), [ccm.own_message(0, KEY_C, nonce, b"", b"", 8), ccm.own_message(0, KEY_C, nonce, ccm.run(0x50, 3), b"", 10),
                               ccm.own_message(0, KEY_C, ccm.run(0x31, 11), b"", ccm.run(0x60, 24), 8)]
    if name == "tag lengths":                             # t = 16 and t = 4 on one message, and t = 16 with its last byte wrong
        nonce, payload = ccm.run(0x70, 13), ccm.run(0x80, 5)
        long, short = ccm.own_message(0, KEY_A, nonce, b"", payload, 16), ccm.own_message(0, KEY_A, nonce, b"", payload, 4)
        return "ab", (KEY_A, KEY_B), [long, short, long[:4] + (long[4][:15] + bytes([long[4][15] ^ 1]),)]
    raise KeyError(name)


def ccm_case(name, toy_server, tc, keys):
    if name not in _results:
        which, clear_keys, messages = _messages(name)
        got = toy_server.aes_ccm_decrypt(keys[which], messages)
        want = ccm.compose(toy_server, tc, keys[which], messages)
        _results[name] = (which, clear_keys, messages, got, want)
    return _results[name]


@pytest.mark.parametrize("name,valid", [("vectors", [1, 1, 1]), ("small", [1, 1, 1]), ("tag lengths", [1, 1, 0])])
def test_toy_ccm_is_the_composition(toy, toy_server, tc, keys, name, valid):
    p = toy.params
    _, clear_keys, messages, (pt, ok, at), (want_pt, want_ok, want_at) = ccm_case(name, toy_server, tc, keys)
    assert at == want_at and pt.shape == (at[-1], 16, 8, p.big1) and ok.shape == (len(messages), p.big1)
    assert np.array_equal(pt, want_pt), "%d plaintext words differ" % int((pt != want_pt).sum())
    assert np.array_equal(ok, want_ok), "%d valid words differ" % int((ok != want_ok).sum())
    assert tc.decrypt_bits(ok).tolist() == valid
    payloads = [aes_clear._ccm_ctr(clear_keys[k], aes_clear.ccm_blocks(nonce, aad, len(ct), len(tag))[2], ct) for k, nonce, aad, ct, tag in messages]
    assert ccm.plaintext_of(tc, pt, at, messages) == payloads
    for i, (k, nonce, aad, ct, tag) in enumerate(messages):
        if valid[i]:
            assert aes_clear.ccm_decrypt(clear_keys[k], nonce, aad, ct + tag, len(tag)) == payloads[i]
        if len(ct) % 16:                                                    # rows beyond the payload's length are zero words
            assert not pt[at[i + 1] - 1].reshape(128, p.big1)[8 * (len(ct) % 16):].any()
    if name == "vectors":
        assert payloads == [ccm.VECTORS[v][3] for v in ("ex1", "ex2", "rfc1")]


def test_toy_corrupted_inputs_are_the_ones_rejected(toy_server, tc, keys):
    """one tag bit flipped in the last compared byte of example 1 (t = 4: byte 3), one ciphertext bit in the RFC vector: exactly those
    two are invalid, and example 2 between them is unchanged word for word"""
    which, _, messages, (pt, ok, at), _ = ccm_case("vectors", toy_server, tc, keys)
    bad = list(messages)
    k, nonce, aad, ct, tag = bad[0]
    bad[0] = (k, nonce, aad, ct, tag[:3] + bytes([tag[3] ^ 0x80]))
    k, nonce, aad, ct, tag = bad[2]
    bad[2] = (k, nonce, aad, ct[:17] + bytes([ct[17] ^ 0x04]) + ct[18:], tag)
    pt2, ok2, at2 = toy_server.aes_ccm_decrypt(keys[which], bad)
    assert at2 == at and tc.decrypt_bits(ok2).tolist() == [0, 1, 0]
    assert np.array_equal(ok2[1], ok[1]) and np.array_equal(pt2[:at[2]], pt[:at[2]])          # examples 1 and 2: the same ciphertexts
    assert not np.array_equal(ok2[0], ok[0])
    assert np.array_equal(pt2[at[2]], pt[at[2]]) and not np.array_equal(pt2[at[2] + 1], pt[at[2] + 1])      # the flipped bit is in block 1


def test_toy_equivalent_paths(toy, toy_server, tc, keys):
    """packed round keys, resident tensors, a ServerGroup of two contexts and the cipher window off or forced: the same words"""
    p = toy.params
    which, _, messages, (pt, ok, at), _ = ccm_case("vectors", toy_server, tc, keys)
    rk = keys[which]
    packed = toy_server.pack_round_keys(rk)
    got = toy_server.aes_ccm_decrypt(packed, messages)
    unpacked = toy_server.aes_ccm_decrypt(toy_server.unpack_round_keys(packed), messages)
    assert np.array_equal(got[0], unpacked[0]) and np.array_equal(got[1], unpacked[1])
    assert tc.decrypt_bits(got[1]).tolist() == [1, 1, 1] and ccm.plaintext_of(tc, got[0], at, messages) == ccm.plaintext_of(tc, pt, at, messages)
    streams, mac, _ = mac_case(toy_server, tc, keys)
    packed192 = toy_server.pack_round_keys(keys["192"])
    p_mac = toy_server.aes_cbc_mac_streams(packed192, streams)
    assert np.array_equal(p_mac, toy_server.aes_cbc_mac_streams(toy_server.unpack_round_keys(packed192), streams))
    assert np.array_equal(tc.decrypt_bytes(p_mac), tc.decrypt_bytes(mac))
    buf, rows = guarded(at[-1] * 128, p.big1)
    vbuf, vrows = guarded(len(messages), p.big1)
    d_pt, d_ok, _ = toy_server.aes_ccm_decrypt(dev(rk), messages, out=rows.view(at[-1], 16, 8, p.big1), valid_out=vrows)
    toy_server.synchronize()
    assert d_pt.is_cuda and guards_intact(buf) and guards_intact(vbuf)
    assert np.array_equal(host(d_pt), pt) and np.array_equal(host(d_ok), ok)
    eng = toy_server.engine
    try:
        for window in (_native.AES_WINDOW_OFF, 2):
            eng.aes_set_window(window)
            w_pt, w_ok, _ = toy_server.aes_ccm_decrypt(rk, messages)
            assert np.array_equal(w_pt, pt) and np.array_equal(w_ok, ok), window
    finally:
        eng.aes_set_window(0)
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        g_pt, g_ok, g_at = group.aes_ccm_decrypt(rk, messages)
        g_mac = group.aes_cbc_mac_streams(keys["192"], streams)
    finally:
        for s in group.servers:
            s.engine.close()
    assert g_at == at and np.array_equal(g_pt, pt) and np.array_equal(g_ok, ok)
    assert np.array_equal(g_mac, mac)


def test_toy_noise_levels(toy, tc):
    """a payload link sums X (2) + P (2) + the round key = 5, the guard's limit and the figure the cipher's own rounds declare (MixColumns'
    four terms + the round key); the links alone are held to 3 and 5 in test_link_kernel_is_the_sum"""
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        rk = srv.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(KEY_A)]))
        _, ok, _ = srv.aes_ccm_decrypt(rk, [ccm.message(0, "ex1")])
        assert srv.engine.noise_level_seen() == (5, 5)
    finally:
        srv.engine.close()
    assert tc.decrypt_bits(ok).tolist() == [1]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_toy_errors_leave_the_outputs_untouched(toy, toy_server, tc, keys):
    p = toy.params
    eng = toy.engine()
    lib, h, D = eng._lib, eng._h, _native.DEVICE
    d_rk = dev(keys["ab"])
    buf, rows = guarded(2 * 128, p.big1)
    vbuf, vrows = guarded(2, p.big1)
    rk, o, v = d_rk.data_ptr(), rows.data_ptr(), vrows.data_ptr()
    u32 = lambda *x: np.array(x, dtype=np.uint32).ctypes.data_as(_native._u32p)
    u8 = lambda x: np.array(x, dtype=np.uint8).ctypes.data_as(_native._u8p)
    clear = u8([0] * 32)

    def mac(rk=rk, bits=128, n_keys=2, n=2, kos=u32(0, 1), sb=u32(1, 1), clr=clear, enc=None, eb=None, init=None, out=o):
        return lib.fheaes_aes_cbc_mac_keyed(h, rk, bits, n_keys, n, kos, sb, clr, enc, eb, init, out, D)

    assert mac(rk=None) == -1 and mac(kos=None) == -1 and mac(sb=None) == -1 and mac(clr=None) == -1 and mac(out=None) == -1
    assert mac(enc=rk) == -1 and mac(eb=u8([16, 16])) == -1                                   # enc and enc_bytes come together
    assert mac(bits=100) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert mac(n_keys=0) == -1 and mac(n_keys=65537) == -1 and b"n_keys" in lib.fheaes_last_error(h)
    assert mac(n=(1 << 20) + 1) == -1 and b"n_streams" in lib.fheaes_last_error(h)
    assert mac(kos=u32(0, 2)) == -1 and b"key_of_block" in lib.fheaes_last_error(h)
    assert mac(sb=u32(1, (1 << 16) + 1)) == -1 and b"stream_blocks" in lib.fheaes_last_error(h)
    assert mac(enc=o + (1 << 30), eb=u8([16, 17])) == -1 and b"enc_bytes" in lib.fheaes_last_error(h)
    assert mac(out=rk) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert mac(init=o) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert mac(enc=o, eb=u8([16, 16])) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert mac(n=0) == 0

    m0, m1 = ccm.message(0, "ex1"), ccm.message(1, "rfc1")
    from tfhe_aes_amd.server import ccm_args
    a = ccm_args([m0, m1])
    pairs = lambda x: _native.u128_pairs(x).ctypes.data_as(_native._u64p)
    u64 = lambda x: np.array(x, dtype=np.uint64).ctypes.data_as(_native._u64p)
    base = dict(rk=rk, bits=128, n_keys=2, n=2, kos=u32(0, 1), hb=u32(*a["head_blocks"]), head=pairs(a["head"]), ctr0=pairs(a["ctr0"]),
                pb=u64(a["payload_bytes"]), ct=u8(list(a["ciphertext"])), tags=u8(a["tags"]), tb=u32(*a["tag_bytes"]), pt=o, ok=v)

    def ccm_open(**kw):
        x = dict(base, **kw)
        return lib.fheaes_aes_ccm_open_keyed(h, x["rk"], x["bits"], x["n_keys"], x["n"], x["kos"], x["hb"], x["head"], x["ctr0"], x["pb"], x["ct"], x["tags"],
                                             x["tb"], x["pt"], x["ok"], D)

    for name in ("rk", "kos", "hb", "head", "ctr0", "pb", "ct", "tags", "tb", "pt", "ok"):
        assert ccm_open(**{name: None}) == -1, name
    assert ccm_open(bits=100) == -1 and ccm_open(n_keys=0) == -1 and ccm_open(n=(1 << 20) + 1) == -1
    assert ccm_open(kos=u32(0, 2)) == -1 and b"key_of_block" in lib.fheaes_last_error(h)
    for t in (2, 5, 18):
        assert ccm_open(tb=u32(t, 8)) == -1 and b"tag" in lib.fheaes_last_error(h)
    assert ccm_open(tb=u32(6, 8)) == -1 and b"B0" in lib.fheaes_last_error(h)                 # an allowed length that is not the one B0 states
    assert ccm_open(hb=u32(0, 2)) == -1 and b"head_blocks" in lib.fheaes_last_error(h)
    assert ccm_open(ctr0=pairs([a["ctr0"][0] & ((1 << 120) - 1), a["ctr0"][1]])) == -1 and b"nonce" in lib.fheaes_last_error(h)       # q - 1 = 0
    assert ccm_open(ctr0=pairs([a["ctr0"][0] | (8 << 120), a["ctr0"][1]])) == -1 and b"nonce" in lib.fheaes_last_error(h)
    assert ccm_open(ctr0=pairs([a["ctr0"][0] | 1, a["ctr0"][1]])) == -1 and b"counter" in lib.fheaes_last_error(h)
    assert ccm_open(pt=rk) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert ccm_open(ok=o) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert ccm_open(n=0) == 0
    for bad in (lambda: toy_server.aes_ccm_decrypt(d_rk, [(0, bytes(6), b"", b"", bytes(4))]),
                lambda: toy_server.aes_ccm_decrypt(d_rk, [(0, bytes(12), b"", b"", bytes(5))]),
                lambda: toy_server.aes_cbc_mac_streams(d_rk, [(0, [1], d_rk[0, :1], [17])])):
        with pytest.raises(ValueError):
            bad()
    toy_server.synchronize()
    assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
    assert bool((vrows == SENTINEL).all().item()) and guards_intact(vbuf)
    pt, ok, at = toy_server.aes_ccm_decrypt(keys["ab"], [])
    assert pt.shape == (0, 16, 8, p.big1) and ok.shape == (0, p.big1) and at == [0]
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_cbc_mac_keyed(keys["ab"], 128, 2, [0], [1], [[0] * 16], None, None, None, np.empty((1, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


# ---- one call at PARAM_OPT -------------------------------------------------------------------------------------------------------------------
# The `valid` bit is the one result a caller cannot check after decryption, and PARAM_OPT is where the guard's limit of 5 and the decision
# in front of K2 carry weight (34.6 sigma for a five-term sum; PARAM_TOY's noise is 2^-30 / 2^-50 and decides nothing).
OPT_VALID = [1, 1, 1, 0]


def _opt_messages():
    """examples 1 and 2 under their key, the RFC vector under its key, and example 1 again with one bit of its tag flipped"""
    k, nonce, aad, ct, tag = ccm.message(0, "ex1")
    return [ccm.message(0, "ex1"), ccm.message(0, "ex2"), ccm.message(1, "rfc1"), (k, nonce, aad, ct, tag[:3] + bytes([tag[3] ^ 0x01]))]


@pytest.fixture(scope="module")
def opt_keys(opt_server, oc):
    return opt_server.aes_key_expansion_many(np.stack([oc.encrypt_aes_key(k) for k in (KEY_A, KEY_B)]))


def opt_case(opt_server, opt_keys):
    if "opt" not in _results:
        _results["opt"] = opt_server.aes_ccm_decrypt(opt_keys, _opt_messages())
    return _results["opt"]


def test_opt_ccm_verdicts_plaintexts_and_the_composition(opt, opt_server, oc, opt_keys):
    p = opt.params
    messages = _opt_messages()
    pt, ok, at = opt_case(opt_server, opt_keys)
    assert at == [0, 1, 2, 4, 5] and pt.shape == (5, 16, 8, p.big1) and ok.shape == (4, p.big1)
    assert oc.decrypt_bits(ok).tolist() == OPT_VALID
    assert ccm.plaintext_of(oc, pt, at, messages) == [ccm.VECTORS[v][3] for v in ("ex1", "ex2", "rfc1", "ex1")]
    want_pt, want_ok, want_at = ccm.compose(opt_server, oc, opt_keys, messages)
    assert want_at == at
    assert np.array_equal(pt, want_pt), "%d plaintext words differ" % int((pt != want_pt).sum())
    assert np.array_equal(ok, want_ok), "%d valid words differ" % int((ok != want_ok).sum())


def test_opt_ccm_gated(opt, opt_server, oc, opt_keys):
    """gate=True: the forged message's plaintext decrypts to zero bytes, the other three as before, `valid` word for word what it was"""
    messages = _opt_messages()
    pt, ok, at = opt_case(opt_server, opt_keys)
    g_pt, g_ok, g_at = opt_server.aes_ccm_decrypt(opt_keys, messages, gate=True)
    assert g_at == at and np.array_equal(g_ok, ok) and oc.decrypt_bits(g_ok).tolist() == OPT_VALID
    assert ccm.plaintext_of(oc, g_pt, at, messages) == [ccm.VECTORS["ex1"][3], ccm.VECTORS["ex2"][3], ccm.VECTORS["rfc1"][3], bytes(4)]
    assert not oc.decrypt_bytes(g_pt[at[3]:]).any()
    assert ccm.plaintext_of(oc, pt, at, messages)[3] == ccm.VECTORS["ex1"][3]                     # ungated: it was there


def test_opt_noise_levels(opt, oc):
    """the payload link's X (2) + P (2) + the round key = 5 is the guard's limit at the parameter set the limit was made for"""
    srv = Server(opt.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        rk = srv.aes_key_expansion_many(np.stack([oc.encrypt_aes_key(KEY_A)]))
        _, ok, _ = srv.aes_ccm_decrypt(rk, [ccm.message(0, "ex1")])
        assert srv.engine.noise_level_seen() == (5, 5)
    finally:
        srv.engine.close()
    assert oc.decrypt_bits(ok).tolist() == [1]


def test_opt_tag_difference_noise(opt, opt_server, oc):
    """What the first tag WoPBS decides on, X + S0 + tag (level 4), for four messages with 16-byte tags under four keys: 64 bytes, no
    round-key word shared between two messages; the outputs of one byte share its GGSWs, so the bytes are counted (64).  The variance
    is noise_model.tag_difference_variance: the two aes_output_variance sums and the round-key word's term twice more, because X and
    S0 of one message add the SAME round-key ciphertext.  Every WoPBS term leaves its first CMUX out; the round key's is carried
    twice, so the bound of what is left out is (1 + 1 + 4) wopbs_left_out().  The ratio against the two sums alone is printed."""
    M = nm.NoiseModel.of_client(opt.client)
    ks = [bytes(np.random.default_rng(0xCC70 + i).integers(0, 256, 16, dtype=np.uint8).tolist()) for i in range(4)]
    rk = opt_server.aes_key_expansion_many(np.stack([oc.encrypt_aes_key(k) for k in ks]))
    messages = [ccm.own_message(i, ks[i], ccm.run(0x10 + i, 13), b"", ccm.run(0x20 + 16 * i, 16), 16) for i in range(4)]
    diff = ccm.tag_difference(opt_server, oc, rk, messages)
    err, vals = nm.wopbs_error(oc, diff)
    assert not vals.any()                                                                         # the tags are right: X + S0 + tag = 0
    var, two_sums = [], []
    for (k, nonce, aad, ct, tag), key in zip(messages, ks):
        s0 = aes_clear.aes_encrypt_block(key, aes_clear.ccm_blocks(nonce, aad, len(ct), 16)[2][0])
        v, t = nm.tag_difference_variance(M, key, _u128(tag) ^ s0, s0)
        var.append(v); two_sums.append(t)
    var, two_sums = np.stack(var), np.stack(two_sums)
    print("tag difference opt: mean(err^2) over the two aes_output_variance sums alone: %.3f" % float(np.mean(err.astype(np.float64) ** 2 / two_sums)))
    n = M.wopbs_independent(64, 8)
    assert n == 64 and err.shape == (4, 16, 8) and nm.rejects_doubling(n)
    nm.assert_noise(err, var, n, "tag difference opt", left_out=6 * M.wopbs_left_out())
