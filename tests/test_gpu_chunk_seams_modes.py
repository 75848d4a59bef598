"""The chunk seams of the later modes, at PARAM_TOY: XTS-AES decryption, AES-CCM with its tag check, CBC-MAC chains and the public calls
with a key per pool entry, each run once across the seams test_gpu_chunk_seams.py was written before (tests/chunk_seams.py, part F, has
the shapes and why each is the smallest that crosses; test_chunk_seams_modes_cpu.py pins them without a GPU).  The seams: the 256 blocks
or slots of one grid pass of xts_whiten_kernel and mac_link_kernel, the 2^20 workgroups of bit_rows_kernel<XtsRows>, the 4,096 bytes of one chunk
of a byte WoPBS inside aes_xts_decrypt_dev, ccm_open_dev, cbc_mac_dev and aes_public_dev, and the 128 inputs of one chunk of the 16-bit
tag WoPBS.  The house rules of the older file hold: a context of its own per test, resident outputs between sentinel guard rows, every
word comparison array_equal / torch.equal on uint64 words, data that differs on both sides of every seam, and the crossing asserted from
the profile counters against a count chunk_seams.py derives by restating the rule."""
import numpy as np
import pytest

import ccm
import chunk_seams as cs
import xts
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, settled, tc  # noqa: F401
from test_gpu_ccm import _edge_blocks
from test_gpu_xts import KEY1, KEY2, _anchor
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server

pytestmark = pytest.mark.gpu

OFF = _native.AES_WINDOW_OFF
NONE = _native.MAC_NONE
SEAM = cs.SLOTS_PER_PASS                                 # 256: the first block or slot of the second grid pass


def _stage(prof, name, launches, units):
    assert (prof[name]["launches"], prof[name]["units"]) == (launches, units), "%s: %r" % (name, prof[name])


def _differ(got, want):
    return "%d words differ" % int((got != want).sum())


def _blocks_with_edges(p, n, seed):
    """n random blocks [n][16][8][kN+1] with the edge-word blocks of test_gpu_ccm at 0, 255 and 256: the last of the first pass and the
    first of the second sum wrapping words"""
    a = cs.random_words(seed, (n, 16, 8, p.big1))
    at = [i for i in (0, SEAM - 1, SEAM) if i < n]
    a[at] = _edge_blocks(p, len(at), seed + 1)
    return a


def _encrypt_round_keys(client, clear):
    """clear round keys [n_keys][11][16] encrypted byte by byte: [n_keys][11][16][8][kN+1]"""
    clear = np.asarray(clear, dtype=np.uint8)
    return client.encrypt_bytes(clear.reshape(-1)).reshape(clear.shape + (8, -1))


def _u128(data):
    return int.from_bytes(data, "big")


# ---- 1. fheaes_xts_whiten alone ----------------------------------------------------------------------------------------------------------
def _whiten_inputs(p):
    n = cs.WHITEN_BLOCKS
    tweaks = _edge_blocks(p, cs.WHITEN_TWEAKS, 0xF10)
    src = _blocks_with_edges(p, n, 0xF11)
    clear = np.random.default_rng(0xF13).integers(0, 256, (n, 16), dtype=np.uint8)
    clear[SEAM - 1], clear[SEAM] = 0xFF, 0x00
    return tweaks, src, clear, cs.whiten_table()


def test_xts_whiten_second_pass_of_the_block_loop(toy, tc):
    """launch_xts_whiten / xts_whiten_kernel: gridDim.y is capped at 16,384 / 64 = 256 blocks and block 256 comes from the
    `blk += gridDim.y` loop.  257 blocks over 5 tweak rows through a table that is not monotone and sends block 256 to another row than
    blocks 0 and 255; edge words at blocks 0, 255 and 256; clear bytes 0xFF at block 255 and 0 at block 256.  The three forms (no src, a
    separate src, in place -- that one with and without clear bytes) against numpy, then host arrays through the staging path"""
    p, n = toy.params, cs.WHITEN_BLOCKS
    tweaks, src, clear, tab = _whiten_inputs(p)
    trivial = tc.trivial_bytes(clear)
    eng = _native.Engine(p, device=0)                                        # no keys: the whitening needs none
    try:
        d_tweaks, d_src = dev(tweaks), dev(src)
        assert eng.noise_level_seen() == (0, 5)
        cases = [("no src", None, clear, tweaks[tab] + trivial, 2), ("a separate src", d_src, clear, tweaks[tab] + src + trivial, 3),
                 ("in place", "dst", clear, tweaks[tab] + src + trivial, 3), ("in place, no clear bytes", "dst", None, tweaks[tab] + src, 3)]
        for what, s, clr, want, level in cases:
            buf, rows = guarded(n * 128, p.big1)
            d_dst = rows.view(n, 16, 8, p.big1)
            if s == "dst":
                settled(d_dst.copy_(d_src))
            eng.profile_reset()
            eng.xts_whiten(d_dst, d_dst if s == "dst" else s, d_tweaks, tab, clr)
            eng.synchronize()
            _stage(eng.profile_read(), "linear", 1, n)
            got = host(d_dst)
            assert guards_intact(buf), what
            assert np.array_equal(got, want), "%s: %s" % (what, _differ(got, want))
            assert eng.noise_level_seen() == (level, 5), what                # 2 without src (tweak + block), 3 with
        out = np.empty_like(src)                                             # host arrays take the same path through staging
        eng.xts_whiten(out, src, tweaks, tab, clear)
        assert np.array_equal(out, tweaks[tab] + src + trivial)
        h_state = src.copy()
        eng.xts_whiten(h_state, h_state, tweaks, tab, None)
        assert np.array_equal(h_state, tweaks[tab] + src)
    finally:
        eng.close()


def test_xts_whiten_refusals(toy):
    p = toy.params
    eng = _native.Engine(p, device=0)
    try:
        lib, h, D = eng._lib, eng._h, _native.DEVICE
        d_tw = dev(_edge_blocks(p, 2, 2))
        buf, rows = guarded(3 * 128, p.big1)
        u32 = lambda *v: np.array(v, dtype=np.uint32).ctypes.data_as(_native._u32p)
        clear = np.zeros(48, dtype=np.uint8).ctypes.data_as(_native._u8p)
        many = np.zeros((1 << 20) + 1, dtype=np.uint32)
        dst, tw, block = rows.data_ptr(), d_tw.data_ptr(), 128 * p.big1 * 8
        assert lib.fheaes_xts_whiten(h, None, None, tw, 2, u32(0, 1), clear, 2, D) == -1
        assert lib.fheaes_xts_whiten(h, dst, None, None, 2, u32(0, 1), clear, 2, D) == -1
        assert lib.fheaes_xts_whiten(h, dst, None, tw, 2, None, clear, 2, D) == -1
        assert lib.fheaes_xts_whiten(h, dst, None, tw, 2, u32(0, 2), clear, 2, D) == -1 and b"tweak_of_block" in lib.fheaes_last_error(h)
        assert lib.fheaes_xts_whiten(h, dst, None, dst, 2, u32(0, 1), clear, 2, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_xts_whiten(h, dst, dst + block, tw, 2, u32(0, 1), clear, 2, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_xts_whiten(h, dst, None, tw, 2, many.ctypes.data_as(_native._u32p), None, (1 << 20) + 1, D) == -1
        assert lib.fheaes_xts_whiten(h, dst, None, tw, 2, u32(0, 1), clear, 0, D) == 0
        eng.synchronize()
        assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
        assert eng.noise_level_seen() == (0, 5)
    finally:
        eng.close()


# ---- 2. fheaes_mac_link over 257 slots --------------------------------------------------------------------------------------------------
def test_mac_link_second_pass_of_the_slot_loop(toy, tc):
    """launch_mac_link / mac_link_kernel: the same cap, slot 256 comes from the `s += gridDim.y` loop.  257 slots read 259 addend blocks:
    slot 256 reads block 0 and slot 0 block 258, slot 255 none; enc_bytes cycles through 0, 1, 15 and 16 with 5 at slot 256; edge words at
    slots 0, 255 and 256 of state, init and enc.  The five cases of test_gpu_ccm.test_link_kernel_is_the_sum against ccm.np_link"""
    p, n = toy.params, cs.LINK_SLOTS
    state, init, enc = _blocks_with_edges(p, n, 0xF21), _blocks_with_edges(p, n, 0xF23), _blocks_with_edges(p, cs.LINK_ENC, 0xF25)
    clear = np.random.default_rng(0xF27).integers(0, 256, (n, 16), dtype=np.uint8)
    clear[0], clear[SEAM - 1], clear[SEAM] = 0xFF, 0, 0xA5
    src, eb = cs.link_tables()
    assert NONE == cs.MAC_NONE
    eng = _native.Engine(p, device=0)                                        # no keys: the link needs none
    try:
        d_init, d_enc, d_start = dev(init), dev(enc), dev(state)
        cases = [("public step", False, None, None), ("payload step", False, None, d_enc), ("first with init", True, d_init, d_enc),
                 ("first without init", True, None, d_enc), ("first, clear only", True, None, None)]
        for what, first, ini, e in cases:
            want = ccm.np_link(tc, state, first, None if ini is None else init, None if e is None else enc, src, eb, clear)
            buf, rows = guarded(n * 128, p.big1)
            d_state = rows.view(n, 16, 8, p.big1)
            settled(d_state.copy_(d_start))
            eng.profile_reset()
            eng.mac_link(d_state, first, ini, e, src, eb, clear)
            eng.synchronize()
            _stage(eng.profile_read(), "linear", 1, n)
            got = host(d_state)
            assert guards_intact(buf), what
            assert np.array_equal(got, want), "%s: %s" % (what, _differ(got, want))
    finally:
        eng.close()


# ---- 3. fheaes_xts_tweaks behind the 2^20-workgroup cap ------------------------------------------------------------------------------------
def _tweak_sources():
    """[4] index tensors on the device over the 122 x 128 output rows: term t of every row of xts.rows(j), 128 (a row of zeros) where a
    row has fewer terms"""
    import torch

    idx = np.full((4, cs.TWEAK_OFFSETS, 128), 128, dtype=np.int64)
    for j in range(cs.TWEAK_OFFSETS):
        for i, sources in enumerate(xts.rows(j)):
            idx[:len(sources), j, i] = sources
    return [settled(torch.from_numpy(idx[t].reshape(-1)).cuda()) for t in range(4)]


def test_xts_tweaks_second_pass_behind_the_grid_cap(toy):
    """launch_xts_tweaks / bit_rows_kernel<XtsRows>: the grid is capped at 2^20 workgroups = 8,192 tweak blocks and the rows from 2^20 on come
    from the `r += gridDim.x` loop.  68 units x 122 offsets = 8,296 tweak blocks = 1,061,888 rows is the smallest shape that crosses (67
    units stay below); the second pass starts at unit 67, offset 18.  4.36 GB of output stay on the GPU: every unit is compared there with
    the wrapping sum of index_select over the source lists of xts.rows(j), and unit 0 and offsets 17..19 of unit 67 -- and the device
    reference itself there -- with xts.np_tweaks on the host"""
    import torch

    p, units, n_off = toy.params, cs.TWEAK_UNITS, cs.TWEAK_OFFSETS
    assert units * n_off == cs.TWEAK_BLOCKS > cs.TWEAK_ROWS_PER_PASS >= (units - 1) * n_off
    anchor = _anchor(p, units, 0xF30)
    assert len({a.tobytes() for a in anchor[:, 5]}) == units                  # an anchor of its own per unit
    eng = _native.Engine(p, device=0)                                        # no keys: the gather needs none
    buf = rows = out = None
    try:
        d_anchor = dev(anchor)
        buf, rows = guarded(units * n_off * 128, p.big1)
        eng.profile_reset()
        eng.xts_tweaks(d_anchor, units, 0, n_off, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "linear", 1, cs.TWEAK_BLOCKS)
        assert guards_intact(buf)
        sources = _tweak_sources()
        zero = torch.zeros((1, p.big1), dtype=torch.int64, device="cuda")
        out = rows.view(units, n_off * 128, p.big1)

        def expected(u):
            ext = torch.cat([d_anchor[u], zero])
            return ext.index_select(0, sources[0]) + ext.index_select(0, sources[1]) + ext.index_select(0, sources[2]) + ext.index_select(0, sources[3])

        wrong = [u for u in range(units) if not torch.equal(out[u], expected(u))]
        assert not wrong, "units %s differ from the device reference" % wrong
        seam_u, seam_off = cs.TWEAK_SEAM
        offs = [seam_off - 1, seam_off, seam_off + 1]
        assert (seam_u, offs) == (67, [17, 18, 19])
        lo, hi = offs[0] * 128, (offs[-1] + 1) * 128
        want0, want_seam = xts.np_tweaks(anchor[0], range(n_off)), xts.np_tweaks(anchor[seam_u], offs)
        got0, got_seam = host(settled(out[0])).reshape(want0.shape), host(settled(out[seam_u, lo:hi])).reshape(want_seam.shape)
        assert np.array_equal(got0, want0), "unit 0: " + _differ(got0, want0)
        assert np.array_equal(got_seam, want_seam), "unit 67, offsets 17..19: " + _differ(got_seam, want_seam)
        assert np.array_equal(host(settled(expected(0))).reshape(want0.shape), want0)
        assert np.array_equal(host(settled(expected(seam_u)[lo:hi])).reshape(want_seam.shape), want_seam)
    finally:
        eng.close()
        del buf, rows, out
        torch.cuda.empty_cache()


# ---- 4. XTS-AES decryption across the whitening, refresh and plan seams ------------------------------------------------------------------
@pytest.fixture(scope="module")
def xts_case(tc):
    """decryption round keys of KEY1 and round keys of KEY2 encrypted byte by byte from the clear ones, and blocks 121 .. 486 of four units
    of 122 blocks with four sector numbers: (dw1, rk2, sectors, plaintext, ciphertext) of the call's 366 blocks"""
    dw1 = _encrypt_round_keys(tc, aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(KEY1)))
    rk2 = _encrypt_round_keys(tc, aes_clear.expand_key(KEY2))
    sectors, bpu = list(cs.XTS_SECTORS), cs.XTS_BPU
    pt = np.random.default_rng(0xF40).bytes(16 * bpu * len(sectors))
    ct = b"".join(aes_clear.xts_encrypt(KEY1, KEY2, sectors[u], pt[16 * bpu * u:16 * bpu * (u + 1)]) for u in range(len(sectors)))
    lo, hi = 16 * cs.XTS_FIRST, 16 * (cs.XTS_FIRST + cs.XTS_BLOCKS)
    return dw1, rk2, sectors, pt[lo:hi], ct[lo:hi]


def test_xts_decrypt_across_the_whitening_refresh_and_plan_seams(toy, tc, xts_case):
    """aes_xts_decrypt_dev and xts_plan: blocks 121 .. 486 of units of 122 blocks.  The first unit has block 121 alone, so its segment 0
    yields the anchor only (lo = XTS_SEGMENT); the class of the two whole units gathers segment 1 from anchors that lie
    anchor_stride_rows = 121 rows apart behind the first class's row; all three classes have two segments.  Segment 0 has 364 tweak
    rows = 5,824 bytes: the identity WoPBS takes two chunks; blocks 256 .. 365 are in the second pass of both whitenings.  Round by round
    the key switch launches 10 times for the four tweak blocks, 1 + 2 + 1 times for the anchors and the two segments and 10 x 2 times in
    the cipher: 34.  The words are xts.compose's (older entry points and numpy), the plaintext is aes_clear's unit by unit, and blocks 0,
    1, 255, 256 and 365 are the words of the call on that one block"""
    p, n, bpu, first = toy.params, cs.XTS_BLOCKS, cs.XTS_BPU, cs.XTS_FIRST
    dw1, rk2, sectors, pt, ct = xts_case
    parts = cs.xts_keyswitch(_native.aes_public_plan([aes_clear.xts_tweak_block(v) for v in sectors]))
    launches, units = cs.total(parts)
    assert launches == 34, parts
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(OFF)
        d_dw1, d_rk2 = dev(dw1), dev(rk2)
        buf, rows = guarded(n * 128, p.big1)
        eng.profile_reset()
        out = srv.aes_xts_decrypt(d_dw1, d_rk2, sectors, ct, unit_bytes=16 * bpu, first_block=first, out=rows.view(n, 16, 8, p.big1))
        srv.synchronize()
        prof = eng.profile_read()
        print("xts keyswitch: %r, derived %r" % (prof["keyswitch"], parts))
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert out.is_cuda and guards_intact(buf)
        got = host(rows).reshape(n, 16, 8, p.big1)
        want, _ = xts.compose(srv, tc, dw1, rk2, sectors, ct, bpu, first)
        assert np.array_equal(got, want), _differ(got, want)
        assert np.array_equal(tc.decrypt_bytes(got), np.frombuffer(pt, dtype=np.uint8).reshape(-1, 16))
        for u, sector in enumerate(sectors):                                  # the clear mode, unit by unit
            lo, hi = max(u * bpu, first) - first, min((u + 1) * bpu, first + n) - first
            assert aes_clear.xts_decrypt(KEY1, KEY2, sector, ct[16 * lo:16 * hi], first_block=(first + lo) % bpu) == pt[16 * lo:16 * hi], u
        for b in cs.XTS_ALONE:                                                # a shard needs nothing from its neighbours
            alone = srv.aes_xts_decrypt(dw1, rk2, sectors, ct[16 * b:16 * b + 16], unit_bytes=16 * bpu, first_block=first + b)
            assert np.array_equal(got[b], alone[0]), "block %d: %s" % (b, _differ(got[b], alone[0]))
    finally:
        eng.close()


def test_xts_decrypt_from_packed_stores_across_the_seams(toy, tc, xts_case):
    """the same call with both keys read from packed stores: the words of the call on the unpacked stores, and the plaintext"""
    p, bpu, first = toy.params, cs.XTS_BPU, cs.XTS_FIRST
    dw1, rk2, sectors, pt, ct = xts_case
    srv = Server(toy.keys, device=0)
    try:
        p1, p2 = srv.pack_round_keys(dw1), srv.pack_round_keys(rk2)
        got = srv.aes_xts_decrypt(p1, p2, sectors, ct, unit_bytes=16 * bpu, first_block=first)
        unpacked = srv.aes_xts_decrypt(srv.unpack_round_keys(p1)[0], srv.unpack_round_keys(p2)[0], sectors, ct, unit_bytes=16 * bpu, first_block=first)
        assert got.shape == (cs.XTS_BLOCKS, 16, 8, p.big1) and np.array_equal(got, unpacked), _differ(got, unpacked)
        assert np.array_equal(tc.decrypt_bytes(got), np.frombuffer(pt, dtype=np.uint8).reshape(-1, 16))
    finally:
        srv.engine.close()


# ---- 5. CCM with 257 messages under 3 keys, and CBC-MAC chains over 257 streams ------------------------------------------------------------
@pytest.fixture(scope="module")
def keys3(tc):
    """3 clear AES-128 keys and their round keys encrypted byte by byte: (keys, [3][11][16][8][kN+1])"""
    rng = np.random.default_rng(0xF50)
    keys = [rng.bytes(16) for _ in range(cs.CCM_KEYS)]
    return keys, _encrypt_round_keys(tc, [aes_clear.expand_key(k) for k in keys])


@pytest.fixture(scope="module")
def ccm_case(keys3):
    """the 257 messages of chunk_seams.ccm_shape with distinct 13-byte nonces, the rejected ones corrupted: one bit of the last compared
    tag byte, at position 256 one ciphertext bit.  (messages, the verdict of every message)"""
    keys, _ = keys3
    rng = np.random.default_rng(0xF51)
    messages = []
    for i in range(cs.CCM_MESSAGES):
        k, aad, payload, t = cs.ccm_shape(i)
        messages.append(ccm.own_message(k, keys[k], rng.bytes(12) + bytes([i & 0xFF]) if i < 256 else b"\xff" * 13, rng.bytes(aad), rng.bytes(payload), t))
    assert len({m[1] for m in messages}) == cs.CCM_MESSAGES and all(len(m[1]) == 13 for m in messages)
    for i in cs.CCM_BAD:
        k, nonce, aad, ct, tag = messages[i]
        if i == cs.CCM_BAD_CIPHERTEXT:
            ct = ct[:2] + bytes([ct[2] ^ 0x20]) + ct[3:]
        else:
            tag = tag[:-1] + bytes([tag[-1] ^ (1 << (i % 8))])
        messages[i] = (k, nonce, aad, ct, tag)
    return messages, [0 if i in cs.CCM_BAD else 1 for i in range(cs.CCM_MESSAGES)]


def _ccm_public_plan(messages):
    """the pool of every round of the call's public batch -- B0, Ctr_0 and the payload counters of every message under its key -- from
    fheaes_aes_public_plan_keyed (host code with CPU tests of its own); the clear data of the last layer does not enter a pool"""
    blocks, keys = [], []
    for k, nonce, aad, ct, tag in messages:
        b0, _, ctr = aes_clear.ccm_blocks(nonce, aad, len(ct), len(tag))
        blocks += [b0] + ctr
        keys += [k] * (1 + len(ctr))
    return _native.aes_public_plan_keyed(blocks, keys, cs.CCM_KEYS)


def test_ccm_of_257_messages_under_3_keys(toy, tc, keys3, ccm_case):
    """ccm_open_dev: 257 messages.  The 8-bit tag WoPBS runs over 16 x 257 = 4,112 bytes (2 chunks, message 256 alone in the second), the
    16-bit one over 257 inputs at 128 a chunk (the 2 GiB CMUX-tree bound: 128 + 128 + 1), and both hipMemcpy2DAsync row gathers run over
    more than one chunk of output.  The pools of the public call (522 blocks) are above 4,096 entries from round 2 on with the key of
    every entry in its head word.  Five messages chain blocks (positions 0, 127, 128, 255, 256: lengths 2, 6, 3, 3, 3), so the stable
    sort moves them to slots 4, 0, 1, 2, 3 and every other message four or two slots back -- message 254 to slot 256, across the pass of
    mac_link_kernel; the live prefixes are 5, 5, 4, 1, 1, 1 (no prefix of a CCM call with these messages is above 256: that is
    test_mac_streams_over_257_streams), but the first link, the tag difference and the final gathers run over all 257 slots and start
    from public blocks 8 + s and 265 + s, above 255 (the plaintext records read public blocks 0..7: the engine puts the payload counters
    first).  The key changes across 128 and across 256, the rejected positions are periodic in neither"""
    p, n = toy.params, cs.CCM_MESSAGES
    clear_keys, rk = keys3
    messages, valid = ccm_case
    five = sorted(cs.CCM_LONG)
    lengths, payload_blocks = cs.ccm_stream_blocks()
    plan = _ccm_public_plan(messages)
    assert sum(plan) > 0 and all(v > cs.CHUNK_BYTES for v in plan[1:])
    assert _native.aes_mac_plan(lengths, payload_blocks)["n_active"] == cs.live_prefixes(lengths) == [5, 5, 4, 1, 1, 1]
    parts = cs.ccm_keyswitch(plan, cs.live_prefixes(lengths))
    assert (parts["tag_bytes"][0], parts["tag_tree"][0]) == (2, 3)
    launches, units = cs.total(parts)
    total = sum(payload_blocks)
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(OFF)
        d_rk = dev(rk)
        buf, rows = guarded(total * 128, p.big1)
        vbuf, vrows = guarded(n, p.big1)
        eng.profile_reset()
        d_pt, d_ok, at = srv.aes_ccm_decrypt(d_rk, messages, out=rows.view(total, 16, 8, p.big1), valid_out=vrows)
        srv.synchronize()
        prof = eng.profile_read()
        print("ccm keyswitch: %r, vertical packing: %r, derived %r" % (prof["keyswitch"], prof["vertical_packing"], parts))
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert prof["vertical_packing"]["launches"] == launches
        assert guards_intact(buf) and guards_intact(vbuf)
        pt, ok = host(d_pt), host(d_ok)
        assert at == [sum(payload_blocks[:i]) for i in range(n + 1)] and ok.shape == (n, p.big1)
        assert tc.decrypt_bits(ok).tolist() == valid
        payloads = [aes_clear._ccm_ctr(clear_keys[k], aes_clear.ccm_blocks(nonce, aad, len(ct), len(tag))[2], ct) for k, nonce, aad, ct, tag in messages]
        assert ccm.plaintext_of(tc, pt, at, messages) == payloads
        for i, (k, nonce, aad, ct, tag) in enumerate(messages):
            opened = aes_clear.ccm_decrypt(clear_keys[k], nonce, aad, ct + tag, len(tag))
            assert (opened is not None) == bool(valid[i]) and opened in (None, payloads[i]), i
            if len(ct) % 16:                                                # rows beyond the payload's length are zero words
                assert not pt[at[i + 1] - 1].reshape(128, p.big1)[8 * (len(ct) % 16):].any(), i
        for i in five:                                                        # sharing is invisible: the message alone gives the same words
            a_pt, a_ok, _ = srv.aes_ccm_decrypt(rk, [messages[i]])
            assert np.array_equal(a_ok[0], ok[i]), "valid bit of message %d: %s" % (i, _differ(a_ok[0], ok[i]))
            assert np.array_equal(a_pt, pt[at[i]:at[i + 1]]), "plaintext of message %d: %s" % (i, _differ(a_pt, pt[at[i]:at[i + 1]]))
        c_pt, c_ok, c_at = ccm.compose(srv, tc, rk, [messages[i] for i in five])     # older entry points and numpy, on the five alone
        for j, i in enumerate(five):
            assert np.array_equal(c_ok[j], ok[i]), "valid bit of message %d against the composition" % i
            assert np.array_equal(c_pt[c_at[j]:c_at[j + 1]], pt[at[i]:at[i + 1]]), "plaintext of message %d against the composition" % i
    finally:
        eng.close()


def test_ccm_of_257_messages_from_a_packed_store(toy, tc, keys3, ccm_case):
    """the same call with the three keys in a packed store: the words of the call on the unpacked store, and the verdicts"""
    _, rk = keys3
    messages, valid = ccm_case
    srv = Server(toy.keys, device=0)
    try:
        packed = srv.pack_round_keys(rk)
        got = srv.aes_ccm_decrypt(packed, messages)
        unpacked = srv.aes_ccm_decrypt(srv.unpack_round_keys(packed), messages)
        assert got[2] == unpacked[2]
        assert np.array_equal(got[0], unpacked[0]), _differ(got[0], unpacked[0])
        assert np.array_equal(got[1], unpacked[1]), _differ(got[1], unpacked[1])
        assert tc.decrypt_bits(got[1]).tolist() == valid
    finally:
        srv.engine.close()


def test_mac_streams_over_257_streams(toy, tc, keys3):
    """cbc_mac_dev / aes_cbc_mac: 257 streams of one block, but three blocks at streams 0 and 256 and none at stream 255.  The sort puts
    stream 256 at slot 1 and the empty stream 255 at slot 256; the first link runs over all 257 slots with init indices above 255 (slot
    256 copies init[255]: got[255] is init[255] word for word), the first cipher pass over the 256 live slots, then the live prefix is 2;
    the final copy into the caller's order reads slot 256 and writes stream 256 from slot 1.  Stream 256 carries an encrypted addend
    whose last block has 5 real bytes (enc index above 255).  Streams 0, 1, 255 and 256 each alone give the same words"""
    p, n = toy.params, cs.MAC_STREAMS
    clear_keys, rk = keys3
    lengths = cs.mac_lengths()
    rng = np.random.default_rng(0xF53)
    key_of = [cs.ccm_shape(s)[0] for s in range(n)]
    blocks = [[_u128(rng.bytes(16)) for _ in range(k)] for k in lengths]
    init_clear = [_u128(rng.bytes(16)) for _ in range(n)]
    init = tc.encrypt_bytes(np.array([list(v.to_bytes(16, "big")) for v in init_clear], dtype=np.uint8).reshape(-1)).reshape(n, 16, 8, p.big1)
    addend = [_u128(rng.bytes(16)), _u128(rng.bytes(16)), _u128(rng.bytes(5)) << 88]
    enc = np.stack([tc.encrypt_u128(addend[0]), tc.encrypt_u128(addend[1]), tc.encrypt_u128(addend[2] | 0xA5A5A5)])      # bytes 13..15 of the last are not real
    streams = [(key_of[s], blocks[s], None, None) for s in range(n)]
    streams[n - 1] = (key_of[n - 1], blocks[n - 1], enc, [16, 16, 5])
    n_active = cs.live_prefixes(lengths)
    assert n_active == _native.aes_mac_plan(lengths)["n_active"] == [SEAM, 2, 2]
    launches, units = cs.chain_keyswitch(n_active)
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(OFF)
        d_rk, d_init, d_enc = dev(rk), dev(init), dev(enc)
        d_streams = list(streams)
        d_streams[n - 1] = (key_of[n - 1], blocks[n - 1], d_enc, [16, 16, 5])
        buf, rows = guarded(n * 128, p.big1)
        eng.profile_reset()
        srv.aes_cbc_mac_streams(d_rk, d_streams, init=d_init, out=rows.view(n, 16, 8, p.big1))
        srv.synchronize()
        prof = eng.profile_read()
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert guards_intact(buf)
        got = host(rows).reshape(n, 16, 8, p.big1)
        assert np.array_equal(got[SEAM - 1], init[SEAM - 1])                  # the stream of no blocks keeps where it starts
        for s in cs.MAC_ALONE:
            alone = srv.aes_cbc_mac_streams(rk, [streams[s]], init=init[s:s + 1])
            assert np.array_equal(got[s], alone[0]), "stream %d: %s" % (s, _differ(got[s], alone[0]))
        chained = [list(b) for b in blocks]
        chained[n - 1] = [b ^ a for b, a in zip(blocks[n - 1], addend)]
        macs = [aes_clear.cbc_mac(clear_keys[key_of[s]], chained[s], init=init_clear[s]) for s in range(n)]
        assert [_u128(bytes(b.tolist())) for b in tc.decrypt_bytes(got)] == macs
    finally:
        eng.close()


# ---- 6. keyed public calls with pools above one chunk ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def public_keys(tc):
    """3 clear AES-128 keys, their round keys and their decryption round keys, encrypted byte by byte"""
    rng = np.random.default_rng(0xF60)
    keys = [rng.bytes(16) for _ in range(cs.PUBLIC_KEYS)]
    expanded = [aes_clear.expand_key(k) for k in keys]
    return keys, _encrypt_round_keys(tc, expanded), _encrypt_round_keys(tc, [aes_clear.inv_mix_columns_round_keys(e) for e in expanded])


@pytest.mark.parametrize("source", ["lwe", "packed"])
@pytest.mark.parametrize("direction", ["encrypt", "decrypt"])
def test_keyed_public_blocks_with_pools_above_one_chunk(toy, tc, public_keys, direction, source):
    """aes_public_dev with a key per pool entry: 300 random blocks under 3 keys share nothing from round 2 on, so the pools have 4,800
    entries and every entry behind the WoPBS seam at 4,096 takes its round key from the key field (h >> 16) of its head word; the pool of
    round 1 has the distinct (key, position, byte) triples, one chunk.  Blocks 0, 255, 256 and 299 alone under their own key give the same
    words; from a packed store the call gives the words of the call on the unpacked store"""
    p, n = toy.params, cs.PUBLIC_BLOCKS
    clear_keys, rk, dw = public_keys
    blocks, kob, data = cs.public_keyed_blocks()
    inverse = direction == "decrypt"
    if inverse:
        plan = _native.aes_decrypt_public_plan_keyed(blocks, kob, cs.PUBLIC_KEYS)
        want = [aes_clear.aes_decrypt_block(clear_keys[k], v) ^ d for k, v, d in zip(kob, blocks, data)]
    else:
        plan, data = _native.aes_public_plan_keyed(blocks, kob, cs.PUBLIC_KEYS), None
        want = [aes_clear.aes_encrypt_block(clear_keys[k], v) for k, v in zip(kob, blocks)]
    launches, units = sum(cs.byte_wopbs(v)[0] for v in plan), sum(cs.byte_wopbs(v)[1] for v in plan)
    assert launches == 1 + 2 * 9 and units == 8 * sum(plan)
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        call = srv.aes_decrypt_public_keyed if inverse else srv.aes_encrypt_public_keyed
        d_keys = dev(dw if inverse else rk)
        if source == "packed":
            d_keys = srv.pack_round_keys(d_keys)
            srv.synchronize()
        buf, rows = guarded(n * 128, p.big1)
        eng.profile_reset()
        call(d_keys, kob, blocks, data=data, out=rows.view(n, 16, 8, p.big1))
        srv.synchronize()
        prof = eng.profile_read()
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert prof["linear"]["launches"] == 11
        assert guards_intact(buf)
        got = host(rows).reshape(n, 16, 8, p.big1)
        if source == "packed":
            unpacked = call(srv.unpack_round_keys(d_keys), kob, blocks, data=data)
            srv.synchronize()
            assert np.array_equal(got, host(unpacked).reshape(got.shape)), _differ(got, host(unpacked).reshape(got.shape))
        for b in cs.PUBLIC_ALONE:
            alone = call(d_keys, [kob[b]], [blocks[b]], data=None if data is None else [data[b]])
            srv.synchronize()
            assert np.array_equal(got[b], host(alone)[0]), "block %d: %s" % (b, _differ(got[b], host(alone)[0]))
        assert [tc.decrypt_u128(got[b]) for b in range(n)] == want
    finally:
        eng.close()
