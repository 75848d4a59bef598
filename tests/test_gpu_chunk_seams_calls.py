"""The chunk seams of the calls that came after test_gpu_chunk_seams_modes.py, at PARAM_TOY: AES-CMAC (cmac_subkeys_dev, cmac_dev), the AES
key unwrap (kw_unwrap_dev) and the gate (gate_call, gate_table, launch_gate), each run once past one chunk (tests/chunk_seams.py, part G,
has the shapes and why each is the smallest that crosses; test_chunk_seams_calls_cpu.py pins them without a GPU).  The seams: the 4,096
bytes of one chunk of a byte WoPBS inside the subkey derivation, the CMAC chain, the unwrap's cipher passes and its payload refresh; the
256 slots or keys of one grid pass of mac_link_kernel and kw_link_kernel; the 128 inputs of one chunk of the 16-bit tag WoPBS; the 65,536
workgroups of one launch of gate_kernel; the 32,768 gates of one circuit bootstrap of a gate call.  All of it is host pointer arithmetic
for a second chunk, which a 10-stream test cannot see.  The house rules of the two older files hold: a context of its own per test,
resident outputs between sentinel guard rows, every word comparison array_equal / torch.equal on uint64 words, data that differs on both
sides of every seam, and the crossing asserted from the profile counters against a count chunk_seams.py derives by restating the rule."""
import numpy as np
import pytest

import ccm
import chunk_seams as cs
import cmac
import gate_model as gm
import keywrap
from gpu_support import SENTINEL, dev, filled, guarded, guards_intact, host, settled, tc  # noqa: F401
from test_gpu_gate import _fourier, _inputs
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server

pytestmark = pytest.mark.gpu

OFF = _native.AES_WINDOW_OFF
LWE, GLWE = _native.GATE_LWE, _native.GATE_GLWE
VALID7 = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)                     # the gates of test_gates_beyond_one_chunk: period 7
BITS5 = np.array([1, 1, 0, 1, 1], dtype=np.uint8)                            # and its bits: period 5


def _stage(prof, name, launches, units):
    assert (prof[name]["launches"], prof[name]["units"]) == (launches, units), "%s: %r" % (name, prof[name])


def _differ(got, want):
    return "%d words differ" % int((got != want).sum())


def _u128(data):
    return int.from_bytes(data, "big")


def _blocks(tc, words):
    """[..][16][8][kN+1] on the host -> the decrypted 16-byte blocks"""
    return [bytes(b.tolist()) for b in tc.decrypt_bytes(words.reshape(-1, 16, 8, words.shape[-1]))]


def _flip(data, i, bit):
    return data[:i] + bytes([data[i] ^ bit]) + data[i + 1:]


# ---- the AES keys of A and B: 259 sets of round keys, resident ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store259(toy, tc):
    """(259 clear AES-128 keys, the SP 800-38B key at index 256; their round keys [259][11][16][8][kN+1], expanded on the GPU and left
    there: 1.5 GB; K1 and K2 of every key by aes_clear, one behind the other)"""
    rng = np.random.default_rng(0x6A0)
    clear = [rng.bytes(16) for _ in range(cs.CMAC_STORE_KEYS)]
    clear[cs.CMAC_VECTOR_KEY] = cmac.VECTORS[128][0]
    assert len(set(clear)) == cs.CMAC_STORE_KEYS
    srv = Server(toy.keys, device=0)
    try:
        d_rk = srv.aes_key_expansion_many(dev(np.stack([tc.encrypt_aes_key(k) for k in clear])))
        srv.synchronize()
    finally:
        srv.engine.close()
    return clear, d_rk, [v for k in clear for v in aes_clear.cmac_subkeys(k)]


def _subkey_plan(m):
    """the pools of the public call on one zero block under each of m keys"""
    return _native.aes_public_plan_keyed([0] * m, list(range(m)), m)


# ---- A. CMAC subkeys of 257 keys -------------------------------------------------------------------------------------------------------------
def test_cmac_subkeys_of_257_keys(toy, tc, store259):
    """cmac_subkeys_dev over 257 keys: the public call on 257 zero blocks that share nothing (pools of 4,112 entries in every round, round
    1 included, the key in the head word), the identity WoPBS over 4,112 bytes of L (2 chunks, key 256 alone in the second),
    bit_rows_kernel<CmacRows> over 65,792 workgroups and the identity WoPBS over 8,224 bytes of K1 | K2 (3 chunks), on workspace pointers taken
    before the calls that may grow workspaces.  Keys 0, 127, 128, 255 and 256 alone on a one-key slice give the same words; all 514
    subkeys decrypt to aes_clear's, index 256 to the K1 and K2 of SP 800-38B D.1"""
    p, m = toy.params, cs.CMAC_KEYS
    clear, d_rk, subkeys = store259
    d_rk = d_rk[:m]
    plan = _subkey_plan(m)
    assert plan == [16 * m] * 10
    parts = cs.cmac_keyswitch(plan, m, [])
    launches, units = cs.total(parts)
    assert launches == 20 + 2 + 3, parts
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(OFF)
        buf, rows = guarded(m * 256, p.big1)
        eng.profile_reset()
        srv.aes_cmac_subkeys(d_rk, out=rows.view(m, 2, 16, 8, p.big1))
        srv.synchronize()
        prof = eng.profile_read()
        print("cmac subkeys keyswitch: %r, derived %r" % (prof["keyswitch"], parts))
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert prof["vertical_packing"]["launches"] == launches
        assert guards_intact(buf)
        got = host(rows).reshape(m, 2, 16, 8, p.big1)
        for j in cs.CMAC_KEYS_ALONE:                                          # sharing is invisible: the key alone gives the same words
            alone = srv.aes_cmac_subkeys(d_rk[j:j + 1])
            srv.synchronize()
            assert np.array_equal(host(alone)[0], got[j]), "key %d: %s" % (j, _differ(host(alone)[0], got[j]))
        dec = _blocks(tc, got)
        assert [_u128(b) for b in dec] == subkeys[:2 * m]
        assert dec[2 * cs.CMAC_VECTOR_KEY:] == [cmac.VECTORS[128][1], cmac.VECTORS[128][2]]
    finally:
        eng.close()


def test_cmac_subkeys_of_257_keys_from_a_packed_store(toy, tc, store259):
    """the same call with the 257 keys in a packed store: the words of the call on the unpacked store, and the subkeys"""
    import torch

    p, m = toy.params, cs.CMAC_KEYS
    _, d_rk, subkeys = store259
    srv = Server(toy.keys, device=0)
    try:
        packed = srv.pack_round_keys(d_rk[:m])
        srv.synchronize()
        got = srv.aes_cmac_subkeys(packed)
        unpacked = srv.aes_cmac_subkeys(srv.unpack_round_keys(packed))
        srv.synchronize()
        assert tuple(got.shape) == (m, 2, 16, 8, p.big1) and torch.equal(got, unpacked), "%d words differ" % int((got != unpacked).sum().item())
        assert [_u128(b) for b in _blocks(tc, host(got))] == subkeys[:2 * m]
    finally:
        srv.engine.close()


# ---- B. CMAC tags and verification over 257 streams ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cmac_case(store259):
    """the 257 messages (key, message, tag) of chunk_seams: stream s under key cmac_key_of_stream(s), cmac_message_bytes(s) random bytes, a
    tag of cmac_tag_bytes(s) bytes; the rejected ones corrupted after the tag was made -- one bit of the last compared tag byte, at stream
    256 one message bit.  (messages, the verdict of every message, the full CMAC of every message as it is sent); one aes_clear.cmac a
    stream, and aes_clear.cmac_verify on the rejected ones and on streams 0 and 2"""
    clear = store259[0]
    rng = np.random.default_rng(0x6B0)
    messages, full = [], []
    for s in range(cs.CMAC_STREAMS):
        k, msg = cs.cmac_key_of_stream(s), rng.bytes(cs.cmac_message_bytes(s))
        t = aes_clear.cmac(clear[k], msg)
        tag = t[:cs.cmac_tag_bytes(s)]
        if s == cs.CMAC_BAD_MESSAGE:
            msg = _flip(msg, 20, 0x20)
            t = aes_clear.cmac(clear[k], msg)
        elif s in cs.CMAC_BAD:
            tag = _flip(tag, len(tag) - 1, 1 << (s % 8))
        messages.append((k, msg, tag))
        full.append(t)
    valid = [0 if s in cs.CMAC_BAD else 1 for s in range(cs.CMAC_STREAMS)]
    for s in cs.CMAC_BAD + [0, 2]:
        k, msg, tag = messages[s]
        assert int(aes_clear.cmac_verify(clear[k], msg, tag)) == valid[s], s
    return messages, valid, full


def _cmac_calls(srv, p, d_rk, messages, d_sub, counts):
    """the call that returns the tags and the call that checks them, both inside guard rows, with the key switch and the blind rotation
    held to `counts` = (the parts of the first call, those of the second): (mac buffer, its rows, valid buffer, its rows)"""
    n, eng = len(messages), srv.engine
    buf, rows = guarded(n * 128, p.big1)
    vbuf, vrows = guarded(n, p.big1)
    for parts, run in zip(counts, (lambda: srv.aes_cmac_streams(d_rk, [m[:2] for m in messages], subkeys=d_sub, out=rows.view(n, 16, 8, p.big1)),
                                   lambda: srv.aes_cmac_verify(d_rk, messages, subkeys=d_sub, valid_out=vrows))):
        launches, units = cs.total(parts)
        eng.profile_reset()
        run()
        srv.synchronize()
        prof = eng.profile_read()
        print("cmac keyswitch: %r, derived %r" % (prof["keyswitch"], parts))
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", launches, units)
        assert prof["vertical_packing"]["launches"] == launches
    assert guards_intact(buf) and guards_intact(vbuf)
    return buf, rows, vbuf, vrows


def test_cmac_of_257_streams_under_257_of_259_keys(toy, tc, store259, cmac_case):
    """cmac_dev with the subkeys derived in the call: keys 5 and 130 of the 259 are never named, so at[] is not the identity, the
    compacted list has 257 keys (both subkey WoPBS above one chunk) and the stream under key 258 reads subkey row 2 x 256 + 1 = 513.
    257 streams of one block -- 16 bytes (K1) and fewer (K2) in turn --, 48 bytes at 0 and 256, 17 at 100, none at 255: the first link
    over 257 slots, a cipher pass over 257 live slots under key_of_slot, then prefixes of 3 and 2, the last link with an encrypted addend
    index above 255, and the mac0 and tag0 record groups over 257 slots behind the chain's records.  Tag WoPBS 1 takes 2 chunks and tag
    WoPBS 2 three.  Every tag and verdict against aes_clear; streams 0, 1, 255 and 256 each alone under their own key give the same words"""
    p, n = toy.params, cs.CMAC_STREAMS
    d_rk = store259[1]
    messages, valid, full = cmac_case
    n_active = cs.live_prefixes(cs.cmac_chain_blocks())
    assert n_active == [257, 3, 2] and len({m[0] for m in messages}) == n
    plan = _subkey_plan(n)                                                    # the compacted list: one zero block under each named key
    counts = (cs.cmac_keyswitch(plan, n, n_active), cs.cmac_keyswitch(plan, n, n_active, n))
    assert [cs.total(c)[0] for c in counts] == [65, 70], counts
    srv = Server(toy.keys, device=0)
    try:
        srv.engine.aes_set_window(OFF)
        buf, rows, vbuf, vrows = _cmac_calls(srv, p, d_rk, messages, None, counts)
        mac, ok = host(rows).reshape(n, 16, 8, p.big1), host(vrows)
        assert _blocks(tc, mac) == full
        assert tc.decrypt_bits(ok).tolist() == valid
        for s in cs.CALL_ALONE:                                               # `used` has one entry: the same words
            a_mac = srv.aes_cmac_streams(d_rk, [messages[s][:2]])
            a_ok = srv.aes_cmac_verify(d_rk, [messages[s]])
            srv.synchronize()
            assert np.array_equal(host(a_mac)[0], mac[s]), "tag of stream %d: %s" % (s, _differ(host(a_mac)[0], mac[s]))
            assert np.array_equal(host(a_ok)[0], ok[s]), "valid bit of stream %d: %s" % (s, _differ(host(a_ok)[0], ok[s]))
    finally:
        srv.engine.close()


def test_cmac_of_257_streams_with_the_callers_subkeys(toy, tc, store259, cmac_case):
    """the same two calls with the subkeys of all 259 keys from fheaes_aes_cmac_subkeys_keyed (at[] the identity, the subkey rows of the
    named keys at 2 x key + which): the words of the calls that derive them, with the chain's and the tag check's launches alone; and
    streams 0, 1, 255 and 256 against cmac.compose_verify and ccm.compose_mac, the compositions of older entry points"""
    import torch

    p, n = toy.params, cs.CMAC_STREAMS
    d_rk = store259[1]
    messages, valid, _ = cmac_case
    n_active = cs.live_prefixes(cs.cmac_chain_blocks())
    plan = _subkey_plan(n)
    srv = Server(toy.keys, device=0)
    try:
        srv.engine.aes_set_window(OFF)
        buf, rows, vbuf, vrows = _cmac_calls(srv, p, d_rk, messages, None, (cs.cmac_keyswitch(plan, n, n_active), cs.cmac_keyswitch(plan, n, n_active, n)))
        d_sub = srv.aes_cmac_subkeys(d_rk)
        srv.synchronize()
        own = (cs.cmac_keyswitch(None, 0, n_active), cs.cmac_keyswitch(None, 0, n_active, n))
        assert [cs.total(c)[0] for c in own] == [40, 45]
        sbuf, srows, svbuf, svrows = _cmac_calls(srv, p, d_rk, messages, d_sub, own)
        assert torch.equal(srows, rows), "%d tag words differ" % int((srows != rows).sum().item())
        assert torch.equal(svrows, vrows), "%d valid words differ" % int((svrows != vrows).sum().item())
        four = list(cs.CALL_ALONE)
        at = settled(torch.tensor([messages[s][0] for s in four], device="cuda"))
        rk4, sub4 = host(settled(d_rk.index_select(0, at))), host(settled(d_sub.index_select(0, at)))
        some = [(j,) + messages[s][1:] for j, s in enumerate(four)]
        want_ok = cmac.compose_verify(srv, tc, rk4, some, sub4)
        want_mac = ccm.compose_mac(srv, tc, rk4, cmac.mac_streams([m[:2] for m in some], sub4))
        mac, ok = host(settled(rows.view(n, 128 * p.big1)[four])).reshape(4, 16, 8, p.big1), host(settled(vrows[four]))
        for j, s in enumerate(four):
            assert np.array_equal(ok[j], want_ok[j]), "valid bit of stream %d against the composition: %s" % (s, _differ(ok[j], want_ok[j]))
            assert np.array_equal(mac[j], want_mac[j]), "tag of stream %d against the composition: %s" % (s, _differ(mac[j], want_mac[j]))
        assert tc.decrypt_bits(ok).tolist() == [valid[s] for s in four]
    finally:
        srv.engine.close()


# ---- C. key unwrap of 257 keys under 3 KEKs --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kw_case(toy, tc):
    """3 AES-128 KEKs, the RFC 3394 one first, and their decryption round keys made on the GPU; 257 payloads of 16 bytes wrapped under KEK
    kw_kek_of_key()[j], the payload of vector 4.1 at key 256; the blobs of KW_BAD with one flipped bit, and key KW_WRONG_KEK named under
    another KEK than its own.  (dec round keys on the host, the KEK named for every key, the blobs, (ok, payload) of every key by
    aes_clear.key_unwrap -- for an untouched blob under its own KEK that is (True, what was wrapped), checked on keys 0 and 256)"""
    kek_v, payload_v, wrapped_v = keywrap.vector("4.1")
    keks = (kek_v, bytes(range(0x40, 0x50)), bytes(range(0xC0, 0xD0)))
    rng = np.random.default_rng(0x6C0)
    payloads = [rng.bytes(16) for _ in range(cs.KW_KEYS)]
    payloads[cs.KW_VECTOR_KEY] = payload_v
    kek_of = cs.kw_kek_of_key()
    blobs = keywrap.wrap_many(keks, kek_of, payloads)                         # 3,084 block encryptions: in numpy
    assert blobs[cs.KW_VECTOR_KEY] == wrapped_v and blobs[0] == aes_clear.key_wrap(keks[kek_of[0]], payloads[0])
    want = [(True, d) for d in payloads]
    for j in cs.KW_BAD:
        blobs[j] = _flip(blobs[j], j % 24, 1 << (j % 8))
    kek_of[cs.KW_WRONG_KEK] = (kek_of[cs.KW_WRONG_KEK] + 1) % cs.KW_KEKS
    for j in cs.KW_BAD + [cs.KW_WRONG_KEK, 0, cs.KW_VECTOR_KEY]:
        ok, data = aes_clear.key_unwrap(keks[kek_of[j]], blobs[j])
        assert ok == (j in (0, cs.KW_VECTOR_KEY)) and (not ok or data == payloads[j]), j
        want[j] = (ok, data)
    srv = Server(toy.keys, device=0)
    try:
        dw = srv.aes_decryption_round_keys_many(srv.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in keks])))
    finally:
        srv.engine.close()
    return dw, kek_of, blobs, want


def _unwrap_and_check(toy, tc, kw_case, window, packed=False, then=None):
    """the call over the 257 blobs under `window` on a context of its own, the launches of the key switch and the blind rotation held to
    chunk_seams, every payload (NOT gated) and verdict against aes_clear, keys 0, 1, 255 and 256 each alone under the same window word for
    word; then(server, keys, valid) on the host arrays, before the context closes"""
    p, n_keys, n = toy.params, cs.KW_KEYS, cs.KW_SEMIBLOCKS
    dw, kek_of, blobs, want = kw_case
    parts = cs.kw_keyswitch(window=0 if window == OFF else window)
    launches, units = cs.total(parts)
    k2 = launches if window == OFF else launches - parts["cipher"][0] + 6 * n * cs.window_launches(n_keys, 10, window)[0]
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(window)
        d_dw = dev(dw)
        if packed:
            d_dw = srv.pack_round_keys(d_dw)
            srv.synchronize()
        kbuf, krows = guarded(n_keys * 64 * n, p.big1)
        vbuf, vrows = guarded(n_keys, p.big1)
        eng.profile_reset()
        srv.aes_key_unwrap(d_dw, blobs, kek_of, out=krows.view(n_keys, 8 * n, 8, p.big1), valid_out=vrows)
        srv.synchronize()
        prof = eng.profile_read()
        print("unwrap keyswitch: %r, blind rotation: %r, derived %r" % (prof["keyswitch"], prof["blind_rotate"], parts))
        _stage(prof, "keyswitch", launches, units)
        _stage(prof, "blind_rotate", k2, units)
        assert guards_intact(kbuf) and guards_intact(vbuf)
        keys, valid = host(krows).reshape(n_keys, 8 * n, 8, p.big1), host(vrows)
        assert _blocks(tc, keys) == [data for _, data in want]
        assert tc.decrypt_bits(valid).tolist() == [int(ok) for ok, _ in want]
        for j in cs.CALL_ALONE:
            a_keys, a_valid = srv.aes_key_unwrap(d_dw, [blobs[j]], [kek_of[j]])
            srv.synchronize()
            assert np.array_equal(host(a_keys)[0], keys[j]), "key %d: %s" % (j, _differ(host(a_keys)[0], keys[j]))
            assert np.array_equal(host(a_valid)[0], valid[j]), "valid bit of key %d: %s" % (j, _differ(host(a_valid)[0], valid[j]))
        if then:
            then(srv, keys, valid)
    finally:
        eng.close()


def test_unwrap_of_257_keys_under_3_keks(toy, tc, kw_case):
    """kw_unwrap_dev: kw_link_kernel inside the real call behind its 256-key grid pass, at the load, every shuffle and the unload; the
    wrapped bytes behind a KEK table of 1,028 bytes padded to 1,056 in the one upload; 12 cipher passes over 257 blocks in 2 chunks, key
    256 behind the seam under a KEK of its own (KeySets.of_block); the identity WoPBS over 4,112 payload bytes with key 256 exactly chunk
    2; the tag check in 2 and 3 chunks.  Round by round the key switch launches 12 x 10 x 2 + 2 + 2 + 3 = 247 times.  Keys 0, 1, 255 and
    256 are also the words of keywrap.compose_unwrap, the composition of np_link and older entry points"""
    dw, kek_of, blobs, _ = kw_case
    assert cs.total(cs.kw_keyswitch())[0] == 247

    def composition(srv, keys, valid):
        four = list(cs.CALL_ALONE)
        c_keys, c_valid = keywrap.compose_unwrap(srv, tc, dw, [kek_of[j] for j in four], [blobs[j] for j in four])
        for i, j in enumerate(four):
            assert np.array_equal(c_keys[i], keys[j]), "key %d against the composition: %s" % (j, _differ(c_keys[i], keys[j]))
            assert np.array_equal(c_valid[i], valid[j]), "valid bit of key %d against the composition: %s" % (j, _differ(c_valid[i], valid[j]))

    _unwrap_and_check(toy, tc, kw_case, OFF, then=composition)


def test_unwrap_of_257_keys_in_windows_of_200(toy, tc, kw_case):
    """the same call in windows of 200 blocks: every pass cuts its 10 x 257 block-rounds into 13 windows, all but the first of a pass from
    a block above 0 or across two steps, so the KEK of a block is read at of_block + first_block with first_block non-zero.  The same
    payloads and verdicts, and the alone calls under the same window word for word"""
    _unwrap_and_check(toy, tc, kw_case, cs.WINDOW)


def test_unwrap_of_257_keys_from_a_packed_kek_store(toy, tc, kw_case):
    """the three KEKs in a packed store: the words of the call on the unpacked store, the payloads and the verdicts"""
    dw, kek_of, blobs, _ = kw_case

    def unpacked(srv, keys, valid):
        u_keys, u_valid = srv.aes_key_unwrap(srv.unpack_round_keys(srv.pack_round_keys(dw)), blobs, kek_of)
        assert np.array_equal(keys, u_keys), _differ(keys, u_keys)
        assert np.array_equal(valid, u_valid), _differ(valid, u_valid)

    _unwrap_and_check(toy, tc, kw_case, OFF, packed=True, then=unpacked)


# ---- D. the gate kernel behind GATE_MAX_GRID -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_case(toy):
    """form -> (GGSWs of random words [4][k+1][k+1][N], the 7 input rows of test_gpu_gate._inputs, the oracle's gate of those rows under
    each of gates 0, 2 and 3: [3][7][words]); computed once"""
    p, k1 = toy.params, toy.params.k + 1
    out = {}
    for form in (LWE, GLWE):
        ggsw_std = np.random.default_rng(0x6D0 + form).integers(0, 1 << 64, (len(cs.GATE_GRID_RUNS), k1, k1, p.N), dtype=np.uint64)
        base = _inputs(p, cs.GATE_ROW_PERIOD, form, 0x6D2 + form)
        out[form] = (ggsw_std, base, np.stack([gm.gate_reference(p, ggsw_std[g], base, form) for g in (0, 2, 3)]))
    return out


@pytest.mark.parametrize("form,in_place", [(LWE, False), (LWE, True), (GLWE, True)], ids=["lwe", "lwe in place", "glwe in place"])
def test_gate_kernel_behind_the_grid_cap(toy, grid_case, form, in_place):
    """launch_gate cuts a table above GATE_MAX_GRID = 65,536 workgroups into several kernel launches, the second from wgs + w0.  Four
    gates with runs 8 x 65,536 + 3, 0, 9 and 1: workgroup 65,536, the first of the second launch, is gate 0's ragged last one with 3
    instances, gate 1 has none, gates 2 and 3 lie wholly in the second launch; 65,540 workgroups.  Row i is row i mod 7 of
    test_gpu_gate._inputs (uniform, the four extremes, the two tie rows; 7 is coprime to 8, so every row meets every slot of a
    workgroup).  All 524,301 rows against the oracle's rows expanded on the device; the rows of workgroups 65,535 to 65,537 and those of
    gates 2 and 3 against the oracle on the host.  vertical_packing counts one launch per launch_gate, so the plan's workgroup count is
    what asserts the crossing"""
    import torch

    p, runs, period = toy.params, cs.GATE_GRID_RUNS, cs.GATE_ROW_PERIOD
    m = sum(runs)
    assert _native.gate_plan(runs, p.k) == {"workgroups": 65540, "instances_per_workgroup": cs.GATE_R} and cs.gate_launches(runs) == [2]
    ggsw_std, base, ref = grid_case[form]
    words = base.shape[1]
    eng = _native.Engine(p, device=0)                                        # no keys: the kernel needs none
    buf = rows = d_in = want = None
    try:
        ggswf = _fourier(eng, p, ggsw_std)
        d_base, d_ref = dev(base), dev(ref.reshape(3 * period, words))
        idx = torch.arange(m, device="cuda")
        slot = torch.zeros(m, dtype=torch.int64, device="cuda")              # which of the three non-empty gates a row is under
        slot[runs[0]:runs[0] + runs[2]] = 1
        slot[runs[0] + runs[2]:] = 2
        buf, rows = guarded(m, words)
        if in_place:
            d_in = rows
            settled(rows.copy_(d_base.index_select(0, idx % period)))
        else:
            d_in = settled(d_base.index_select(0, idx % period))
        eng.profile_reset()
        eng.gate_ggsw(ggswf, runs, d_in, m, form, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "vertical_packing", 1, m * (p.N if form == GLWE else 1))
        assert guards_intact(buf)
        want = settled(d_ref.index_select(0, slot * period + idx % period))
        same = torch.equal(rows, want)
        assert same, "%d rows differ, the first at %d" % (int((rows != want).any(dim=1).sum().item()), int((rows != want).any(dim=1).int().argmax().item()))
        lo = cs.gate_table(runs)[cs.GATE_MAX_GRID - 1][0]                     # from workgroup 65,535 on: 8 + 3 rows of gate 0, gates 2 and 3
        assert (lo, m - lo) == (8 * 65535, 8 + 3 + 9 + 1)
        of_row = [0] * (runs[0] - lo) + [1] * runs[2] + [2] * runs[3]
        oracle = np.stack([ref[g][(lo + i) % period] for i, g in enumerate(of_row)])
        got = host(settled(rows[lo:]))
        assert np.array_equal(got, oracle), "rows %s" % sorted(set((lo + np.nonzero(got != oracle)[0]).tolist()))
    finally:
        eng.close()
        del buf, rows, d_in, want
        torch.cuda.empty_cache()


# ---- E. both gate seams in one bootstrapped call -----------------------------------------------------------------------------------------------
def _boot_counters(prof, p, n, units):
    for stage in ("keyswitch", "blind_rotate", "pfpks"):
        _stage(prof, stage, 2, n)
    _stage(prof, "ggsw_fft", 2, n * (p.k + 1) ** 2)
    _stage(prof, "vertical_packing", 2, units)


def test_gate_bits_across_the_chunk_seam_and_the_grid_cut(toy, tc):
    """gate_call with both offsets non-zero: 32,769 gates, valid of period 7 over bits of period 5.  Gate 0 has a run of 8 x 32,771, gate
    32,767 -- the last of chunk 1 -- a run of 0, gate 32,768 -- alone in chunk 2 -- a run of 9 (two workgroups, both naming gate 0 of
    the workspace), every other gate a run of 1.  Chunk 1 has 32,771 + 32,766 = 65,537 workgroups, so launch_gate cuts it between gates
    32,765 and 32,766 with `tab + wg0 + w0`, and chunk 2 starts at tab + 65,537 with chunk_end[1] - wg0 = 2 workgroups.  The head (the
    first and the last 9 instances of gate 0) and gates 32,765 to 32,768 -- both sides of the grid cut and of the chunk seam -- against
    the same call alone, word for word; the last 600 bits decrypted against valid x bit; every row written"""
    import torch

    p, n, runs = toy.params, cs.GATE_BOOT_GATES, cs.gate_boot_runs()
    m = sum(runs)
    assert cs.gate_launches(runs, chunk=cs.MAX_CHUNK_BITS) == [2, 1] and _native.gate_plan(runs, p.k)["workgroups"] == 65537 + 2
    eng = _native.Engine(p, device=0)
    buf = rows = d_ct = None
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        d_gates = settled(dev(tc.encrypt_bits(VALID7))[torch.arange(n, device="cuda") % 7].contiguous())
        d_ct = settled(dev(tc.encrypt_bits(BITS5))[torch.arange(m, device="cuda") % 5].contiguous())
        buf, rows = guarded(m, p.big1)
        eng.profile_reset()
        eng.gate_bits(d_gates, runs, d_ct, m, rows)
        eng.synchronize()
        _boot_counters(eng.profile_read(), p, n, m)
        assert guards_intact(buf)

        def alone(g_lo, g_hi, sub_runs, r_lo):
            k = sum(sub_runs)
            out = filled((k, p.big1), SENTINEL)
            eng.gate_bits(settled(d_gates[g_lo:g_hi].contiguous()), sub_runs, settled(d_ct[r_lo:r_lo + k].contiguous()), k, out)
            eng.synchronize()
            got = host(settled(rows[r_lo:r_lo + k]))
            assert np.array_equal(got, host(out)), "gates %d..%d, rows from %d: %s" % (g_lo, g_hi, r_lo, _differ(got, host(out)))

        alone(0, 1, [9], 0)                                                   # the head: gate 0's first and last 9 instances
        alone(0, 1, [9], runs[0] - 9)
        tail = list(cs.GATE_BOOT_TAIL)
        alone(n - 4, n, tail, m - sum(tail))                                  # gates 32,765 .. 32,768 with their runs
        of_gate = np.repeat(np.arange(n), runs)
        want = VALID7[of_gate % 7] * BITS5[np.arange(m) % 5]
        assert tc.decrypt_bits(host(settled(rows[m - 600:]))).tolist() == want[m - 600:].tolist()
        assert tc.decrypt_bits(host(settled(rows[:20]))).tolist() == want[:20].tolist()
        assert not bool((rows == SENTINEL).all(dim=1).any().item())           # every row was written
    finally:
        eng.close()
        del buf, rows, d_ct
        torch.cuda.empty_cache()


def test_gate_packed_across_the_chunk_seam(toy, tc):
    """the GLWE form across the chunk seam alone: 32,769 gates over GLWEs from Server.pack of periodic bits, 7 distinct ones indexed on the
    device, one a gate but none under gate 32,767 and two under gate 32,768.  The tail and the head against the call alone, and
    decrypt_packed on the tail"""
    import torch

    p, n, runs = toy.params, cs.GATE_BOOT_GATES, cs.gate_packed_runs()
    g_all, gw = sum(runs), (p.k + 1) * p.N
    bits = np.random.default_rng(0x6E0).integers(0, 2, 7 * p.N).astype(np.uint8)
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    buf = rows = d_glwe = None
    try:
        packed7 = srv.pack(dev(tc.encrypt_bits(bits)))
        srv.synchronize()
        which = np.arange(g_all)
        which = (which + which // 7) % 7                                      # not the gates' period: every GLWE under gates of both values
        d_glwe = settled(packed7.index_select(0, torch.from_numpy(which).cuda()))
        d_gates = settled(dev(tc.encrypt_bits(VALID7))[torch.arange(n, device="cuda") % 7].contiguous())
        buf, rows = guarded(g_all, gw)
        eng.profile_reset()
        srv.gate_packed(d_glwe, d_gates, runs, out=rows)
        srv.synchronize()
        _boot_counters(eng.profile_read(), p, n, g_all * p.N)
        assert guards_intact(buf)

        def alone(g_lo, g_hi, sub_runs, r_lo):
            k = sum(sub_runs)
            out = srv.gate_packed(settled(d_glwe[r_lo:r_lo + k].contiguous()), settled(d_gates[g_lo:g_hi].contiguous()), sub_runs)
            srv.synchronize()
            got = host(settled(rows[r_lo:r_lo + k]))
            assert np.array_equal(got, host(out)), "gates %d..%d: %s" % (g_lo, g_hi, _differ(got, host(out)))
            return got

        alone(0, 2, [1, 1], 0)
        tail = alone(n - 4, n, [1, 1, 0, 2], g_all - 4)
        of_gate = np.repeat(np.arange(n), runs)
        want = np.concatenate([VALID7[of_gate[j] % 7] * bits[which[j] * p.N:(which[j] + 1) * p.N] for j in range(g_all - 4, g_all)])
        assert tc.decrypt_packed(tail, 4 * p.N).tolist() == want.tolist()
        assert not bool((rows == SENTINEL).all(dim=1).any().item())
    finally:
        eng.close()
        del buf, rows, d_glwe
        torch.cuda.empty_cache()
