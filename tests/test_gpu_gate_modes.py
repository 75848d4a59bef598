"""gate=True on the MI355X at PARAM_TOY: aes_ccm_decrypt, aes_key_unwrap and aes_key_unwrap_packed release a plaintext or a key only
under its own `valid` bit.  The words are Server.gate applied to the gate=False result, a forged message's plaintext and a tampered
blob's key decrypt to zeros, `valid` is what it was, and a ServerGroup of two contexts gives the same words.  That gate=False writes
what it always wrote is the older tests' business (test_gpu_ccm.py, test_gpu_keywrap.py).  The last test runs the gated key unwrap
once at PARAM_OPT."""
import numpy as np
import pytest

import ccm
import keywrap
from gpu_support import dev, guarded, guards_intact, host, oc, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.server import ServerGroup

pytestmark = pytest.mark.gpu

KEY_A, KEY_B = ccm.VECTORS["ex1"][0], ccm.VECTORS["rfc1"][0]
V41 = keywrap.vector("4.1")


def _flip(data, i, bit=0x01):
    return data[:i] + bytes([data[i] ^ bit]) + data[i + 1:]


# ---- CCM ------------------------------------------------------------------------------------------------------------------------------------
def test_ccm_plaintext_is_gated_on_valid(toy, toy_server, tc):
    """example 1 (4 bytes), example 2 with one tag bit flipped (16 bytes), the RFC vector (23 bytes, two blocks) under two keys"""
    p = toy.params
    rk = toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in (KEY_A, KEY_B)]))
    k, nonce, aad, ct, tag = ccm.message(0, "ex2")
    messages = [ccm.message(0, "ex1"), (k, nonce, aad, ct, _flip(tag, len(tag) - 1, 0x10)), ccm.message(1, "rfc1")]
    pt, ok, at = toy_server.aes_ccm_decrypt(rk, messages)
    g_pt, g_ok, g_at = toy_server.aes_ccm_decrypt(rk, messages, gate=True)
    assert at == g_at == [0, 1, 2, 4] and g_pt.shape == pt.shape == (4, 16, 8, p.big1)
    assert np.array_equal(g_ok, ok) and tc.decrypt_bits(ok).tolist() == [1, 0, 1]
    runs = [128 * (at[i + 1] - at[i]) for i in range(3)]
    want = toy_server.gate(pt, ok, runs)
    assert np.array_equal(g_pt, want), "%d words differ" % int((g_pt != want).sum())
    assert not np.array_equal(g_pt, pt)
    payloads = [ccm.VECTORS[v][3] for v in ("ex1", "ex2", "rfc1")]
    assert ccm.plaintext_of(tc, pt, at, messages) == payloads                                     # ungated: the forged message's plaintext is there
    assert ccm.plaintext_of(tc, g_pt, at, messages) == [payloads[0], bytes(16), payloads[2]]      # gated: zeros
    assert not tc.decrypt_bytes(g_pt[1]).any()
    # rows beyond a payload's length are zero words before the gate and after it
    assert not pt[0].reshape(128, p.big1)[32:].any() and not g_pt[0].reshape(128, p.big1)[32:].any()
    # resident tensors inside guard rows, and equal runs without naming them
    buf, rows = guarded(4 * 128, p.big1)
    vbuf, vrows = guarded(3, p.big1)
    d_pt, d_ok, _ = toy_server.aes_ccm_decrypt(dev(rk), messages, out=rows.view(4, 16, 8, p.big1), valid_out=vrows, gate=True)
    toy_server.synchronize()
    assert guards_intact(buf) and guards_intact(vbuf) and np.array_equal(host(d_pt), g_pt) and np.array_equal(host(d_ok), ok)
    assert np.array_equal(toy_server.gate(pt[:2], ok[:2]), want[:2])
    with pytest.raises(ValueError):
        toy_server.gate(pt, ok)                                                                    # 512 ciphertexts under 3 gates
    with pytest.raises(ValueError):
        toy_server.gate(pt, ok, [128, 128, 128])


# ---- key unwrap -----------------------------------------------------------------------------------------------------------------------------
def test_unwrapped_keys_are_gated_on_valid(toy, toy_server, tc):
    """the RFC 3394 section 4.1 vector and a copy with one bit of C[1] flipped"""
    p = toy.params
    kek, payload, right = V41
    wrapped = [right, _flip(right, 8 + 2, 0x40)]
    assert [int(aes_clear.key_unwrap(kek, w)[0]) for w in wrapped] == [1, 0]
    kek_rk = toy_server.aes_decryption_round_keys_many(toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(kek)])))
    keys, ok = toy_server.aes_key_unwrap(kek_rk, wrapped)
    g_keys, g_ok = toy_server.aes_key_unwrap(kek_rk, wrapped, gate=True)
    assert g_keys.shape == keys.shape == (2, 16, 8, p.big1)
    assert np.array_equal(g_ok, ok) and tc.decrypt_bits(ok).tolist() == [1, 0]
    want = toy_server.gate(keys, ok)
    assert np.array_equal(g_keys, want), "%d words differ" % int((g_keys != want).sum())
    dec = lambda a: [bytes(k.tolist()) for k in tc.decrypt_bytes(a)]
    assert dec(keys) == [payload, aes_clear.key_unwrap(kek, wrapped[1])[1]] and dec(keys)[1] != bytes(16)     # ungated: a key is there
    assert dec(g_keys) == [payload, bytes(16)]
    # straight into a packed store: gated before the expansion, so the tampered blob's entry is the round keys of the all-zero key
    store, s_ok = toy_server.aes_key_unwrap_packed(kek_rk, wrapped, gate=True)
    want_store = toy_server.pack_round_keys(toy_server.aes_key_expansion_many(g_keys))
    assert store.key_bits == 128 and store.n_keys == 2
    assert np.array_equal(store.data, want_store.data) and np.array_equal(s_ok, ok)
    for i, key in enumerate((payload, bytes(16))):
        got = tc.decrypt_packed_bytes(store.data[i], 11 * 16).reshape(11, 16)
        assert np.array_equal(got, np.array(aes_clear.expand_key(key), dtype=np.uint8)), i
    # two contexts on one GPU: whole keys and whole gates per context, the same words
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        q_keys, q_ok = group.aes_key_unwrap(kek_rk, wrapped, gate=True)
        q_gate = group.gate(keys, ok)
        q_store, q_sok = group.aes_key_unwrap_packed(kek_rk, wrapped, gate=True)
        q_packed = group.gate_packed(want_store.data, ok)
    finally:
        for s in group.servers:
            s.engine.close()
    assert np.array_equal(q_keys, g_keys) and np.array_equal(q_ok, ok) and np.array_equal(q_gate, want)
    assert np.array_equal(q_store.data, store.data) and np.array_equal(q_sok, ok)
    assert np.array_equal(q_packed, toy_server.gate_packed(want_store.data, ok))
    assert not tc.decrypt_packed_bytes(q_packed[1], 11 * 16).any()                                # the second store entry, gated away whole


# ---- one call at PARAM_OPT -------------------------------------------------------------------------------------------------------------------
def test_opt_unwrapped_keys_are_gated_on_valid(opt, opt_server, oc):
    """RFC 3394 vector 4.1 and a copy with one bit flipped, gate=True on resident tensors (the ungated call: test_gpu_keywrap.py; CCM's
    gated form at PARAM_OPT: test_gpu_ccm.py).  The gate's circuit bootstrap decides on `valid`, a 16-bit WoPBS output."""
    kek, payload, right = V41
    bad = _flip(right, 23, 0x80)
    assert [int(aes_clear.key_unwrap(kek, w)[0]) for w in (right, bad)] == [1, 0]
    d_rk = opt_server.aes_key_expansion(dev(oc.encrypt_aes_key(kek)))
    d_dw = opt_server.aes_decryption_round_keys(d_rk)
    keys, valid = opt_server.aes_key_unwrap(d_dw, [right, bad], gate=True)
    opt_server.synchronize()
    assert keys.is_cuda and tuple(keys.shape) == (2, 16, 8, opt.params.big1)
    assert oc.decrypt_bits(host(valid)).tolist() == [1, 0]
    assert [bytes(k.tolist()) for k in oc.decrypt_bytes(host(keys))] == [payload, bytes(16)]
    assert aes_clear.key_unwrap(kek, bad)[1] != bytes(16)                                         # ungated, a key would be there
