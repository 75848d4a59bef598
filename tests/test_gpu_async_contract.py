"""The contract of FHEAES_DEVICE calls (include/fheaes.h): enqueued on the context's stream and not synchronised, their host side arrays
borrowed for the duration of the call -- so a call is finished with those arrays when it returns -- and every launch and copy on the
stream the caller set.

Borrowed arrays.  Every entry point that takes a host side array together with resident data runs through the raw binding
(Engine._lib: the Python wrapper's own copies must not hide the library's behaviour) with its side arrays in PINNED host memory, where
a copy the library merely enqueued would read them late; the context runs on a stream that a chain of matmuls keeps busy, so nothing
the call enqueues has run when it returns (the chain's end event is asserted not to have been reached); the moment the call
returns every side array is overwritten with OTHER VALID values -- key indices swapped, other blocks, other message bytes of the same
lengths, other runs of the same total: a library that still read them would give wrong words, not a bad address -- and only then is the
stream synchronised.  The words must be those of the host-memspace call on the original arrays, which differ from those of the
host-memspace call on the overwritten ones.

A caller's stream.  A producer of more than 5 ms, a copy into the state, three engine calls, a clone and a fill of the result, all on
one torch stream and only that stream synchronised: one launch or copy of the engine on its own stream or on the null stream would
overtake the producer and read the state before the copy."""
import ctypes

import numpy as np
import pytest

import ccm
import cmac
import workspace_state as ws
from aes_vectors import BASE, F1_KEY, F1_PT, own_client
from gpu_support import dev, host
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd._native import DEVICE, HOST, u128_pairs
from tfhe_aes_amd.server import ccm_args, cmac_args

pytestmark = pytest.mark.gpu

KOB = ws.KOB
U32, U64, U8 = np.uint32, np.uint64, np.uint8
CTYPE = {np.dtype(U32): ctypes.c_uint32, np.dtype(U64): ctypes.c_uint64, np.dtype(U8): ctypes.c_uint8}


def side_ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(CTYPE[a.dtype]))


def pinned_like(a):
    """a numpy view of pinned host memory with a's shape, type and values (the tensor is returned too: it owns the memory)"""
    import torch

    t = torch.empty(max(a.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    assert t.is_pinned()
    view = t.numpy()[:a.nbytes].view(a.dtype).reshape(a.shape)
    view[...] = a
    return view, t


def words(shape):
    return np.zeros(shape, dtype=U64)


@pytest.fixture(scope="module")
def ctx(toy):
    """one Server for the module, the encrypted keys of workspace_state.KEYS in both forms, and a client of its own"""
    from tfhe_aes_amd.server import Server

    class Ctx:
        pass

    c = Ctx()
    c.client = own_client(toy)
    c.p = toy.params
    c.srv = Server(toy.keys, device=0)
    c.rk = ws.key_sets(c.client, ws.KEYS)
    c.dw = ws.key_sets(c.client, ws.KEYS, inverse=True)
    yield c
    c.srv.synchronize()
    c.srv.engine.close()


# A spec: (data, sides_a, sides_b, outputs, call).  data: {name: host words} that travel with the call's memspace; outputs: the names in
# data the call writes (each run gets copies); sides_a / sides_b: {name: host array}, same shapes and types; call(lib, h, P, S, space) -> rc
# with P[name] the address of a data array and S[name] the typed pointer of a side array.
def spec_keyed(symbol, inverse):
    def make(c):
        data = {"rk": c.dw if inverse else c.rk, "state": ws.enc_blocks(c.client, [BASE, F1_PT[0], F1_PT[1]])}
        a, b = {"kob": np.array(KOB, dtype=U32)}, {"kob": np.array([0, 1, 0], dtype=U32)}
        return data, a, b, ["state"], lambda lib, h, P, S, sp: getattr(lib, symbol)(h, P["rk"], 128, 2, S["kob"], P["state"], 3, sp)
    return make


def blocks_pairs(seed, n):
    return u128_pairs(ws.rand_blocks(seed, n))


def spec_encrypt_public(c):
    data = {"rk": c.rk[0], "out": words((3, 16, 8, c.p.big1))}
    return (data, {"blocks": u128_pairs([BASE, BASE + 1, F1_PT[0]])}, {"blocks": blocks_pairs(0xB1, 3)}, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_encrypt_public_bits(h, P["rk"], 128, S["blocks"], 3, P["out"], sp))


def spec_ctr(symbol):
    def make(c):
        data = {"rk": c.rk[1], "out": words((3, 16, 8, c.p.big1))}
        a = {"iv": u128_pairs([(BASE & ~0xFFFFFFFF) | 0xFFFFFFFE]), "data": u128_pairs(F1_PT[:3])}
        b = {"iv": blocks_pairs(0xC7, 1), "data": blocks_pairs(0xC8, 3)}
        return data, a, b, ["out"], lambda lib, h, P, S, sp: getattr(lib, symbol)(h, P["rk"], 128, S["iv"], 1, S["data"], 3, P["out"], sp)
    return make


def spec_decrypt_public(c):
    data = {"dw": c.dw[0], "out": words((3, 16, 8, c.p.big1))}
    return (data, {"blocks": blocks_pairs(0xD1, 3), "data": blocks_pairs(0xD2, 3)}, {"blocks": blocks_pairs(0xD3, 3), "data": blocks_pairs(0xD4, 3)}, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_decrypt_public_bits(h, P["dw"], 128, S["blocks"], S["data"], 3, P["out"], sp))


def spec_cbc(c):
    data = {"dw": c.dw[1], "out": words((3, 16, 8, c.p.big1))}
    return (data, {"iv": blocks_pairs(0xCB0, 1), "ct": blocks_pairs(0xCB1, 3)}, {"iv": blocks_pairs(0xCB2, 1), "ct": blocks_pairs(0xCB3, 3)}, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_cbc_decrypt_bits(h, P["dw"], 128, S["iv"], S["ct"], 3, P["out"], sp))


def spec_xts(c):
    """2 units of 2 blocks, the call covering blocks 1..3"""
    data = {"dw1": c.dw[0], "rk2": c.rk[1], "out": words((3, 16, 8, c.p.big1))}
    a = {"tweaks": u128_pairs([aes_clear.xts_tweak_block(s) for s in (0x3333333333, 0x3333333334)]), "ct": blocks_pairs(0x715, 3)}
    b = {"tweaks": u128_pairs([aes_clear.xts_tweak_block(s) for s in (7, 0xFE)]), "ct": blocks_pairs(0x716, 3)}
    return (data, a, b, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_xts_decrypt_bits(h, P["dw1"], P["rk2"], 128, S["tweaks"], 2, 2, 1, S["ct"], 3, P["out"], sp))


def spec_public_keyed(symbol, inverse):
    def make(c):
        data = {"rk": c.dw if inverse else c.rk, "out": words((3, 16, 8, c.p.big1))}
        a = {"kob": np.array(KOB, dtype=U32), "blocks": u128_pairs([BASE, BASE, BASE + 1]), "data": u128_pairs(F1_PT[:3])}
        b = {"kob": np.array([0, 1, 0], dtype=U32), "blocks": blocks_pairs(0xE7, 3), "data": blocks_pairs(0xE8, 3)}
        return data, a, b, ["out"], lambda lib, h, P, S, sp: getattr(lib, symbol)(h, P["rk"], 128, 2, S["kob"], S["blocks"], S["data"], 3, P["out"], sp)
    return make


def spec_cbc_mac(c):
    """2 streams of 2 and 1 blocks; the other arrays: the keys swapped, 1 and 2 blocks, other bytes, another count of encrypted bytes"""
    rng = np.random.default_rng(0x3AC)
    data = {"rk": c.rk, "enc": ws.enc_blocks(c.client, ws.rand_blocks(0x3AD, 3)), "out": words((2, 16, 8, c.p.big1))}
    a = {"kos": np.array([1, 0], dtype=U32), "len": np.array([2, 1], dtype=U32), "clear": rng.integers(0, 256, (3, 16)).astype(U8), "eb": np.array([0, 16, 5], dtype=U8)}
    b = {"kos": np.array([0, 1], dtype=U32), "len": np.array([1, 2], dtype=U32), "clear": rng.integers(0, 256, (3, 16)).astype(U8), "eb": np.array([9, 0, 16], dtype=U8)}
    return (data, a, b, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_cbc_mac_keyed(h, P["rk"], 128, 2, 2, S["kos"], S["len"], S["clear"], P["enc"], S["eb"], None, P["out"], sp))


def _ccm_sides(messages):
    a = ccm_args(messages)
    return {"kos": np.array(a["key_of_stream"], dtype=U32), "hb": np.array(a["head_blocks"], dtype=U32), "head": u128_pairs(a["head"]), "ctr0": u128_pairs(a["ctr0"]),
            "pb": np.array(a["payload_bytes"], dtype=U64), "ct": np.frombuffer(a["ciphertext"], dtype=U8).copy(), "tags": np.array(a["tags"], dtype=U8),
            "tb": np.array(a["tag_bytes"], dtype=U32)}


def spec_ccm(c):
    """2 messages of 5 and 16 payload bytes with 3 and 0 bytes of AAD; the other arrays: the same lengths, other keys, nonces and bytes"""
    def messages(keys, seed):
        rng = np.random.default_rng(seed)
        return [ccm.own_message(keys[0], ws.KEYS[keys[0]], rng.bytes(13), rng.bytes(3), rng.bytes(5), 6),
                ccm.own_message(keys[1], ws.KEYS[keys[1]], rng.bytes(13), b"", rng.bytes(16), 6)]

    data = {"rk": c.rk, "pt": words((2, 16, 8, c.p.big1)), "valid": words((2, c.p.big1))}
    return (data, _ccm_sides(messages((0, 1), 0xCC1)), _ccm_sides(messages((1, 0), 0xCC2)), ["pt", "valid"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_ccm_open_keyed(h, P["rk"], 128, 2, 2, S["kos"], S["hb"], S["head"], S["ctr0"], S["pb"], S["ct"], S["tags"], S["tb"],
                                                                   P["pt"], P["valid"], sp))


def _cmac_sides(messages):
    a = cmac_args(messages)
    return {"kos": np.array(a["key_of_stream"], dtype=U32), "mb": np.array(a["message_bytes"], dtype=U64), "data": np.frombuffer(a["data"], dtype=U8).copy(),
            "tags": np.array(a["tags"], dtype=U8), "tb": np.array(a["tag_bytes"], dtype=U32)}


def spec_cmac(c):
    """2 messages of 16 and 40 bytes with tags of 16 and 8 bytes; the other arrays: the same lengths, the keys swapped, other bytes"""
    def messages(keys, seed):
        rng = np.random.default_rng(seed)
        m = [rng.bytes(16), rng.bytes(40)]
        return [(keys[0], m[0], aes_clear.cmac(ws.KEYS[keys[0]], m[0])), (keys[1], m[1], aes_clear.cmac(ws.KEYS[keys[1]], m[1], 8))]

    data = {"rk": c.rk, "mac": words((2, 16, 8, c.p.big1)), "valid": words((2, c.p.big1))}
    return (data, _cmac_sides(messages((0, 1), 0xC3A)), _cmac_sides(messages((1, 0), 0xC3B)), ["mac", "valid"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_cmac_keyed(h, P["rk"], 128, 2, None, 2, S["kos"], S["mb"], S["data"], S["tags"], S["tb"], P["mac"], P["valid"], sp))


def spec_unwrap(c):
    def blobs(keks, seed):
        rng = np.random.default_rng(seed)
        return np.frombuffer(b"".join(aes_clear.key_wrap(ws.KEYS[k], rng.bytes(16)) for k in keks), dtype=U8).reshape(2, 24).copy()

    data = {"dw": c.dw, "keys": words((2, 16, 8, c.p.big1)), "valid": words((2, c.p.big1))}
    a, b = {"kok": np.array([0, 1], dtype=U32), "wrapped": blobs((0, 1), 0x3394)}, {"kok": np.array([1, 0], dtype=U32), "wrapped": blobs((1, 0), 0x3395)}
    return (data, a, b, ["keys", "valid"],
            lambda lib, h, P, S, sp: lib.fheaes_aes_kw_unwrap_keyed(h, P["dw"], 128, 2, 2, S["kok"], 2, S["wrapped"], P["keys"], P["valid"], sp))


def spec_gate_bits(c):
    data = {"gates": c.client.encrypt_bits(np.array([1, 0], dtype=U8)), "ct": c.client.encrypt_bits(np.array([1, 1, 1], dtype=U8)), "out": words((3, c.p.big1))}
    return (data, {"runs": np.array([2, 1], dtype=U64)}, {"runs": np.array([1, 2], dtype=U64)}, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_gate_bits(h, P["gates"], 2, S["runs"], P["ct"], 3, P["out"], sp))


def spec_gate_packed(c):
    k1n = (c.p.k + 1) * 512
    glwes = c.srv.pack(c.client.encrypt_bits(np.ones(513, dtype=U8)))
    data = {"gates": c.client.encrypt_bits(np.array([1, 0], dtype=U8)), "glwe": np.ascontiguousarray(glwes), "out": words((2, k1n))}
    return (data, {"runs": np.array([1, 1], dtype=U64)}, {"runs": np.array([2, 0], dtype=U64)}, ["out"],
            lambda lib, h, P, S, sp: lib.fheaes_gate_packed(h, P["gates"], 2, S["runs"], P["glwe"], 2, P["out"], sp))


def spec_add_scalar(c):
    data = {"state": ws.enc_blocks(c.client, [BASE, (1 << 64) - 0x10])}
    return (data, {"cnt": u128_pairs([0x1234, (1 << 64) + 0x25])}, {"cnt": u128_pairs([(3 << 64) + 0x1FF, 7])}, ["state"],
            lambda lib, h, P, S, sp: lib.fheaes_add_scalar(h, P["state"], 2, S["cnt"], sp))


def spec_expand(c):
    rng = np.random.default_rng(0x5EED)
    data = {"bodies": rng.integers(0, 1 << 64, 3, dtype=U64), "out": words((3, c.p.big1))}
    a, b = {"mk": rng.integers(0, 1 << 32, 8, dtype=U64).astype(U32)}, {"mk": rng.integers(0, 1 << 32, 8, dtype=U64).astype(U32)}
    return (data, a, b, ["out"], lambda lib, h, P, S, sp: lib.fheaes_expand_lwe_seeded(h, S["mk"], (1 << 32) - 2, P["bodies"], 3, P["out"], sp))


BUSY_STEPS = 96          # about 100 ms of matmuls in front of every call (1.0 ms each, measured); the longest enqueue, the key unwrap's, stays below 31 ms
# the calls that upload more than one table wait on the host for their own first upload, so for the stream (workspace_state.WAITS_INSIDE)
WAITS_INSIDE = {"aes_xts_decrypt", "aes_ccm_open_keyed", "aes_cmac_keyed", "aes_kw_unwrap_keyed", "aes_cbc_mac_keyed"}

SPECS = {
    "aes_encrypt_keyed": spec_keyed("fheaes_aes_encrypt_keyed", False), "aes_decrypt_keyed": spec_keyed("fheaes_aes_decrypt_keyed", False),
    "aes_decrypt_equivalent_keyed": spec_keyed("fheaes_aes_decrypt_equivalent_keyed", True),
    "aes_encrypt_public": spec_encrypt_public, "aes_decrypt_public": spec_decrypt_public,
    "aes_public_keyed": spec_public_keyed("fheaes_aes_public_keyed", False), "aes_decrypt_public_keyed": spec_public_keyed("fheaes_aes_decrypt_public_keyed", True),
    "aes_ctr": spec_ctr("fheaes_aes_ctr_bits"), "aes_ctr32": spec_ctr("fheaes_aes_ctr32_bits"), "aes_cbc_decrypt": spec_cbc, "aes_xts_decrypt": spec_xts,
    "aes_cbc_mac_keyed": spec_cbc_mac, "aes_ccm_open_keyed": spec_ccm, "aes_cmac_keyed": spec_cmac, "aes_kw_unwrap_keyed": spec_unwrap,
    "gate_bits": spec_gate_bits, "gate_packed": spec_gate_packed, "add_scalar": spec_add_scalar, "expand_lwe_seeded": spec_expand,
}


def host_run(c, spec, sides):
    data, _, _, outputs, call = spec
    arrays = {name: (a.copy() if name in outputs else np.ascontiguousarray(a)) for name, a in data.items()}
    E = c.srv.engine
    E._check(call(E._lib, E._h, {n: a.ctypes.data for n, a in arrays.items()}, {n: side_ptr(a) for n, a in sides.items()}, HOST))
    return [arrays[name] for name in outputs]


@pytest.mark.parametrize("name", list(SPECS))
def test_a_device_call_is_done_with_its_host_arrays_when_it_returns(name, ctx):
    import torch

    c, E = ctx, ctx.srv.engine
    spec = SPECS[name](c)
    data, sides_a, sides_b, outputs, call = spec
    assert sorted(sides_a) == sorted(sides_b) and all(sides_a[n].shape == sides_b[n].shape and sides_a[n].dtype == sides_b[n].dtype for n in sides_a)
    assert any(not np.array_equal(sides_a[n], sides_b[n]) for n in sides_a)
    want_a, want_b = host_run(c, spec, sides_a), host_run(c, spec, sides_b)
    assert not all(np.array_equal(x, y) for x, y in zip(want_a, want_b)), "the overwritten arrays describe the same call"
    # resident data, pinned side arrays holding the original values
    resident = {n: dev(a) for n, a in data.items()}
    pinned = {n: pinned_like(a) for n, a in sides_a.items()}
    s, a = torch.cuda.Stream(), ws.producer_matrix()
    E.set_stream(s.cuda_stream)
    try:
        t0, t1, keep = ws.producer(s, a, BUSY_STEPS)          # the stream is busy: what the call enqueues runs long after its return
        rc = call(E._lib, E._h, {n: t.data_ptr() for n, t in resident.items()}, {n: side_ptr(v) for n, (v, _) in pinned.items()}, DEVICE)
        for n, (view, _) in pinned.items():                   # the call has returned: its borrowed arrays are the caller's again
            view[...] = sides_b[n]
        still_busy = not t1.query()
        E._check(rc)
        E.synchronize()
    finally:
        E.set_stream(None)
    assert still_busy or name in WAITS_INSIDE, "the call returned after the %d matmuls in front of it (%.1f ms) were done: nothing was in flight" % (BUSY_STEPS, t0.elapsed_time(t1))
    got = [host(resident[n]) for n in outputs]
    for g, a in zip(got, want_a):
        assert np.array_equal(g.reshape(-1), a.reshape(-1)), "%s read a host side array after it returned" % name


# ---- a caller's stream ---------------------------------------------------------------------------------------------------------------------
PRODUCER_STEPS = 16                                # a chain of 4,096^3 fp32 matmuls, each the input of the next: 17.0 ms measured (48 took 189.1 ms in a fresh process)
PRODUCER_MIN_MS = 5.0


def test_every_launch_and_copy_is_on_the_caller_s_stream(toy):
    import torch

    from tfhe_aes_amd.server import Server

    client = own_client(toy)
    p = toy.params
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        rk = ws.key_sets(client, ws.KEYS)
        src = ws.enc_blocks(client, [BASE, F1_PT[0], F1_PT[1]])
        valid = client.encrypt_bits(np.array([1, 0], dtype=U8))
        iv, data, runs = (BASE & ~0xFFFFFFFF) | 0xFFFFFFFE, F1_PT[:3], [128, 256]

        def calls(rk_, state, valid_):
            """the three engine calls, in the memory space of their arguments: (the state, in place; the gated CTR blocks)"""
            srv.aes_encrypt_keyed(rk_, KOB, state)                                   # uploads its key table through the pinned buffer
            ctr = srv.aes_ctr(rk_[1], iv, 0, 3, data=data)                           # a new output
            return state, srv.gate(ctr, valid_, runs)

        # host memspace, while nothing else is set: the reference
        want_state, want_gated = calls(rk, src.copy(), valid)
        assert ws.dec_blocks(client, want_state) == [aes_clear.aes_encrypt_block(ws.KEYS[k], b) for k, b in zip(KOB, [BASE, F1_PT[0], F1_PT[1]])]
        ks = aes_clear.ctr_keystream(F1_KEY, iv, 0, 3)
        assert ws.dec_blocks(client, want_gated) == [ks[0] ^ data[0], 0, 0]

        d_rk, d_src, d_valid = dev(rk), dev(src), dev(valid)
        d_state = dev(np.zeros_like(src))                                            # what a call that overtook the copy would encrypt
        a = ws.producer_matrix()
        s = torch.cuda.Stream()
        eng.set_stream(s.cuda_stream)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            t0.record(s)
            x = a
            for _ in range(PRODUCER_STEPS):
                x = x @ a
            t1.record(s)
            d_state.copy_(d_src)
            state, result = calls(d_rk, d_state, d_valid)
            out, out_state = result.clone(), state.clone()
            result.fill_(-1)
        s.synchronize()                                                              # s only: not the device, not the context
        ms = t0.elapsed_time(t1)
        print("producer: %d matmuls of %d x %d took %.1f ms" % (PRODUCER_STEPS, ws.PRODUCER_SIZE, ws.PRODUCER_SIZE, ms))
        assert ms >= PRODUCER_MIN_MS, "the producer took %.2f ms: too short to hide a launch on another stream; enlarge PRODUCER_STEPS" % ms
        assert np.array_equal(host(out_state), want_state), "aes_encrypt_keyed on a caller's stream"
        assert np.array_equal(host(out), want_gated), "aes_ctr + gate on a caller's stream"
        assert bool((result == -1).all().item())                                     # nothing of the engine's landed after the fill
        # a host-memspace call while s is set returns complete results
        again_state, again_gated = calls(rk, src.copy(), valid)
        assert np.array_equal(again_state, want_state) and np.array_equal(again_gated, want_gated)
        # back on the context's own stream
        eng.set_stream(None)
        d_state2 = dev(src)
        state2, result2 = calls(d_rk, d_state2, d_valid)
        srv.synchronize()
        assert np.array_equal(host(state2), want_state) and np.array_equal(host(result2), want_gated)
        del x
    finally:
        eng.set_stream(None)
        srv.synchronize()
        eng.close()
