"""Every device allocation of every call is refused once, and the call is made again (the contract at FHEAES_ERR_NOMEM, include/fheaes.h).

A full device is the design point of the engine: the caller's arrays fill it and the workspace grows at request time, so the hipMalloc
that fails is the engine's, in the middle of a call.  fheaes_alloc_debug makes the runtime itself refuse the n-th allocation of a
context (it is asked for twice the device's memory), so the error state left behind is the real one.  The sweep gives every case of
workspace_state.CASES a Server of its own and runs, on resident inputs,

  1. anchor   W0 on the fresh context, checked as test_gpu_workspace_state.py does
  2. count    release, arm far ahead, run: A allocations, W0 again, the anchor's sizes
  3. fail     for every j in 1..A: release, arm j, run on fresh inputs: -4 with a message that names hipMalloc and a byte count; the
              stream synchronises; the hook is disarmed and has seen exactly j allocations; the workspace is what j - 1 allocations
              leave with the buffer of allocation j empty: all empty at j = 1, every size one that an earlier allocation asked for or 0,
              an empty buffer that holds at least the refused bytes later, and from j to j + 1 at most two buffers change -- the one of
              allocation j from 0 to the bytes refusal j named, the one of allocation j + 1 to 0 where ensure() frees before it grows
              (never a partly grown buffer); read-only inputs are bit-identical to their host
              copies; the probe (keyswitch_batch on one fixed ciphertext, a launcher that ends in hipGetLastError) returns the oracle's row
  4. retry    after j in {1, ceil(A / 2), A}: the call again on fresh inputs without a release is W0 and leaves the anchor's sizes
  5. parking  the k2_park_read counters are unchanged over the whole case

and the calls outside the table each get a test of their own below."""
import threading

import numpy as np
import pytest

import alloc_failures as af
import workspace_state as ws
from edge_words import PARAM_EDGE
from gpu_support import PAIR, dev, filled, host
from test_gpu_workspace_state import as_tuple, once, resident, same, sizes
from tfhe_aes_amd import PARAM_TOY, _native
from tfhe_aes_amd._native import FheAesError

pytestmark = pytest.mark.gpu

RELEASE = _native.WS_POISON_RELEASE


@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


@pytest.fixture(scope="module")
def probe(env):
    return af.probe_inputs(env)


def refused(call, code=af.NOMEM):
    """call() must raise FheAesError `code`; for -4 the message names hipMalloc and a byte count, which is returned"""
    with pytest.raises(FheAesError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if code != af.NOMEM:
        return None
    nbytes = af.refused_bytes(str(e.value))
    assert "hipMalloc" in str(e.value) and nbytes is not None and nbytes > 0, str(e.value)
    return nbytes


def run_probe(E, probe):
    """the probe on context E: rc 0 and the oracle's words"""
    import torch

    x = dev(probe["x"])
    out = torch.zeros((1, E.params.n + 1), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    E.keyswitch_batch(x, out, 1)
    E.synchronize()
    assert np.array_equal(host(out), probe["want"]), "the probe after a refused allocation"


def unchanged(d, inputs, names):
    return all(np.array_equal(host(d[n]).reshape(-1), np.ascontiguousarray(inputs[n]).view(np.uint64).reshape(-1)) for n in names)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.name)
def test_every_allocation_of_the_call_refused_once(case, toy, env, probe):
    from tfhe_aes_amd.server import Server

    h0 = case.build(env, 0)
    read_only = [n for n in h0["dev"] if n not in af.written(case)]
    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        park = E.k2_park_read()
        # 1. anchor
        d = resident(h0)
        w0 = as_tuple(case.run(srv, d))
        srv.synchronize()
        case.check_clear(env, h0, [host(t) for t in w0])
        assert unchanged(d, h0, read_only), "a successful call wrote an input listed as read-only"
        anchor = sizes(srv)
        if case.uses:
            assert all(anchor[name] > 0 for name in case.uses)
        # 2. count
        E.workspace_poison(RELEASE)
        assert E.alloc_debug(af.FAR) >= 0
        assert same(once(srv, case, h0), w0)
        a = E.alloc_debug(0)
        print("allocations %s A=%d" % (case.name, a))
        assert sizes(srv) == anchor
        assert a >= sum(1 for v in anchor.values() if v) and a >= len(case.uses)
        if not case.uses:
            assert a == 0 and sum(anchor.values()) == 0
        assert a == af.ALLOCATIONS[case.name]
        # 3. fail each allocation, 4. retry
        positions = af.fail_positions(a, case.name in af.THINNED)
        retries = af.retry_positions(a)
        snap, named = {}, {}
        for j in positions:
            E.workspace_poison(RELEASE)
            assert all(v == 0 for v in sizes(srv).values())
            E.alloc_debug(j)
            d = resident(h0)
            named[j] = refused(lambda: case.run(srv, d))
            srv.synchronize()                                     # rc 0: nothing that was enqueued before the refusal is in error
            snap[j] = sizes(srv)
            if j == 1:
                assert all(v == 0 for v in snap[1].values()), "allocation 1 was refused and a buffer is not empty: %s" % snap[1]
            assert E.alloc_debug(0) == j and E.alloc_debug(0) == 0, "the hook fires once, at allocation %d" % j
            assert unchanged(d, h0, read_only), "a read-only input changed in the call refused at allocation %d" % j
            run_probe(E, probe)
            if j in retries:
                assert same(once(srv, case, h0), w0), "the call again after the refusal of allocation %d of %d" % (j, a)
                assert sizes(srv) == anchor
        # what the refusals left: snap[j] is the workspace after allocations 1 .. j - 1 with the buffer of allocation j empty -- never
        # grown, or freed by ensure() before the larger request that was refused
        snap[a + 1] = anchor
        for j in positions:
            earlier = {0} | {named[i] for i in positions if i < j}
            later = [snap[i] for i in sorted(snap) if i > j]
            if case.name not in af.THINNED:
                assert all(v in earlier for v in snap[j].values()), "a size that no earlier allocation asked for: %s" % ((j, snap[j], named),)
                assert sum(1 for v in snap[j].values() if v) <= j - 1
            # the buffer of allocation j: empty now, and holding at least the bytes the refusal named once the allocation has succeeded
            # (exactly those, unless the very next allocation grows the same buffer again: K1's digit planes, then K3's)
            assert any(snap[j][n] == 0 and any(s[n] >= named[j] for s in later) for n in anchor), "no empty buffer takes the %d bytes of allocation %d: %s" % (
                named[j], j, snap[j])
            if j + 1 in snap:
                # from j to j + 1 allocation j succeeds (0 -> its bytes) and the buffer of allocation j + 1 is emptied, if it held anything
                moved = [n for n in anchor if snap[j][n] != snap[j + 1][n]]
                filled_now = [n for n in moved if snap[j][n] == 0 and snap[j + 1][n] == named[j]]
                emptied = [n for n in moved if snap[j + 1][n] == 0 and snap[j][n] in earlier]
                assert len(filled_now) <= 1 and len(emptied) <= 1 and sorted(filled_now + emptied) == sorted(moved), (j, moved, snap[j], snap[j + 1], named[j])
                if j == a:
                    assert len(filled_now) == 1 and not emptied
        # 5. parking counters
        after = E.k2_park_read()
        assert (after["fallbacks"], after["violations"]) == (park["fallbacks"], park["violations"]) and after["violations"] == 0
        assert (after["owner"] == park["owner"]).all()
    finally:
        E.alloc_debug(0)
        srv.synchronize()
        E.close()


# ---- the hook alone ----------------------------------------------------------------------------------------------------------------------
def test_a_hooked_refusal_is_immediate_and_reserves_nothing(toy):
    """the assumption of the hook: the runtime refuses twice the device's memory at once and keeps nothing of it"""
    import torch

    from tfhe_aes_amd.server import Server

    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        torch.cuda.synchronize()
        free0, total = torch.cuda.mem_get_info()
        E.alloc_debug(1)
        refused(lambda: E.reserve(64))
        free1, _ = torch.cuda.mem_get_info()
        assert free1 == free0 and total > 0
        assert all(v == 0 for v in sizes(srv).values())
        assert E.alloc_debug(0) == 1
    finally:
        E.close()


def test_hook_armed_and_disarmed_fails_nothing_and_counts_a_reservation(toy):
    from tfhe_aes_amd.server import Server

    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        E.alloc_debug(0)
        E.alloc_debug(1)
        assert E.alloc_debug(0) == 0
        E.reserve(64)
        grown = sizes(srv)
        assert E.alloc_debug(af.FAR) == 4                       # ws_small, ws_pbs, ws_ggsw, ws_ggswf; 64 bits take the latency form, which parks nothing
        assert sorted(n for n, v in grown.items() if v) == ["ws_ggsw", "ws_ggswf", "ws_pbs", "ws_small"]
        E.reserve(64)
        assert E.alloc_debug(0) == 0                            # nothing to grow: nothing allocated
        E.workspace_poison(RELEASE)
        E.alloc_debug(af.FAR)
        E.reserve(64)
        assert E.alloc_debug(0) == 4 and sizes(srv) == grown
    finally:
        E.close()


# ---- fheaes_reserve ----------------------------------------------------------------------------------------------------------------------
def test_reserve_refused_at_each_allocation(toy, env, probe):
    from tfhe_aes_amd.server import Server

    case = ws.BY_NAME["many_sbox"]
    h0 = case.build(env, 0)
    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        w0 = once(srv, case, h0)
        case.check_clear(env, h0, [host(t) for t in w0])
        E.workspace_poison(RELEASE)
        E.reserve(64)
        full = sizes(srv)
        names = ["ws_small", "ws_pbs", "ws_ggsw", "ws_ggswf"]            # ensure_wopbs_ws' order
        for j in range(1, 5):
            E.workspace_poison(RELEASE)
            E.alloc_debug(j)
            assert refused(lambda: E.reserve(64)) == full[names[j - 1]]
            E.synchronize()
            now = sizes(srv)
            assert [now[n] for n in names] == [full[n] for n in names[:j - 1]] + [0] * (5 - j)
            assert E.alloc_debug(0) == j
            run_probe(E, probe)
            E.reserve(64)
            assert {n: v for n, v in sizes(srv).items() if n != "ws_digits"} == {n: v for n, v in full.items() if n != "ws_digits"}
            assert same(once(srv, case, h0), w0)
    finally:
        E.close()


# ---- the key uploads ---------------------------------------------------------------------------------------------------------------------
def key_arrays(kit, form, space):
    sk = kit.keys.compress()
    arrays = (sk.ksk_body, sk.bsk_body, sk.pfpksk_body) if form == "seeded" else (kit.keys.ksk, kit.keys.bsk, kit.keys.pfpksk)
    arrays = [np.ascontiguousarray(a) for a in arrays]
    if space == "device":
        arrays = [dev(a) for a in arrays]
    return (lambda E: E.upload_keys_seeded(sk.mask_seed, *arrays)) if form == "seeded" else (lambda E: E.upload_keys(*arrays))


def key_images_are(E, kit, first):
    """K1 and K3 on 5 rows of random words against the oracle, three GGSWs of the Fourier BSK against the first context's"""
    p = kit.params
    x = np.random.default_rng(0xA110C).integers(0, 1 << 64, (5, p.big1), dtype=np.uint64)
    a = np.zeros((5, p.n + 1), dtype=np.uint64)
    E.keyswitch_batch(x, a, 5)
    assert np.array_equal(a, kit.oracle.keyswitch(x))
    g = np.zeros((5, p.k + 1, (p.k + 1) * 512), dtype=np.uint64)
    E.pfpks_batch(x, g, 5)
    assert np.array_equal(g.reshape(-1), np.ascontiguousarray(kit.oracle.pfpks(x)).view(np.uint64).reshape(-1))
    for i in (0, p.n // 2, p.n - 1):
        assert np.array_equal(E.read_bsk_fourier(i).view(np.uint64), first.read_bsk_fourier(i).view(np.uint64))


def evaluation_is_refused(E, code):
    p = E.params
    x, a = np.zeros((1, p.big1), dtype=np.uint64), np.zeros((1, p.n + 1), dtype=np.uint64)
    refused(lambda: E.keyswitch_batch(x, a, 1), code)


@pytest.mark.parametrize("form,space", sorted(af.UPLOAD_ALLOCATIONS), ids=lambda v: v)
def test_upload_refused_at_each_allocation(form, space, toy):
    upload = key_arrays(toy, form, space)
    first = toy.engine()
    n_alloc = af.UPLOAD_ALLOCATIONS[(form, space)]
    E = _native.Engine(PARAM_TOY, device=0)
    try:
        E.alloc_debug(af.FAR)
        upload(E)
        assert E.alloc_debug(0) == n_alloc
    finally:
        E.close()
    for j in range(1, n_alloc + 1):
        E = _native.Engine(PARAM_TOY, device=0)
        try:
            E.alloc_debug(j)
            refused(lambda: upload(E))                              # -4, not -3
            assert E.alloc_debug(0) == j
            evaluation_is_refused(E, af.NOKEYS)
            upload(E)
            key_images_are(E, toy, first)
        finally:
            E.close()
    # a context that HAS keys: the images are there, only the staging arrays are allocated; the old images are not evaluated with
    E = _native.Engine(PARAM_TOY, device=0)
    try:
        upload(E)
        E.alloc_debug(af.FAR)
        upload(E)
        assert E.alloc_debug(0) == n_alloc - af.IMAGES
        for j in range(1, n_alloc - af.IMAGES + 1):
            key_images_are(E, toy, first)
            E.alloc_debug(j)
            refused(lambda: upload(E))
            assert E.alloc_debug(0) == j
            evaluation_is_refused(E, af.NOKEYS)
            upload(E)
        key_images_are(E, toy, first)
    finally:
        E.close()


# ---- fheaes_clone_keys -------------------------------------------------------------------------------------------------------------------
def test_clone_refused_at_each_image(toy):
    src = toy.engine()
    p = toy.params
    x = np.random.default_rng(0xC10E).integers(0, 1 << 64, (5, p.big1), dtype=np.uint64)
    k1 = np.zeros((5, p.n + 1), dtype=np.uint64)
    src.keyswitch_batch(x, k1, 5)
    assert np.array_equal(k1, toy.oracle.keyswitch(x))
    for j in range(1, af.IMAGES + 1):
        E = _native.Engine(PARAM_TOY, device=0)
        try:
            E.alloc_debug(j)
            refused(lambda: E.clone_keys_from(src))
            assert E.alloc_debug(0) == j                            # counted on the destination
            evaluation_is_refused(E, af.NOKEYS)
            again = np.zeros_like(k1)
            src.keyswitch_batch(x, again, 5)
            assert np.array_equal(again, k1), "the source of a refused clone"
            E.clone_keys_from(src)
            key_images_are(E, toy, src)
            assert E.clone_info()["path"] == "same_device"
        finally:
            E.close()


# ---- fheaes_audit_set --------------------------------------------------------------------------------------------------------------------
def test_audit_set_refused_at_each_buffer(toy, env, probe):
    """audit_rows stays 0 until all three buffers exist (fheaes_audit_set): a half-set audit never launches on a missing buffer"""
    from tfhe_aes_amd.server import Server

    case = ws.BY_NAME["many_sbox"]                                  # one WoPBS of 24 bits: every row is sampled with 64 audit rows
    h0 = case.build(env, 0)
    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        w0 = once(srv, case, h0)
        case.check_clear(env, h0, [host(t) for t in w0])
        for j in range(1, 4):
            E.audit_set(0)
            E.alloc_debug(j)
            refused(lambda: E.audit_set(64, 0, 7))
            assert E.alloc_debug(0) == j
            run_probe(E, probe)
            assert same(once(srv, case, h0), w0)
            r = E.audit_read()
            assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (0, 0, 0)
            E.audit_set(64, 0, 7)
            assert same(once(srv, case, h0), w0)
            r = E.audit_read()
            assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, 24, 0)
            E.audit_debug(5, 0, 1 << 62)
            assert not same(once(srv, case, h0), w0)
            r = E.audit_read()
            assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (2, 48, 1) and int(r["records"][0][1]) == 5
    finally:
        E.audit_set(0)
        E.close()


# ---- a host-memspace call ----------------------------------------------------------------------------------------------------------------
def test_host_call_refused_at_each_staging_buffer(toy, env, probe):
    from tfhe_aes_amd.server import Server

    p = toy.params
    x = env.client.encrypt_bytes(ws.STAGE_BYTES[0])
    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        w0 = srv.many_sbox(x, False)
        assert [[int(b) for b in row] for row in env.client.decrypt_bytes(w0)] == ws.BY_NAME["many_sbox"].build(env, 0)["expect"]
        full = sizes(srv)
        assert full["stage[0]"] == x.nbytes and full["stage[1]"] == w0.nbytes and full["stage[2]"] == 0
        for j in (1, 2):
            E.workspace_poison(RELEASE)
            E.alloc_debug(j)
            out = np.full(w0.shape, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
            keep = x.copy()
            assert refused(lambda: E.many_sbox(x, 3, False, out)) == (x.nbytes, w0.nbytes)[j - 1]
            assert (out == 0xA5A5A5A5A5A5A5A5).all(), "a refused host-memspace call wrote the caller's output"
            assert np.array_equal(x, keep)
            now = sizes(srv)
            assert now["stage[%d]" % (j - 1)] == 0 and sum(now.values()) == (0, x.nbytes)[j - 1]
            assert E.alloc_debug(0) == j
            run_probe(E, probe)
            assert np.array_equal(srv.many_sbox(x, False), w0)
    finally:
        E.close()


# ---- k = 4: the paired form's parking slab and owner words ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_keys():
    """PARAM_EDGE (the k = 4 kernels on n = 24) under zero KSK / PFPKSK and a BSK of random words, as test_gpu_edge_words.py sets it up;
    769 rows, the smallest paired launch, seven distinct ones, and the oracle's rows"""
    from oracle import oracle as orc

    p = PARAM_EDGE
    rng = np.random.default_rng(0x9A12)
    bsk = rng.integers(0, 1 << 64, p.bsk_words, dtype=np.uint64)
    base = rng.integers(0, 1 << 64, (7, p.n + 1), dtype=np.uint64)
    oracle = orc.Oracle(p, np.zeros(1, dtype=np.uint64), bsk, np.zeros(1, dtype=np.uint64))
    idx = np.arange(769) % 7
    return {"zeros": (filled((p.ksk_words,), 0), filled((p.pfpksk_words,), 0)), "bsk": dev(bsk), "x": dev(base[idx]), "want": dev(oracle.cbs_pbs(base)[idx])}


@pytest.mark.parametrize("j,what", [(1, "ws_park"), (2, "owner words")], ids=["ws_park", "owner_words"])
def test_paired_launch_refused_at_its_parking(j, what, edge_keys):
    import torch

    p, m = PARAM_EDGE, 769
    E = _native.Engine(p, device=0)
    try:
        E.upload_keys(edge_keys["zeros"][0], edge_keys["bsk"], edge_keys["zeros"][1])
        pl = E.k2_plan(m)
        assert pl["form"] == 2 and pl["kernel"].startswith(PAIR) and "claimed" in pl["kernel"], pl
        out = filled((m, p.big1), 0)
        E.alloc_debug(j)
        refused(lambda: E.cbs_pbs_batch(edge_keys["x"], out, m))
        E.synchronize()
        assert E.alloc_debug(0) == j
        info = {b["name"]: b["bytes"] for b in E.workspace_info()}
        assert (info["ws_park"] == 0) == (j == 1) and sum(v for n, v in info.items() if n != "ws_park") == 0
        r = E.k2_park_read()
        assert (r["fallbacks"], r["violations"]) == (0, 0) and not r["owner"].any()
        E.alloc_debug(af.FAR)
        E.cbs_pbs_batch(edge_keys["x"], out, m)
        E.synchronize()
        assert E.alloc_debug(0) == 3 - j                           # what the refused call had not allocated: the slab (j = 1) and the owner words
        assert torch.equal(out, edge_keys["want"])
        r = E.k2_park_read()
        assert (r["fallbacks"], r["violations"]) == (0, 0) and r["owner"].shape == (1024,) and not r["owner"].any()
    finally:
        E.close()


# ---- two contexts ------------------------------------------------------------------------------------------------------------------------
def test_a_refusal_armed_on_one_context_never_fires_on_another(toy, env, probe):
    from tfhe_aes_amd.server import Server

    case = ws.BY_NAME["many_sbox"]
    h0 = case.build(env, 0)
    a = Server(toy.keys, device=0)
    b = Server(None, device=0, clone_from=a)
    try:
        w0 = once(a, case, h0)
        case.check_clear(env, h0, [host(t) for t in w0])
        n_alloc = af.ALLOCATIONS["many_sbox"]
        for j in (1, n_alloc):
            a.engine.workspace_poison(RELEASE)
            b.engine.workspace_poison(RELEASE)
            a.engine.alloc_debug(j)
            b.engine.alloc_debug(af.FAR)
            da, db = resident(h0), resident(h0)
            got = {}

            def other():
                try:
                    got["out"] = as_tuple(case.run(b, db))
                    b.synchronize()
                except Exception as e:                              # reported by the assertion below
                    got["error"] = e

            t = threading.Thread(target=other)
            t.start()
            refused(lambda: case.run(a, da))
            t.join()
            a.synchronize()
            assert "error" not in got, got.get("error")
            assert same(got["out"], w0)
            assert b.engine.alloc_debug(0) == n_alloc and a.engine.alloc_debug(0) == j
            run_probe(a.engine, probe)
            run_probe(b.engine, probe)
            assert same(once(a, case, h0), w0)
    finally:
        a.engine.close()
        b.engine.close()
