"""No call may depend on what an earlier call left in the context's scratch, on where that scratch lay, on how large it was, or on a
call that is still in flight.  Every case of workspace_state.CASES gets a Server of its own and runs, on resident inputs,

  a. anchor        on the fresh context: W0, checked against the clear model (or the CPU oracle's words); the buffers the case is known
                   to use are not empty
  b. poison        fheaes_workspace_poison(FILL): the byte count is the sum of fheaes_workspace_info's sizes and every buffer reads
                   back as the pattern of its class; the run's words are W0
  c. grown behind  a different, larger call (the pairing of the table) leaves ws_misc and the f64 buffer larger than the case needs;
                   FILL again; W0
  d. grown inside  fheaes_workspace_poison(RELEASE): every size is 0; W0 from nothing; reserve(64) gives the call's own growth
                   sequence a second starting size; W0
  e. twice         the two variants back to back on a caller's stream that a chain of matmuls keeps busy, so that the first call is
                   wholly in flight when the second is made; each is its own single-call result; then the other order

Every comparison is torch.equal on the 64-bit words.  The park-slot counters are state, not scratch: the hooks leave them alone.
A call that uses no scratch at all (uses == ()) asserts exactly that after its anchor -- there is nothing of its own to poison -- and
meets the poisoned scratch of the larger call in step c."""
import time

import pytest

import workspace_state as ws
from gpu_support import dev, host
from tfhe_aes_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


def as_tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def resident(inputs):
    d = dict(inputs)
    for name in inputs["dev"]:
        d[name] = dev(inputs[name])
    return d


def start(srv, case, inputs):
    """the call enqueued on fresh resident inputs, nothing synchronised: (the outputs, what must stay alive until they are read)"""
    d = resident(inputs)
    return as_tuple(case.run(srv, d)), d


def once(srv, case, inputs):
    outs, d = start(srv, case, inputs)
    srv.synchronize()
    return outs


def same(a, b):
    import torch

    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def sizes(srv):
    return {b["name"]: b["bytes"] for b in srv.engine.workspace_info()}


def poison_fill(srv):
    """FILL, with step b's assertions: the byte count, and the pattern of every non-empty buffer at both ends"""
    before = srv.engine.workspace_info()
    filled = srv.engine.workspace_poison(_native.WS_POISON_FILL)
    assert filled == sum(b["bytes"] for b in before)
    after = srv.engine.workspace_info()
    assert [(b["name"], b["bytes"], b["class"]) for b in after] == [(b["name"], b["bytes"], b["class"]) for b in before]
    for b in after:
        if b["bytes"]:
            assert (b["first"], b["last"]) == ws.pattern_words(b["class"], b["bytes"]), "%s (%d bytes, %s) is not poisoned: %#x .. %#x" % (
                b["name"], b["bytes"], b["class"], b["first"], b["last"])
    return filled


@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.name)
def test_no_call_depends_on_the_state_of_the_scratch(case, toy, env):
    from tfhe_aes_amd.server import Server

    h0, h1 = case.build(env, 0), case.build(env, 1)
    srv = Server(toy.keys, device=0)
    try:
        park = srv.engine.k2_park_read()
        assert all(v == 0 for v in sizes(srv).values())
        # a. anchor
        w0 = once(srv, case, h0)
        case.check_clear(env, h0, [host(t) for t in w0])
        anchor = sizes(srv)
        if case.uses:
            assert sum(anchor.values()) > 0
            assert all(anchor[name] > 0 for name in case.uses), {name: anchor[name] for name in case.uses}
        else:
            assert sum(anchor.values()) == 0, "a call listed as using no scratch grew %s" % {k: v for k, v in anchor.items() if v}
        # b. poisoned
        assert poison_fill(srv) == sum(anchor.values())
        assert same(once(srv, case, h0), w0), "after a fill of its own scratch"
        # c. grown behind it
        g = ws.GROWERS[case.pair]
        hg = g.build(env, 0)
        g.check_clear(env, hg, [host(t) for t in once(srv, g, hg)])
        grown = sizes(srv)
        assert all(grown[name] > anchor[name] for name in ws.GROWN), {name: (anchor[name], grown[name]) for name in ws.GROWN}
        assert all(grown[name] >= anchor[name] for name in anchor)
        assert poison_fill(srv) == sum(grown.values())
        assert same(once(srv, case, h0), w0), "after a larger call and a fill of its scratch"
        # d. grown inside it
        assert srv.engine.workspace_poison(_native.WS_POISON_RELEASE) == sum(grown.values())
        assert all(v == 0 for v in sizes(srv).values())
        assert same(once(srv, case, h0), w0), "grown from nothing"
        assert sizes(srv) == anchor                          # the same growth as on the fresh context
        srv.engine.reserve(64)
        d = resident(h0)
        clock = time.perf_counter()
        again = as_tuple(case.run(srv, d))
        enqueue_ms = 1e3 * (time.perf_counter() - clock)      # what the host needs to enqueue the call: sizes the chain of step e
        srv.synchronize()
        assert same(again, w0), "after reserve(64) on what the call grew"
        # ... and with the reservation as the starting size of the call's own growth: some buffers there already, too small or not
        held = sum(sizes(srv).values())
        assert srv.engine.workspace_poison(_native.WS_POISON_RELEASE) == held
        srv.engine.reserve(64)
        reserved = sizes(srv)
        assert sum(reserved.values()) > 0 and all(v == 0 for v in (reserved["ws_misc"], reserved["ws_vp"], reserved["ws_tree"]))
        assert same(once(srv, case, h0), w0), "grown from a reservation of 64 bits"
        # e. twice in flight
        w1 = once(srv, case, h1)
        case.check_clear(env, h1, [host(t) for t in w1])
        assert not same(w0, w1)
        # On a stream of the caller's that a chain of matmuls keeps busy: everything the first call enqueues -- the upload of its tables
        # out of the one pinned buffer among it -- is still waiting when the second call is made.  The chain is sized from the time the
        # host took to enqueue the call, and the end event says whether it was long enough.
        import torch

        s, a = torch.cuda.Stream(), ws.producer_matrix()
        steps = max(8, int((4 * enqueue_ms + 8) / ws.PRODUCER_MS_PER_STEP) + 1)
        srv.engine.set_stream(s.cuda_stream)
        for first, second in ((h0, h1), (h1, h0)):
            d1, d2 = resident(first), resident(second)
            t0, t1, keep = ws.producer(s, a, steps)
            o1 = as_tuple(case.run(srv, d1))
            in_flight = not t1.query()
            o2 = as_tuple(case.run(srv, d2))
            srv.synchronize()
            assert in_flight or case.name in ws.WAITS_INSIDE, "the first call returned after %d matmuls (%.1f ms) were done" % (steps, t0.elapsed_time(t1))
            assert same(o1, w0 if first is h0 else w1), "the first of two calls in flight"
            assert same(o2, w1 if first is h0 else w0), "the second of two calls in flight"
        srv.engine.set_stream(None)
        after = srv.engine.k2_park_read()
        assert (after["fallbacks"], after["violations"]) == (park["fallbacks"], park["violations"]) and after["violations"] == 0
        assert (after["owner"] == park["owner"]).all()
    finally:
        srv.engine.set_stream(None)
        srv.synchronize()
        srv.engine.close()


def test_workspace_hooks_on_a_live_context(toy):
    """the enumeration ends at WS_BUFFERS, a bad mode is refused with a message, an empty context fills and frees nothing, and neither
    hook touches the keys: a call after RELEASE needs no new upload"""
    import ctypes

    from tfhe_aes_amd.server import Server

    srv = Server(toy.keys, device=0)
    E = srv.engine
    try:
        info = E.workspace_info()
        assert len(info) == _native.WS_BUFFERS and len({b["name"] for b in info}) == _native.WS_BUFFERS
        assert {b["class"] for b in info if b["name"] == "ws_ggswf"} == {"f64"}
        assert {b["name"] for b in info if b["class"] == "tables"} == {"ws_misc", "stage[0]", "stage[1]", "stage[2]", "stage[3]"}
        assert all((b["bytes"], b["first"], b["last"]) == (0, 0, 0) for b in info)
        assert E._lib.fheaes_workspace_info(E._h, _native.WS_BUFFERS, None, 0, None, None, None, None) == -1
        assert b"index" in E._lib.fheaes_last_error(E._h)
        for mode in (2, -1):
            assert E._lib.fheaes_workspace_poison(E._h, mode, None) == -1
            assert b"mode" in E._lib.fheaes_last_error(E._h)
        assert E.workspace_poison(_native.WS_POISON_FILL) == 0 and E.workspace_poison(_native.WS_POISON_RELEASE) == 0
        # a host-memspace call stages its arguments: the staging buffers are scratch like the rest
        c = ws.own_client(toy)
        x = c.encrypt_bytes([0x53, 0xA7])
        want = srv.many_sbox(x, False)
        staged = {b["name"]: b["bytes"] for b in E.workspace_info()}
        assert staged["stage[0]"] == x.nbytes and staged["stage[1]"] == want.nbytes and staged["stage[2]"] == 0
        assert poison_fill(srv) == sum(staged.values())
        assert (srv.many_sbox(x, False) == want).all()
        assert E.workspace_poison(_native.WS_POISON_RELEASE) == sum(staged.values())
        assert (srv.many_sbox(x, False) == want).all()
        n = ctypes.c_uint64(7)
        assert E._lib.fheaes_workspace_poison(E._h, _native.WS_POISON_FILL, ctypes.byref(n)) == 0 and n.value == sum(staged.values())
    finally:
        E.close()
