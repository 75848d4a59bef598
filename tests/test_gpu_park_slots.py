"""The claimed parking slots of the paired blind-rotation kernel (kern_blindrot_pair.h), tested as a protocol and not only by its words.

A workgroup claims one of its XCC's 128 slots with a compare-and-swap on an owner word, probing from a hardware-id hint and wrapping,
falls back to the private slot 1024 + its index when all 128 are owned, and releases the slot (an exchange to 0) after its last parking
store has been acknowledged.  The kernel counts fallbacks and releases of a word that was not its own; fheaes_k2_park_debug lets a
launch start from owner words that mark slots as taken by someone else and records {slot, XCC} per workgroup.  That makes the paths a
nearly free pool never takes run on purpose: the exhausted pool, one free slot per XCC handed from workgroup to workgroup, a random half
taken.  Every launch is compared word for word with a private-parking launch of the same inputs, whose rows of the first, a middle and
the last (ragged) workgroup are compared with the CPU oracle."""
from contextlib import contextmanager

import numpy as np
import pytest

from gpu_support import dev, filled, host, unit_rows
from tfhe_aes_amd import _native

pytestmark = pytest.mark.gpu

SLOTS, PER_XCC, XCCS = _native.K2_PARK_SLOTS, 128, 8
TAKEN = 0xFFFFFFFF                 # an owner word no workgroup of a launch can have (1 + its index)
SIZES = (16384, 4096, 1001)        # 11 generations of 2,816 workgroups; 768 workgroups; 251 four-ciphertext ones, the last with one row


@pytest.fixture(scope="module")
def park(opt):
    """per size: seeded small-LWE inputs on the GPU, the private-parking output (checked against the oracle on the rows of the first, a
    middle and the last workgroup) and the grid"""
    p, E = opt.params, opt.engine()
    data = {}
    try:
        E.k2_set_parking(False)
        for m in SIZES:
            plan = E.k2_plan(m)
            assert plan["form"] == 2 and plan["kernel"].endswith("parking=private")
            grid = plan["units_main"] + plan["units_tail"]
            rng = np.random.default_rng(0x9A60000 + m)
            small_np = rng.integers(0, 1 << 64, (m, p.n + 1), dtype=np.uint64)
            small = dev(small_np)
            want = filled((m, p.big1), -1)
            E.cbs_pbs_batch(small, want, m)
            E.synchronize()
            first, mid, last = unit_rows(plan, 0, m), unit_rows(plan, grid // 2, m), unit_rows(plan, grid - 1, m)
            rows = [first[0], first[-1], mid[0], mid[-1]] + last
            assert np.array_equal(host(want[rows]), opt.oracle.cbs_pbs(small_np[rows])), m
            data[m] = (small, want, grid)
    finally:
        E.k2_set_parking(True)
    return data


@contextmanager
def _hook(E, initial=None, record=True):
    E.k2_park_debug(initial, record)
    try:
        yield
    finally:
        E.k2_park_debug(None, False)
        E.k2_set_parking(True)


def _launch(opt, park, m):
    """one claimed-or-private launch of the size's inputs; (output, counters before, counters and records after)"""
    E = opt.engine()
    small, want, _ = park[m]
    before = E.k2_park_read()
    out = filled(want.shape, -1)
    E.cbs_pbs_batch(small, out, m)
    after = E.k2_park_read()
    return out, before, after


def _same(out, want, what):
    import torch

    if not torch.equal(out, want):
        rows = torch.nonzero((out != want).any(dim=1)).flatten().tolist()
        raise AssertionError("%s: %d rows differ from the private-parking launch, the first %s" % (what, len(rows), rows[:8]))


def _deltas(before, after):
    return after["fallbacks"] - before["fallbacks"], after["violations"] - before["violations"]


def test_default_pool_claims_a_slot_of_its_own_xcc(opt, park):
    import torch

    E = opt.engine()
    seen_xcc = set()
    for m in SIZES:
        with _hook(E, None, True):
            out, before, after = _launch(opt, park, m)
        _, want, grid = park[m]
        assert _deltas(before, after) == (0, 0), m
        assert not after["owner"].any(), "owner words left taken after a %d-bit launch: %s" % (m, np.flatnonzero(after["owner"])[:16])
        rec = after["record"]
        assert rec.shape == (grid, 2), m
        slot, xcc = rec[:, 0], rec[:, 1]
        assert (xcc < XCCS).all() and (slot < SLOTS).all(), m
        assert (slot // PER_XCC == xcc).all(), "a workgroup claimed a slot of another XCC's pool (%d bits)" % m
        _same(out, want, "%d bits" % m)
        seen_xcc |= set(xcc.tolist())
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert seen_xcc == set(range(XCCS))


@pytest.mark.parametrize("m", [16384, 1001])
def test_exhausted_pool_falls_back_to_the_private_slot_of_every_workgroup(opt, park, m):
    """every owner word taken: all 128 compare-and-swaps of every workgroup fail, and workgroup i parks in slot 1024 + i of the slab
    (16,384 bits: grid 2,816, the highest slot k2_pair_park_bytes provides)"""
    E = opt.engine()
    pattern = np.full(SLOTS, TAKEN, dtype=np.uint32)
    with _hook(E, pattern, True):
        out, before, after = _launch(opt, park, m)
    _, want, grid = park[m]
    fallbacks, violations = _deltas(before, after)
    assert fallbacks == grid
    rec = after["record"]
    assert rec.shape == (grid, 2) and (rec[:, 1] < XCCS).all()
    assert np.array_equal(rec[:, 0], SLOTS + np.arange(grid, dtype=np.uint32))
    assert np.array_equal(after["owner"], pattern), "a workgroup released a slot it never claimed"
    assert violations == 0
    _same(out, want, "%d bits" % m)


def test_one_free_slot_per_xcc_is_handed_on_and_probes_wrap(opt, park):
    """one free slot per XCC, at a different local index on each (0 and 127 among them): a probe that starts past it must wrap.  At
    16,384 bits the slot goes from workgroup to workgroup over 11 generations while the others of its XCC fall back -- the test of
    "release only after the last parking store is acknowledged": a hand-over too early corrupts the next owner's parked words"""
    E = opt.engine()
    free_local = [0, 127, 37, 90, 5, 64, 111, 23]
    free = np.array([x * PER_XCC + free_local[x] for x in range(XCCS)])
    pattern = np.full(SLOTS, TAKEN, dtype=np.uint32)
    pattern[free] = 0
    m = 16384
    with _hook(E, pattern, True):
        out, before, after = _launch(opt, park, m)
    _, want, grid = park[m]
    fallbacks, violations = _deltas(before, after)
    rec = after["record"]
    assert rec.shape == (grid, 2)
    slot, xcc = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64)
    assert (xcc < XCCS).all()
    claimed = slot < SLOTS
    assert np.array_equal(slot[claimed], free[xcc[claimed]]), "a claim of a taken slot or of another XCC's free one"
    assert np.array_equal(slot[~claimed], SLOTS + np.flatnonzero(~claimed))
    claims = np.bincount(xcc[claimed], minlength=XCCS)
    ran = np.bincount(xcc, minlength=XCCS)
    assert ((claims >= 1) | (ran == 0)).all(), "an XCC whose free slot nobody claimed: claims %s, workgroups %s" % (claims, ran)
    assert fallbacks == grid - int(claimed.sum())
    assert not after["owner"][free].any(), "a free slot left owned"
    assert np.array_equal(after["owner"], pattern)
    assert violations == 0
    _same(out, want, "%d bits" % m)
    print("one free slot per XCC, %d bits: %d claims (per XCC %s), %d fallbacks of %d workgroups"
          % (m, int(claimed.sum()), claims.tolist(), fallbacks, grid))


def test_random_half_taken_is_never_claimed(opt, park):
    """a seeded random half of each XCC's slots owned by someone else: no workgroup lands on one, and with 64 free slots per XCC for at
    most 32 resident workgroups (one per CU) nobody falls back"""
    E = opt.engine()
    rng = np.random.default_rng(0x4A1F)
    pattern = np.zeros(SLOTS, dtype=np.uint32)
    for x in range(XCCS):
        idx = x * PER_XCC + rng.choice(PER_XCC, PER_XCC // 2, replace=False)
        pattern[idx] = 0x80000000 | idx                 # distinct, and no workgroup's 1 + index
    for m in (16384, 4096):
        with _hook(E, pattern, True):
            out, before, after = _launch(opt, park, m)
        _, want, grid = park[m]
        rec = after["record"]
        assert rec.shape == (grid, 2), m
        slot, xcc = rec[:, 0], rec[:, 1]
        assert (slot < SLOTS).all() and (slot // PER_XCC == xcc).all(), m
        assert not pattern[slot].any(), "claims of taken slots (%d bits): %s" % (m, np.unique(slot[pattern[slot] != 0])[:16])
        assert _deltas(before, after) == (0, 0), m
        assert np.array_equal(after["owner"], pattern), m
        _same(out, want, "%d bits" % m)


def test_park_hook_leaves_other_modes_and_contexts_alone(opt, toy, park):
    import ctypes as C

    E = opt.engine()
    m = 1001
    _, want, grid = park[m]
    pattern = np.full(SLOTS, TAKEN, dtype=np.uint32)
    # private parking: the pattern and the recording do nothing, the owner words and the counters do not move
    with _hook(E, pattern, True):
        E.k2_set_parking(False)
        out, before, after = _launch(opt, park, m)
    assert _deltas(before, after) == (0, 0)
    assert np.array_equal(after["owner"], before["owner"]) and after["record"].shape == (0, 2)
    _same(out, want, "%d bits" % m)
    # after the hook is cleared, a claimed launch starts from a free pool again
    out, before, after = _launch(opt, park, m)
    assert _deltas(before, after) == (0, 0) and not after["owner"].any()
    _same(out, want, "%d bits" % m)
    # a record buffer shorter than the last recorded launch is refused
    with _hook(E, None, True):
        out, _, after = _launch(opt, park, m)
        assert after["record"].shape == (grid, 2)
        lib, buf, n = _native.load_library(), np.zeros((grid, 2), dtype=np.uint32), C.c_uint64()
        u32p = C.POINTER(C.c_uint32)
        assert lib.fheaes_k2_park_read(E._h, None, None, None, buf.ctypes.data_as(u32p), grid - 1, C.byref(n)) == -1
        assert lib.fheaes_k2_park_read(E._h, None, None, None, buf.ctypes.data_as(u32p), grid, C.byref(n)) == 0
        assert n.value == grid and np.array_equal(buf, after["record"])
    # k = 1 (toy): never the paired kernel; the calls are accepted and change nothing
    T, tp = toy.engine(), toy.params
    assert T.k2_plan(2048)["form"] != 2
    rng = np.random.default_rng(0x70F1)
    small = dev(rng.integers(0, 1 << 64, (2048, tp.n + 1), dtype=np.uint64))
    ref = filled((2048, tp.big1), -1)
    T.cbs_pbs_batch(small, ref, 2048)
    with _hook(T, pattern, True):
        before = T.k2_park_read()
        got = filled(ref.shape, -1)
        T.cbs_pbs_batch(small, got, 2048)
        after = T.k2_park_read()
    assert _deltas(before, after) == (0, 0) and after["record"].shape == (0, 2) and np.array_equal(after["owner"], before["owner"])
    _same(got, ref, "k = 1, 2,048 bits")
