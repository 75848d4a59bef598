"""ServerGroup on 1, 3 and 5 contexts at PARAM_TOY: every case of group_splits.CASES -- every public method of the group -- with host
arrays on the groups of 3 and of 5, and with resident tensors on the group of 3.  The words must be those of ONE Server for the same call
(the engine is deterministic, so the comparison is exact), and they must decrypt to what the clear model says: a wrong offset produces
perfectly formed ciphertexts of the wrong blocks, which only the second check sees when both sides share the mistake, and which the
audit cannot see at all.  test_group_splits_cpu.py pins the same table for g = 1..6 and n = 0..7 on an echo model, without a GPU.

A test box has one GPU, so all nine contexts sit on device 0: one key upload and g - 1 device-to-device clones per group."""
import numpy as np
import pytest

import group_splits as gs
from gpu_support import dev, guarded, guards_intact, host, settled, toy_server  # noqa: F401
from tfhe_aes_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(toy, toy_server):  # noqa: F811
    return gs.Env(toy, toy_server)


@pytest.fixture(scope="module")
def groups(toy):
    from tfhe_aes_amd.server import ServerGroup

    made = {g: ServerGroup(toy.keys, devices=(0,) * g) for g in (1, 3, 5)}
    yield made
    for grp in made.values():
        for s in grp.servers:
            s.engine.close()


@pytest.fixture(scope="module")
def reference(env):
    """(the inputs, one Server's words) of a run of the table, computed once, checked against the clear model, and left unchanged"""
    done = {}

    def of(case, n):
        if (case.name, n) not in done:
            h = case.build(env, n)
            want = gs.flat(gs.call(env.server, case, gs.fresh(h)))
            env.server.synchronize()
            case.check_clear(env, h, want)
            done[case.name, n] = (h, want)
        return done[case.name, n]

    return of


def same(got, want):
    return len(got) == len(want) and all(tuple(a.shape) == tuple(b.shape) and np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("g", (3, 5))
@pytest.mark.parametrize("run", gs.RUNS, ids=gs.run_id)
def test_a_group_writes_the_words_of_one_server_on_host_arrays(run, g, groups, reference, env):
    case, n = run
    h, want = reference(case, n)
    got = gs.flat(gs.call(groups[g], case, gs.fresh(h)))
    words = "the same words" if same(got, want) else "OTHER WORDS"
    try:                                                                             # both verdicts in one failure: a wrong split shows in each
        case.check_clear(env, h, got)
        clear = "decrypts to the clear model's answer"
    except AssertionError as e:
        clear = "DECRYPTS TO SOMETHING ELSE (%s)" % (str(e).splitlines() or ["assert"])[0][:200]
    assert (words, clear) == ("the same words", "decrypts to the clear model's answer"), "%s on %d items over %d contexts against one context: %s, %s" % (
        case.name, n, g, words, clear)


@pytest.mark.parametrize("run", [r for r in gs.RUNS if r[0].name in gs.IN_PLACE_BLOCKS and r[1] == 4], ids=gs.run_id)
def test_a_group_of_one_is_one_server(run, groups, reference):
    case, n = run
    h, want = reference(case, n)
    assert same(gs.flat(gs.call(groups[1], case, gs.fresh(h))), want)


@pytest.mark.parametrize("run", gs.RUNS, ids=gs.run_id)
def test_a_group_writes_the_same_words_into_resident_tensors(run, groups, reference):
    """every array of ciphertext words resident and settled, the state of an in-place call inside guard rows; nothing is synchronised
    here after the call returns: what comes back must be finished"""
    case, n = run
    h, want = reference(case, n)
    d = gs.map_words({"a": h["a"], "kw": h["kw"]}, dev)
    buf = None
    if h["state"] is not None:
        state = h["a"][h["state"]]
        buf, rows = guarded(state.size // state.shape[-1], state.shape[-1])
        rows.copy_(d["a"][h["state"]].view(rows.shape))
        d["a"][h["state"]] = settled(rows.view(state.shape))
    got = gs.flat(getattr(groups[3], case.method)(*d["a"], **d["kw"]))
    assert not isinstance(got[0], np.ndarray) and all(t.is_cuda for t in got if not isinstance(t, np.ndarray))     # block_of_message is a list
    if case.method == "aes_key_unwrap_packed":
        assert got[0].is_cuda and got[1].is_cuda                                      # the store and `valid`
    assert buf is None or guards_intact(buf)
    assert same(tuple(t if isinstance(t, np.ndarray) else host(t) for t in got), want), "%s on %d resident items differs from the host-array words" % (case.name, n)


def test_a_refused_argument_in_one_shard_raises_on_the_caller_and_leaves_the_other_shards_done(groups, reference, env):
    """key index n_keys in the last block only: a refused argument (FHEAES_ERR_INVALID), not a device fault.  4 blocks are 2 + 1 + 1"""
    import threading

    case = gs.BY_NAME["aes_encrypt_keyed"]
    h, want = reference(case, 4)
    rk, kob, state = gs.fresh(h)["a"]
    before = state.copy()
    caller = threading.get_ident()
    with pytest.raises(_native.FheAesError) as e:
        groups[3].aes_encrypt_keyed(rk, kob[:3] + [int(rk.shape[0])], state)
    assert e.value.code == -1 and threading.get_ident() == caller
    assert np.array_equal(state[:3], want[0][:3]), "the shards beside the refused one did not finish"
    assert np.array_equal(state[3], before[3]), "the refused shard wrote"
    assert same(gs.flat(gs.call(groups[3], case, gs.fresh(h))), want), "the group after a refused call"


def test_the_audit_of_a_group_sums_its_contexts_and_an_idle_context_adds_nothing(groups, reference, env):
    case = gs.BY_NAME["aes_encrypt"]
    h, want = reference(case, 4)                                                      # 1 + 1 + 1 + 1 + 0 on 5 contexts
    from tfhe_aes_amd.server import Server

    grp = groups[5]
    one = Server(None, device=0, clone_from=env.server)                                # a context of its own: the session's stays unaudited
    try:
        one.audit(rows=1, seed=7)
        rk, state = gs.fresh(h)["a"]
        one.aes_encrypt(rk, state[:1])
        single = one.audit_report()
        assert single.launches > 0 and single.rows_checked > 0 and single.rows_wrong == 0
        grp.audit(rows=1, seed=7)
        assert same(gs.flat(gs.call(grp, case, gs.fresh(h))), want)
        per_context = [s.audit_report() for s in grp.servers]
        total = grp.audit_report()
        assert total.rows_wrong == 0 and grp.audit_check().rows_wrong == 0
        assert [(r.launches, r.rows_checked, r.rows_wrong) for r in per_context] == [(single.launches, single.rows_checked, 0)] * 4 + [(0, 0, 0)]
        assert total.launches == 4 * single.launches and total.rows_checked == 4 * single.rows_checked
    finally:
        one.engine.close()
        grp.audit(rows=0)
