"""The audit of the two key switches (include/fheaes.h, "audit of the key switches"; kern_audit.h, launch_keyswitch_audit): sampled rows of
every K1 and K3 launch computed again by the plain form and compared on the device.

  1. the plain form by itself, every row: fheaes_audit_plain_batch against the product launch and against the oracle, word for word and
     inside guard rows, at 1, 127, 128 and 129 rows, at PARAM_TOY and PARAM_EDGE, K1 at column counts on both sides of a tile, K3 over all
     key blocks and over one, on the edge inputs and edge keys of edge_words.py
  2. clean calls: with all three stages audited the calls write the words of the unaudited call, every stage counts its own launches and
     rows, and the blind rotation counts and samples what it does alone
  3. one XOR each through fheaes_audit_stage_debug, in a sampled row and outside the sample
  4. the edges of the mechanism, the allocations, and a ServerGroup

Every test has a context of its own.  Every expected value is exact: the stages are integer arithmetic mod 2^64.  What these tests were
shown to fail on: DESIGN.md section 5, "The key-switch audit under test"."""
import dataclasses
from contextlib import contextmanager

import numpy as np
import pytest

import audit_calls as ac
import audit_model as am
import audit_stages as st
import edge_words as ew
import workspace_state as ws
from edge_words import PARAM_EDGE
from gpu_support import dev, guarded, guards_intact, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_TOY, _native
from tfhe_aes_amd.server import AuditMismatch, Server, ServerGroup

pytestmark = pytest.mark.gpu

KS, K2, PF = st.KS, st.K2, st.PF
SEED, MASK = st.SEED, st.MASK


@contextmanager
def private(server):
    """a Server on a context of its own with `server`'s keys"""
    srv = Server(None, device=0, clone_from=server)
    try:
        yield srv
    finally:
        srv.engine.set_stream(None)
        srv.synchronize()
        srv.engine.close()


def counters(E, stage):
    r = E.audit_stage_read(stage)
    return r["launches"], r["rows_checked"], r["rows_wrong"]


def records(E, stage):
    return [[int(x) for x in rec] for rec in E.audit_stage_read(stage)["records"]]


def all_on(E, rows, min_rows=0, seed=SEED):
    for s in st.STAGES:
        E.audit_stage_set(s, rows, min_rows, seed)


def big_rows(p, m, tag):
    return dev(np.random.default_rng(0x57A6E + tag).integers(0, 1 << 64, (m, p.big1), dtype=np.uint64))


def launch(E, stage, x, m):
    """one product launch of the stage on m rows into guard rows; (buffer, its m rows), settled"""
    buf, out = guarded(m, st.row_words(E.params, stage))
    (E.keyswitch_batch if stage == KS else E.pfpks_batch)(x[:m], out, m)
    E.synchronize()
    return buf, out


def plain(E, stage, x, m, block=-1):
    buf, out = guarded(m, st.row_words(E.params, stage, block))
    E.audit_plain_batch(stage, x[:m], out, m, block)
    E.synchronize()
    return buf, out


# ---- 1. the plain form, every row ----------------------------------------------------------------------------------------------------------
class Keyed:
    """an engine under edge keys, the edge inputs of both key switches (129 rows) and the oracle's words for them, computed once"""

    def __init__(self, p, pattern, k3=True):
        self.p = p
        ksk = ew.key_words(pattern, (p.big, p.ks_level, p.n + 1), seed=0x6E7 + p.n)
        pf = ew.key_words(pattern, (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8) if k3 else np.zeros(p.pfpksk_words, dtype=np.uint64)
        bsk = np.zeros(p.bsk_words, dtype=np.uint64)
        self.E = _native.Engine(p, device=0)
        self.E.upload_keys(ksk, bsk, pf)
        o = orc.Oracle(p, ksk, bsk, pf)
        self.x = {KS: ew.ks_inputs(p, "K1", st.ROWS_MAX)[0], PF: ew.ks_inputs(p, "K3", st.ROWS_MAX)[0]}
        self.want = {KS: o.keyswitch(self.x[KS])}
        if k3:
            self.want[PF] = o.pfpks(self.x[PF])                          # [129][k+1][(k+1)N]
        self.x_d = {s: dev(a) for s, a in self.x.items()}
        self.pattern = pattern


@pytest.fixture(scope="module", params=["mixture", "m128"])
def toy_keyed(request):
    kit = Keyed(PARAM_TOY, request.param)
    yield kit
    kit.E.close()


@pytest.fixture(scope="module")
def edge_keyed():
    kit = Keyed(PARAM_EDGE, "mixture")
    yield kit
    kit.E.close()


def check_every_row(kit, m):
    p, E = kit.p, kit.E
    gsz = (p.k + 1) * p.N
    for stage in (KS, PF):
        want = kit.want[stage][:m].reshape(m, -1)
        buf_p, got_p = launch(E, stage, kit.x_d[stage], m)
        buf_a, got_a = plain(E, stage, kit.x_d[stage], m)
        assert guards_intact(buf_p) and guards_intact(buf_a), "%s, m = %d: a store outside the %d output rows" % (stage, m, m)
        a, b = host(got_a), host(got_p)
        assert np.array_equal(a, want), "%s, m = %d: the plain form differs from the oracle at %s" % (stage, m, np.argwhere(a != want)[:8].tolist())
        assert np.array_equal(b, want), "%s, m = %d: the product launch differs from the oracle" % (stage, m)
    for block in (0, p.k):
        buf, got = plain(E, PF, kit.x_d[PF], m, block)
        assert guards_intact(buf) and tuple(got.shape) == (m, gsz)
        assert np.array_equal(host(got), kit.want[PF][:m, block]), "K3, m = %d: key block %d alone" % (m, block)


@pytest.mark.parametrize("m", st.ROW_COUNTS)
def test_plain_form_is_the_product_launch_and_the_oracle_at_param_toy(m, toy_keyed):
    check_every_row(toy_keyed, m)


def test_the_edge_rows_are_among_the_inputs(toy_keyed):
    """whole rows of 0, 2^64 - 1, 2^63 and 2^63 - 1, and the row that drives an int32 accumulator of K3 to its bound Q 128 128 under the
    key whose bytes are all -128"""
    p = toy_keyed.p
    for stage, name in ((KS, "K1"), (PF, "K3")):
        words = list(ew.ks_words(p, name))
        for w, v in zip(("zero", "all_ones", "top_bit", "below_top"), ew.EXTREMES):
            row = toy_keyed.x[stage][words.index(w)]
            assert ew.ks_words(p, name)[w] == v and (row == np.uint64(v)).all() and words.index(w) < st.ROW_COUNTS[1]
    row = toy_keyed.x[PF][list(ew.ks_words(p, "K3")).index("lo_m128_hi_8")]
    peak, bound = ew.k3_accumulator_peak(row, ew.KEY_M128, p)
    assert peak == bound
    assert ew.balanced_bytes(ew.KEY_M128) == [-128] * 8


@pytest.mark.parametrize("m", st.ROW_COUNTS)
def test_plain_form_is_the_product_launch_and_the_oracle_at_param_edge(m, edge_keyed):
    """k = 4: 12,800 K3 columns, Q = 6,147 rows"""
    assert st.row_words(PARAM_EDGE, PF) == 12800
    check_every_row(edge_keyed, m)


@pytest.mark.parametrize("n", st.K1_SMALL_N)
def test_k1_plain_form_on_both_sides_of_a_column_tile(n):
    p = dataclasses.replace(PARAM_TOY, name="PARAM_TOY_N%d" % n, lwe_dimension=n)
    kit = Keyed(p, "mixture", k3=False)
    try:
        for m in st.ROW_COUNTS:
            want = kit.want[KS][:m]
            buf_p, got_p = launch(kit.E, KS, kit.x_d[KS], m)
            buf_a, got_a = plain(kit.E, KS, kit.x_d[KS], m)
            assert guards_intact(buf_p) and guards_intact(buf_a) and tuple(got_a.shape) == (m, n + 1)
            assert np.array_equal(host(got_a), want), np.argwhere(host(got_a) != want)[:8].tolist()
            assert np.array_equal(host(got_p), want)
    finally:
        kit.E.close()


def test_plain_batch_bad_arguments(toy_keyed):
    E, p = toy_keyed.E, toy_keyed.p
    x = toy_keyed.x_d[KS]
    out = guarded(1, st.row_words(p, PF))[1]
    for stage, block in ((KS, 0), (KS, p.k), (PF, p.k + 1), (PF, -2), (K2, -1), ("linear", -1)):
        with pytest.raises(_native.FheAesError) as err:
            E.audit_plain_batch(stage, x, out, 1, block)
        assert err.value.code == -1, (stage, block)


# ---- 2. clean calls ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


def resident(inputs):
    d = dict(inputs)
    for name in inputs["dev"]:
        d[name] = dev(inputs[name])
    return d


def once(srv, case, inputs):
    out = case.run(srv, resident(inputs))
    srv.synchronize()
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def same(a, b):
    import torch

    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(st.CLEAN_CALLS))
def test_calls_are_clean_with_all_three_stages_audited(name, toy_server, env):
    case, sizes = ws.BY_NAME[name], st.CLEAN_CALLS[name]
    h = case.build(env, 0)
    with private(toy_server) as srv:
        E = srv.engine
        w0 = once(srv, case, h)
        case.check_clear(env, h, [host(t) for t in w0])
        assert all(counters(E, s) == (0, 0, 0) for s in st.STAGES)
        for rows in (1, 256):
            srv.audit(rows=rows, seed=SEED)                                # the blind rotation alone: what its audit counts by itself
            once(srv, case, h)
            k2_alone = E.audit_read()
            srv.audit(rows=rows, seed=SEED, stages=st.STAGES)
            E.profile_reset()
            w = once(srv, case, h)
            prof = E.profile_read()
            assert same(w, w0), "%d rows: the audited call writes other words" % rows
            reports = srv.audit_reports()
            assert list(reports) == list(st.STAGES)
            for s in st.STAGES:
                r = reports[s]
                assert (r.launches, r.rows_checked) == st.counters_after(sizes[s], rows), (s, rows, r)
                assert r.launches == prof[s]["launches"] and sum(sizes[s]) == prof[s]["units"], (s, rows)
                assert r.rows_wrong == 0 and r.records == [], "false alarm in %s: %r" % (s, r.records)
            k2 = E.audit_read()
            assert all(k2[key] == k2_alone[key] for key in ("launches", "rows_checked", "rows_wrong"))
            assert srv.audit_check().launches == len(sizes[K2])
        srv.audit(rows=0)
        assert once(srv, case, h) and all(counters(E, s) == (0, 0, 0) for s in st.STAGES)


def test_k2_samples_the_rows_of_a_k2_only_audit(toy_server, tc):
    """every stage has a launch number of its own: with K1 audited before it, the first blind rotation is still ITS launch 0"""
    p, m, rows = toy_server.params, 24, 8
    named = [am.audit_rows(SEED, j, m, rows) for j in range(3)]
    row = next(r for r in named[0] if r not in named[1] and r not in named[2])
    ct = tc.encrypt_bytes([0x53, 0x00, 0xE1])
    with private(toy_server) as srv:
        E = srv.engine
        srv.audit(rows=rows, seed=SEED, stages=st.STAGES)
        E.audit_debug(row, p.big, MASK)
        d = dev(ct)
        srv.sbox(d, False)
        srv.synchronize()
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 1) and [int(v) for v in r["records"][0][:3]] == [0, row, p.big]
        assert counters(E, KS) == (1, rows, 0)
        assert counters(E, PF)[:2] == (1, rows)                             # K3 ran on the tampered row; both of its forms read the same input
        assert counters(E, PF)[2] == 0
        with pytest.raises(AuditMismatch) as err:
            srv.audit_check()
        assert err.value.stage == K2 and set(err.value.reports) == set(st.STAGES)


def test_param_opt_one_block_with_64_rows_per_stage(opt_server, opt_rk128, oc):
    import torch

    from aes_vectors import F5
    from tfhe_aes_amd import aes_clear

    pt = 0x6BC1BEE22E409F96E93D7E117393172A
    state = oc.encrypt_u128(pt)[None]
    outs = []
    try:
        for stages in ((), st.STAGES):
            opt_server.audit(rows=64 if stages else 0, seed=SEED, stages=stages or (K2,))
            opt_server.engine.profile_reset()
            d = dev(state)
            opt_server.aes_encrypt(opt_rk128, d)
            opt_server.synchronize()
            outs.append(d)
            if stages:
                prof = opt_server.engine.profile_read()
                for s, r in opt_server.audit_reports().items():
                    assert (r.launches, r.rows_checked, r.rows_wrong, r.records) == (10, 640, 0, []), s
                    assert prof[s]["launches"] == 10 and prof[s]["units"] == 1280
                opt_server.audit_check()
    finally:
        opt_server.audit(rows=0)
    assert torch.equal(outs[1], outs[0])
    got = oc.decrypt_bytes(host(outs[1]))
    assert bytes(int(b) for b in got.reshape(-1)) == aes_clear.aes128_encrypt_block(F5[128][0], pt).to_bytes(16, "big")


# ---- 3. tampers ----------------------------------------------------------------------------------------------------------------------------
def found(srv, stage, launch_no, row, word, want_word, n_launches, checked):
    """the stage has exactly one wrong row with this record, audit_check names the stage, and the other stages are clean"""
    E = srv.engine
    assert counters(E, stage) == (n_launches, checked, 1)
    assert records(E, stage) == [[launch_no, row, word, want_word ^ MASK, want_word]]
    for other in st.STAGES:
        if other != stage:
            assert counters(E, other)[2] == 0 and records(E, other) == []
    with pytest.raises(AuditMismatch) as err:
        srv.audit_check()
    assert err.value.stage == stage and err.value.report.rows_wrong == 1
    assert [(r.launch, r.row, r.word, r.got ^ r.want, r.device) for r in err.value.records] == [(launch_no, row, word, MASK, None)]


TAMPERS = [(KS, "first column"), (KS, "last column"), (PF, "key block 0"), (PF, "key block k, last word")]


@pytest.mark.parametrize("stage,where", TAMPERS, ids=["%s-%s" % (s, w.replace(" ", "-").replace(",", "")) for s, w in TAMPERS])
def test_tamper_in_a_sampled_row_of_a_stage_call(stage, where, toy_server):
    import torch

    m, rows = 130, 32
    p = toy_server.params
    gsz = (p.k + 1) * p.N
    word = {"first column": 0, "last column": p.n, "key block 0": 3, "key block k, last word": p.k * gsz + gsz - 1}[where]
    assert word < st.row_words(p, stage) and (where != "key block k, last word" or word == st.row_words(p, stage) - 1)
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, m, word)
        _, want = launch(E, stage, x, m)
        srv.audit(rows=rows, seed=SEED, stages=st.STAGES)
        row = _native.audit_rows(SEED, 0, m, rows)[7]
        E.audit_stage_debug(stage, row, word, MASK)
        buf, out = launch(E, stage, x, m)
        assert torch.nonzero(out != want).tolist() == [[row, word]] and guards_intact(buf)
        found(srv, stage, 0, row, word, int(host(want)[row, word]), 1, rows)
        _, out = launch(E, stage, x, m)                                   # one shot: clean again, the wrong-row counter is sticky
        assert torch.equal(out, want) and counters(E, stage) == (2, 2 * rows, 1)


@pytest.mark.parametrize("stage", [KS, PF])
def test_tamper_outside_the_sample_changes_one_word_and_is_not_reported(stage, toy_server):
    import torch

    m, rows = 130, 32
    p = toy_server.params
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, m, 77)
        _, want = launch(E, stage, x, m)
        all_on(E, rows)
        named = set(_native.audit_rows(SEED, 0, m, rows))
        row = next(r for r in range(m - 1, -1, -1) if r not in named)
        word = st.row_words(p, stage) - 1
        E.audit_stage_debug(stage, row, word, MASK)
        buf, out = launch(E, stage, x, m)
        assert torch.nonzero(out != want).tolist() == [[row, word]] and guards_intact(buf)
        assert int(host(out)[row, word]) ^ int(host(want)[row, word]) == MASK
        assert counters(E, stage) == (1, rows, 0) and records(E, stage) == []
        # a row beyond the launch drops the hook without a write, and it does not wait for a larger launch
        E.audit_stage_debug(stage, m, 0, MASK)
        buf, out = launch(E, stage, x, m)
        assert torch.equal(out, want) and guards_intact(buf)
        _, out = launch(E, stage, x, m)
        assert torch.equal(out, want) and counters(E, stage) == (3, 3 * rows, 0)


def test_tamper_in_pack_s_single_block_launch(toy_server, tc):
    """pack on 513 bits: one K3 launch of key block k alone, (k+1)N words a row; the record's word is the offset inside that block"""
    import torch

    p, m, rows = toy_server.params, 513, 32
    gsz = (p.k + 1) * p.N
    ct = tc.encrypt_bits(np.random.default_rng(0x9AC).integers(0, 2, m).astype(np.uint8))
    with private(toy_server) as srv:
        E = srv.engine
        d = dev(ct)
        clean = srv.pack(d)
        srv.synchronize()
        _, block_k = plain(E, PF, d, m, p.k)
        srv.audit(rows=rows, seed=SEED, stages=st.STAGES)
        row, word = _native.audit_rows(SEED, 0, m, rows)[rows - 1], gsz - 1
        E.audit_stage_debug(PF, row, word, MASK)
        out = srv.pack(d)
        srv.synchronize()
        assert not torch.equal(out, clean)
        found(srv, PF, 0, row, word, int(host(block_k)[row, word]), 1, rows)
        # a word beyond the single block's row is dropped without a write, although the stage's widest row has it
        E.audit_stage_debug(PF, row, gsz, MASK)
        out = srv.pack(d)
        srv.synchronize()
        assert torch.equal(out, clean) and counters(E, PF) == (2, 2 * rows, 1)


def test_tamper_in_a_later_launch_of_a_windowed_aes_encrypt(toy_server, tc):
    """window 2 over 5 blocks: 25 launches of 256 rows of K2 and K3 per call, and 30 of K1, which switches the two segments of a window
    that straddles two steps by themselves.  After one clean call the next K3 launch is K3's launch 25 -- not 80, although 30 audited
    launches of K1 and 25 of K2 lie between -- and checks the rows of launch 25; its input is the first window's"""
    from aes_vectors import BASE, FIPS_C, MASK128
    from tfhe_aes_amd import aes_clear

    p, rows = toy_server.params, 32
    pts = [BASE, 0, MASK128, 0x3243F6A8885A308D313198A2E0370734, BASE + 1]
    rk = ws.enc_round_keys(tc, aes_clear.expand_key(FIPS_C[128][0]))
    state = ws.enc_blocks(tc, pts)
    first = dev((state[:2] + rk[0][None]).reshape(256, p.big1))
    E0 = toy_server.engine
    small, pbs = guarded(256, p.n + 1)[1], guarded(256, p.big1)[1]
    E0.keyswitch_batch(first, small, 256)
    E0.cbs_pbs_batch(small, pbs, 256)
    _, want3 = launch(E0, PF, pbs, 256)
    launches, k1_launches = ac.window_launch_rows(5, 10, 2), st.window_k1_rows(5, 10, 2)
    assert launches == [256] * 25 and sorted(k1_launches) == [128] * 10 + [256] * 20
    per_call = {KS: st.counters_after(k1_launches, rows), K2: st.counters_after(launches, rows), PF: st.counters_after(launches, rows)}
    assert per_call == {KS: (30, 960), K2: (25, 800), PF: (25, 800)}
    with private(toy_server) as srv:
        E = srv.engine
        E.aes_set_window(2)
        d_rk = dev(rk)

        def run():
            d = dev(state)
            srv.aes_encrypt(d_rk, d)
            srv.synchronize()
            return (d,)

        clean = run()
        assert ws.dec_blocks(tc, host(clean[0])) == [aes_clear.aes_encrypt_block(FIPS_C[128][0], v) for v in pts]
        srv.audit(rows=rows, seed=SEED, stages=st.STAGES)
        assert same(run(), clean) and all(counters(E, s) == per_call[s] + (0,) for s in st.STAGES)
        named = _native.audit_rows(SEED, 25, 256, rows)
        row = next(r for r in named if r not in _native.audit_rows(SEED, 0, 256, rows) and r not in _native.audit_rows(SEED, 80, 256, rows))
        word = p.k * (p.k + 1) * p.N                                      # key block k, its first word
        E.audit_stage_debug(PF, row, word, MASK)
        assert not same(run(), clean)
        found(srv, PF, 25, row, word, int(host(want3)[row, word]), 50, 50 * rows)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [KS, PF])
def test_257_rows_on_256_samples_min_rows_and_a_new_stage_set(stage, toy_server):
    import torch

    p = toy_server.params
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, 257, 5)
        _, want = launch(E, stage, x, 257)
        E.audit_stage_set(stage, 256, 0, SEED)
        buf, out = launch(E, stage, x, 257)
        assert torch.equal(out, want) and guards_intact(buf) and counters(E, stage) == (1, 256, 0)
        _, out = launch(E, stage, x, 2)                                   # m < rows: every row
        assert torch.equal(out, want[:2]) and counters(E, stage) == (2, 258, 0)
        E.audit_stage_set(stage, 32, 258, SEED)                           # min_rows above the launch's m: not audited
        launch(E, stage, x, 257)
        assert counters(E, stage) == (0, 0, 0)
        E.audit_stage_set(stage, 32, 257, SEED)                           # at it
        launch(E, stage, x, 257)
        launch(E, stage, x, 256)
        assert counters(E, stage) == (1, 32, 0)
        # the launch number: the next launch is launch 1 and checks launch 1's rows; after a new stage_set it is launch 0 again
        rows0, rows1 = (_native.audit_rows(SEED, j, 257, 32) for j in (0, 1))
        E.audit_stage_debug(stage, next(r for r in rows1 if r not in rows0), 1, MASK)
        launch(E, stage, x, 257)
        assert counters(E, stage) == (2, 64, 1) and records(E, stage)[0][:3] == [1, next(r for r in rows1 if r not in rows0), 1]
        E.audit_stage_set(stage, 32, 0, SEED)
        assert counters(E, stage) == (0, 0, 0) and records(E, stage) == []
        row0 = next(r for r in rows0 if r not in rows1)
        E.audit_stage_debug(stage, row0, 2, MASK)
        launch(E, stage, x, 257)
        assert counters(E, stage) == (1, 32, 1) and records(E, stage)[0][:3] == [0, row0, 2]
        other = PF if stage == KS else KS
        assert counters(E, other) == (0, 0, 0) and counters(E, K2) == (0, 0, 0)


def test_seventeen_wrong_rows_against_sixteen_records(toy_server):
    p, m, rows = toy_server.params, 130, 32
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, m, 17)
        _, want = launch(E, KS, x, m)
        want = host(want)
        E.audit_stage_set(KS, rows, 0, SEED)
        hooks = [(_native.audit_rows(SEED, j, m, rows)[j], j) for j in range(17)]
        for row, word in hooks:
            E.audit_stage_debug(KS, row, word, MASK)
            launch(E, KS, x, m)
        assert counters(E, KS) == (17, 17 * rows, 17)
        assert records(E, KS) == [[j, row, word, int(want[row, word]) ^ MASK, int(want[row, word])] for j, (row, word) in enumerate(hooks[:16])]


def test_two_audited_calls_in_flight_on_a_caller_s_stream_and_a_host_call(toy_server):
    import torch

    p, m, rows = toy_server.params, 130, 32
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, m, 9)
        want = {s: launch(E, s, x, m)[1] for s in (KS, PF)}
        all_on(E, rows)
        bufs = {s: guarded(m, st.row_words(p, s)) for s in (KS, PF)}
        stream = torch.cuda.Stream()
        E.set_stream(stream.cuda_stream)
        try:
            for _ in range(2):
                E.keyswitch_batch(x, bufs[KS][1], m)
                E.pfpks_batch(x, bufs[PF][1], m)
            stream.synchronize()                                          # the stream only: not the device, not the context
            for s in (KS, PF):
                assert counters(E, s) == (2, 2 * rows, 0) and torch.equal(bufs[s][1], want[s]) and guards_intact(bufs[s][0])
        finally:
            E.set_stream(None)
        # host memory: staged in, audited on the device, copied back
        x_h = host(x)
        for s in (KS, PF):
            out = np.zeros((m, st.row_words(p, s)), dtype=np.uint64)
            (E.keyswitch_batch if s == KS else E.pfpks_batch)(x_h, out, m)
            assert np.array_equal(out, host(want[s])) and counters(E, s) == (3, 3 * rows, 0)
            with pytest.raises(ValueError):                               # the hook itself takes device tensors only
                E.audit_plain_batch(s, x_h, out, m)
        assert counters(E, K2) == (0, 0, 0)


def test_bad_arguments_of_the_stage_calls(toy_server):
    p = toy_server.params
    with private(toy_server) as srv:
        E = srv.engine
        lib, h = E._lib, E._h
        for stage in (3, 4, 5, 6, -1):
            assert lib.fheaes_audit_stage_set(h, stage, 1, 0, 1) == -1
            assert lib.fheaes_audit_stage_read(h, stage, None, None, None, None, 0, None) == -1
            assert lib.fheaes_audit_stage_debug(h, stage, 0, 0, 1) == -1
        for stage in (0, 1, 2):
            assert lib.fheaes_audit_stage_set(h, stage, _native.AUDIT_MAX_ROWS + 1, 0, 1) == -1
            assert lib.fheaes_audit_stage_debug(h, stage, 0, 0, 0) == -1
        assert lib.fheaes_audit_stage_debug(h, 0, 0, p.n + 1, 1) == -1 and lib.fheaes_audit_stage_debug(h, 0, 0, p.n, 1) == 0
        assert lib.fheaes_audit_stage_debug(h, 2, 0, st.row_words(p, PF), 1) == -1 and lib.fheaes_audit_stage_debug(h, 2, 0, st.row_words(p, PF) - 1, 1) == 0
        # stage 1 IS the blind rotation's audit: one state behind both spellings
        E.audit_stage_set(K2, 8, 0, SEED)
        small = dev(np.random.default_rng(1).integers(0, 1 << 64, (24, p.n + 1), dtype=np.uint64))
        out = guarded(24, p.big1)[1]
        E.cbs_pbs_batch(small, out, 24)
        E.synchronize()
        assert counters(E, K2) == (1, 8, 0) and E.audit_read()["rows_checked"] == 8
        E.audit_set(0)
        assert counters(E, K2) == (0, 0, 0)
        # the word bound of stage 1 is the blind rotation's: a ciphertext of kN + 1 words
        assert lib.fheaes_audit_stage_debug(h, 1, 0, p.big1, 1) == -1 and lib.fheaes_audit_stage_debug(h, 1, 0, p.big1 - 1, 1) == 0


def k2_batch(E, small):
    """one blind-rotation launch of 24 rows into guard rows; its rows, settled"""
    buf, out = guarded(24, E.params.big1)
    E.cbs_pbs_batch(small, out, 24)
    E.synchronize()
    assert guards_intact(buf)
    return out


@pytest.mark.parametrize("hook,read", [("stage", "first"), ("first", "stage")], ids=["stage_debug-audit_read", "audit_debug-stage_read"])
def test_k2_hook_set_through_one_spelling_is_seen_through_the_other(hook, read, toy_server):
    import torch

    p, m, rows = toy_server.params, 24, 8
    assert _native.Engine._audit_stage(K2) == 1
    small = dev(np.random.default_rng(2).integers(0, 1 << 64, (m, p.n + 1), dtype=np.uint64))
    row, word = _native.audit_rows(SEED, 0, m, rows)[5], p.big1 - 2
    with private(toy_server) as srv:
        E = srv.engine
        want = k2_batch(E, small)
        (E.audit_stage_set(K2, rows, 0, SEED) if hook == "stage" else E.audit_set(rows, 0, SEED))
        (E.audit_stage_debug(K2, row, word, MASK) if hook == "stage" else E.audit_debug(row, word, MASK))
        out = k2_batch(E, small)
        assert torch.nonzero(out != want).tolist() == [[row, word]]
        r = E.audit_read() if read == "first" else E.audit_stage_read(K2)
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 1)
        w = int(host(want)[row, word])
        assert [[int(v) for v in rec] for rec in r["records"]] == [[0, row, word, w ^ MASK, w]]
        out = k2_batch(E, small)                                          # one shot: clean again, the wrong-row counter is sticky
        assert torch.equal(out, want)
        assert counters(E, K2) == (2, 2 * rows, 1) and E.audit_read()["launches"] == 2
        assert counters(E, KS) == (0, 0, 0) and counters(E, PF) == (0, 0, 0)


def test_k2_allocations_are_the_same_under_both_spellings(toy_server):
    with private(toy_server) as srv:
        E = srv.engine
        E.audit_set(0)
        E.alloc_debug(0)
        E.audit_set(8, 0, SEED)
        first = E.alloc_debug(0)
        assert first == 3                                                 # the gathered inputs, the latency form's rows and the state
        E.audit_set(0)
        E.alloc_debug(0)
        E.audit_stage_set(K2, 8, 0, SEED)
        assert E.alloc_debug(0) == first
        E.audit_stage_set(K2, 256, 0, SEED)                               # sized for 256 rows whatever `rows` was
        assert E.alloc_debug(0) == 0
        E.audit_stage_set(K2, 0)                                          # frees all three
        E.alloc_debug(0)
        E.audit_stage_set(K2, 8, 0, SEED)
        assert E.alloc_debug(0) == first


def test_audit_set_0_turns_k2_off_and_leaves_the_key_switches_on(toy_server, env):
    """three entries, not aliases: K2 off through its first spelling, K1 and K3 still count"""
    case = ws.BY_NAME["wopbs_8_bits_shared_luts"]
    h = case.build(env, 0)
    with private(toy_server) as srv:
        E = srv.engine
        all_on(E, 256)
        E.audit_set(0)
        once(srv, case, h)
        assert counters(E, K2) == (0, 0, 0) and E.audit_read()["launches"] == 0
        assert counters(E, KS) == (1, 24, 0) and counters(E, PF) == (1, 24, 0)


# ---- memory --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [KS, PF])
def test_each_allocation_of_stage_set_refused_in_turn(stage, toy_server):
    import torch

    p, m = toy_server.params, 40
    with private(toy_server) as srv:
        E = srv.engine
        x = big_rows(p, m, 3)
        _, want = launch(E, stage, x, m)
        E.alloc_debug(0)
        E.audit_stage_set(stage, 16, 0, SEED)
        assert E.alloc_debug(0) == 2                                      # the gathered rows and the state
        for nth in (1, 2):
            E.audit_stage_set(stage, 0)                                   # frees both
            E.alloc_debug(nth)
            with pytest.raises(_native.FheAesError) as err:
                E.audit_stage_set(stage, 16, 0, SEED)
            assert err.value.code == -4
            assert E.alloc_debug(0) == nth
            _, out = launch(E, stage, x, m)                               # the stage is off: nothing is counted, the call is healthy
            assert torch.equal(out, want) and counters(E, stage) == (0, 0, 0)
            E.audit_stage_set(stage, 16, 0, SEED)
            _, out = launch(E, stage, x, m)
            assert torch.equal(out, want) and counters(E, stage) == (1, 16, 0)
        E.audit_stage_set(stage, 0)
        E.alloc_debug(0)
        E.audit_stage_set(stage, 0)
        assert E.alloc_debug(0) == 0


def test_an_audited_call_allocates_nothing(toy_server, env):
    case = ws.BY_NAME["wopbs_8_bits_shared_luts"]
    h = case.build(env, 0)
    with private(toy_server) as srv:
        E = srv.engine
        w0 = once(srv, case, h)                                           # grows the workspace
        srv.audit(rows=256, seed=SEED, stages=st.STAGES)
        d = resident(h)
        E.alloc_debug(0)
        out = case.run(srv, d)
        srv.synchronize()
        assert E.alloc_debug(0) == 0
        assert same((out,) if not isinstance(out, (tuple, list)) else tuple(out), w0)
        assert all(counters(E, s) == (1, 24, 0) for s in st.STAGES)


# ---- ServerGroup ---------------------------------------------------------------------------------------------------------------------------
def test_server_group_on_three_contexts(toy, toy_server, tc):
    p = toy.params
    rk = tc.encrypt_bytes(list(range(176))).reshape(11, 16, 8, p.big1)           # any ciphertexts do as round keys here
    state = tc.encrypt_bytes(list(range(100, 148))).reshape(3, 16, 8, p.big1)
    want = toy_server.aes_encrypt(rk, state.copy())
    g = ServerGroup(toy.keys, devices=(0, 0, 0))
    try:
        g.audit(rows=32, seed=SEED, stages=(PF, KS, K2))
        assert all(s._audit_stages == st.STAGES for s in g.servers)
        got = g.aes_encrypt(rk, state.copy())
        assert np.array_equal(got, want)
        reports = {s: g.audit_report(s) for s in st.STAGES}               # a group has audit_report(stage) and audit_check()
        assert all(list(srv.audit_reports()) == list(st.STAGES) for srv in g.servers)
        for s in st.STAGES:                                               # one block each: ten 128-row launches per stage and context
            assert [counters(srv.engine, s) for srv in g.servers] == [(10, 320, 0)] * 3
            assert (reports[s].launches, reports[s].rows_checked, reports[s].rows_wrong, reports[s].records) == (30, 960, 0, [])
        assert g.audit_check().launches == 30
        # context 1's next K3 launch (its launch 10) under its own seed, SEED + 1
        row = _native.audit_rows(SEED + 1, 10, 128, 32)[9]
        g.servers[1].engine.audit_stage_debug(PF, row, 5, MASK)
        g.aes_encrypt(rk, state.copy())
        with pytest.raises(AuditMismatch) as err:
            g.audit_check()
        assert err.value.stage == PF
        report = err.value.report
        assert (report.launches, report.rows_checked, report.rows_wrong) == (60, 1920, 1)
        assert [(r.launch, r.row, r.word, r.got ^ r.want, r.device) for r in report.records] == [(10, row, 5, MASK, 0)]
        assert g.audit_report(KS).rows_wrong == 0 and g.audit_report().rows_wrong == 0
        g.audit(rows=0)
        assert all(s._audit_stages == () and s.audit_reports() == {} for s in g.servers)
    finally:
        for s in g.servers:
            s.engine.close()
