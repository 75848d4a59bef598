"""The audit (include/fheaes.h, "audit"; launch_blind_rotate_audit in csrc/engine_launch.h) under every call and at every launch site.  It can fail in
two ways: a false alarm (rows_wrong > 0, or other words, on a correct engine in a call or launch shape nobody ran with it on) and a silent
miss (a launch that is not audited, or a gather and compare that read other rows than the sample names).  test_gpu_audit.py holds the
mechanism to its contract through fheaes_cbs_pbs_batch; this file holds the engine to "every blind-rotation launch":

  1. every case of workspace_state.CASES, audit off / 1 row / 256 rows: the same words, the same profile (the audit is not a launch), and
     counters that are exact -- (L, L, 0) with one row, sum(min(256, m_i)) where audit_calls.launch_list has the launch sizes, bracketed
     by L and min(256 L, U) elsewhere, (0, 0, 0) where no blind rotation runs.  gate_packed, the keyed and the packed-key ciphers are
     among the 50
  2. one tamper (fheaes_audit_debug: an XOR into a valid word of a valid row) at each of the four callers of launch_cbs_pbs, in a row the
     sample names: counted once, recorded with the word the stage calls (keyswitch_batch, cbs_pbs_batch on another context) give for
     that row, visible in the call's output -- the hook sat upstream of K3 --, and gone in the next call
  3. the chunk seams of wopbs_dev and gate_call and the first row count past the latency form, clean
  4. PARAM_OPT: the parked 16-form, the 16-form above 768 bits, a paired launch with both unit sizes, each with one tamper; one whole
     call in the automatic window
  5. host memory, two audited calls in flight, more wrong rows than records, and fheaes_audit_set between calls

Every test has a context of its own, cloned device to device from the module's server.  Every expected value is exact: the engine is
deterministic and all forms write the same words, so there are no tolerances.

Wall time on an MI355X (pytest --durations=0) and the three wrong-result builds these tests were shown to fail on: DESIGN.md section 5,
"The audit under test"."""
import ctypes
import time
from contextlib import contextmanager

import numpy as np
import pytest

import audit_calls as ac
import chunk_seams as cs
import workspace_state as ws
from aes_vectors import BASE, F5, FIPS_C, MASK128
from gpu_support import (HOME, PAIR, PARKED, dev, guarded, guards_intact, host, oc, opt_rk128, opt_server, plan_tuple, settled, tc,  # noqa: F401
                         toy_server, unit_rows)
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import AuditMismatch, Server, gen_lut

pytestmark = pytest.mark.gpu

SEED, MASK = ac.SEED, ac.MASK
OFF = _native.AES_WINDOW_OFF


@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


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


def as_tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def resident(inputs):
    d = dict(inputs)
    for name in inputs["dev"]:
        d[name] = dev(inputs[name])
    return d


def once(srv, case, inputs):
    """the case on fresh resident copies of `inputs`, settled"""
    d = resident(inputs)
    outs = as_tuple(case.run(srv, d))
    srv.synchronize()
    return outs


def same(a, b):
    import torch

    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a, b))


def counters(E):
    r = E.audit_read()
    return r["launches"], r["rows_checked"], r["rows_wrong"]


def records(E):
    return [[int(x) for x in rec] for rec in E.audit_read()["records"]]


def k2_profile(E):
    p = E.profile_read()["blind_rotate"]
    return p["launches"], p["units"]


def stage_k2(E, rows_in):
    """what K2 must write for the LWE ciphertexts rows_in [m][kN+1]: the two stage calls on context E (never the audited one)"""
    import torch

    m = int(rows_in.shape[0])
    small = torch.empty((m, E.params.n + 1), dtype=torch.int64, device="cuda")
    out = torch.empty((m, E.params.big1), dtype=torch.int64, device="cuda")
    E.keyswitch_batch(rows_in, small, m)
    E.cbs_pbs_batch(small, out, m)
    E.synchronize()
    return host(out)


def detect(srv, run, m0, rows, word, want_rows, n_launches, checked, min_bits=0):
    """steps 2 .. 7 of a detection test.  run() makes the call on fresh inputs and returns its settled outputs; m0: the rows of the first
    audited launch; want_rows: the stage calls' words for that launch (None: only got ^ want is held); n_launches, checked: what one call
    counts.  Returns the record"""
    E = srv.engine
    clean = run()
    assert counters(E) == (0, 0, 0)
    E.audit_set(rows, min_bits, SEED)
    named = _native.audit_rows(SEED, 0, m0, rows)
    row = named[len(named) // 2]
    E.audit_debug(row, word, MASK)
    out = run()
    assert counters(E) == (n_launches, checked, 1)
    recs = records(E)
    assert len(recs) == 1 and recs[0][:3] == [0, row, word], recs
    assert recs[0][3] ^ recs[0][4] == MASK
    if want_rows is not None:
        assert recs[0][4] == int(want_rows[row, word]), "the audit's word is not the stage calls'"
    assert not same(out, clean), "the tampered word did not reach the call's output"
    again = run()                                                         # one shot: clean again, the wrong-row counter is sticky
    assert same(again, clean) and counters(E) == (2 * n_launches, 2 * checked, 1) and len(records(E)) == 1
    return recs[0]


# ---- 1. every call of the table, clean -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.name)
def test_every_call_of_the_table_is_clean_under_the_audit(case, toy_server, env):
    h = case.build(env, 0)
    with private(toy_server) as srv:
        E = srv.engine
        E.profile_reset()
        w0 = once(srv, case, h)
        L, U = k2_profile(E)
        case.check_clear(env, h, [host(t) for t in w0])
        assert counters(E) == (0, 0, 0)
        assert (L > 0) == ac.launches_k2(case)
        plan = ac.launch_list(case.name, h)
        if plan is not None:
            assert (L, U) == (len(plan), sum(plan)), "the launch list of audit_calls.py is not this call's"
        for rows in (1, 256):
            E.audit_set(rows, 0, SEED)
            E.profile_reset()
            w = once(srv, case, h)
            assert same(w, w0), "%d rows: the audited call writes other words" % rows
            assert k2_profile(E) == (L, U), "the audit counts as a launch"
            r = E.audit_read()
            got = (r["launches"], r["rows_checked"], r["rows_wrong"])
            assert len(r["records"]) == 0 and got[2] == 0, "false alarm: %r %r" % (got, r["records"])
            if L == 0:
                assert got == (0, 0, 0), "an audit without a blind rotation counted %r" % (got,)
            elif rows == 1:
                assert got == (L, L, 0)
            else:
                assert got[0] == L and L <= got[1] <= min(256 * L, U)
                if plan is not None:
                    assert got[1] == ac.rows_checked(plan, 256)            # == U where no launch has more than 256 rows


# ---- 2. detection at each launch site ---------------------------------------------------------------------------------------------------
def test_wopbs_dev_tamper_is_found_with_the_stage_calls_word(toy_server, tc):
    p = toy_server.params
    values = [0x53, 0x00, 0xE1]
    ct = tc.encrypt_bytes(values)
    want = stage_k2(toy_server.engine, dev(ct.reshape(24, p.big1)))
    with private(toy_server) as srv:
        def run():
            d = dev(ct)
            srv.sbox(d, False)
            srv.synchronize()
            return (d,)

        assert [int(b) for b in tc.decrypt_bytes(host(run()[0]))] == [aes_clear.SBOX[v] for v in values]
        detect(srv, run, 24, 8, p.big, want, 1, 8)


PTS5 = [BASE, 0, MASK128, 0x3243F6A8885A308D313198A2E0370734, BASE + 1]
KOB5 = [0, 1, 1, 0, 1]


@pytest.fixture(scope="module")
def five_blocks(toy_server, tc):
    """5 blocks under FIPS-197 C.1's key, their encryption round by round with the audit off (held to AES), and the same under two keys"""
    key = FIPS_C[128][0]
    rk = ws.enc_round_keys(tc, aes_clear.expand_key(key))
    sets = ws.key_sets(tc, ws.KEYS)
    st = ws.enc_blocks(tc, PTS5)
    with private(toy_server) as srv:
        srv.engine.aes_set_window(OFF)
        d, dk, dp, d_rk, d_sets = dev(st), dev(st), dev(st), dev(rk), dev(sets)
        srv.aes_encrypt(d_rk, d)
        srv.aes_encrypt_keyed(d_sets, KOB5, dk)
        store = srv.pack_round_keys(d_sets)                                # packing is a key switch: other words than the LWE form's
        srv.aes_encrypt_keyed(store, KOB5, dp)
        srv.synchronize()
        assert counters(srv.engine) == (0, 0, 0)
    assert ws.dec_blocks(tc, host(d)) == [aes_clear.aes_encrypt_block(key, v) for v in PTS5]
    for words in (dk, dp):
        assert ws.dec_blocks(tc, host(words)) == [aes_clear.aes_encrypt_block(ws.KEYS[k], v) for k, v in zip(KOB5, PTS5)]
    return {"rk": rk, "sets": sets, "st": st, "enc": d, "enc_keyed": dk, "enc_packed": dp}


def test_aes_run_dev_tamper_in_the_first_window(toy_server, five_blocks):
    """window 2 over 5 blocks: the first launch is blocks 0 and 1 of step 0, whose K1 input is the state plus round key 0 (add_bcast_kernel:
    a wrapping add of the words); 25 launches of 256 rows, every third of two segments"""
    p, f = toy_server.params, five_blocks
    first = (f["st"][:2] + f["rk"][0][None]).reshape(256, p.big1)
    want = stage_k2(toy_server.engine, dev(first))
    with private(toy_server) as srv:
        srv.engine.aes_set_window(2)
        d_rk = dev(f["rk"])

        def run():
            d = dev(f["st"])
            srv.aes_encrypt(d_rk, d)
            srv.synchronize()
            return (d,)

        assert same(run(), (f["enc"],))                                   # the windowed schedule writes the words of the one without
        assert len(ac.window_launch_rows(5, 10, 2)) == 25
        detect(srv, run, 256, 32, p.big, want, 25, 32 * 25)


@pytest.mark.parametrize("w", [2, 3])
def test_aes_run_dev_windows_are_audited_launch_by_launch(toy_server, five_blocks, w):
    """clean, two-segment windows among them: the plain, the keyed and the packed-key form, each launch counted with its 32 rows"""
    f = five_blocks
    launches = ac.window_launch_rows(5, 10, w)
    assert len(launches) == -(-10 * 5 // w) and min(launches) >= 32
    with private(toy_server) as srv:
        E = srv.engine
        E.aes_set_window(w)
        d_rk, d_sets = dev(f["rk"]), dev(f["sets"])
        store = srv.pack_round_keys(d_sets)
        srv.synchronize()
        for form, keys, extra, want in (("plain", d_rk, (), f["enc"]), ("keyed", d_sets, (KOB5,), f["enc_keyed"]), ("packed", store, (KOB5,), f["enc_packed"])):
            E.audit_set(32, 0, SEED)
            E.profile_reset()
            d = dev(f["st"])
            (srv.aes_encrypt_keyed if extra else srv.aes_encrypt)(keys, *extra, d)
            srv.synchronize()
            assert same((d,), (want,)), form
            assert k2_profile(E) == (len(launches), sum(launches)), form
            assert counters(E) == (len(launches), 32 * len(launches), 0) and records(E) == [], form


def test_gate_call_tamper_in_the_gates_bootstrap(toy_server, tc):
    p = toy_server.params
    valid, ct, runs = tc.encrypt_bits(np.array([1, 0], dtype=np.uint8)), tc.encrypt_bits(np.array([1, 1, 1], dtype=np.uint8)), [2, 1]
    want = stage_k2(toy_server.engine, dev(valid))
    with private(toy_server) as srv:
        def run():
            d_ct, d_valid = dev(ct), dev(valid)
            out = srv.gate(d_ct, d_valid, runs)
            srv.synchronize()
            return (out,)

        assert [int(b) for b in tc.decrypt_bits(host(run()[0]))] == [1, 1, 0]
        assert _native.audit_rows(SEED, 0, 2, 64) == [0, 1]                # S = 2: every row is sampled
        detect(srv, run, 2, 64, p.big, want, 1, 2)


def test_a_later_launch_of_a_call_is_the_first_audited_one(toy, toy_server, env):
    """aes_encrypt_public on the table's 3 blocks: pools of 33, 36 and then 48 bytes.  With min_bits at the largest pool the call's first
    two launches are not audited and the hook waits for the third, which is audited launch 0.  Its input is the pool of round 3, rebuilt
    with aes_model: the call writes the words of aes_encrypt on the trivial state (test_gpu_ctr_public.py), so the pool's 48 distinct
    entries, numbered in (block, position) order of first occurrence (include/fheaes.h, aes_model.rule), are the model's state after two
    rounds on the CPU oracle's WoPBS"""
    from aes_model import ENC_MULS, MC, AesModel, _luts
    from tfhe_aes_amd.client import u128_to_bytes

    case, p = ws.BY_NAME["aes_encrypt_public"], toy.params
    h = case.build(env, 0)
    plan = _native.aes_public_plan(h["blocks"])
    min_bits, rounds = ac.largest_pool_launches(plan)
    assert rounds == list(range(2, 10)) and min_bits == 8 * max(plan) == 8 * 16 * len(h["blocks"])       # from round 3 on nothing is shared
    enc_round = _luts([lambda x, m=m: aes_clear.gf_mul(aes_clear.SBOX[x], m) for m in ENC_MULS])
    st = env.client.trivial_bytes([u128_to_bytes(b) for b in h["blocks"]]) + h["rk"][0]
    for rnd in (1, 2):
        y = toy.oracle.wopbs_batch(np.ascontiguousarray(st).reshape(48, 8, p.big1), enc_round).reshape(3, 16, 3, 8, p.big1)
        st = AesModel._mix(y, MC, ENC_MULS, +1) + h["rk"][rnd]
    want = stage_k2(toy_server.engine, dev(st.reshape(min_bits, p.big1)))
    with private(toy_server) as srv:
        clean = once(srv, case, h)
        case.check_clear(env, h, [host(t) for t in clean])
        rec = detect(srv, lambda: once(srv, case, h), min_bits, 32, p.big, want, len(rounds), 32 * len(rounds), min_bits=min_bits)
        assert rec[0] == 0


# ---- 3. seams and odd launch sizes, clean ----------------------------------------------------------------------------------------------
BITS7 = np.array([1, 0, 0, 1, 1, 0, 1], dtype=np.uint8)
BITS5 = np.array([1, 1, 0, 1, 0], dtype=np.uint8)


def test_wopbs_batch_across_the_chunk_seam(toy_server, tc):
    """33,281 one-bit inputs under NOT: launches of 32,768 and of 513 rows"""
    import torch

    p, n = toy_server.params, cs.M_BITS
    assert ac.wopbs_launch_rows(n, 1) == [32768, 513]
    lut = gen_lut(2, 1, 512, 1, lambda v: 1 - v)
    with private(toy_server) as srv:
        E = srv.engine
        d_x = settled(dev(tc.encrypt_bits(BITS7))[torch.arange(n, device="cuda") % 7].contiguous()).reshape(n, 1, p.big1)
        d_lut = dev(lut[None])
        outs = []
        for rows, want in ((0, (0, 0, 0)), (256, (2, 512, 0)), (1, (2, 2, 0))):
            E.audit_set(rows, 0, SEED)
            buf, out = guarded(n, p.big1)
            E.profile_reset()
            E.wopbs_batch(d_x, n, 1, d_lut, 1, False, out)
            E.synchronize()
            assert k2_profile(E) == (2, n) and guards_intact(buf)
            assert counters(E) == want and records(E) == []
            outs.append(out)
        assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])
        for sl in (slice(0, 14), slice(32761, 32775), slice(n - 14, n)):       # both ends and both sides of the seam
            assert tc.decrypt_bits(host(settled(outs[0][sl]))).tolist() == (1 - BITS7[np.arange(n)[sl] % 7]).tolist()
        del outs, buf, out
    torch.cuda.empty_cache()


def test_gates_across_the_chunk_seam_and_a_launch_of_one_row(toy_server, tc):
    """32,769 bootstrapped gates: launches of 32,768 rows and of ONE row.  The hook on row 0 belongs to the first launch, although row 0 is
    the only row the second has"""
    import torch

    p, n, runs = toy_server.params, cs.GATE_BOOT_GATES, cs.gate_boot_runs(head=9)
    m = sum(runs)
    assert ac.gate_launch_rows(n) == [32768, 1]
    gates7 = tc.encrypt_bits(BITS7)
    want0 = stage_k2(toy_server.engine, dev(gates7[:1]))                   # gate 0 alone: every form writes the same words for a row
    with private(toy_server) as srv:
        E = srv.engine
        d_gates = settled(dev(gates7)[torch.arange(n, device="cuda") % 7].contiguous())
        d_ct = settled(dev(tc.encrypt_bits(BITS5))[torch.arange(m, device="cuda") % 5].contiguous())

        def run():
            buf, out = guarded(m, p.big1)
            E.profile_reset()
            E.gate_bits(d_gates, runs, d_ct, m, out)
            E.synchronize()
            assert k2_profile(E) == (2, n) and guards_intact(buf)
            return out

        clean = run()
        of_gate = np.repeat(np.arange(n), runs)
        expect = BITS7[of_gate % 7] * BITS5[np.arange(m) % 5]
        assert tc.decrypt_bits(host(settled(clean[m - 40:]))).tolist() == expect[m - 40:].tolist()
        E.audit_set(64, 0, SEED)
        assert torch.equal(run(), clean) and counters(E) == (2, 65, 0) and records(E) == []
        # a seed under which launch 0 samples its row 0 (the first of 64 strata of 512 rows), found on the host
        seed = next(s for s in range(SEED, SEED + (1 << 16)) if _native.audit_rows(s, 0, 32768, 64)[0] == 0)
        E.audit_set(64, 0, seed)
        E.audit_debug(0, p.big, MASK)
        out = run()
        assert counters(E) == (2, 65, 1)
        w = int(want0[0, p.big])
        assert records(E) == [[0, 0, p.big, w ^ MASK, w]]
        assert not torch.equal(out[:9], clean[:9]) and torch.equal(out[9:], clean[9:])      # gate 0 gates the first 9 rows
        del clean, out
    torch.cuda.empty_cache()


def test_cbs_pbs_batch_of_257_rows_with_256_samples(toy_server):
    """the first row count past the latency form, S = 256: 255 strata of one row and one of two"""
    import torch

    m, rows = 257, 256
    with private(toy_server) as srv:
        E = srv.engine
        assert E.k2_plan(m)["form"] == 1 and E.k2_plan(256)["form"] == 0
        small = dev(np.random.default_rng(0xA0D257).integers(0, 1 << 64, (m, E.params.n + 1), dtype=np.uint64))
        buf, want = guarded(m, E.params.big1)
        E.cbs_pbs_batch(small, want, m)
        E.synchronize()
        E.audit_set(rows, 0, SEED)
        buf2, out = guarded(m, E.params.big1)
        E.cbs_pbs_batch(small, out, m)
        E.synchronize()
        assert counters(E) == (1, 256, 0) and records(E) == []
        assert torch.equal(out, want) and guards_intact(buf) and guards_intact(buf2)
        named = _native.audit_rows(SEED, 0, m, rows)
        assert len(named) == 256 and all(a < b for a, b in zip(named, named[1:])) and 0 <= named[0] and named[-1] < m


# ---- 4. forms the audit has not met (PARAM_OPT) -------------------------------------------------------------------------------------------
# (rows, (allow_pair, allow_home), plan at 256 CUs, kernel prefix, the tampered word, which rows may carry the tamper)
OPT_FORMS = [
    (600, (True, False), (1, 200, 3, 0, 2), PARKED, "body", lambda r: True),                 # the 16-form without its LDS home
    (800, (False, True), (1, 267, 3, 0, 2), HOME, "body", lambda r: True),                    # the 16-form above 768 bits: the paired form denied
    (2100, (True, True), (2, 26, 6, 486, 4), PAIR, 0, lambda r: r < 26 * 6 and r % 6 == 4),   # inside a six-ciphertext unit, its fifth row
]


@pytest.mark.parametrize("m,forms,plan,kernel,word,eligible", OPT_FORMS, ids=["parked-600", "denied-pair-800", "paired-2100"])
def test_param_opt_forms_under_the_audit(opt_server, m, forms, plan, kernel, word, eligible):
    import torch

    rows = 64
    with private(opt_server) as srv:
        E = srv.engine
        E.k2_set_forms(*forms)
        pl = E.k2_plan(m)
        assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl
        word = E.params.big if word == "body" else word
        small = dev(np.random.default_rng(0xA0D17 + m).integers(0, 1 << 64, (m, E.params.n + 1), dtype=np.uint64))

        def launch():
            buf, out = guarded(m, E.params.big1)
            E.cbs_pbs_batch(small, out, m)
            E.synchronize()
            return buf, out

        _, want = launch()
        # a seed under which the third launch samples an eligible row, found on the host
        seed, row = next((s, r) for s in range(SEED, SEED + 4096) for r in _native.audit_rows(s, 2, m, rows) if eligible(r))
        if plan[0] == 2:
            assert unit_rows(plan, row // 6, m)[4] == row and row // 6 < plan[1]
        E.audit_set(rows, 0, seed)
        for n in (1, 2):
            buf, out = launch()
            assert guards_intact(buf) and torch.equal(out, want)
            assert counters(E) == (n, n * rows, 0) and records(E) == []
        E.audit_debug(row, word, MASK)
        buf, out = launch()
        assert counters(E) == (3, 3 * rows, 1)
        w = int(host(want)[row, word])
        assert records(E) == [[2, row, word, w ^ MASK, w]]
        assert torch.nonzero(out != want).tolist() == [[row, word]] and guards_intact(buf)


def test_param_opt_whole_call_in_the_automatic_window(opt_server, opt_rk128, oc):
    """aes_encrypt on 13 blocks: window 12 at 256 CUs, every launch across a step boundary"""
    import torch

    n, t, key = 13, 10, F5[128][0]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = _native.aes_window_plan(n, t, cus, 4)
    pts = [(BASE + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
    st = np.stack([oc.encrypt_u128(v) for v in pts])
    with private(opt_server) as srv:
        E = srv.engine
        assert E.aes_window(n, t) == plan["window"] and (cus != 256 or plan["window"] == 12)
        outs = []
        for rows in (0, 64):
            E.audit_set(rows, 0, SEED)
            E.profile_reset()
            d = dev(st)
            srv.aes_encrypt(opt_rk128, d)
            srv.synchronize()
            assert k2_profile(E) == (plan["launches"], t * n * 128)
            assert counters(E) == ((plan["launches"], 64 * plan["launches"], 0) if rows else (0, 0, 0)) and records(E) == []
            outs.append(d)
        assert torch.equal(outs[1], outs[0])
        assert [oc.decrypt_u128(b) for b in host(outs[0])] == [aes_clear.aes_encrypt_block(key, v) for v in pts]


# ---- 5. state and transport ------------------------------------------------------------------------------------------------------------------
def test_host_memory_calls_are_audited_and_a_tamper_shows_in_the_host_output(toy_server, tc):
    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        p = E.params
        small = np.random.default_rng(0xA0D05).integers(0, 1 << 64, (m, p.n + 1), dtype=np.uint64)
        want = np.zeros((m, p.big1), dtype=np.uint64)
        E.cbs_pbs_batch(small, want, m)
        d_small, d_out = dev(small), dev(np.zeros((m, p.big1), dtype=np.uint64))
        E.cbs_pbs_batch(d_small, d_out, m)
        E.synchronize()
        assert np.array_equal(want, host(d_out))                            # host memory and resident: the same words
        E.audit_set(rows, 0, SEED)
        got = np.zeros_like(want)
        E.cbs_pbs_batch(small, got, m)
        assert np.array_equal(got, want) and counters(E) == (1, rows, 0)
        row, word = _native.audit_rows(SEED, 1, m, rows)[20], 7
        E.audit_debug(row, word, MASK)
        E.cbs_pbs_batch(small, got, m)
        assert np.argwhere(got != want).tolist() == [[row, word]] and int(got[row, word]) == int(want[row, word]) ^ MASK
        assert counters(E) == (2, 2 * rows, 1)
        assert records(E) == [[1, row, word, int(want[row, word]) ^ MASK, int(want[row, word])]]
        # a whole call on numpy arrays
        values = [0x53, 0xA7, 0x00]
        ct = tc.encrypt_bytes(values)
        E.audit_set(0)
        off = srv.sbox(ct.copy(), False)
        E.audit_set(rows, 0, SEED)
        on = srv.sbox(ct.copy(), False)
        assert isinstance(on, np.ndarray) and np.array_equal(on, off) and counters(E) == (1, 24, 0) and records(E) == []
        assert [int(b) for b in tc.decrypt_bytes(on)] == [aes_clear.SBOX[v] for v in values]


def test_two_audited_calls_in_flight(toy_server, env):
    """the two variants of aes_encrypt_keyed back to back on a caller's stream that a chain of matmuls keeps busy; only that stream is
    synchronised.  The audit's buffers are one set per context: the second call's gathers must queue behind the first call's compares"""
    import torch

    case, rows = ws.BY_NAME["aes_encrypt_keyed"], 32
    h = [case.build(env, v) for v in (0, 1)]
    with private(toy_server) as srv:
        E = srv.engine
        single, count, enqueue_ms = [], [], 0.0
        for v in (0, 1):
            E.audit_set(rows, 0, SEED)
            d = resident(h[v])
            clock = time.perf_counter()
            out = as_tuple(case.run(srv, d))
            enqueue_ms = max(enqueue_ms, 1e3 * (time.perf_counter() - clock))
            srv.synchronize()
            case.check_clear(env, h[v], [host(t) for t in out])
            single.append(out)
            count.append(counters(E))
        assert count[0] == count[1] == (10, 10 * rows, 0) and not same(single[0], single[1])
        s, a = torch.cuda.Stream(), ws.producer_matrix()
        steps = max(8, int((4 * enqueue_ms + 8) / ws.PRODUCER_MS_PER_STEP) + 1)
        E.set_stream(s.cuda_stream)
        for first in (0, 1):
            E.audit_set(rows, 0, SEED)
            d1, d2 = resident(h[first]), resident(h[1 - first])
            t0, t1, keep = ws.producer(s, a, steps)
            o1 = as_tuple(case.run(srv, d1))
            in_flight = not t1.query()
            o2 = as_tuple(case.run(srv, d2))
            s.synchronize()                                               # the caller's stream only
            assert in_flight, "the first call returned after %d matmuls (%.1f ms) were done" % (steps, t0.elapsed_time(t1))
            assert same(o1, single[first]) and same(o2, single[1 - first])
            assert counters(E) == (20, 20 * rows, 0) and records(E) == []
            srv.synchronize()
        E.set_stream(None)


def test_more_wrong_rows_than_records(toy_server):
    """17 launches of 100 rows, every row sampled, each with one tamper: 17 counted, the first 16 recorded in launch order"""
    m, rows = 100, 256
    hooks = ac.cap_hooks()
    with private(toy_server) as srv:
        E = srv.engine
        small = dev(np.random.default_rng(0xA0DCA9).integers(0, 1 << 64, (m, E.params.n + 1), dtype=np.uint64))
        buf, out = guarded(m, E.params.big1)
        E.cbs_pbs_batch(small, out, m)
        E.synchronize()
        want = host(out).copy()
        srv.audit(rows=rows, seed=SEED)
        for row, word in hooks:
            E.audit_debug(row, word, MASK)
            E.cbs_pbs_batch(small, out, m)
        E.synchronize()
        assert guards_intact(buf)
        assert counters(E) == (17, 17 * m, 17)
        assert records(E) == [[j, row, word, int(want[row, word]) ^ MASK, int(want[row, word])] for j, (row, word) in enumerate(hooks[:16])]
        lib, h = E._lib, E._h
        n = ctypes.c_uint64()
        rec = (ctypes.c_uint64 * (5 * 16))()
        assert lib.fheaes_audit_read(h, None, None, None, rec, 15, ctypes.byref(n)) == -1          # FHEAES_ERR_INVALID: 16 records do not fit
        wrong = ctypes.c_uint64()
        assert lib.fheaes_audit_read(h, None, None, ctypes.byref(wrong), rec, 16, ctypes.byref(n)) == 0 and (n.value, wrong.value) == (16, 17)
        assert [rec[5 * 15 + i] for i in range(3)] == [15, 75, 15]
        with pytest.raises(AuditMismatch) as err:
            srv.audit_check()
        assert err.value.report.rows_wrong == 17 and len(err.value.records) == 16 and err.value.report.launches == 17
        assert [(r.launch, r.row, r.word) for r in err.value.records] == [(j, 5 * j, j) for j in range(16)]


def test_audit_set_between_calls_keeps_the_words_and_restarts_the_counters(toy_server, tc):
    values = [0x53, 0xE1, 0x00]
    ct = tc.encrypt_bytes(values)
    with private(toy_server) as srv:
        E = srv.engine

        def run():
            d = dev(ct)
            srv.sbox(d, False)
            srv.synchronize()
            return (d,)

        w0 = run()
        assert [int(b) for b in tc.decrypt_bytes(host(w0[0]))] == [aes_clear.SBOX[v] for v in values]
        for rows in (32, 256, 0, 32):
            E.audit_set(rows, 0, SEED)
            assert counters(E) == (0, 0, 0)                                 # restarted, whatever the setting before counted
            for n in (1, 2):
                assert same(run(), w0)
                assert counters(E) == ((n, 24 * n, 0) if rows else (0, 0, 0)) and records(E) == []
