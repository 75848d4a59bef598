"""The audit of the blind rotation (include/fheaes.h, "audit"; kern_audit.h): sampled rows of a K2 launch re-run through the latency form
and compared on the device.

Every test has a context of its own, cloned device to device from the module's server, so no counter, seed or hook of one test is
another's.  Inputs are arbitrary 64-bit words (K2 is defined on any words).  The smallest shapes that reach each path: the latency form
audited by itself (100 rows, 1 row), the toy set's 16-form of 67 units of 8 (530 rows), and at PARAM_OPT the 16-form (600 rows) and the
paired form in 200 units of 4 (800 rows).  An audited launch must write the words of the same launch with the audit off, inside its guard
rows, and count (launches, min(rows, m), 0).

The tamper hook (fheaes_audit_debug) XORs one mask into one word between the product kernel and the audit: in a row fheaes_audit_rows names
it must be counted and recorded, in any other row it must change the output and nothing else -- which shows that the hook wrote and that
only sampled rows are reported."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest

from gpu_support import HOME, PAIR, dev, guarded, guards_intact, host, opt_server, plan_tuple, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native
from tfhe_aes_amd.server import AuditMismatch, AuditRecord, Server, ServerGroup

pytestmark = pytest.mark.gpu

SEED = 0x5EED0A0D17
MASK = 1 << 40


@contextmanager
def private(server):
    """a Server on a context of its own with `server`'s keys"""
    srv = Server(None, device=0, clone_from=server)
    try:
        yield srv
    finally:
        srv.engine.close()


def small_rows(params, m, tag):
    return dev(np.random.default_rng(0xA0D17 + tag).integers(0, 1 << 64, (m, params.n + 1), dtype=np.uint64))


def launch(E, small, m):
    """one blind-rotation launch of m rows into guard rows; (buffer, its m rows), settled"""
    buf, out = guarded(m, E.params.big1)
    E.cbs_pbs_batch(small[:m], out, m)
    E.synchronize()
    return buf, out


def counters(E):
    r = E.audit_read()
    return r["launches"], r["rows_checked"], r["rows_wrong"]


# (server fixture, m, rows, plan at 256 CUs, kernel prefix)
FORMS = [
    ("toy_server", 100, 256, (0, 100, 1, 0, 0), "blind_rotate_latency_kernel<2,5,8>"),        # S = m: every row is checked, by the form that wrote it
    ("toy_server", 1, 64, (0, 1, 1, 0, 0), "blind_rotate_latency_kernel<2,5,8>"),
    ("toy_server", 530, 32, (1, 67, 8, 0, 0), "blind_rotate16_kernel<2,5,8,8"),               # 67 units of 8, the last with 2 rows
    ("opt_server", 600, 64, (1, 200, 3, 0, 2), HOME),
    ("opt_server", 800, 64, (2, 0, 6, 200, 4), PAIR),                                         # 200 units of 4
]


@pytest.mark.parametrize("fixture,m,rows,plan,kernel", FORMS, ids=["%s-%d" % (c[0][:3], c[1]) for c in FORMS])
def test_audited_launch_writes_the_same_words_and_counts_its_rows(fixture, m, rows, plan, kernel, request):
    import torch

    with private(request.getfixturevalue(fixture)) as srv:
        E = srv.engine
        pl = E.k2_plan(m)
        assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl
        small = small_rows(E.params, m, m)
        _, want = launch(E, small, m)
        assert counters(E) == (0, 0, 0)                                   # off: nothing is counted
        E.audit_set(rows, 0, SEED)
        S = min(rows, m)
        for n in (1, 2):
            buf, out = launch(E, small, m)
            assert guards_intact(buf) and torch.equal(out, want)
            r = E.audit_read()
            assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (n, n * S, 0) and len(r["records"]) == 0
        if S == m:
            assert _native.audit_rows(SEED, 0, m, rows) == list(range(m))


def test_tamper_in_a_sampled_row_is_counted_and_recorded(toy_server):
    import torch

    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 1)
        _, want = launch(E, small, m)
        E.audit_set(rows, 0, SEED)
        named = _native.audit_rows(SEED, 0, m, rows)
        row, word = named[5], 17
        E.audit_debug(row, word, MASK)
        buf, out = launch(E, small, m)
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 1)
        assert r["records"].shape == (1, 5)
        rec = AuditRecord(*(int(x) for x in r["records"][0]))
        assert (rec.launch, rec.row, rec.word) == (0, row, word) and rec.got ^ rec.want == MASK
        assert rec.want == int(host(want)[row, word])
        diff = torch.nonzero(out != want).tolist()
        assert diff == [[row, word]] and guards_intact(buf)
        # one shot: the next launch is clean, and the wrong-row counter is sticky
        _, out = launch(E, small, m)
        assert torch.equal(out, want) and counters(E) == (2, 2 * rows, 1)


def test_tamper_outside_the_sample_changes_the_output_and_is_not_reported(toy_server):
    import torch

    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 2)
        _, want = launch(E, small, m)
        E.audit_set(rows, 0, SEED)
        named = set(_native.audit_rows(SEED, 0, m, rows))
        row = next(r for r in range(m - 1, -1, -1) if r not in named)     # near the end: the ragged last unit's neighbourhood
        E.audit_debug(row, E.params.big, MASK)                            # the body, the row's last word
        _, out = launch(E, small, m)
        assert torch.nonzero(out != want).tolist() == [[row, E.params.big]]
        assert int(host(out)[row, -1]) ^ int(host(want)[row, -1]) == MASK
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 0) and len(r["records"]) == 0
        # a row beyond the launch drops the hook without a write, and it does not wait for a larger launch
        E.audit_debug(m, 0, MASK)
        buf, out = launch(E, small, m)
        assert torch.equal(out, want) and guards_intact(buf)
        _, out = launch(E, small, m)
        assert torch.equal(out, want) and counters(E) == (3, 3 * rows, 0)


def test_launch_1_checks_its_own_rows(toy_server):
    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 3)
        E.audit_set(rows, 0, SEED)
        rows0, rows1 = _native.audit_rows(SEED, 0, m, rows), _native.audit_rows(SEED, 1, m, rows)
        row = next(r for r in rows1 if r not in rows0)
        launch(E, small, m)
        assert counters(E) == (1, rows, 0)
        E.audit_debug(row, 0, MASK)
        launch(E, small, m)
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (2, 2 * rows, 1)
        assert [int(x) for x in r["records"][0][:3]] == [1, row, 0]
        # a new audit_set zeroes the counters and the launch number: the next launch is launch 0 again and checks launch 0's rows
        E.audit_set(rows, 0, SEED)
        assert counters(E) == (0, 0, 0)
        row0 = next(r for r in rows0 if r not in rows1 and r not in _native.audit_rows(SEED, 2, m, rows))
        E.audit_debug(row0, 1, MASK)
        launch(E, small, m)
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 1)
        assert [int(x) for x in r["records"][0][:3]] == [0, row0, 1]


def test_tamper_inside_a_four_ciphertext_unit_of_the_paired_form(opt_server):
    import torch

    m, rows = 800, 64
    with private(opt_server) as srv:
        E = srv.engine
        assert plan_tuple(E.k2_plan(m)) == (2, 0, 6, 200, 4)
        small = small_rows(E.params, m, 4)
        _, want = launch(E, small, m)
        E.audit_set(rows, 0, SEED)
        row = next(r for r in _native.audit_rows(SEED, 0, m, rows) if r % 4 == 2)      # the third ciphertext of its unit
        word = E.params.big                                               # word 2,048 of 2,049: the odd last word of an 8-byte-aligned row
        E.audit_debug(row, word, MASK)
        buf, out = launch(E, small, m)
        r = E.audit_read()
        assert (r["launches"], r["rows_checked"], r["rows_wrong"]) == (1, rows, 1)
        rec = [int(x) for x in r["records"][0]]
        assert rec[:3] == [0, row, word] and rec[3] ^ rec[4] == MASK and rec[4] == int(host(want)[row, word])
        assert torch.nonzero(out != want).tolist() == [[row, word]] and guards_intact(buf)


def test_min_bits_off_and_bad_arguments(toy_server):
    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 5)
        E.audit_set(rows, m + 1, SEED)                                    # min_bits = 531: a 530-bit launch is not audited
        launch(E, small, m)
        assert counters(E) == (0, 0, 0)
        E.audit_set(rows, m, SEED)
        launch(E, small, m)
        launch(E, small, 256)                                             # below min_bits
        assert counters(E) == (1, rows, 0)
        E.audit_set(0)                                                    # off: nothing more is counted
        launch(E, small, m)
        assert counters(E) == (0, 0, 0)
        lib, h = E._lib, E._h
        assert lib.fheaes_audit_set(h, _native.AUDIT_MAX_ROWS + 1, 0, 1) == -1
        assert lib.fheaes_audit_debug(h, 0, 0, 0) == -1 and lib.fheaes_audit_debug(h, 0, E.params.big1, 1) == -1
        assert lib.fheaes_audit_debug(h, 0, E.params.big, 1) == 0
        # records that do not fit are refused, as fheaes_k2_park_read does
        E.audit_set(rows, 0, SEED)
        E.audit_debug(_native.audit_rows(SEED, 0, m, rows)[0], 0, MASK)
        launch(E, small, m)
        n = ctypes.c_uint64()
        buf = (ctypes.c_uint64 * 5)()
        assert lib.fheaes_audit_read(h, None, None, None, buf, 0, ctypes.byref(n)) == -1
        assert lib.fheaes_audit_read(h, None, None, None, None, 0, ctypes.byref(n)) == 0 and n.value == 1
        assert lib.fheaes_audit_read(h, None, None, None, buf, 1, ctypes.byref(n)) == 0 and buf[2] == 0 and buf[3] ^ buf[4] == MASK


def test_a_whole_call_is_audited_launch_by_launch(toy_server, tc):
    """sbox over 64 bytes: the audit sees every blind-rotation launch of the call, the words and the stage's units do not change"""
    import torch

    with private(toy_server) as srv:
        E = srv.engine
        ct = tc.encrypt_bytes(list(range(7, 71)))
        off, on = dev(ct), dev(ct)
        E.profile_reset()
        srv.sbox(off, False)
        srv.synchronize()
        k2_off = E.profile_read()["blind_rotate"]
        srv.audit(rows=64, seed=SEED)
        E.profile_reset()
        srv.sbox(on, False)
        srv.synchronize()
        k2_on = E.profile_read()["blind_rotate"]
        report = srv.audit_check()
        assert torch.equal(on, off)
        assert k2_on["launches"] == k2_off["launches"] >= 1 and k2_on["units"] == k2_off["units"] == 64 * 8
        assert (report.launches, report.rows_checked, report.rows_wrong, report.records) == (k2_on["launches"], 64 * k2_on["launches"], 0, [])


def test_counters_are_complete_on_a_caller_s_stream(toy_server):
    import torch

    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 6)
        _, want = launch(E, small, m)
        E.audit_set(rows, 0, SEED)
        buf, out = guarded(m, E.params.big1)
        s = torch.cuda.Stream()
        E.set_stream(s.cuda_stream)
        try:
            E.cbs_pbs_batch(small, out, m)
            E.cbs_pbs_batch(small, out, m)
            s.synchronize()                                               # s only: not the device, not the context
            assert counters(E) == (2, 2 * rows, 0)
            assert torch.equal(out, want) and guards_intact(buf)
        finally:
            E.set_stream(None)


def test_audit_check_raises_with_the_record(toy_server):
    m, rows = 530, 32
    with private(toy_server) as srv:
        E = srv.engine
        small = small_rows(E.params, m, 7)
        srv.audit(rows=rows, seed=SEED)
        launch(E, small, m)
        ok = srv.audit_check()
        assert (ok.launches, ok.rows_checked, ok.rows_wrong, ok.records) == (1, rows, 0, [])
        row = _native.audit_rows(SEED, 1, m, rows)[31]
        E.audit_debug(row, 3, MASK)
        launch(E, small, m)
        with pytest.raises(AuditMismatch) as err:
            srv.audit_check()
        assert isinstance(err.value, _native.FheAesError)
        assert err.value.report.rows_wrong == 1 and len(err.value.records) == 1
        rec = err.value.records[0]
        assert (rec.launch, rec.row, rec.word, rec.got ^ rec.want, rec.device) == (1, row, 3, MASK, None)
        srv.audit()                                                       # a drawn seed, the default 64 rows; the counters start over
        launch(E, small, m)
        ok = srv.audit_check()
        assert (ok.launches, ok.rows_checked, ok.rows_wrong) == (1, 64, 0)


def test_server_group_sums_its_contexts(toy, toy_server, tc):
    p = toy.params
    rk = tc.encrypt_bytes(list(range(176))).reshape(11, 16, 8, p.big1)           # any ciphertexts do as round keys here
    state = tc.encrypt_bytes(list(range(100, 132))).reshape(2, 16, 8, p.big1)
    want = toy_server.aes_encrypt(rk, state.copy())
    g = ServerGroup(toy.keys, devices=(0, 0))
    try:
        g.audit(rows=32, seed=SEED)
        got = g.aes_encrypt(rk, state.copy())
        assert np.array_equal(got, want)
        report = g.audit_check()
        per = [s.audit_report() for s in g.servers]
        assert [(r.launches, r.rows_checked) for r in per] == [(10, 320), (10, 320)]             # one block each: ten 128-bit launches
        assert (report.launches, report.rows_checked, report.rows_wrong, report.records) == (20, 640, 0, [])
        # context 1's next launch (its launch 10) under its own seed, SEED + 1
        row = _native.audit_rows(SEED + 1, 10, 128, 32)[9]
        g.servers[1].engine.audit_debug(row, 0, MASK)
        g.aes_encrypt(rk, state.copy())
        with pytest.raises(AuditMismatch) as err:
            g.audit_check()
        report = err.value.report
        assert (report.launches, report.rows_checked, report.rows_wrong) == (40, 1280, 1)
        assert [(r.launch, r.row, r.word, r.device) for r in report.records] == [(10, row, 0, 0)]
    finally:
        for s in g.servers:
            s.engine.close()
