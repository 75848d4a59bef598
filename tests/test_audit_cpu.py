"""The audit's host side without a GPU: fheaes_audit_rows against the Python-integer model of audit_model.py, the properties of the rows
it names (one per stratum, ascending, distinct, below m; every row when S = m; other rows for another launch or seed), the run-length
guarantee checked exhaustively at m = 530 with 32 samples, and the four entry points' place in the header, the binding and the bad-argument
codes.  None of the four takes a memspace: they are configuration and counters, not compute entry points (test_workspace_state_cpu.py)."""
import ctypes
import re

import numpy as np
import pytest

import audit_model as am
from tfhe_aes_amd import _build, _native

NAMES = ("fheaes_audit_set", "fheaes_audit_rows", "fheaes_audit_read", "fheaes_audit_debug")
MS = (1, 2, 255, 256, 257, 530, 800, 16384, 32768)
ROWS = (1, 7, 64, 256)
SEEDS = (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 0x0123456789ABCDEF)
LAUNCHES = (0, 1, 2, 1000, (1 << 64) - 1)


def header_text():
    return re.sub(r"/\*.*?\*/", "", (_build.ROOT / "include" / "fheaes.h").read_text(), flags=re.S)


def test_splitmix64_is_the_published_generator():
    """the first outputs of splitmix64 from state 0 (Vigna's reference implementation, seed 0): sm(0), then the state advanced by the
    golden-ratio increment"""
    assert am.splitmix64(0) == 0xE220A8397B1DCDAF
    assert am.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert am.splitmix64((2 * 0x9E3779B97F4A7C15) & am.MASK) == 0x06C45D188009454F


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("rows", ROWS)
def test_c_function_equals_the_model(m, rows):
    for seed in SEEDS:
        for launch in LAUNCHES:
            assert _native.audit_rows(seed, launch, m, rows) == am.audit_rows(seed, launch, m, rows), (seed, launch)
    assert _native.Engine.audit_rows(SEEDS[2], 3, m, rows) == am.audit_rows(SEEDS[2], 3, m, rows)        # the Engine's spelling of it


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("rows", ROWS)
def test_rows_are_one_per_stratum_ascending_distinct_and_below_m(m, rows):
    S = min(rows, m)
    st = am.strata(m, rows)
    assert len(st) == S and st[0][0] == 0 and st[-1][1] == m
    assert all(hi > lo for lo, hi in st) and all(st[i][1] == st[i + 1][0] for i in range(S - 1))
    for seed in SEEDS[:3]:
        for launch in LAUNCHES[:3]:
            got = _native.audit_rows(seed, launch, m, rows)
            assert len(got) == S
            assert all(lo <= r < hi for r, (lo, hi) in zip(got, st))
            assert got == sorted(set(got)) and got[-1] < m
            if S == m:
                assert got == list(range(m))                              # every row is checked


@pytest.mark.parametrize("m,rows", [(530, 32), (800, 64), (16384, 64), (16384, 256), (32768, 256)])
def test_rows_differ_between_launches_and_between_seeds(m, rows):
    base = _native.audit_rows(SEEDS[4], 0, m, rows)
    assert _native.audit_rows(SEEDS[4], 1, m, rows) != base
    assert _native.audit_rows(SEEDS[4] + 1, 0, m, rows) != base
    # seed + launch is mixed before the sample index is: (seed, launch 1) and (seed + 1, launch 0) name the same rows, on purpose -- a
    # ServerGroup's seeds differ by more than its launches only if the caller draws them, as the default does
    assert _native.audit_rows(SEEDS[4], 1, m, rows) == _native.audit_rows(SEEDS[4] + 1, 0, m, rows)
    # the offsets move from launch to launch: 64 launches name several times as many rows as one does (every stratum here has 12 rows or more)
    seen = {r for launch in range(64) for r in _native.audit_rows(SEEDS[4], launch, m, rows)}
    assert len(seen) >= 8 * rows


def test_every_run_of_the_guaranteed_length_is_caught_at_530_by_32():
    """any 2 ceil(m / S) - 1 = 33 consecutive wrong rows hold a whole stratum, so whatever the offsets the audit names one of them:
    every start, several seeds and launches; and the bound is tight -- some run one row shorter escapes"""
    m, rows = 530, 32
    L = am.caught_run_length(m, rows)
    assert L == 33
    for lo, hi in am.strata(m, rows):
        assert hi - lo in (16, 17)
    for seed in SEEDS:
        for launch in LAUNCHES[:4]:
            named = _native.audit_rows(seed, launch, m, rows)
            hit = np.zeros(m + 1, dtype=np.int64)
            hit[np.asarray(named) + 1] = 1
            cum = np.cumsum(hit)                                          # cum[i]: named rows below i
            for start in range(m - L + 1):
                assert cum[start + L] - cum[start] >= 1, "rows %d..%d escape the audit (seed %#x, launch %d)" % (start, start + L - 1, seed, launch)
    # tight: between the first row of one 17-row stratum and the last row of the next lie 32 rows that nobody checks, and some seed puts
    # the samples there (the longest unchecked run over 512 seeds, by the model, which is the C function's equal above)
    longest = 0
    for seed in range(512):
        named = [-1] + am.audit_rows(seed, 0, m, rows) + [m]
        longest = max(longest, max(b - a - 1 for a, b in zip(named, named[1:])))
    assert longest == L - 1


def test_round_6_detection_probability_is_what_the_documents_say():
    """W scattered wrong rows escape S of m sampled rows with probability about (1 - S / m)^W: 230 rows, 16,384 bits, 256 samples"""
    assert round(1 - (1 - 256 / 16384) ** 230, 2) == 0.97


def test_the_four_names_are_declared_bound_and_take_no_memspace():
    text = header_text()
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.header_symbols()
        args = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text).group(1)
        assert "memspace" not in args, name
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
    for method in ("audit_set", "audit_rows", "audit_read", "audit_debug"):
        assert callable(getattr(_native.Engine, method))


def test_header_constants_equal_the_binding_s():
    text = header_text()
    assert int(re.search(r"#define\s+FHEAES_AUDIT_MAX_ROWS\s+(\d+)", text).group(1)) == _native.AUDIT_MAX_ROWS == am.MAX_ROWS == 256
    assert int(re.search(r"#define\s+FHEAES_AUDIT_RECORDS\s+(\d+)", text).group(1)) == _native.AUDIT_RECORDS == 16


def test_null_context_and_bad_arguments():
    lib = _native.load_library()
    u64 = ctypes.c_uint64
    a, b, c, n = u64(), u64(), u64(), u64()
    rec = (u64 * (5 * _native.AUDIT_RECORDS))()
    for rows in (0, 1, 256, 257):
        assert lib.fheaes_audit_set(None, rows, 0, 1) == -1
    assert lib.fheaes_audit_read(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), rec, _native.AUDIT_RECORDS, ctypes.byref(n)) == -1
    assert lib.fheaes_audit_read(None, None, None, None, None, 0, None) == -1
    assert lib.fheaes_audit_debug(None, 0, 0, 1) == -1
    assert lib.fheaes_audit_debug(None, 0, 0, 0) == -1
    out = (u64 * 256)()
    assert lib.fheaes_audit_rows(1, 0, 530, 32, out) == 0
    assert lib.fheaes_audit_rows(1, 0, 0, 32, out) == -1                # no rows to sample from
    assert lib.fheaes_audit_rows(1, 0, 530, 0, out) == -1               # no samples
    assert lib.fheaes_audit_rows(1, 0, 530, 257, out) == -1             # more than FHEAES_AUDIT_MAX_ROWS
    assert lib.fheaes_audit_rows(1, 0, 530, 32, None) == -1
    for bad in ((1, 0, 0, 32), (1, 0, 530, 0), (1, 0, 530, 257)):
        with pytest.raises(_native.FheAesError):
            _native.audit_rows(*bad)


def test_a_huge_batch_does_not_overflow_the_stratum_arithmetic():
    """m is a uint64 in the C ABI: s * m leaves 64 bits long before m does, and the function must not form it"""
    for m in ((1 << 64) - 1, (1 << 63) + 12345, (1 << 56) + 1):
        assert _native.audit_rows(SEEDS[4], 7, m, 256) == am.audit_rows(SEEDS[4], 7, m, 256)
