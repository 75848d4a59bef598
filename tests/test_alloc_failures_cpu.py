"""What test_gpu_alloc_failures.py rests on, pinned without a GPU: the hook refuses a NULL context and is bound as the header declares it,
every case of workspace_state.CASES has its row in alloc_failures.py, the positions of the sweep, and the allocation sites: every
device allocation of a live context goes through ctx_malloc, so a `hipMalloc(` anywhere else in csrc/ is fheaes_create's or the
developer build's StampReport."""
import ctypes
import re

import alloc_failures as af
import workspace_state as ws
from tfhe_aes_amd import _build, _native


def test_hook_rejects_a_null_context_and_is_bound_as_declared():
    lib = _native.load_library()
    seen = ctypes.c_uint64(7)
    for nth in (0, 1, af.FAR):
        assert lib.fheaes_alloc_debug(None, nth, ctypes.byref(seen)) == af.INVALID
        assert lib.fheaes_alloc_debug(None, nth, None) == af.INVALID
    assert seen.value == 7
    res, args = _native.SIGNATURES["fheaes_alloc_debug"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    text = re.sub(r"/\*.*?\*/", "", (_build.ROOT / "include" / "fheaes.h").read_text(), flags=re.S)
    assert re.search(r"int\s+fheaes_alloc_debug\(fheaes_ctx \*ctx, uint64_t fail_nth, uint64_t \*seen_out\);", text)
    assert callable(_native.Engine.alloc_debug)


def test_error_codes_restate_the_header():
    text = (_build.ROOT / "include" / "fheaes.h").read_text()
    defines = dict(line.split()[1:3] for line in text.splitlines() if line.startswith("#define FHEAES_ERR_") or line.startswith("#define FHEAES_OK"))
    assert [int(defines[n]) for n in ("FHEAES_OK", "FHEAES_ERR_INVALID", "FHEAES_ERR_NOKEYS", "FHEAES_ERR_DEVICE", "FHEAES_ERR_NOMEM")] == [
        af.OK, af.INVALID, af.NOKEYS, af.DEVICE, af.NOMEM] == [0, -1, -2, -3, -4]


def test_every_case_has_a_row():
    assert set(af.ALLOCATIONS) == set(ws.BY_NAME) and len(af.ALLOCATIONS) == 50
    for c in ws.CASES:
        a = af.ALLOCATIONS[c.name]
        assert isinstance(a, int) and a >= len(c.uses), c.name
        assert (a == 0) == (not c.uses), c.name                   # resident inputs: no staging, so a call without scratch allocates nothing
        assert all(af.REFUSAL[e] == af.NOMEM for e in c.entry)
        assert af.written(c) <= {"state", "x"}
    assert af.THINNED <= set(ws.BY_NAME)
    outside = {"fheaes_reserve", "fheaes_upload_keys", "fheaes_upload_keys_seeded", "fheaes_clone_keys", "fheaes_audit_set", "fheaes_k2_park_debug"}
    assert outside <= set(af.REFUSAL) <= set(_native.SIGNATURES) and set(af.REFUSAL.values()) == {af.NOMEM}


def test_positions_of_the_sweep():
    assert af.retry_positions(0) == [] and af.fail_positions(0) == []
    assert af.retry_positions(1) == [1] and af.retry_positions(2) == [1, 2] and af.retry_positions(3) == [1, 2, 3]
    assert af.retry_positions(7) == [1, 4, 7] and af.retry_positions(12) == [1, 6, 12]
    assert af.fail_positions(7) == [1, 2, 3, 4, 5, 6, 7]
    assert af.fail_positions(12, thinned=True) == [1, 3, 5, 6, 7, 9, 11, 12]
    for a in range(1, 40):
        assert set(af.retry_positions(a)) <= set(af.fail_positions(a, thinned=True)) <= set(af.fail_positions(a)) == set(range(1, a + 1))
    assert af.refused_bytes("fheaes error -4: hipMalloc(4104 bytes): out of memory") == 4104 and af.refused_bytes("hipMalloc: out of memory") is None
    assert af.UPLOAD_ALLOCATIONS == {("plain", "host"): 4, ("plain", "device"): 3, ("seeded", "host"): 5, ("seeded", "device"): 4} and af.IMAGES == 3


def sources():
    return {p.name: p.read_text() for p in sorted(_build.CSRC.iterdir()) if p.suffix in (".h", ".hip", ".c")}


def test_every_allocation_of_a_live_context_goes_through_ctx_malloc():
    src = sources()
    ctx = src["engine_ctx.h"]
    body = re.search(r"\nint ctx_malloc\(fheaes_ctx \*c, void \*\*p, size_t bytes\)\n\{.*?\n\}\n", ctx, flags=re.S)
    assert body and body.group(0).count("hipMalloc(p, ask)") == 1 and "(void)hipGetLastError();" in body.group(0) and "FHEAES_ERR_NOMEM" in body.group(0)
    src["engine_ctx.h"] = ctx.replace(body.group(0), "\n")
    calls = {name: len(re.findall(r"\bctx_malloc\(", text)) for name, text in src.items()}
    # ensure(); the three key images, the staging array and the bodies' staging array of upload_keys_impl, the images of fheaes_clone_keys
    assert {n: v for n, v in calls.items() if v} == {"engine_ctx.h": 1, "engine.hip": 6}
    raw = {name: re.findall(r"[^\n]*\bhipMalloc\([^\n]*", text) for name, text in src.items()}
    raw = {n: v for n, v in raw.items() if v}
    assert set(raw) == {"engine_ctx.h", "engine.hip"}
    assert len(raw["engine_ctx.h"]) == 1 and "waves * EP_NPH" in raw["engine_ctx.h"][0]           # StampReport (EP_STAMPS builds only)
    assert len(raw["engine.hip"]) == 3 and all("return bail(\"hipMalloc\", e)" in line for line in raw["engine.hip"])      # fheaes_create
    # FHEAES_ERR_NOMEM is produced in ctx_malloc and nowhere else
    assert all("fail(FHEAES_ERR_NOMEM" not in text for text in src.values())
    # the pinned buffer is host memory: out, like fheaes_create
    assert sum(text.count("hipHostMalloc(") for text in src.values()) == 1
