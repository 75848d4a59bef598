"""The audit's call tests, pinned without a GPU (tests/audit_calls.py): which of the 50 cases of workspace_state.CASES launch a blind
rotation, the launch sizes of the cases whose schedule follows from a plan function -- restated here as literals, so a chunk constant, a
window rule or a pool size that changes turns this file red before the GPU file miscounts --, what an audit of 1 and of 256 rows must
count for them, the shapes of the detection and seam tests, the rows fheaes_audit_rows names at m = 257 (the first row count past the
latency form: strata of 1 and 2 rows), and the arithmetic of the record cap."""
import pytest

import audit_calls as ac
import audit_model as am
import chunk_seams as cs
import workspace_state as ws
from tfhe_aes_amd import _native


@pytest.fixture(scope="module")
def env(toy):
    return ws.Env(toy)


# the launch sizes of variant 0 of every case that has a plan, in launch order (PARAM_TOY, automatic window = none: the toy set has no
# paired form).  The public call: 33 distinct (position, byte) pairs in round 1 -- two of its three blocks share 15 bytes --, 36 in round
# 2 (one column of the pair differs), 48 from round 3 on
PUBLIC_PLAN = [33, 36, 48, 48, 48, 48, 48, 48, 48, 48]
EXPECTED = {
    "k1_keyswitch": [], "k3_pfpks": [], "k4_forward_fourier": [], "k5_vertical_packing": [], "pack_unpack_round_keys": [], "pack_unpack_513": [],
    "pack_unpack_513_width16": [], "expand_seeded": [],
    "k2_cbs_pbs": [3], "gate_ggsw": [2], "gate": [2], "gate_packed": [2],
    "wopbs_8_bits_shared_luts": [24], "wopbs_9_bits_per_input_luts": [27], "wopbs_11_bits_tree": [33],
    "sbox": [24], "sbox_inv": [24], "many_sbox": [24], "many_sbox_inv": [24],
    "aes_encrypt": [256] * 10, "aes_decrypt": [256] * 19, "aes_decrypt_equivalent": [256] * 10,
    "aes_encrypt_keyed": [384] * 10, "aes_decrypt_keyed": [384] * 19, "aes_decrypt_equivalent_keyed": [384] * 10,
    "aes_encrypt_keyed_packed": [384] * 10, "aes_decrypt_keyed_packed": [384] * 19, "aes_decrypt_equivalent_keyed_packed": [384] * 10,
    "aes_encrypt_public": [8 * u for u in PUBLIC_PLAN],
}


def test_the_50_cases_split_into_k2_and_no_k2_as_the_table_says():
    assert len(ws.CASES) == 50
    no_k2 = {c.name for c in ws.CASES if not ac.launches_k2(c)}
    assert no_k2 == set(ac.NO_K2) and len(no_k2) == 8
    for c in ws.CASES:
        grows = {"ws_small", "ws_pbs"} <= set(c.uses)
        if c.name in ("k2_cbs_pbs", "gate_ggsw"):
            assert not grows and "fheaes_cbs_pbs_batch" in c.entry           # the K2 stage call: into the caller's buffer
        else:
            assert ac.launches_k2(c) == grows, c.name
            assert "fheaes_cbs_pbs_batch" not in c.entry
        assert ("ws_small" in c.uses) == ("ws_pbs" in c.uses), c.name       # K1's output exists only to be K2's input


def test_launch_lists_are_the_literals(env):
    listed = {}
    for c in ws.CASES:
        got = ac.launch_list(c.name, c.build(env, 0) if c.name == "aes_encrypt_public" else None)
        if got is not None:
            listed[c.name] = got
    assert listed == EXPECTED
    for name, launches in listed.items():
        assert (launches == []) == (name in ac.NO_K2), name
        assert all(1 <= m <= cs.MAX_CHUNK_BITS for m in launches)
    # the other 21 cases launch K2 and have no list: the GPU test brackets their row count instead
    assert {c.name for c in ws.CASES} - set(listed) == {c.name for c in ws.CASES if ac.launches_k2(c) and not ac.has_launch_list(c.name)}
    assert set(listed) == {c.name for c in ws.CASES if ac.has_launch_list(c.name)} and len(listed) == 29


def test_public_plan_is_the_plan_function_s_and_its_largest_pool_is_a_later_launch(env):
    for v, want in ((0, PUBLIC_PLAN), (1, None)):
        h = ws.BY_NAME["aes_encrypt_public"].build(env, v)
        plan = _native.aes_public_plan(h["blocks"])
        assert len(plan) == 10 and plan[0] == cs.public_pool_round_1(h["blocks"]) and max(plan) == 48
        if want:
            assert plan == want
    min_bits, rounds = ac.largest_pool_launches(PUBLIC_PLAN)
    assert (min_bits, rounds) == (384, list(range(2, 10)))                 # the call's launches 0 and 1 stay below min_bits: 8 audited launches


def test_counts_of_one_row_and_of_256_rows():
    for name, launches in EXPECTED.items():
        L, U = len(launches), sum(launches)
        assert ac.rows_checked(launches, 1) == L
        full = ac.rows_checked(launches, 256)
        assert L <= full <= min(256 * L, U)
        if all(m <= 256 for m in launches):
            assert full == U                                                # every row of every launch
    assert ac.rows_checked(EXPECTED["aes_encrypt_keyed"], 256) == 2560 and ac.rows_checked(EXPECTED["aes_encrypt_public"], 256) == 256 * 10
    assert ac.rows_checked(EXPECTED["aes_decrypt"], 256) == sum(EXPECTED["aes_decrypt"]) == 19 * 256


@pytest.mark.parametrize("direction", sorted(ac.STEPS))
@pytest.mark.parametrize("n,w", [(2, 1), (3, 2), (5, 2), (5, 3), (5, 7)])
def test_window_launch_rows_against_the_window_count(direction, n, w):
    steps = ac.STEPS[direction]
    rows = ac.window_launch_rows(n, steps, w)
    assert len(rows) == cs.window_launches(n, steps, min(w, n))[0] == -(-steps * n // min(w, n))
    assert sum(rows) == steps * n * 128 and set(rows[:-1]) <= {128 * min(w, n)} and 128 <= rows[-1] <= 128 * min(w, n)
    assert ac.window_launch_rows(n, steps, 0) == [128 * n] * steps
    # the toy set never rolls by itself (no paired form at k = 1), so the table's calls are round by round
    assert _native.aes_window_plan(n, steps, 256, 1)["window"] == 0 and _native.aes_window_plan(n, steps, 256, 1)["launches"] == steps


def test_detection_shapes():
    """the first audited launch of each site and its sample: S = min(rows, m0)"""
    assert ac.launch_list("sbox") == [24] and len(_native.audit_rows(ac.SEED, 0, 24, 8)) == 8
    forced = ac.window_launch_rows(5, 10, 2)
    assert forced[0] == 256 and len(forced) == 25 and set(forced) == {256}
    assert len(ac.window_launch_rows(5, 10, 3)) == 17 and ac.window_launch_rows(5, 10, 3)[-1] == 256
    # a window of 2 over 5 blocks: the first launch lies inside step 0, the third (blocks 4 and 0) is the first of two segments
    assert [(2 * j) % 5 + 2 > 5 for j in range(4)] == [False, False, True, False]
    assert ac.rows_checked(forced, 32) == 32 * 25
    assert ac.gate_launch_rows(2) == [2] and _native.audit_rows(ac.SEED, 0, 2, 64) == [0, 1]      # S = 2: every row is sampled
    assert ac.MASK == 1 << 62


def test_seam_shapes():
    assert cs.M_BITS == 33281 and ac.wopbs_launch_rows(cs.M_BITS, 1) == [32768, 513]
    assert ac.rows_checked([32768, 513], 256) == 512 and ac.rows_checked([32768, 513], 1) == 2
    assert cs.GATE_BOOT_GATES == 32769 and ac.gate_launch_rows(32769) == [32768, 1]
    assert ac.rows_checked([32768, 1], 64) == 65
    runs = cs.gate_boot_runs(head=9)
    assert len(runs) == 32769 and sum(runs) == 9 + 32764 + sum(cs.GATE_BOOT_TAIL) and runs[32767] == 0 and runs[32768] == 9
    # the second launch's only row is row 0, so a hook on row 0 must be used up by the FIRST launch to be recorded as launch 0
    assert _native.audit_rows(ac.SEED, 1, 1, 64) == [0] and _native.audit_rows(ac.SEED, 0, 32768, 64)[0] < 512


@pytest.mark.parametrize("seed", [ac.SEED, 0, 1, (1 << 64) - 1])
def test_audit_rows_at_257_by_256(seed):
    m, rows = 257, 256
    st = am.strata(m, rows)
    assert len(st) == 256 and sorted({hi - lo for lo, hi in st}) == [1, 2] and [hi - lo for lo, hi in st].count(2) == 1
    for launch in (0, 1, 2, 1000):
        got = _native.audit_rows(seed, launch, m, rows)
        assert got == am.audit_rows(seed, launch, m, rows)
        assert len(got) == 256 and all(a < b for a, b in zip(got, got[1:])) and 0 <= got[0] and got[-1] < m
        assert len(set(range(m)) - set(got)) == 1                           # one row of the two-row stratum is left out


def test_record_cap_arithmetic():
    hooks = ac.cap_hooks()
    assert len(hooks) == ac.RECORDS + 1 == 17
    rows = [r for r, _ in hooks]
    assert rows == [5 * j for j in range(17)] and max(rows) < 100 and len(set(rows)) == 17
    assert all(w == j and w < 513 for j, (_, w) in enumerate(hooks))        # a word of the toy set's 513-word row
    assert _native.audit_rows(ac.SEED, 3, 100, 256) == list(range(100))      # S = m: whatever the launch number, every hook row is sampled
    assert min(len(hooks), ac.RECORDS) == 16                                # what fheaes_audit_read reports as record_n


def test_param_opt_forms_by_the_plan_function():
    import ctypes as C

    lib = _native.load_library()

    def plan(m, allow_pair):
        form, um, rm, ut, rt = C.c_int(), C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        assert lib.fheaes_k2_launch_plan_forms(m, 256, 4, allow_pair, C.byref(form), C.byref(um), C.byref(rm), C.byref(ut), C.byref(rt)) == 0
        return form.value, um.value, rm.value, ut.value, rt.value

    assert plan(600, 1) == (1, 200, 3, 0, 2)
    assert plan(800, 0) == (1, 267, 3, 0, 2)                                # the 16-form above 768 bits: 266 units of 3 and one of 2 rows
    assert plan(2100, 1) == (2, 26, 6, 486, 4) and 26 * 6 + 486 * 4 == 2100
