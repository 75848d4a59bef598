"""fheaes_aes_window_plan: when the block ciphers roll their rounds over windows of blocks, and how wide the window is (host logic
only, include/fheaes.h).  The fixed points are DESIGN.md section 5's; the properties hold for every batch up to 300 blocks and every
step count the three ciphers have.  A Python model of the cut itself (which segments a launch covers) states what the executor in
csrc/aes_schedule.h must do: tests/test_gpu_aes_windows.py checks its words and launch counts against it on the GPU."""
import ctypes as C

import pytest

from tfhe_aes_amd import _native

BLOCK_BITS = 128
MAX_WINDOW = 256                      # MAX_CHUNK_BITS / 128
STEP_COUNTS = (10, 12, 14, 19, 23, 27)        # Nr and 2 Nr - 1 for AES-128 / 192 / 256


def plan(n, steps, cus=256, k=4):
    return _native.aes_window_plan(n, steps, cus, k)


def k2_generations(bits, cus):
    """generations of one workgroup per CU of a paired launch, counted with fheaes_k2_launch_plan; up to 768 bits: one"""
    if bits == 0:
        return 0
    if bits <= 768:
        return 1
    lib = _native.load_library()
    form, um, rm, ut, rt = C.c_int(), C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert lib.fheaes_k2_launch_plan(bits, cus, 4, C.byref(form), C.byref(um), C.byref(rm), C.byref(ut), C.byref(rt)) == 0
    assert form.value == 2
    return -(-(um.value + ut.value) // cus)


@pytest.mark.parametrize("n, window, launches, gens, by_round", [
    (128, 120, 11, 107, 110),         # the bench shape: ten full windows and one of 80 blocks (6 six-generations + 1 four-generation)
    (64, 60, 11, 54, 60),
    (32, 24, 14, 27, 30),
    (13, 12, 11, 11, 20),
    (256, 252, 11, 214, 220),
    (1024, 252, 41, 854, 880),        # round by round: four chunks of 32,768 bits per step
    (12, 0, 10, 10, 10),              # already whole generations
    (120, 0, 10, 100, 100),
    (8, 0, 10, 10, 10),               # smaller than the smallest window
    (23, 0, 10, 20, 20),              # window 12 would give 19 launches of one generation and one of 256 bits: 20 either way
])
def test_fixed_points_on_256_cus_with_ten_steps(n, window, launches, gens, by_round):
    assert plan(n, 10) == {"window": window, "launches": launches, "generations": gens, "generations_by_round": by_round}


def test_other_devices_step_counts_and_parameter_sets():
    # 304 CUs: lcm(128, 1,824) / 128 = 57 blocks = 4 generations
    assert plan(60, 10, cus=304) == {"window": 57, "launches": 11, "generations": 43, "generations_by_round": 50}
    # 128 blocks there are 8.98 generations: 9 x 10 round by round, 11 x 8 + 2 in windows of 114 blocks -- nothing to gain, not rolled
    assert plan(128, 10, cus=304) == {"window": 0, "launches": 10, "generations": 90, "generations_by_round": 90}
    assert plan(57, 10, cus=304)["window"] == 0 and plan(56, 10, cus=304)["window"] == 0
    # the reference's decrypt (19 steps) on the 32-block shard: 57 generations round by round, 25 x 2 + 1 rolled
    assert plan(32, 19) == {"window": 24, "launches": 26, "generations": 51, "generations_by_round": 57}
    assert plan(128, 19)["window"] == 120 and plan(128, 14)["window"] == 120
    assert plan(32, 14) == {"window": 24, "launches": 19, "generations": 38, "generations_by_round": 42}
    # k = 1 has no paired form: never rolled
    for n in (13, 32, 128, 1024):
        assert plan(n, 10, k=1)["window"] == 0
    # up to 768 bits the full batch is not a paired launch
    for n in range(1, 7):
        assert plan(n, 10)["window"] == 0


@pytest.mark.parametrize("steps", STEP_COUNTS)
def test_plan_properties_for_every_batch_up_to_300_blocks(steps):
    cus = 256
    for n in range(1, 301):
        pl = plan(n, steps, cus)
        w = pl["window"]
        chunks = [MAX_WINDOW] * (n // MAX_WINDOW) + ([n % MAX_WINDOW] if n % MAX_WINDOW else [])
        assert pl["generations_by_round"] == steps * sum(k2_generations(c * BLOCK_BITS, cus) for c in chunks), (n, steps)
        if w == 0:
            assert pl["launches"] == steps * len(chunks) and pl["generations"] == pl["generations_by_round"], (n, steps)
            continue
        assert w <= min(n, MAX_WINDOW), (n, steps)
        assert w * BLOCK_BITS % (6 * cus) == 0, (n, steps)
        assert (w + 12) > min(n, MAX_WINDOW), (n, steps)                           # the largest multiple of 12 that fits
        assert n * BLOCK_BITS % (6 * cus) != 0, (n, steps)
        total = steps * n
        assert pl["launches"] == -(-total // w), (n, steps)
        assert pl["generations"] == (total // w) * (w * BLOCK_BITS // (6 * cus)) + k2_generations(total % w * BLOCK_BITS, cus), (n, steps)
        assert pl["generations"] < pl["generations_by_round"], (n, steps)


def window_segments(n, steps, w):
    """The cut the executor makes: launch j covers stream indices [j w, j w + w) of the steps x n block-rounds in (step, block) order.
    Per launch the list of (step, first block, blocks): one segment, or the end of a step and the start of the next."""
    assert 1 <= w <= n
    out = []
    for i0 in range(0, steps * n, w):
        length = min(w, steps * n - i0)
        s, b0 = divmod(i0, n)
        segs = [(s, b0, min(length, n - b0))]
        if segs[0][2] < length:
            segs.append((s + 1, 0, length - segs[0][2]))
        out.append(segs)
    return out


@pytest.mark.parametrize("n, steps, w", [(5, 10, 1), (5, 10, 3), (5, 10, 4), (5, 10, 5), (5, 27, 3), (13, 10, 12), (32, 19, 24),
                                         (128, 10, 120), (300, 14, 252)])
def test_model_of_the_cut_covers_every_block_round_once_and_in_order(n, steps, w):
    launches = window_segments(n, steps, w)
    assert len(launches) == -(-steps * n // w)
    next_step = [0] * n                                  # the step block b is due for
    for segs in launches:
        assert 1 <= len(segs) <= 2 and sum(s[2] for s in segs) <= w
        if len(segs) == 2:
            (s0, b0, c0), (s1, b1, c1) = segs
            assert s1 == s0 + 1 and b0 + c0 == n and b1 == 0 and c1 <= b0          # no block twice in a launch
        touched = set()
        for s, b0, count in segs:
            assert count >= 1 and b0 + count <= n and s < steps
            for b in range(b0, b0 + count):
                assert next_step[b] == s and b not in touched                     # reads only what earlier launches wrote
                touched.add(b)
        for b in touched:
            next_step[b] += 1
    assert next_step == [steps] * n


def test_bad_arguments_and_null_contexts_fail():
    lib = _native.load_library()
    w, la, g, gr = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    out = (C.byref(w), C.byref(la), C.byref(g), C.byref(gr))
    assert lib.fheaes_aes_window_plan(128, 10, 256, 4, *out) == 0
    for bad in ((0, 10, 256), (128, 0, 256), (128, 10, 0)):
        assert lib.fheaes_aes_window_plan(bad[0], bad[1], bad[2], 4, *out) == -1
    for i in range(4):
        args = list(out)
        args[i] = None
        assert lib.fheaes_aes_window_plan(128, 10, 256, 4, *args) == -1
    assert lib.fheaes_aes_context_window(None, 128, 10, C.byref(w)) == -1
    assert lib.fheaes_aes_set_window(None, 0) == -1
    assert lib.fheaes_aes_set_window(None, _native.AES_WINDOW_OFF) == -1
