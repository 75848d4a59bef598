"""Every launch shape of the blind rotation (K2) at PARAM_OPT, and both occupancy fallbacks, word for word.

engine_launch.h::k2_plan cuts a batch into workgroups of 1, 2, 3, 4 or 6 ciphertexts, with ragged last units, one or several
generations and a units_main / units_tail split; k2_launch then picks the kernel after two occupancy queries that always succeed on an
MI355X.  The fallbacks behind those queries -- the 16-form above 768 bits where the paired kernel cannot be placed, and the parked
variant blind_rotate16_kernel<5,5,8,3,2,false> where two LDS-home workgroups do not fit a CU -- run here through the deny-only hook
fheaes_k2_set_forms.  Every case asserts the plan it exists for first, so a later change to the plan fails the case instead of moving
it silently onto another branch.

One input for the whole module: 2,112 rows of arbitrary 64-bit words (K2 is defined on any words).  Two references:
  * the cut reference: all rows through 256-bit launches (latency form, one ciphertext per workgroup: no units, no ragged slots, no
    parking), kept on the device, itself pinned against the oracle on 32 rows spread evenly;
  * the oracle (opt.oracle.cbs_pbs) on the rows where a shape can go wrong: the first unit, the last main unit, the first tail unit and
    the valid rows of the last unit -- at most 20 rows per shape, cached by row index, at most ORACLE_ROW_CAP distinct rows for the file.
Each shape is ONE launch into rows [2 : 2 + m] of a sentinel-filled device tensor of m + 4 rows: the guard rows must keep the sentinel
(a ragged unit's suppressed stores), all m rows must equal the cut reference, the selected rows the oracle.  All comparisons are exact.

The same guard rows for the ragged tiles of K1, K3, K4, K5 and the CMUX tree, against what the same call returns through host arrays
(which test_gpu_stages.py and test_gpu_aes.py pin against the oracle).

The CMUX tree at k = 4 (cmux_level_kernel<5,15,3>) at the depths the tag check runs, 12, 13 and 16 bits, inside guard rows and word for
word against the oracle (opt.oracle.wopbs_batch): the last section.

Wall time on an MI355X (pytest --durations=0): NOT MEASURED YET, see DESIGN.md section 5, "Launch shapes and fallback forms under test".
"""
import numpy as np
import pytest

from gpu_support import FORMS, HOME, LATENCY, PAIR, PARKED, dev, guarded, guards_intact, host, plan_tuple, unit_rows
from oracle import oracle as orc
from tfhe_aes_amd import _native

pytestmark = pytest.mark.gpu

ROWS = 2112                          # the largest shape is 2,101 bits; 2,112 = 32 x 66
ORACLE_ROW_CAP = 400                 # distinct rows the oracle may be asked for in this file (about 10 ms each on 16 cores)

# (forms, m, (form, units_main, r_main, units_tail, r_tail) at 256 CUs, kernel-name prefix): engine_launch.h::k2_plan / k2_launch
CASES = [
    ("default", 256, (0, 256, 1, 0, 0), LATENCY),              # the last latency launch
    ("default", 257, (1, 0, 3, 129, 2), HOME),                 # first 16-form launch: two-ciphertext units, ragged 1 of 2
    ("default", 512, (1, 0, 3, 256, 2), HOME),                 # one two-ciphertext unit on every CU
    ("default", 513, (1, 171, 3, 0, 2), HOME),                 # first three-ciphertext home units
    ("default", 514, (1, 172, 3, 0, 2), HOME),                 # ragged 1 of 3
    ("default", 766, (1, 256, 3, 0, 2), HOME),                 # ragged home unit on the last CU, 1 of 3
    ("default", 768, (1, 256, 3, 0, 2), HOME),                 # the last 16-form launch
    ("default", 769, (2, 0, 6, 193, 4), PAIR),                 # first paired launch, ragged 1 of 4
    ("default", 1023, (2, 0, 6, 256, 4), PAIR),                # ragged four-unit, 3 of 4
    ("default", 1025, (2, 1, 6, 255, 4), PAIR),                # a single six-unit in front of 255 four-units
    ("default", 1535, (2, 256, 6, 0, 4), PAIR),                # six-units only, no tail, ragged 5 of 6
    ("default", 1536, (2, 256, 6, 0, 4), PAIR),                # six-units only, exact
    ("default", 1537, (2, 0, 6, 385, 4), PAIR),                # one and a half generations of four-units, ragged 1 of 4
    ("default", 2101, (2, 27, 6, 485, 4), PAIR),               # two generations, ragged last four-unit, 3 of 4
    ("pair denied", 769, (1, 257, 3, 0, 2), HOME),             # two home workgroups on one CU
    ("pair denied", 1536, (1, 512, 3, 0, 2), HOME),            # every slot taken: all 160 KB of LDS on every CU
    ("pair denied", 1537, (1, 513, 3, 0, 2), HOME),            # one unit beyond the slots
    ("pair denied", 2048, (1, 0, 3, 1024, 2), HOME),           # two generations of two-ciphertext units only
    ("pair denied", 2100, (1, 52, 3, 972, 2), HOME),           # mixed generations: the units_main split
    ("home denied", 514, (1, 172, 3, 0, 2), PARKED),           # the parked three-ciphertext body, ragged
    ("home denied", 768, (1, 256, 3, 0, 2), PARKED),           # ... and full
    ("both denied", 2100, (1, 52, 3, 972, 2), PARKED),         # parked three- and two-units in generations
]


def _corner_rows(plan, m):
    """rows of the first unit, the last main unit, the first tail unit and the last unit of a launch, ragged slots left out"""
    _, um, _, ut, _ = plan
    units = {0, um + ut - 1} | ({um - 1} if um else set()) | ({um} if ut else set())
    rows = sorted({i for u in units for i in unit_rows(plan, u, m)})
    assert 0 < len(rows) <= 20 and rows[-1] == m - 1
    return rows


class K2Ref:
    """the module's input, the cut reference on the device, and the oracle's rows by index"""

    def __init__(self, opt):
        import torch

        p, E = opt.params, opt.engine()
        self.opt = opt
        self.small = np.random.default_rng(0x2112).integers(0, 1 << 64, (ROWS, p.n + 1), dtype=np.uint64)
        self.small_d = dev(self.small)
        pl = E.k2_plan(256)
        assert pl["form"] == 0 and pl["kernel"].startswith(LATENCY)
        self.cut = torch.empty((ROWS, p.big1), dtype=torch.int64, device="cuda")
        for lo in range(0, ROWS, 256):
            n = min(256, ROWS - lo)
            E.cbs_pbs_batch(self.small_d[lo:lo + n], self.cut[lo:lo + n], n)
        E.synchronize()
        self._rows = {}

    def oracle(self, rows):
        missing = [r for r in rows if r not in self._rows]
        assert len(self._rows) + len(missing) <= ORACLE_ROW_CAP, "this file asks the oracle for more than %d distinct rows" % ORACLE_ROW_CAP
        if missing:
            for r, w in zip(missing, self.opt.oracle.cbs_pbs(np.ascontiguousarray(self.small[missing]))):
                self._rows[r] = w
        return np.stack([self._rows[r] for r in rows])


@pytest.fixture(scope="module")
def k2ref(opt):
    return K2Ref(opt)


def test_cut_reference_against_the_oracle(k2ref):
    """the reference every shape below is compared with in full is itself the oracle's on 32 rows spread evenly over the input"""
    rows = list(range(0, ROWS, ROWS // 32))
    assert len(rows) == 32
    assert np.array_equal(host(k2ref.cut[rows]), k2ref.oracle(rows))


@pytest.mark.parametrize("forms,m,plan,kernel", CASES, ids=["%s-%d" % (c[0].replace(" ", "_"), c[1]) for c in CASES])
def test_k2_launch_shape(forms, m, plan, kernel, opt, k2ref):
    import torch

    p, E = opt.params, opt.engine()
    try:
        E.k2_set_forms(*FORMS[forms])
        pl = E.k2_plan(m)
        assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl           # the launch this case exists for
        buf, out = guarded(m, p.big1)
        E.cbs_pbs_batch(k2ref.small_d[:m], out, m)
        E.synchronize()
    finally:
        E.k2_set_forms(True, True)
    assert guards_intact(buf), "a store outside the %d output rows" % m
    if not torch.equal(out, k2ref.cut[:m]):
        bad = torch.nonzero((out != k2ref.cut[:m]).any(dim=1)).flatten().cpu().numpy()
        raise AssertionError("%d of %d rows differ from the cut reference: %s ..." % (len(bad), m, bad[:24]))
    rows = _corner_rows(plan, m)
    assert np.array_equal(host(out[rows]), k2ref.oracle(rows))


def test_pair_denied_launch_leaves_the_parking_pool_alone(opt, k2ref):
    """with the pair denied a batch above 768 bits is a 16-form launch: the paired kernel's owner words are not reset, no record is
    written under the recording hook, and the counters stand still"""
    import torch

    p, E = opt.params, opt.engine()
    m = 770                                                      # (1, 257, 3, 0, 2), ragged 2 of 3
    taken = np.full(_native.K2_PARK_SLOTS, 7, dtype=np.uint32)
    try:
        E.k2_park_debug(taken, record=True)                      # a paired launch would start from these words and record its slots
        before = E.k2_park_read()
        E.k2_set_forms(False, True)
        pl = E.k2_plan(m)
        assert plan_tuple(pl) == (1, 257, 3, 0, 2) and pl["kernel"].startswith(HOME)
        buf, out = guarded(m, p.big1)
        E.cbs_pbs_batch(k2ref.small_d[:m], out, m)
        E.synchronize()
        after = E.k2_park_read()
    finally:
        E.k2_set_forms(True, True)
        E.k2_park_debug(None, record=False)
    assert len(after["record"]) == 0 and (after["fallbacks"], after["violations"]) == (before["fallbacks"], before["violations"])
    assert np.array_equal(after["owner"], before["owner"])
    assert guards_intact(buf) and torch.equal(out, k2ref.cut[:m])


def test_forms_hook_is_per_context_and_deny_only(opt, toy):
    """fheaes_k2_set_forms on one context changes that context's launches only; arguments other than 0 / 1 are FHEAES_ERR_INVALID and
    change nothing; k = 1 has neither form and plans the same kernel under every setting; (1, 1) restores what the queries allow"""
    E, T = opt.engine(), toy.engine()
    other = _native.Engine(opt.params)                           # a second context on the same device (plans need no keys)
    sizes = (256, 514, 768, 2100)
    try:
        default = [E.k2_plan(m) for m in sizes]
        assert [d["kernel"] for d in default] == [LATENCY, HOME, HOME, PAIR + " parking=claimed"]
        names_other = [other.k2_plan(m)["kernel"] for m in sizes]
        assert names_other == [d["kernel"] for d in default]
        toy_plan = T.k2_plan(530)
        assert toy_plan["kernel"].startswith("blind_rotate16_kernel<2,5,8,8") and plan_tuple(toy_plan)[:4] == (1, 67, 8, 0)
        E.k2_set_forms(False, False)
        assert [E.k2_plan(m)["kernel"] for m in sizes] == [LATENCY, PARKED, PARKED, PARKED]
        assert plan_tuple(E.k2_plan(2100)) == (1, 52, 3, 972, 2)
        assert [other.k2_plan(m)["kernel"] for m in sizes] == names_other
        assert T.k2_plan(530) == toy_plan
        for bad in ((2, 1), (1, 2), (-1, 0), (0, 7)):
            assert E._lib.fheaes_k2_set_forms(E._h, *bad) == -1
        assert [E.k2_plan(m)["kernel"] for m in sizes] == [LATENCY, PARKED, PARKED, PARKED]      # a refused call changes nothing
        E.k2_set_forms(False, True)
        assert [E.k2_plan(m)["kernel"] for m in sizes] == [LATENCY, HOME, HOME, HOME]
        E.k2_set_forms(True, False)
        assert [E.k2_plan(m)["kernel"] for m in sizes] == [LATENCY, PARKED, PARKED, PAIR + " parking=claimed"]
        T.k2_set_forms(False, False)
        assert T.k2_plan(530) == toy_plan
        E.k2_set_forms(True, True)
        assert [E.k2_plan(m) for m in sizes] == default
    finally:
        E.k2_set_forms(True, True)
        T.k2_set_forms(True, True)
        other.close()


# ---- guard rows for the ragged tiles of the other stages: device tensors padded with the sentinel on both sides, the words against
# ---- the same call through host arrays (pinned against the oracle in test_gpu_stages.py / test_gpu_aes.py) --------------------------
def test_k1_keyswitch_stays_inside_its_output(opt):
    p, E = opt.params, opt.engine()
    m = 200                                                      # four 64-ciphertext tiles, ragged last one
    x = np.random.default_rng(0x1200).integers(0, 1 << 64, (m, p.big1), dtype=np.uint64)
    want = np.zeros((m, p.n + 1), dtype=np.uint64)
    E.keyswitch_batch(x, want, m)
    buf, out = guarded(m, p.n + 1)
    E.keyswitch_batch(dev(x), out, m)
    E.synchronize()
    assert guards_intact(buf) and np.array_equal(host(out), want) and want.any()


def test_k3_pfpks_stays_inside_its_output(opt):
    p, E = opt.params, opt.engine()
    m, words = 33, (p.k + 1) * (p.k + 1) * 512                   # one ragged 128-ciphertext tile
    x = np.random.default_rng(0x3033).integers(0, 1 << 64, (m, p.big1), dtype=np.uint64)
    want = np.zeros((m, words), dtype=np.uint64)
    E.pfpks_batch(x, want, m)
    buf, out = guarded(m, words)
    E.pfpks_batch(dev(x), out, m)
    E.synchronize()
    assert guards_intact(buf) and np.array_equal(host(out), want) and want.any()


@pytest.mark.parametrize("polys", [17, 300])
def test_k4_forward_fourier_stays_inside_its_output(polys, opt):
    E = opt.engine()                                             # 16 polynomials per workgroup: 17 and 300 end in a ragged one
    x = np.random.default_rng(0x4000 + polys).integers(0, 1 << 64, (polys, 512), dtype=np.uint64)
    want = np.zeros((polys, 256, 2), dtype=np.float64)
    E.forward_fourier_batch(x, want, polys)
    buf, out = guarded(polys, 512)
    E.forward_fourier_batch(dev(x), out, polys)
    E.synchronize()
    assert guards_intact(buf) and np.array_equal(host(out), want.view(np.uint64).reshape(polys, 512)) and want.any()


def _ggsw_fourier(opt, x):
    """the engine's own K1 - K4 on LWE inputs x [inputs][bits][kN+1] -> Fourier GGSWs [inputs][bits][(k+1)^2][256][2] (host)"""
    p, E = opt.params, opt.engine()
    m, k1 = x.shape[0] * x.shape[1], p.k + 1
    small = np.zeros((m, p.n + 1), dtype=np.uint64)
    E.keyswitch_batch(np.ascontiguousarray(x.reshape(m, p.big1)), small, m)
    pbs = np.zeros((m, p.big1), dtype=np.uint64)
    E.cbs_pbs_batch(small, pbs, m)
    gg = np.zeros((m, k1, k1 * 512), dtype=np.uint64)
    E.pfpks_batch(pbs, gg, m)
    ff = np.zeros((m * k1 * k1, 256, 2), dtype=np.float64)
    E.forward_fourier_batch(np.ascontiguousarray(gg.reshape(-1, 512)), ff, m * k1 * k1)
    return ff.reshape(x.shape[0], x.shape[1], k1 * k1, 256, 2)


def test_k5_vertical_packing_stays_inside_its_output(opt):
    """2 inputs x 4 LUTs of 8 bits (32 instances per input against 3 per workgroup: ragged), and the add_scalar shape: 9 bits, 2 LUTs
    that differ per input (18 instances per input; the 9-iteration instance, per-input LUT indexing)"""
    from tfhe_aes_amd.server import gen_lut

    p, E, c = opt.params, opt.engine(), opt.client
    luts8 = orc.build_lutset(orc.LUTSET_DEC_MUL)
    bits9 = np.random.default_rng(95).integers(0, 2, (2, 9)).astype(np.uint8)
    luts9 = np.stack([np.stack([gen_lut(2, 1, 512, 9, lambda v, a=a: ((v & 0xFF) + (v >> 8) + a) % 256),
                                gen_lut(2, 1, 512, 9, lambda v, a=a: 1 if (v & 0xFF) + (v >> 8) + a > 255 else 0)]) for a in (0x7F, 0xF3)])
    for x, bits, luts, n_luts, per_input in ((c.encrypt_bytes([0x53, 0xE1]), 8, luts8, 4, False), (c.encrypt_bits(bits9), 9, luts9, 2, True)):
        ggsw_f = np.ascontiguousarray(_ggsw_fourier(opt, x))
        rows = 2 * n_luts * bits
        want = np.zeros((rows, p.big1), dtype=np.uint64)
        E.vertical_packing_batch(ggsw_f, 2, bits, luts, n_luts, per_input, want)
        buf, out = guarded(rows, p.big1)
        E.vertical_packing_batch(dev(ggsw_f), 2, bits, dev(luts), n_luts, per_input, out)
        E.synchronize()
        assert guards_intact(buf) and np.array_equal(host(out), want) and want.any(), bits


def test_cmux_tree_11bit_stays_inside_its_output(opt):
    """2 inputs of 11 bits, 1 LUT at k = 4: 11 instances per input are no multiple of the 3 a workgroup carries, in both tree levels and
    in the vertical packing behind them (test_gpu_aes.py pins the host call against the oracle)"""
    from tfhe_aes_amd.server import gen_lut

    p, E, c, nb = opt.params, opt.engine(), opt.client, 11
    luts = np.stack([gen_lut(2, 1, 512, nb, lambda v: (v * 37 + 5) % (1 << nb))])
    x = c.encrypt_bits(np.array([[(v >> j) & 1 for j in range(nb)] for v in (0x3A5, 0x5C2)], dtype=np.uint8))
    want = np.zeros((2 * nb, p.big1), dtype=np.uint64)
    E.wopbs_batch(x, 2, nb, luts, 1, False, want)
    buf, out = guarded(2 * nb, p.big1)
    E.wopbs_batch(dev(x), 2, nb, dev(luts), 1, False, out)
    E.synchronize()
    assert guards_intact(buf) and np.array_equal(host(out), want) and want.any()


# ---- the CMUX tree at k = 4, word for word against the oracle ----------------------------------------------------------------------------
# cmux_level_kernel<5,15,3> at every depth the product uses: a job is (instance, node), a workgroup carries R = 3 of them, an inner
# level reads ((inst * 2 nodes_out + 2 node) * K1 + p) * N of one half of ws_tree and writes the other, and the root is handed to
# vertical_packing_kernel<5,15,3> from the half the last level wrote.  Two inputs per case, chosen so that together they take both
# branches at every tree level; Engine.wopbs_batch on device tensors inside guard rows; every word against opt.oracle.wopbs_batch.
def _random_table_lut(width, seed):
    from tfhe_aes_amd.server import gen_lut

    table = np.random.default_rng(seed).integers(0, 1 << width, 1 << width)
    return table, gen_lut(2, 1, 512, width, lambda v: int(table[v]))


def _cmux_tree_case(opt, width, vals, luts, per_input, fs):
    """luts [n_sets][n_luts][width][2^width]; fs[set][lut]: the clear functions.  Returns the engine's words [2][n_luts][width][kN+1]."""
    p, E, c = opt.params, opt.engine(), opt.client
    high = ((1 << width) - 1) & ~0x1FF
    assert (vals[0] ^ vals[1]) & high == high                              # the two inputs differ in every bit that drives a tree level
    n_luts = luts.shape[1]
    x = c.encrypt_bits(np.array([[(v >> j) & 1 for j in range(width)] for v in vals], dtype=np.uint8))
    rows = 2 * n_luts * width
    buf, out = guarded(rows, p.big1)
    E.wopbs_batch(dev(x), 2, width, dev(luts if per_input else luts[0]), n_luts, per_input, out)
    E.synchronize()
    got = host(out).reshape(2, n_luts, width, p.big1)
    assert guards_intact(buf)
    want = opt.oracle.wopbs_batch(x, luts if per_input else luts[0], lut_per_input=per_input)
    diff = np.argwhere((got != want).any(axis=-1))
    assert diff.size == 0, "%d words differ, first at (input, LUT, output bit) %s" % (int((got != want).sum()), diff[0].tolist())
    dec = c.decrypt_bits(got)
    for i, v in enumerate(vals):
        for li in range(n_luts):
            assert int(sum(int(dec[i, li, j]) << j for j in range(width))) == fs[i if per_input else 0][li](v), (v, li)
    return got


# width, n_luts, per input, the two inputs.  Jobs per input and level: 12 bits 48, 24, 12 (whole workgroups, root in half 0); with two
# LUTs 96, 48, 24 and the leaves read set = input; 13 bits 104, 52, 26, 13 (ragged at every level, root in half 1); 16 bits 1,024 ..
# 16 over 7 levels, all ragged, root in half 0.
@pytest.mark.parametrize("width,n_luts,per_input,vals", [(12, 1, False, (0xBA5, 0x5C2)), (12, 2, True, (0x3A5, 0xDC2)), (13, 1, False, (0x15A5, 0x0BC2)),
                                                         (16, 1, False, (0xA5A5, 0x5BC2))])
def test_cmux_tree_at_k4_is_the_oracle(opt, width, n_luts, per_input, vals):
    sets = []
    for s in range(2 if per_input else 1):
        sets.append([_random_table_lut(width, 0x7EE0 + 64 * width + 8 * s + li) for li in range(n_luts)])
    luts = np.stack([np.stack([lut for _, lut in one]) for one in sets])
    for one in sets:
        for table, _ in one:
            assert all(len(set(((table >> j) & 1).tolist())) == 2 for j in range(width))       # no constant output row
    fs = [[lambda v, t=table: int(t[v]) for table, _ in one] for one in sets]
    got = _cmux_tree_case(opt, width, vals, luts, per_input, fs)
    assert got.any(axis=-1).all()


def test_cmux_tree_16bit_tag_lut_at_k4_is_the_oracle(opt):
    """the engine's own 16-bit LUT (tag_check_dev's second WoPBS: input == 0) on 0 and 0xFFFF, branch 0 and branch 1 at all 7 levels,
    the verdicts 1 and 0.  Output rows 1..15 of that LUT are constant zero: their ciphertexts are exact zero words."""
    import ccm

    eq0 = ccm.tag_luts()[1]
    assert eq0.shape == (16, 1 << 16) and eq0[0].any() and not eq0[1:].any()
    got = _cmux_tree_case(opt, 16, (0, 0xFFFF), eq0[None, None], False, [[lambda v: int(v == 0)]])
    assert got[:, 0, 0].any(axis=-1).all() and not got[:, 0, 1:].any()
