"""Every kernel of the hot path on the edge words of edge_words.py, word for word.

The other GPU tests feed the kernels honest ciphertexts or uniform random words, which reach the ties and the wrap of the modulus
switch, an all-zero row of switched masks, the ties of the back-conversion to the torus, a balanced-byte carry through all eight
bytes or an int32 accumulator near its bound with probability 2^-11 .. 2^-54 per word, or never.  Here those words are the input.
test_edge_words_cpu.py has pinned the oracle against plain references on the same sets and asserted what the sets contain; this
file compares the kernels with the oracle on all rows, and with the plain references where they give a whole output.

K2 runs at PARAM_EDGE (edge_words.py: the <5,5,8,...> kernels of PARAM_OPT on n = 24) under three bootstrapping keys, and every
edge row passes through each of the seven kernel bodies in every slot of a unit; every case asserts the plan and the kernel name
first, as test_gpu_k2_shapes.py does.  Engines with crafted keys are made here and closed when the module ends.

Wall time on an MI355X (pytest --durations=0): see DESIGN.md section 5, "Edge words under test".
"""
import numpy as np
import pytest

import edge_words as ew
from edge_words import PARAM_EDGE
from gpu_support import FORMS, HOME, LATENCY, PAIR, PARKED, dev, filled, guarded, guards_intact, host, plan_tuple, settled
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_TOY, _native

pytestmark = pytest.mark.gpu

# (body, forms, m, plan at 256 CUs, kernel, ciphertexts per unit): one unit size per launch, so that row j sits in slot j mod unit
K2_BODIES = [
    ("latency", "default", 256, (0, 256, 1, 0, 0), LATENCY, 1),
    ("home-2", "default", 512, (1, 0, 3, 256, 2), HOME, 2),
    ("home-3", "default", 768, (1, 256, 3, 0, 2), HOME, 3),
    ("parked-2", "home denied", 512, (1, 0, 3, 256, 2), PARKED, 2),
    ("parked-3", "both denied", 768, (1, 256, 3, 0, 2), PARKED, 3),
    ("pair-4", "default", 1024, (2, 0, 6, 256, 4), PAIR, 4),
    ("pair-6", "default", 1536, (2, 256, 6, 0, 4), PAIR, 6),
]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- engines ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_engine():
    """a PARAM_EDGE context and zero KSK / PFPKSK on the device (K2 needs keys uploaded, not these two: 630 MB that never cross PCIe)"""
    p = PARAM_EDGE
    E = _native.Engine(p, device=0)
    zeros = filled((p.ksk_words,), 0), filled((p.pfpksk_words,), 0)
    yield E, zeros
    E.close()


@pytest.fixture(scope="module")
def toy_engine():
    E = _native.Engine(PARAM_TOY, device=0)
    yield E
    E.close()


class K2Edge:
    """the K2 edge rows, one bootstrapping key on the engine, and the oracle's output for every row (host and device)"""

    def __init__(self, kind, E, zeros):
        p = PARAM_EDGE
        rng = np.random.default_rng(0xB5C)
        self.kind, self.E, self.s = kind, E, None
        if kind == "trivial":
            self.s = rng.integers(0, 2, p.n, dtype=np.uint64)
            bsk = ew.trivial_bsk(self.s, p)
        elif kind == "random":
            bsk = rng.integers(0, 1 << 64, p.bsk_words, dtype=np.uint64)
        else:
            bsk = np.array([0, 1, ew.M64, 1 << 63, (1 << 63) - 1], dtype=np.uint64)[rng.integers(0, 5, p.bsk_words)]
        self.x, _ = ew.k2_rows(p.n)
        self.rows = self.x.shape[0]
        assert self.rows % 12 == 0                                   # a cyclic shift keeps every row's slot residue for units of 2, 3, 4, 6
        E.upload_keys(zeros[0], dev(bsk), zeros[1])
        oracle = orc.Oracle(p, np.zeros(1, dtype=np.uint64), bsk, np.zeros(1, dtype=np.uint64))
        self.want = oracle.cbs_pbs(self.x)
        self.x_d, self.want_d = dev(self.x), dev(self.want)


@pytest.fixture(scope="module", params=["trivial", "random", "extreme"])
def k2edge(request, edge_engine):
    return K2Edge(request.param, *edge_engine)


# ---- K2 ----------------------------------------------------------------------------------------------------------------------------
def test_k2_trivial_key_reference_is_the_closed_form(k2edge):
    """under the noise-free key the oracle's rows are the closed form of edge_words.blind_rotation_trivial; under the other two keys
    the outputs are not degenerate (no all-zero mask)"""
    p = PARAM_EDGE
    if k2edge.kind == "trivial":
        assert np.array_equal(k2edge.want, ew.blind_rotation_trivial(k2edge.x, k2edge.s, p))
    else:
        assert np.count_nonzero(k2edge.want[:, :p.big].any(axis=1)) > k2edge.rows // 2


@pytest.mark.parametrize("body,forms,m,plan,kernel,unit", K2_BODIES, ids=[c[0] for c in K2_BODIES])
def test_k2_edge_rows_through_every_kernel_body(body, forms, m, plan, kernel, unit, k2edge):
    """launches of m cyclically consecutive edge rows starting at i m - o, for every o < unit: every edge row passes through this
    body in every slot of a unit (the first and the last among them), into guarded output rows, against the oracle on all rows"""
    import torch

    p, E, n_rows = PARAM_EDGE, k2edge.E, k2edge.rows
    seen = np.zeros((n_rows, unit), dtype=bool)
    try:
        E.k2_set_forms(*FORMS[forms])
        pl = E.k2_plan(m)
        assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl                # the launch this case exists for
        for o in range(unit):
            for i in range(-(-n_rows // m)):
                idx = (np.arange(m) + i * m - o) % n_rows
                idx_d = dev(idx)
                buf, out = guarded(m, p.big1)
                rows_d = settled(k2edge.x_d[idx_d].contiguous())
                E.cbs_pbs_batch(rows_d, out, m)
                E.synchronize()
                assert guards_intact(buf), "a store outside the %d output rows" % m
                if not torch.equal(out, k2edge.want_d[idx_d]):
                    bad = torch.nonzero((out != k2edge.want_d[idx_d]).any(dim=1)).flatten().cpu().numpy()
                    raise AssertionError("%s key, %s, offset %d, launch %d: %d of %d rows differ from the oracle, edge rows %s ..."
                                         % (k2edge.kind, body, o, i, len(bad), m, idx[bad[:16]]))
                seen[idx, np.arange(m) % unit] = True
    finally:
        E.k2_set_forms(True, True)
    assert seen.all()


def test_k2_edge_rows_on_the_toy_kernels(toy_engine):
    """the same rows (PARAM_TOY has the same n) through the k = 1 kernels under a key of random words, in one launch"""
    p, E = PARAM_TOY, toy_engine
    rng = np.random.default_rng(0x701)
    x, _ = ew.k2_rows(p.n)
    m = x.shape[0]
    ksk, pf = np.zeros(p.ksk_words, dtype=np.uint64), np.zeros(p.pfpksk_words, dtype=np.uint64)
    bsk = rng.integers(0, 1 << 64, p.bsk_words, dtype=np.uint64)
    E.upload_keys(ksk, bsk, pf)
    pl = E.k2_plan(m)
    assert pl["kernel"].startswith("blind_rotate16_kernel<2,5,8,8") and plan_tuple(pl) == (1, m // 8, 8, 0, 0), pl
    buf, out = guarded(m, p.big1)
    x_d = dev(x)                                                # named: alive until the context's stream is done with it
    E.cbs_pbs_batch(x_d, out, m)
    E.synchronize()
    want = orc.Oracle(p, ksk, bsk, pf).cbs_pbs(x)
    got = host(out)
    assert guards_intact(buf)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:16]


# ---- K1 / K3 -----------------------------------------------------------------------------------------------------------------------
def _plain_rows(p, stage, m):
    """4 rows for the plain reference: the first full row, the last full row, the first mixed row, the last row of the ragged tile"""
    full = len(ew.ks_words(p, stage))
    return [0, full - 1, full, m - 1]


@pytest.mark.parametrize("pattern", ew.KEY_PATTERNS)
def test_key_switches_toy_edge_inputs_and_keys(pattern, toy_engine):
    """m = 130: two 128-ciphertext workgroup tiles, the second one ragged.  All rows against the oracle, 4 against the plain product"""
    p, E, m = PARAM_TOY, toy_engine, 130
    ksk = ew.key_words(pattern, (p.big, p.ks_level, p.n + 1))
    pf = ew.key_words(pattern, (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8)
    bsk = np.zeros(p.bsk_words, dtype=np.uint64)
    E.upload_keys(ksk, bsk, pf)
    o = orc.Oracle(p, ksk, bsk, pf)
    x1, _ = ew.ks_inputs(p, "K1", m)
    x3, _ = ew.ks_inputs(p, "K3", m)
    x1_d, x3_d = dev(x1), dev(x3)
    buf1, out1 = guarded(m, p.n + 1)
    buf3, out3 = guarded(m, (p.k + 1) ** 2 * p.N)
    E.keyswitch_batch(x1_d, out1, m)
    E.pfpks_batch(x3_d, out3, m)
    E.synchronize()
    got1, got3 = host(out1), host(out3).reshape(m, p.k + 1, (p.k + 1) * p.N)
    assert guards_intact(buf1) and guards_intact(buf3)
    want1, want3 = o.keyswitch(x1), o.pfpks(x3)
    assert np.array_equal(got1, want1), np.flatnonzero((got1 != want1).any(axis=1))[:16]
    assert np.array_equal(got3, want3), np.flatnonzero((got3 != want3).any(axis=(1, 2)))[:16]
    r1, r3 = _plain_rows(p, "K1", m), _plain_rows(p, "K3", m)
    assert np.array_equal(got1[r1], ew.keyswitch_plain(x1[r1], ksk, p))
    assert np.array_equal(got3[r3], ew.pfpks_plain(x3[r3], pf, p))


def test_key_switches_k4_edge_inputs_mixture_keys():
    """k = 4, the mixture keys, m = 20, against the oracle (one 630 MB PFPKSK, uploaded once: the longest case of this file)"""
    p, m = PARAM_EDGE, 20
    ksk = ew.key_words("mixture", (p.big, p.ks_level, p.n + 1))
    pf = ew.key_words("mixture", (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8)
    bsk = np.zeros(p.bsk_words, dtype=np.uint64)
    x1, _ = ew.ks_inputs(p, "K1", m)
    x3, _ = ew.ks_inputs(p, "K3", m)
    E = _native.Engine(p, device=0)
    try:
        E.upload_keys(ksk, bsk, pf)
        x1_d, x3_d = dev(x1), dev(x3)
        buf1, out1 = guarded(m, p.n + 1)
        buf3, out3 = guarded(m, (p.k + 1) ** 2 * p.N)
        E.keyswitch_batch(x1_d, out1, m)
        E.pfpks_batch(x3_d, out3, m)
        E.synchronize()
        got1, got3 = host(out1), host(out3).reshape(m, p.k + 1, (p.k + 1) * p.N)
        assert guards_intact(buf1) and guards_intact(buf3)
    finally:
        E.close()
    o = orc.Oracle(p, ksk, bsk, pf)
    want1, want3 = o.keyswitch(x1), o.pfpks(x3)
    assert np.array_equal(got1, want1), np.flatnonzero((got1 != want1).any(axis=1))[:16]
    assert np.array_equal(got3, want3), np.flatnonzero((got3 != want3).any(axis=(1, 2)))[:16]


# ---- K4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 1])
def test_k4_edge_polynomials(k, edge_engine, toy_engine):
    E = edge_engine[0] if k == 4 else toy_engine
    x, _ = ew.k4_polys()
    buf, out = guarded(x.shape[0], 512)
    x_d = dev(x)
    E.forward_fourier_batch(x_d, out, x.shape[0])
    E.synchronize()
    want = orc.polys_to_fourier(x)
    assert guards_intact(buf)
    got = host(out)
    assert np.array_equal(got, _bits(want).reshape(x.shape[0], 512)), np.flatnonzero((got != _bits(want).reshape(x.shape[0], 512)).any(axis=1))


# ---- K5 / CMUX -----------------------------------------------------------------------------------------------------------------------
def _vp_oracle(p, ggsw_f, luts, per_input):
    bits = ggsw_f.shape[1]
    return np.stack([orc.vertical_packing(p, ggsw_f[i], bits, luts[i if per_input else 0]) for i in range(ggsw_f.shape[0])])


def _vp_engine(E, p, ggsw_f, luts, n_luts, per_input):
    n_inputs, bits = ggsw_f.shape[0], ggsw_f.shape[1]
    rows = n_inputs * n_luts * bits
    buf, out = guarded(rows, p.big1)
    ggsw_d, luts_d = dev(_bits(ggsw_f)), dev(luts)
    E.vertical_packing_batch(ggsw_d, n_inputs, bits, luts_d, n_luts, per_input, out)
    E.synchronize()
    assert guards_intact(buf)
    return host(out).reshape(n_inputs, n_luts, bits, p.big1)


@pytest.mark.parametrize("k", [4, 1])
def test_cmux_constant_spectrum_against_exact_rounding(k, edge_engine, toy_engine):
    """3 inputs x 2 LUTs of 10 bits with a LUT set per input: 20 instances per input against 3 (k = 4) or 8 (k = 1) per workgroup
    leave a ragged unit in the tree level and in the packing behind it.  Against torus_round (exact) and against the oracle"""
    E, p = (edge_engine[0], PARAM_EDGE) if k == 4 else (toy_engine, PARAM_TOY)
    for off in ew.CMUX_OFFSETS[k]:
        (ggsw_f, luts, want), _ = ew.cmux_constant_family(p, 3, 2, off)
        got = _vp_engine(E, p, ggsw_f, luts, 2, True)
        assert np.array_equal(got, want), (off, np.argwhere(got != want)[:8])
        assert np.array_equal(got, _vp_oracle(p, ggsw_f, luts, True)), off


@pytest.mark.parametrize("bits", [1, 9, 11])
@pytest.mark.parametrize("k", [4, 1])
def test_cmux_generic_spectra_against_the_oracle(k, bits, edge_engine, toy_engine):
    """spectra of +0.0, -0.0, +-2^63 and honest-scale values per entry; 11 bits has two tree levels, the inner one reads the outer's"""
    E, p = (edge_engine[0], PARAM_EDGE) if k == 4 else (toy_engine, PARAM_TOY)
    (ggsw_f, luts), _ = ew.cmux_generic_family(p, 3, 2, bits)
    got = _vp_engine(E, p, ggsw_f, luts, 2, False)
    want = _vp_oracle(p, ggsw_f, luts[None], False)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
