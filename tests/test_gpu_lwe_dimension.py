"""The lwe_dimension range fheaes_create accepts: 1 <= n <= 4096 with k in {1, 4}.  The other tests run n = 24 and n = 669.

What depends on n is the tiling and pipeline edge code: K1's column tiling (ncols = n + 1, 16 columns a tile, 4 tiles a workgroup,
the clamp of a tile beyond the last, the body column n), the ragged last ChaCha20 block of a KSK mask row in the seeded upload, the
blind rotations' fetches one iteration ahead (the next mask word, the key rows of iteration it + 1) where n is smaller than the
pipeline is deep, and at the top the raw-buffer descriptor of the Fourier bootstrapping key, (int)(n x GGSW bytes): 2,097,152,000 bytes
at k = 4 and n = 4096, 50,331,648 short of 2^31.

  k = 1, honest keys, n in {1, 2, 15, 16, 63, 64}: ncols 2, 3, 16, 17, 64, 65 = 1, 1, 1, 2, 4, 5 column tiles (one tile only; ncols a
     multiple of 16; a tile count that is a multiple of 4; at 65 a second workgroup whose only real column is the body column).  K1,
     the seeded upload, K2 in both of its forms, and many_sbox against the oracle and the S-Box.
  k = 4, n in {1, 2}: K2 in the latency form, the 16-form and the paired form, under a key of random words, against the oracle.
  k = 4, n = 4096: K2 in the three forms under the noise-free key of edge_words.trivial_bsk, made on the device; the corner rows against
     the closed form, all rows against the latency form.
The parameter sets that are refused are test_limits_cpu.py's.  Parameter sets are made with dataclasses.replace, as PARAM_EDGE is.
Wall time: DESIGN.md section 5, "Limits under test".
"""
import dataclasses

import numpy as np
import pytest

import edge_words as ew
from gpu_support import HOME, LATENCY, PAIR, dev, filled, guarded, guards_intact, host, plan_tuple, settled, unit_rows
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native, aes_clear
from tfhe_aes_amd.client import Client

pytestmark = pytest.mark.gpu

SMALL_N = [1, 2, 15, 16, 63, 64]
COLTILES = {1: 1, 2: 1, 15: 1, 16: 2, 63: 4, 64: 5}
LATENCY_K1, FORM16_K1 = "blind_rotate_latency_kernel<2,5,8>", "blind_rotate16_kernel<2,5,8,8"
# m -> (plan at 256 CUs, kernel) at k = 4: the latency form, two-ciphertext 16-form units, four-ciphertext paired units
K4_LAUNCHES = {7: ((0, 7, 1, 0, 0), LATENCY), 300: ((1, 0, 3, 150, 2), HOME), 800: ((2, 0, 6, 200, 4), PAIR)}


def _k2_inputs(n, m, seed=0):
    """m rows of the K2 edge set at this n, taken with a stride so that every class of it is among them"""
    x, _ = ew.k2_rows(n)
    return np.ascontiguousarray(x[(np.arange(m) * 7 + seed) % x.shape[0]])


# ---- k = 1, honest keys --------------------------------------------------------------------------------------------------------------------
class SmallKit:
    def __init__(self, n):
        self.p = p = dataclasses.replace(PARAM_TOY, name="PARAM_TOY_N%d" % n, lwe_dimension=n)
        self.client = Client(1, 0, 0, params=p, seed=0x1D1 + n)
        self.keys = self.client.server_keys()
        self.oracle = orc.Oracle(p, self.keys.ksk, self.keys.bsk, self.keys.pfpksk)
        self.E = _native.Engine(p, device=0)
        self.E.upload_keys(self.keys.ksk, self.keys.bsk, self.keys.pfpksk)


@pytest.fixture(scope="module", params=SMALL_N, ids=["n=%d" % n for n in SMALL_N])
def small(request):
    kit = SmallKit(request.param)
    yield kit
    kit.E.close()


def test_k1_column_tiling(small):
    """m = 130: two 128-ciphertext workgroups, the second ragged.  Every word against the oracle, 8 rows against the plain product"""
    p, E, m = small.p, small.E, 130
    assert (p.n + 1 + 15) // 16 == COLTILES[p.n]
    x = np.random.default_rng(0xC01 + p.n).integers(0, 1 << 64, (m, p.big1), dtype=np.uint64)
    x[:4] = small.client.encrypt_bits([0, 1, 1, 0])
    buf, out = guarded(m, p.n + 1)
    x_d = dev(x)
    E.keyswitch_batch(x_d, out, m)
    E.synchronize()
    got, want = host(out), small.oracle.keyswitch(x)
    assert guards_intact(buf)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    rows = [0, 1, 63, 64, 127, 128, 129, 3]
    assert np.array_equal(got[rows], ew.keyswitch_plain(x[rows], small.keys.ksk, p))


def test_seeded_upload_is_the_plain_upload(small):
    """a KSK mask row has n words: it ends inside a ChaCha20 block of 8 words for n = 1, 2, 15, 63 and on a block boundary for 16, 64"""
    p = small.p
    assert (p.n % 8 == 0) == (p.n in (16, 64))
    sk = small.keys.compress()
    E = _native.Engine(p, device=0)
    try:
        E.upload_keys_seeded(sk.mask_seed, sk.ksk_body, sk.bsk_body, sk.pfpksk_body)
        for i in {0, p.n - 1}:
            assert np.array_equal(E.read_bsk_fourier(i).view(np.uint64), small.E.read_bsk_fourier(i).view(np.uint64)), i
        m = 19
        x = np.random.default_rng(0x5EED + p.n).integers(0, 1 << 64, (m, p.big1), dtype=np.uint64)
        for call, words in (("keyswitch_batch", p.n + 1), ("pfpks_batch", (p.k + 1) ** 2 * p.N)):
            a, b = np.zeros((m, words), dtype=np.uint64), np.zeros((m, words), dtype=np.uint64)
            getattr(E, call)(x, a, m)
            getattr(small.E, call)(x, b, m)
            assert np.array_equal(a, b) and a.any(), call
    finally:
        E.close()


@pytest.mark.parametrize("m", [1, 21, 300])
def test_k2_both_forms_at_small_n(small, m):
    """the latency form (m = 1, 21) and the 16-form (m = 300, 38 units of 8, the last ragged): every word against the oracle"""
    p, E = small.p, small.E
    pl = E.k2_plan(m)
    assert pl["kernel"].startswith(LATENCY_K1 if m <= 256 else FORM16_K1) and plan_tuple(pl) == ((0, m, 1, 0, 0) if m <= 256 else (1, 38, 8, 0, 0)), pl
    x = _k2_inputs(p.n, m, m)
    buf, out = guarded(m, p.big1)
    x_d = dev(x)
    E.cbs_pbs_batch(x_d, out, m)
    E.synchronize()
    got, want = host(out), small.oracle.cbs_pbs(x)
    assert guards_intact(buf)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:16]
    assert np.count_nonzero(want[:, :p.big].any(axis=1)) > m // 2            # honest key: no degenerate outputs


def test_many_sbox_at_small_n(small):
    p, E = small.p, small.E
    vals = [0x53, 0xA7]
    ct = small.client.encrypt_bytes(vals)
    got = np.zeros((2, 3, 8, p.big1), dtype=np.uint64)
    E.many_sbox(ct, 2, False, got)
    want = small.oracle.wopbs_batch(ct, orc.build_lutset(orc.LUTSET_ENC_ROUND))
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    dec = small.client.decrypt_bytes(got)
    for i, v in enumerate(vals):
        s = aes_clear.SBOX[v]
        assert list(dec[i]) == [s, aes_clear.mul2(s), aes_clear.mul3(s)]


# ---- k = 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zero_pfpksk():
    """630 MB of zeros on the device for the three k = 4 contexts of this file (K2 needs keys uploaded, not this one)"""
    return filled((PARAM_OPT.pfpksk_words,), 0)


@pytest.mark.parametrize("n", [1, 2])
def test_k2_three_forms_at_k_4_and_tiny_n(n, zero_pfpksk):
    """the fetches that run ahead of the loop have nothing to fetch: iteration it + 1 of 1 or 2 does not exist after the first or second"""
    p = dataclasses.replace(PARAM_OPT, name="PARAM_OPT_N%d" % n, lwe_dimension=n)
    rng = np.random.default_rng(0xB5C + n)
    bsk = rng.integers(0, 1 << 64, p.bsk_words, dtype=np.uint64)
    oracle = orc.Oracle(p, np.zeros(1, dtype=np.uint64), bsk, np.zeros(1, dtype=np.uint64))
    E = _native.Engine(p, device=0)
    try:
        E.upload_keys(filled((p.ksk_words,), 0), dev(bsk), zero_pfpksk)
        for m, (plan, kernel) in K4_LAUNCHES.items():
            pl = E.k2_plan(m)
            assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl
            x = _k2_inputs(n, m, m)
            buf, out = guarded(m, p.big1)
            x_d = dev(x)
            E.cbs_pbs_batch(x_d, out, m)
            E.synchronize()
            got, want = host(out), oracle.cbs_pbs(x)
            assert guards_intact(buf), m
            assert np.array_equal(got, want), (m, np.flatnonzero((got != want).any(axis=1))[:16])
            assert np.count_nonzero(want[:, :p.big].any(axis=1)) > m // 2
    finally:
        E.close()


def _trivial_bsk_on_device(s, p):
    """edge_words.trivial_bsk(s, p) without the host array (2.1 GB at n = 4096)"""
    import torch

    bsk = torch.zeros((p.n, p.pbs_level, p.k + 1, p.k + 1, p.N), dtype=torch.int64, device="cuda")
    s_d = dev(np.asarray(s, dtype=np.uint64))
    for l in range(p.pbs_level):
        bsk[:, l, p.k, p.k, 0] = s_d << (64 - p.pbs_base_log * (l + 1))
    return settled(bsk)


def test_trivial_bsk_on_device_is_edge_words():
    p = dataclasses.replace(PARAM_OPT, lwe_dimension=5)
    s = [1, 0, 1, 1, 0]
    assert np.array_equal(host(_trivial_bsk_on_device(s, p)), ew.trivial_bsk(s, p))


def test_k2_at_the_top_of_the_range(zero_pfpksk):
    """n = 4096 at k = 4: the Fourier bootstrapping key is one raw buffer of 2,097,152,000 bytes.  The secret bits of the first and of the
    last GGSW are 1, so that both ends of the image are read and count.  Corner rows of every launch against the closed form, all rows
    against the same rows through the latency form in slices of 256"""
    import torch

    p = dataclasses.replace(PARAM_OPT, name="PARAM_OPT_N4096", lwe_dimension=4096)
    rng = np.random.default_rng(0x4096)
    s = rng.integers(0, 2, p.n, dtype=np.uint64)
    s[0] = s[-1] = 1
    E = _native.Engine(p, device=0)
    try:
        assert E.key_words(1) * 8 == 2_097_152_000 == (1 << 31) - 50_331_648
        bsk = _trivial_bsk_on_device(s, p)
        E.upload_keys(filled((p.ksk_words,), 0), bsk.view(-1), zero_pfpksk)
        E.synchronize()
        del bsk
        torch.cuda.empty_cache()
        first, last = E.read_bsk_fourier(0), E.read_bsk_fourier(p.n - 1)
        assert first.any() and np.array_equal(first.view(np.uint64), last.view(np.uint64))      # the same bit under the same key
        for m, (plan, kernel) in K4_LAUNCHES.items():
            pl = E.k2_plan(m)
            assert plan_tuple(pl) == plan and pl["kernel"].startswith(kernel), pl
            x = rng.integers(0, 1 << 64, (m, p.n + 1), dtype=np.uint64)
            x[m - 1, :p.n] = 0                                               # the last row: the body alone decides, whatever s is
            x[0, 1:p.n - 1] = 0                                              # the first row: the first and the last GGSW alone
            buf, out = guarded(m, p.big1)
            x_d = dev(x)
            E.cbs_pbs_batch(x_d, out, m)
            E.synchronize()
            assert guards_intact(buf), m
            units = {0, pl["units_main"] + pl["units_tail"] - 1}
            rows = sorted({i for u in units for i in unit_rows(plan, u, m)})
            assert rows[0] == 0 and rows[-1] == m - 1 and len(rows) <= 12
            got = host(out[dev(np.array(rows))])
            want = ew.blind_rotation_trivial(x[rows], s, p)
            assert np.array_equal(got, want), (m, [rows[i] for i in np.flatnonzero((got != want).any(axis=1))])
            for lo in range(0, m, 256):
                n_rows = min(256, m - lo)
                assert E.k2_plan(n_rows)["kernel"].startswith(LATENCY)
                buf2, again = guarded(n_rows, p.big1)
                E.cbs_pbs_batch(settled(x_d[lo:lo + n_rows]), again, n_rows)
                E.synchronize()
                assert guards_intact(buf2)
                if not torch.equal(out[lo:lo + n_rows], again):
                    bad = torch.nonzero((out[lo:lo + n_rows] != again).any(dim=1)).flatten().cpu().numpy() + lo
                    raise AssertionError("m = %d: rows %s differ from the latency form" % (m, bad[:16]))
    finally:
        E.close()
