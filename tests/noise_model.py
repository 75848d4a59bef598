"""The noise budget of every stage of a WoPBS, from the parameter set -- and the one checker the noise tests share.

Every GPU parity test compares the kernels with oracle/fheaes_oracle.c word for word, and the oracle evaluates the same expression tree:
a flaw the two share (a gadget rule that drops a level, a level order read backwards, a transform that loses more bits than believed, a
biased modulus switch) leaves those tests green.  What such a flaw cannot leave alone is the noise.  This module predicts the variance of
every stage from first principles; test_noise_model_cpu.py holds the oracle to it, test_gpu_noise.py the HIP kernels.  A plain module like
edge_words.py: imported by name, not collected.

Inputs of the model: a WopbsParameters; the Hamming weights of the kit's two secret keys (the real ones, not n/2); the moments E[d],
E[d^2] of the digits of the two decomposition rules, taken by enumeration or sampling from the plain references edge_words.decompose /
edge_words.decompose_offset (B^2/12 is not taken on trust: at ks_base_log = 2 the second moment is about 1.3 and differs by level); and the
ONE measured input, the error of the f64 transform: orc.negacyclic_mul_fft against the exact schoolbook product orc.negacyclic_mul_exact
with digits drawn from each gadget's range (the kernels produce the transform's product bit for bit, so its error is theirs).

Units: every variance is in (2^-64)^2, i.e. of the error as a signed 64-bit integer.  sigma_x = x_noise_std 2^64; R = 64 - level base_log
of the gadget in question is the number of low bits a decomposition rounds away; a rounded word's error is uniform over 2^R values,
variance 2^(2R)/12.  h_small / h_big are the Hamming weights of the LWE key and of the GLWE key (all k polynomials together)."""
import functools
import math

import numpy as np

import edge_words as ew


# ---- inputs: digit moments and the transform's error ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def digit_moments(rule, base_log, level):
    """(E[d_l], E[d_l^2]) for l = 0 .. level-1 (index 0 = the most significant level) of a uniform torus word under rule "signed"
    (edge_words.decompose: K1, K3) or "offset" (edge_words.decompose_offset: the external products).  The digits depend on the top
    level base_log + 1 bits only (the last of them is the rounding bit): up to 17 such bits every value is enumerated, so the moments
    are exact; beyond that 2^16 uniform words are sampled (fixed seed; the relative error of E[d^2] is then below 0.4 %)."""
    fn = {"signed": ew.decompose, "offset": ew.decompose_offset}[rule]
    top = base_log * level + 1
    if top <= 17:
        words = [i << (64 - top) for i in range(1 << top)]
    else:
        words = np.random.default_rng(0xD161 + 64 * base_log + level).integers(0, 1 << 64, 1 << 16, dtype=np.uint64).tolist()
    d = np.array([fn(int(w), base_log, level) for w in words], dtype=np.float64)
    return tuple(d.mean(axis=0)), tuple((d * d).mean(axis=0))


def sum_d2(rule, base_log, level):
    """sum over the levels of E[d_l^2]"""
    return float(sum(digit_moments(rule, base_log, level)[1]))


@functools.lru_cache(maxsize=None)
def fft_variance(base_log, products=384, seed=0xFF7):
    """v_fft(B): the per-coefficient variance of (f64 transform product - exact product) of one digit polynomial, digits uniform in
    [-B/2, B/2), with one uniform torus polynomial of N = 512 coefficients.  MEASURED, not derived: the oracle's transform against its
    exact schoolbook product (about 2^43.4 for B = 2^8 and 2^57.4 for B = 2^15: std 2^21.7 and 2^28.7)."""
    from oracle import oracle as orc

    rng = np.random.default_rng(seed + base_log)
    half = 1 << (base_log - 1)
    acc = 0.0
    for _ in range(products):
        d = rng.integers(-half, half, 512, dtype=np.int64)
        t = rng.integers(0, 1 << 64, 512, dtype=np.uint64)
        e = (orc.negacyclic_mul_fft(d, t) - orc.negacyclic_mul_exact(d, t)).view(np.int64).astype(np.float64)
        acc += float((e * e).mean())
    return acc / products


@functools.lru_cache(maxsize=None)
def fft_chain_variance(k, base_log, level, chains=48, seed=0xC4A1):
    """v_chain(B, T): the per-coefficient variance of one output column of an external product against the exact value, T = (k+1) level
    products accumulated in the Fourier domain and transformed back once -- what the kernels do.  MEASURED like fft_variance, through
    orc.external_product_add on uniform rows and a uniform GLWE, against T exact schoolbook products of the plain rule's digits.
    It is NOT T v_fft: the pointwise multiply-accumulate is one sequential fma chain per point, every step rounds the running sum, and
    the sum grows, so the chain's error exceeds that of T separate products by about 1.5 % per term (4 % at T = 2, 15 % at T = 10,
    38 % at T = 25); test_noise_model_cpu.py pins those ratios.
    Returns (v_chain, a).  The error is white across coefficients but for its lowest frequencies, where the transform's twiddles are
    exact or nearly so: a = E[(sum_j +-e_j)^2] / (N v_chain), the signs those of a negacyclic product with the all-ones polynomial, is
    about 0.75 instead of 1.  It matters because a binary key polynomial is its mean h/N plus a zero-mean part (see extprod)."""
    import dataclasses

    from oracle import oracle as orc
    from tfhe_aes_amd import PARAM_TOY

    p = dataclasses.replace(PARAM_TOY, glwe_dimension=k)                        # the oracle reads k and N of it only
    k1 = k + 1
    rng = np.random.default_rng(seed + 64 * base_log + 8 * level + k)
    acc, low = 0.0, 0.0
    for _ in range(chains):
        rows = rng.integers(0, 1 << 64, (level, k1, k1, 512), dtype=np.uint64)
        lam = rng.integers(0, 1 << 64, (k1, 512), dtype=np.uint64)
        got = orc.external_product_add(p, level, base_log, rows, lam, np.zeros_like(lam)).reshape(k1, 512)
        d = offset_digits(lam, base_log, level)
        exact = np.zeros((k1, 512), dtype=np.uint64)
        with np.errstate(over="ignore"):
            for l in range(level):
                for r in range(k1):
                    for c in range(k1):
                        exact[c] += orc.negacyclic_mul_exact(d[l, r], rows[l, r, c])
        e = (got - exact).view(np.int64).astype(np.float64)
        acc += float((e * e).mean())
        ones = 2.0 * np.cumsum(e, axis=1) - e.sum(axis=1, keepdims=True)         # (e * (1 + X + ... + X^(N-1)))[c] = sum_{j<=c} e_j - sum_{j>c} e_j
        low += float((ones * ones).mean()) / 512
    return acc / chains, low / acc


def rounding_variance(R):
    """a word rounded to its closest multiple of 2^R: the error is uniform over 2^R consecutive integers"""
    return 2.0 ** (2 * R) / 12.0


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
class NoiseModel:
    """The variance of every stage for one parameter set and one pair of secret keys.  `h_polys`: the Hamming weight of each of the k
    polynomials of the GLWE key.  `v_chain_pbs` / `v_chain_cbs`: the transform's error per coefficient of one output column of an external product
    (fft_chain_variance) with the gadget of the blind rotation and of the CMUXes; measured on first use if not given."""

    def __init__(self, params, h_small, h_polys, v_chain_pbs=None, v_chain_cbs=None):
        self.p = params
        self.h_small = int(h_small)
        self.h_polys = tuple(int(h) for h in h_polys)
        assert len(self.h_polys) == params.k
        self.h_big = sum(self.h_polys)
        self._v_chain = {"pbs": v_chain_pbs, "cbs": v_chain_cbs}

    @classmethod
    def of_client(cls, client, **kw):
        p = client.params
        return cls(p, int(client.lwe_sk.sum()), client.glwe_sk.reshape(p.k, p.N).sum(axis=1), **kw)

    def v_chain(self, gadget):
        """(v_chain, a) of fft_chain_variance for this gadget"""
        if self._v_chain[gadget] is None:
            self._v_chain[gadget] = fft_chain_variance(self.p.k, *self._gadget(gadget))
        return self._v_chain[gadget]

    def _gadget(self, gadget):
        p = self.p
        return {"pbs": (p.pbs_base_log, p.pbs_level), "cbs": (p.cbs_base_log, p.cbs_level)}[gadget]

    # -- K1 --
    def k1(self):
        """phase_small(out) - phase_big(in) of the LWE key switch.  out = (0, b) - sum_{i < kN, l} d_il KSK_il, KSK_il an encryption of
        s_i 2^(64 - b(l+1)) under the small key with noise e_il of std sigma_lwe: the phase is b - sum_i s_i round(a_i) - sum d_il e_il, so
        the difference is sum_i s_i (a_i - round(a_i)) - sum_il d_il e_il:
            kN sum_l E[d_l^2] sigma_lwe^2  +  h_big 2^(2R)/12,   R = 64 - ks_level ks_base_log,   digits of the "signed" rule."""
        p = self.p
        s = p.lwe_noise_std * 2.0 ** 64
        return p.big * sum_d2("signed", p.ks_base_log, p.ks_level) * s * s + self.h_big * rounding_variance(64 - p.ks_level * p.ks_base_log)

    # -- the modulus switch in front of K2 --
    def modswitch(self):
        """K2 rounds each of the n + 1 words of its input to the closest multiple of 2^54 (2N = 1024 steps): the body's error and the
        errors of the h_small mask words that meet a key bit add up in the phase:  (1 + h_small) 2^108/12."""
        return (1 + self.h_small) * rounding_variance(54)

    # -- one external product --
    def extprod(self, s_i, gadget="pbs"):
        """The phase of GGSW(s_i) (x) Lambda minus s_i times the phase of Lambda, per coefficient.  The product is
        sum_{r <= k, l} d_rl * ROW_rl with d_rl the level-l digit polynomial of column r of Lambda and ROW_rl a GLWE encryption of
        -s_i S_r 2^(64-b(l+1)) (r < k) or s_i 2^(64-b(l+1)) (r = k) with noise polynomial e_rl of std sigma_glwe.  Its phase is
        s_i (round(B) - sum_r round(A_r) S_r) + sum_rl d_rl * e_rl + (the transform's error), hence three terms:
          key noise   (k+1) L N E[d^2] sigma_glwe^2     a coefficient of d * e sums N products; "offset" rule, every level alike
          rounding    s_i (1 + h_big) 2^(2R)/12          the body's rounding and, through S_r, h_big roundings of mask coefficients
          transform   (1 + sum_r h_r (1 - (1 - a) h_r / N)) v_chain(B, (k+1) L)
        Each output column is a chain of (k+1) L products, off by v_chain per coefficient; v_chain is (k+1) L v_fft(B) and 1 to 38 % more
        (fft_chain_variance).  The body column counts once.  A mask column's error e is multiplied by S_r = h_r/N + (S_r - h_r/N): the
        zero-mean part meets e as white noise and gives N (h_r/N)(1 - h_r/N) v_chain; the mean part gives (h_r/N)^2 times the variance
        of a signed sum of all N coefficients of e, N a v_chain with a about 0.75 (the error's lowest frequencies are weaker).  With
        a = 1 this is the (1 + h_big) v_chain of white noise; at h_r = N/2 it is an eighth less."""
        p = self.p
        b, L = self._gadget(gadget)
        s = p.glwe_noise_std * 2.0 ** 64
        d2 = sum_d2("offset", b, L)                                                          # = L E[d^2]
        return ((p.k + 1) * p.N * d2 * s * s + (1 if s_i else 0) * (1 + self.h_big) * rounding_variance(64 - b * L)
                + self.extprod_transform_term(gadget))

    def extprod_transform_term(self, gadget="pbs"):
        """the third term of extprod alone: the phase-level error of the f64 transform in one external product"""
        v, a = self.v_chain(gadget)
        return (1 + sum(h * (1 - (1 - a) * h / self.p.N) for h in self.h_polys)) * v

    # -- K2 --
    def k2(self):
        """The phase of K2's output minus bit 2^(64 - cbs_base_log): the errors of the blind rotation's external products add up
        (acc <- acc + GGSW(s_i) (x) ((X^a_i - 1) acc): an earlier error is only rotated by later steps).  Two corrections to "n times
        extprod": the first step starts from the trivial accumulator, whose difference has zero masks and a body of 0 and +-2^(64 -
        cbs_base_log) entries -- digits 0 and +-2 at one level, no rounding, so that step has 2^-10 of a generic step's key-noise
        and transform terms and no rounding term, and is counted as free; and a step whose switched mask word a_i is 0
        (probability 1/2N) is skipped.  So
            (n - 1)(1 - 1/2N) extprod(0)  +  h_small (n - 1)/n (1 + h_big) 2^(2R)/12."""
        p = self.p
        steps = (p.n - 1) * (1.0 - 1.0 / (2 * p.N))
        return steps * self.extprod(0, "pbs") + self.h_small * (p.n - 1) / p.n * (self.extprod(1, "pbs") - self.extprod(0, "pbs"))

    # -- K3 --
    def pfks(self):
        """The key-noise term of the private functional packing key switch, per coefficient of every output row:
        out_z = -sum_{i <= kN, l} d_il KEY_zil, each KEY a GLWE with fresh noise of std sigma_pfks per coefficient, "signed" digits:
            (kN + 1) sum_l E[d_l^2] sigma_pfks^2."""
        p = self.p
        s = p.pfks_noise_std * 2.0 ** 64
        return p.big1 * sum_d2("signed", p.pfks_base_log, p.pfks_level) * s * s

    def k3_carried(self):
        """W: what K3 carries of its input into the coefficients that hold the message: the input's own error (K2's) and the rounding of
        its kN + 1 words to the gadget's grid, the body once and the mask words that meet a key bit:  V_K2 + (1 + h_big) 2^(2R)/12."""
        p = self.p
        return self.k2() + (1 + self.h_big) * rounding_variance(64 - p.pfks_level * p.pfks_base_log)

    def k3(self, row, key_bit=None):
        """The rows of the circuit-bootstrapped GGSW against their messages, per coefficient.
        Row k is f(phase) = phase at coefficient 0: coefficient 0 has pfks() + k3_carried(), every other coefficient pfks() alone
        (`key_bit` = 1 / 0 selects the two; None: the mean over the row, pfks() + k3_carried() / N).
        Row j < k is -S_j(X) phase: a coefficient where S_j is 1 (`key_bit` = 1) has pfks() + k3_carried(), one where it is 0 has pfks()
        alone; None: the mean over the row, pfks() + (h_j / N) k3_carried()."""
        p = self.p
        if key_bit is not None:
            return self.pfks() + (self.k3_carried() if key_bit else 0.0)
        share = 1.0 / p.N if row == p.k else self.h_polys[row] / p.N
        return self.pfks() + share * self.k3_carried()

    # -- K5 / the WoPBS output --
    def cmux(self, bit):
        """One generic CMUX acc <- acc + GGSW(bit) (x) (X^-t acc - acc) with the circuit-bootstrapped GGSW (cbs_level rows per column):
        extprod with the rows' own errors in place of fresh key noise.  Row r's error polynomial e_r has sum_c Var e_r[c] =
        N k3(r), and a coefficient of d * e_r has variance E[d^2] times that sum:
            E[d^2] L N sum_r k3(r)  +  bit (1 + h_big) 2^(2R)/12  +  extprod's transform term at the CMUX gadget."""
        p = self.p
        b, L = self._gadget("cbs")
        rows = sum(self.k3(r) for r in range(p.k + 1))
        return (sum_d2("offset", b, L) * p.N * rows + (1 if bit else 0) * (1 + self.h_big) * rounding_variance(64 - b * L)
                + self.extprod_transform_term("cbs"))

    def first_cmux(self, width):
        """the index of the input bit whose CMUX works on the trivial LUT polynomials: bit 0 (the first blind-rotation step) up to 9 bits,
        bit 9 (the leaves of the tree) above"""
        return 0 if width <= 9 else 9

    def wopbs(self, width, x):
        """The phase of a WoPBS output minus its table bit 2^63, for an input of `width` bits of value `x` (an integer or an array).
        Every output passes width CMUXes: the blind rotation's over bits 0..8 and, above 9 bits, one per level of the tree on the path
        to the root (cmux(g, c0, c1) = c0 + g (x) (c1 - c0) has the selected branch's phase plus its own error).  The CMUX that works on
        the trivial LUT polynomials (first_cmux) is LEFT OUT: its differences are 0 or 2^63 in the body and 0 in the masks, exact on the
        gadget's grid, so it has no rounding term, and its other two terms are below wopbs_left_out().  So
            (width - 1) cmux(0)  +  popcount(x without that bit) (cmux(1) - cmux(0)).
        The result depends on x: the gadget's rounding enters only where the GGSW holds a 1.
        It holds for an output row whose table is NOT constant.  Where every entry of a row is 0 (rows 1..15 of the tag check's 16-bit
        LUT, ccm.tag_luts) all LUT polynomials are zero, every CMUX difference is zero, its digits are zero and the transform of zeros
        is zero: the output is the exact zero ciphertext, mask and body, with no error at all.  Such rows sit outside the model."""
        x = np.asarray(x, dtype=np.int64)
        keep = x & ~np.int64(1 << self.first_cmux(width))
        ones = np.zeros(x.shape, dtype=np.float64)
        for j in range(width):
            ones += (keep >> j) & 1
        out = (width - 1) * self.cmux(0) + ones * (self.cmux(1) - self.cmux(0))
        return float(out) if out.ndim == 0 else out

    def wopbs_left_out(self):
        """The bound of the term wopbs() leaves out (upper side only): the first CMUX's digits are 0 in the masks and 0 or -2^(cbs_base_log
        - 1) in the body, so its key-noise term is at most 2^(2 cbs_base_log - 2) (N pfks() + k3_carried()) -- all N digits non-zero, the
        carried error of row k's coefficient 0 met once -- and its transform term at most a generic one."""
        p = self.p
        return 2.0 ** (2 * p.cbs_base_log - 2) * (p.N * self.pfks() + self.k3_carried()) + self.extprod_transform_term("cbs")

    def wopbs_independent(self, n_inputs, outputs_per_input, width=8):
        """The count of independent errors among the WoPBS outputs of n_inputs inputs, for assert_noise.  Every output has a mask of its
        own, but the outputs of one input share its GGSWs, and the GGSWs' carried errors (one scalar per GGSW, k3_carried) set the
        size of cmux(0): given them the outputs are independent, their common variance is not.  Where cmux(0)'s share of the variance is
        below a tenth (PARAM_TOY: 3 %, the rounding term leads) the outputs count one each; above (PARAM_OPT: 64 %) only the
        inputs count."""
        shared = (width - 1) * self.cmux(0) / self.wopbs_mean(width)
        return n_inputs * (outputs_per_input if shared < 0.1 else 1)

    def wopbs_mean(self, width):
        """wopbs() averaged over uniform inputs: (width - 1) (cmux(0) + cmux(1)) / 2"""
        return (width - 1) * (self.cmux(0) + self.cmux(1)) / 2.0

    # -- the decision in front of K2 --
    def decision_margin(self, terms=5, width=8):
        """How many sigma the phase that K2 decides on lies from the decision boundary: the message sits at 0 or 2^63, the boundaries at
        +-2^62 from it, and the phase carries the `terms` WoPBS outputs the linear layers summed (MixColumns' four and the round key: the
        noise guard's limit of 5), K1's added error and the modulus switch:  2^62 / sqrt(terms wopbs_max + k1 + modswitch), with the
        largest WoPBS variance over the inputs (every GGSW bit 1)."""
        worst = self.wopbs(width, (1 << width) - 1) + self.wopbs_left_out()
        return 2.0 ** 62 / math.sqrt(terms * worst + self.k1() + self.modswitch())

    def log2_sigmas(self):
        """log2 of the standard deviation of every stage: what the closed-value test pins and DESIGN.md tabulates"""
        h = lambda v: 0.5 * math.log2(v)
        return {"k1": h(self.k1()), "modswitch": h(self.modswitch()), "extprod0": h(self.extprod(0)), "extprod1": h(self.extprod(1)),
                "k2": h(self.k2()), "pfks": h(self.pfks()), "k3_carried": h(self.k3_carried()), "cmux0": h(self.cmux(0)),
                "cmux1": h(self.cmux(1)), "wopbs8": h(self.wopbs_mean(8)), "aes_out": h(2 * self.wopbs_mean(8)),
                "wopbs16": h(self.wopbs_mean(16)), "wopbs16_x0": h(self.wopbs(16, 0))}


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def max_sigmas(n_samples):
    """t such that n P(|z| > t) < 2^-30 for n Gaussian samples, in steps of one half and not below the 8 that test_pack_cpu.py argues
    for up to 2^15 samples (8 -> 2^-34.5 at 2^15)."""
    t = 8.0
    while n_samples * math.erfc(t / math.sqrt(2.0)) >= 2.0 ** -30:
        t += 0.5
    return t


def band(n_independent):
    """the half-width of the band of mean(err^2) / variance: the mean of n squared unit Gaussians has standard deviation sqrt(2/n), and
    five of them is a sampling bound (2^-20.7 two-sided), not a tuned one"""
    return 5.0 * math.sqrt(2.0 / n_independent)


def rejects_doubling(n_independent):
    """the hard condition on every GPU case: a variance twice the model's lies outside the band"""
    return 1.0 + band(n_independent) < 2.0


def assert_noise(err, variance, n_independent, what, left_out=0.0):
    """err: the measured errors (signed integers or floats); variance: the model's, one number or an array that broadcasts against err
    (then every error is weighed by its own); n_independent: the number of ciphertexts whose errors do not share a mask -- NOT the
    coefficients of one GLWE, nor outputs that share their GGSWs; left_out: the bound of a term the model omits on purpose, which widens
    the upper side only.  Asserts |err| <= t sigma for every sample (max_sigmas) and mean(err^2 / variance) within 1 +- band; prints the
    figures first.  Returns the ratio."""
    err = np.asarray(err, dtype=np.float64)
    var = np.broadcast_to(np.asarray(variance, dtype=np.float64), err.shape)
    assert err.size and (var > 0).all()
    up = 1.0 + float(np.mean(left_out / var))                              # the omitted term adds at most this to the mean of err^2 / variance
    z = np.abs(err) / np.sqrt(var + left_out)                             # the worst sample is held to the variance with the bound added
    ratio = float(np.mean(err * err / var))
    t, w = max_sigmas(err.size), band(n_independent)
    print("%s: sigma 2^%.2f, measured rms 2^%.2f, variance ratio %.3f (band %.3f .. %.3f, %d independent), worst %.2f sigma (limit %.1f, %d samples)"
          % (what, 0.5 * math.log2(float(var.mean())), 0.5 * math.log2(float(np.mean(err * err))), ratio, 1 - w, up * (1 + w),
             n_independent, float(z.max()), t, err.size))
    assert z.max() <= t, "%s: worst error %.2f sigma, limit %.1f" % (what, float(z.max()), t)
    assert 1.0 - w <= ratio <= up * (1.0 + w), "%s: variance ratio %.3f outside %.3f .. %.3f" % (what, ratio, 1 - w, up * (1 + w))
    return ratio


# ---- helpers the noise tests share --------------------------------------------------------------------------------------------------------
def signed(words):
    """uint64 words as the signed integers they stand for on the torus"""
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)


def small_lwe(lwe_sk, bits, variance, rng):
    """honest LWE encryptions of bit 2^63 under the small key, Gaussian noise of the given variance: [m][n+1] words and the noise"""
    s = np.asarray(lwe_sk, dtype=np.uint64)
    m = len(bits)
    out = np.empty((m, s.size + 1), dtype=np.uint64)
    out[:, :s.size] = rng.integers(0, 1 << 64, (m, s.size), dtype=np.uint64)
    e = np.rint(rng.normal(0.0, math.sqrt(variance), m)).astype(np.int64)
    with np.errstate(over="ignore"):
        out[:, s.size] = (out[:, :s.size] * s).sum(axis=1, dtype=np.uint64) + (np.asarray(bits, dtype=np.uint64) << np.uint64(63)) + e.view(np.uint64)
    return out, e


def key_polys(client):
    """the GLWE key as [k][N] 0/1"""
    p = client.params
    return client.glwe_sk.reshape(p.k, p.N).astype(np.int64)


def offset_digits(x, base_log, level):
    """edge_words.decompose_offset over an array: uint64 [...] -> int64 [level][...] (index 0 = the most significant level); the CPU
    test holds it to the plain reference"""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    r = 64 - base_log * level
    with np.errstate(over="ignore"):
        z = x + np.uint64((1 << (r - 1)) if r > 0 else 0)
        for l in range(level):
            z = z + np.uint64((1 << (base_log - 1)) << (64 - base_log * (l + 1)))
    half = 1 << (base_log - 1)
    return np.stack([((z >> np.uint64(64 - base_log * (l + 1))) & np.uint64((1 << base_log) - 1)).astype(np.int64) - half
                     for l in range(level)])


def aes_output_variance(model, key, ciphertexts):
    """[n][16][1]: the variance of every word of byte p of aes_encrypt's output blocks, AES-128.  The last round is ShiftRows(S-Box WoPBS)
    + w[10], a two-term sum: a fresh S-Box output, whose input byte is INV_SBOX[ct_p ^ w10_p], and the round-key word, itself the output
    of the key expansion's identity WoPBS on the byte w10_p.  `key` as aes_clear.expand_key takes it; `ciphertexts`: the clear
    128-bit results."""
    from tfhe_aes_amd import aes_clear
    from tfhe_aes_amd.client import u128_to_bytes

    w = np.array(aes_clear.expand_key(key)[-1], dtype=np.int64)
    ct = np.array([u128_to_bytes(v) for v in ciphertexts], dtype=np.int64)
    inv = np.array(aes_clear.INV_SBOX, dtype=np.int64)
    return (model.wopbs(8, inv[ct ^ w]) + model.wopbs(8, w)[None, :])[:, :, None]


def tag_difference_variance(model, key, x, s0):
    """[16][1]: the variance of every word of byte p of X + S0 + trivial(tag), what the first WoPBS of a tag check decides on; x, s0 the
    clear 128-bit values.  X and S0 are cipher outputs under ONE key, each a fresh S-Box output plus the word of the last round key at
    its position (aes_output_variance) -- and that round-key word is the same ciphertext in both, so the sum carries its error twice:
    e_X + e_S0 + 2 e_rk, variance V_X + V_S0 + 4 V_rk.  That is the two aes_output_variance sums, which count V_rk once each, plus
    2 V_rk; the trivial tag adds nothing.  The message survives (2 bit 2^63 = 0), the doubled error does not cancel.  Returns (the
    variance, the two sums alone): the oracle leaves the band of the second at PARAM_TOY (test_noise_model_cpu.py: 1.59 over 1,024 words)."""
    from tfhe_aes_amd import aes_clear

    w = np.array(aes_clear.expand_key(key)[-1], dtype=np.int64)
    two_sums = aes_output_variance(model, key, [x])[0] + aes_output_variance(model, key, [s0])[0]
    return two_sums + 2.0 * model.wopbs(8, w)[:, None], two_sums


def k3_errors(client, ggsw_rows, bits):
    """the four classes of the circuit-bootstrapped GGSW's rows [m][k+1][(k+1)N] against their messages: (row k coefficient 0, row k
    elsewhere, rows j < k where the key polynomial is 1, where it is 0), each a flat array"""
    p = client.params
    ph = signed(client.glwe_phase(ggsw_rows)).astype(np.float64)             # [m][k+1][N]
    msg = np.asarray(bits, dtype=np.float64) * 2.0 ** (64 - p.cbs_base_log)
    S = key_polys(client)
    last = ph[:, p.k].copy()
    last[:, 0] -= msg
    low = ph[:, :p.k] + msg[:, None, None] * S[None]
    return last[:, 0], last[:, 1:].reshape(-1), low[:, S == 1].reshape(-1), low[:, S == 0].reshape(-1)


def wopbs_error(client, out):
    """phase minus the decrypted bit 2^63, and the decrypted values: out [n][L][bits][kN+1] -> (int64 of that shape, [n][L] integers)"""
    bits, ph = client.decrypt_bits(out, return_phase=True)
    vals = (bits.astype(np.int64) << np.arange(bits.shape[-1])).sum(axis=-1)
    return signed(ph - (bits.astype(np.uint64) << np.uint64(63))), vals
