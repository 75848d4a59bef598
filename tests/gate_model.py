"""The gate out = GGSW(valid) (x) ct (csrc/kern_gate.h): its reference model in numpy and the variance it adds, derived from the
parameter set through noise_model.NoiseModel.  A plain module like noise_model.py: imported by name, not collected.

The model.  An LWE ciphertext (a, b) under the big key is coefficient 0 of a GLWE: `embed` builds that GLWE (the inverse of the sample
extraction at index 0), `extract` takes coefficient 0 back out, and the gate of the LWE form is extract(GGSW (x) embed(ct)) with the
oracle's external product -- the kernel never writes the GLWE, but these are its words.  The GLWE form is the external product alone.

The variance.  GGSW(g) (x) Lambda = sum_r d_r * ROW_r with d_r the one-level digit polynomial (gadget base 2^15, "offset" rule) of
column r of Lambda and ROW_r row r of the circuit-bootstrapped GGSW, a GLWE encryption of -g S_r 2^49 (r < k) or g 2^49 (r = k) whose
error polynomial E_r the model knows after K3 (NoiseModel.k3).  Per coefficient of the phase, against g * phase(Lambda):

  digits     E[d^2] sum_r sum_c Var E_r[c] = E[d^2] N sum_r k3(r): a coefficient of d_r * E_r sums N products.  With sigma_ggsw^2 the mean
             of k3 over the rows this is (k+1) N E[d^2] sigma_ggsw^2.  LWE form: the body column of embed(ct) is b at coefficient 0 and
             zero elsewhere, and a zero word has digit 0, so row k gives E[d^2] Var E_k[0] = E[d^2] k3(k, key_bit = 1) instead of its
             N-coefficient sum: the LWE form adds LESS than the GLWE form.
  rounding   g^2 (1 + h_big) 2^(2 (64 - 15)) / 12: the body's rounding to the gadget's grid and, through S_r, that of the h_big =
             kN E[s^2] mask coefficients that meet a key bit; zero under a gate of 0.
  transform  the f64 transform's error as the model measures it for this gadget (extprod_transform_term("cbs")); taken whole for the LWE
             form too, where one of the k+1 digit polynomials is nearly empty: an over-estimate of a term that is 2^-30 of the total.

The GLWE form's sum is NoiseModel.cmux(g) term for term: a gate IS one CMUX iteration of K5 with ct0 = 0, of which every WoPBS output
carries width - 1 = 7 or more.  That is what backs "a gated ciphertext keeps the level of its input": level_ratio() below."""
import numpy as np

import noise_model as nm


# ---- the reference model --------------------------------------------------------------------------------------------------------------------
def embed(ct, k, N=512):
    """[..., kN+1] LWE ciphertexts -> [..., k+1, N] GLWEs whose coefficient 0 is that ciphertext: mask polynomial p holds a[pN] at
    coefficient 0 and -a[pN + N - j] at j = 1..N-1, the body polynomial b at coefficient 0 and zeros"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    assert ct.shape[-1] == k * N + 1
    out = np.zeros(ct.shape[:-1] + (k + 1, N), dtype=np.uint64)
    a = ct[..., :k * N].reshape(ct.shape[:-1] + (k, N))
    out[..., :k, 0] = a[..., 0]
    with np.errstate(over="ignore"):
        out[..., :k, 1:] = np.uint64(0) - a[..., :0:-1]
    out[..., k, 0] = ct[..., k * N]
    return out


def extract(glwe):
    """[..., k+1, N] GLWEs -> [..., kN+1]: the sample extraction at coefficient 0 (sample_extract_kernel's rule at i = 0)"""
    glwe = np.ascontiguousarray(glwe, dtype=np.uint64)
    k, N = glwe.shape[-2] - 1, glwe.shape[-1]
    out = np.empty(glwe.shape[:-2] + (k * N + 1,), dtype=np.uint64)
    a = out[..., :k * N].reshape(glwe.shape[:-2] + (k, N))
    a[..., 0] = glwe[..., :k, 0]
    with np.errstate(over="ignore"):
        a[..., 1:] = np.uint64(0) - glwe[..., :k, :0:-1]
    out[..., k * N] = glwe[..., k, 0]
    return out


def gate_reference(p, ggsw_std, ct, form):
    """the gate's words through the oracle: ggsw_std [k+1][k+1][N] (standard domain, one level), ct [m][kN+1] (form 0) or
    [m][(k+1)N] (form 1)"""
    from oracle import oracle as orc

    k1 = p.k + 1
    rows = np.ascontiguousarray(ggsw_std, dtype=np.uint64).reshape(1, k1, k1, p.N)
    glwes = embed(ct, p.k, p.N) if form == 0 else np.ascontiguousarray(ct, dtype=np.uint64).reshape(-1, k1, p.N)
    prod = np.stack([orc.external_product_add(p, 1, p.cbs_base_log, rows, g, np.zeros_like(g)).reshape(k1, p.N) for g in glwes])
    return extract(prod) if form == 0 else prod.reshape(-1, k1 * p.N)


# ---- the variance a gate adds ---------------------------------------------------------------------------------------------------------------
def gate_terms(model, valid, lwe_form=True):
    """(digits, rounding, transform) of the docstring above for a gate holding `valid` in {0, 1}"""
    p = model.p
    assert p.cbs_level == 1
    d2 = nm.sum_d2("offset", p.cbs_base_log, p.cbs_level)
    rows = sum(model.k3(r) for r in range(p.k)) * p.N
    rows += model.k3(p.k, key_bit=1) if lwe_form else model.k3(p.k) * p.N
    rounding = (1 if valid else 0) * (1 + model.h_big) * nm.rounding_variance(64 - p.cbs_base_log * p.cbs_level)
    return d2 * rows, rounding, model.extprod_transform_term("cbs")


def gate_variance(model, valid, lwe_form=True):
    return float(sum(gate_terms(model, valid, lwe_form)))


def gate_shared_share(model, valid, lwe_form=True):
    """the part of gate_variance that the ciphertexts of one gate share: the GGSW's carried error (NoiseModel.k3_carried, one scalar per
    circuit bootstrap) sets the size of the rows' errors where the key is 1.  Above a tenth, only the gates count as independent
    (NoiseModel.wopbs_independent's rule)."""
    p = model.p
    d2 = nm.sum_d2("offset", p.cbs_base_log, p.cbs_level)
    carried = d2 * model.k3_carried() * (model.h_big + 1)
    return carried / gate_variance(model, valid, lwe_form)


def gate_independent(model, valid, n_gates, bits_per_gate, lwe_form=True):
    return n_gates * (bits_per_gate if gate_shared_share(model, valid, lwe_form) < 0.1 else 1)


def level_ratio(model, width=8):
    """{name: ratio}: the worst gate (GLWE form, gate of 1) against one CMUX iteration of K5 and against the nominal WoPBS output"""
    worst = gate_variance(model, 1, lwe_form=False)
    return {"gate / cmux(1)": worst / model.cmux(1), "gate / wopbs": worst / model.wopbs_mean(width),
            "gate(0) / wopbs": gate_variance(model, 0, lwe_form=False) / model.wopbs_mean(width)}
