"""The gate on the MI355X (csrc/kern_gate.h).  gate_kernel alone (fheaes_gate_ggsw) word for word against the oracle's external
product on GGSWs made of random words, on random, extreme and tie inputs inside guard rows, both forms, R = 3 and R = 8; in place and
the refusals; fheaes_gate_bits and fheaes_gate_packed word for word against the four stage entry points followed by the kernel, and as
decrypted values; the chunk seam of the gates' circuit bootstrap; the noise a gate adds, held to tests/gate_model.py."""
import numpy as np
import pytest

import chunk_seams as cs
import edge_words as ew
import gate_model as gm
import noise_model as nm
from gpu_support import SENTINEL, dev, filled, guarded, guards_intact, host, oc, opt_server, settled, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native

pytestmark = pytest.mark.gpu

LWE, GLWE = _native.GATE_LWE, _native.GATE_GLWE
M64 = (1 << 64) - 1


def _kit(request, which):
    return request.getfixturevalue(which)


def _fourier(eng, p, ggsw_std):
    """[n][k+1][k+1][N] torus words -> the engine's Fourier GGSWs on the device, [n][1][k+1][k+1][256][2] (K4 needs no keys)"""
    import torch

    n, k1 = ggsw_std.shape[0], p.k + 1
    out = torch.empty((n, 1, k1, k1, 256, 2), dtype=torch.float64, device="cuda")
    eng.forward_fourier_batch(dev(ggsw_std), settled(out), n * k1 * k1)
    eng.synchronize()
    return out


def tie_words():
    """the words the one-level gadget of base 2^15 rounds at a tie (low 49 bits = 2^48) and their neighbours, at the bottom, in the
    middle and at the top of the digit range -- where the rounded digit wraps --, the negatives of all of them, the half-digit words,
    and the extremes.  The half-digit words are written out: edge_words.half_digit_words speaks of the key switches' rule, under which
    one level alone never holds -B/2 (it has no answer for level = 1); under the external products' rule the digit B/2 2^49 = 2^63 wraps
    to -B/2, and the words one rounding step to either side of it are the ones that matter."""
    h = (1 << 14) << 49
    w = [h, (h - (1 << 48)) & M64, (h - (1 << 48) - 1) & M64, (h + (1 << 48)) & M64]
    for t in (0, 1, (1 << 14) - 1, 1 << 14, (1 << 15) - 2, (1 << 15) - 1):
        for e in (-1, 0, 1):
            x = ((t << 49) + (1 << 48) + e) & M64
            w += [x, (-x) & M64]
    return sorted(set(w) | set(ew.EXTREMES))


def _inputs(p, m, form, seed):
    """[m][words] uniform rows; rows 1..4 the four extreme words as whole rows; the tie words cycled through all of row 5 and, rotated
    by one, row 6 (LWE form: mask word pN + N - j is coefficient j >= 1, where the embedding negates before the digit is taken)"""
    words = p.big1 if form == LWE else (p.k + 1) * p.N
    x = np.random.default_rng(seed).integers(0, 1 << 64, (m, words), dtype=np.uint64)
    for i, v in enumerate(ew.EXTREMES):
        x[1 + i] = v
    T = np.array(tie_words(), dtype=np.uint64)
    x[5] = T[np.arange(words) % T.size]
    x[6] = T[(np.arange(words) + 1) % T.size]
    return x


def _reference(p, ggsw_std, runs, x, form):
    out, at = [], 0
    for g, run in enumerate(runs):
        if run:
            out.append(gm.gate_reference(p, ggsw_std[g], x[at:at + run], form))
        at += run
    return np.concatenate(out)


# ---- 1. the kernel alone, bit-exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [LWE, GLWE], ids=["lwe", "glwe"])
@pytest.mark.parametrize("which,R", [("toy", 8), ("opt", 3)])
def test_kernel_is_the_oracles_external_product(request, which, R, form):
    """three gates with runs (1, R + 1, 2R - 1): a single-instance workgroup, a full one with a ragged one behind it, and a full one
    with one slot short; GGSWs of random words, so exactness does not depend on a GGSW being meaningful"""
    p = _kit(request, which).params
    assert _native.gate_plan([1], p.k)["instances_per_workgroup"] == R
    runs = [1, R + 1, 2 * R - 1]
    m, k1 = sum(runs), p.k + 1
    assert m >= 7 and _native.gate_plan(runs, p.k)["workgroups"] == 5
    rng = np.random.default_rng(0x6A7E0 + 16 * R + form)
    ggsw_std = rng.integers(0, 1 << 64, (3, k1, k1, p.N), dtype=np.uint64)
    x = _inputs(p, m, form, 0x1A7 + R + form)
    want = _reference(p, ggsw_std, runs, x, form)
    eng = _native.Engine(p, device=0)                                        # no keys: the kernel needs none
    try:
        ggswf = _fourier(eng, p, ggsw_std)
        buf, rows = guarded(m, x.shape[1])
        eng.gate_ggsw(ggswf, runs, dev(x), m, form, rows)
        eng.synchronize()
        got = host(rows)
        assert guards_intact(buf)                                            # the ragged workgroups' masked stores
        assert np.array_equal(got, want), "%d words differ, rows %s" % (int((got != want).sum()), sorted(set(np.nonzero(got != want)[0].tolist())))
        assert eng.noise_level_seen() == (0, 5)                              # ciphertexts carry no level between calls
        prof = eng.profile_read()["vertical_packing"]
        assert (prof["launches"], prof["units"]) == (1, m * (p.N if form == GLWE else 1))
        h_out = np.empty_like(x)                                             # host arrays take the staging path: the same words
        eng.gate_ggsw(ggswf.cpu().numpy(), runs, x, m, form, h_out)
        assert np.array_equal(h_out, want)
    finally:
        eng.close()


# ---- 2. in place, and the refusals ----------------------------------------------------------------------------------------------------------
def test_in_place_and_refusals(toy):
    p = toy.params
    k1, runs = p.k + 1, [0, 9, 1, 8]
    m = sum(runs)
    rng = np.random.default_rng(0x1291)
    ggsw_std = rng.integers(0, 1 << 64, (4, k1, k1, p.N), dtype=np.uint64)
    eng = _native.Engine(p, device=0)
    try:
        ggswf = _fourier(eng, p, ggsw_std)
        lib, h, D = eng._lib, eng._h, _native.DEVICE
        for form in (LWE, GLWE):
            x = _inputs(p, m, form, 0x77 + form)
            want = _reference(p, ggsw_std, runs, x, form)
            buf, rows = guarded(m, x.shape[1])
            settled(rows.copy_(dev(x)))
            eng.gate_ggsw(ggswf, runs, rows, m, form, rows)                  # out == in
            eng.synchronize()
            assert guards_intact(buf) and np.array_equal(host(rows), want), form
            h_x = x.copy()
            eng.gate_ggsw(ggswf.cpu().numpy(), runs, h_x, m, form, h_x)
            assert np.array_equal(h_x, want), form
        # refusals: nothing is launched and the output stays as it was
        x = _inputs(p, m, LWE, 0x78)
        d_x = dev(x)
        buf, rows = guarded(m + 1, p.big1)
        u64 = lambda *v: np.array(v, dtype=np.uint64).ctypes.data_as(_native._u64p)
        g, i, o = ggswf.data_ptr(), d_x.data_ptr(), rows.data_ptr()
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 7), i, m, LWE, o, D) == -1 and b"add up" in lib.fheaes_last_error(h)
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 9), i, m, LWE, o, D) == -1
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), i, m, LWE, g, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), g, m, LWE, g, D) == -1 and b"overlaps the gates" in lib.fheaes_last_error(h)
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), o, m, LWE, o + 8 * p.big1, D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), i, m, 2, o, D) == -1 and b"form" in lib.fheaes_last_error(h)
        assert lib.fheaes_gate_ggsw(h, g, 4, None, i, m, LWE, o, D) == -1
        assert lib.fheaes_gate_ggsw(h, None, 4, u64(0, 9, 1, 8), i, m, LWE, o, D) == -1
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), None, m, LWE, o, D) == -1
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 9, 1, 8), i, m, LWE, None, D) == -1
        assert lib.fheaes_gate_ggsw(h, g, 4, u64(0, 0, 0, 0), None, 0, LWE, None, D) == 0              # m == 0 is FHEAES_OK
        assert lib.fheaes_gate_ggsw(h, None, 0, None, None, 0, LWE, None, D) == 0
        # the two calls that bootstrap need evaluation keys; the kernel alone does not
        assert lib.fheaes_gate_bits(h, i, 4, u64(0, 9, 1, 8), i, m, o, D) == -2
        assert lib.fheaes_gate_packed(h, i, 4, u64(0, 9, 1, 8), i, m, o, D) == -2
        eng.synchronize()
        assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
    finally:
        eng.close()


# ---- 3. fheaes_gate_bits / fheaes_gate_packed are the four stage calls and the kernel ------------------------------------------------------------
def _bootstrap_by_stages(eng, p, d_gates):
    """fheaes_keyswitch_batch, fheaes_cbs_pbs_batch at level 1, fheaes_pfpks_batch, fheaes_forward_fourier_batch on device tensors"""
    import torch

    n, k1 = int(d_gates.shape[0]), p.k + 1
    small = torch.empty((n, p.n + 1), dtype=torch.int64, device="cuda")
    pbs = torch.empty((n, p.big1), dtype=torch.int64, device="cuda")
    rows = torch.empty((n, k1, k1 * p.N), dtype=torch.int64, device="cuda")
    ggswf = torch.empty((n, 1, k1, k1, 256, 2), dtype=torch.float64, device="cuda")
    settled(ggswf)
    eng.keyswitch_batch(d_gates, small, n)
    eng.cbs_pbs_batch(small, pbs, n, 1)
    eng.pfpks_batch(pbs, rows, n)
    eng.forward_fourier_batch(rows, ggswf, n * k1 * k1)
    eng.synchronize()
    return ggswf


@pytest.mark.parametrize("which,valid,runs", [("toy", [1, 1, 0, 1, 0], [0, 1, 8, 9, 15]), ("opt", [1, 0], [4, 4])])
def test_gate_bits_is_the_composition(request, which, valid, runs):
    kit = _kit(request, which)
    p, eng, client = kit.params, kit.engine(), request.getfixturevalue("tc" if which == "toy" else "oc")
    m = sum(runs)
    bits = (np.arange(m) % 3 != 1).astype(np.uint8)                          # 1, 0, 1, 1, 0, 1, ..: both values under gates of both values
    d_gates, d_ct = dev(client.encrypt_bits(np.array(valid, dtype=np.uint8))), dev(client.encrypt_bits(bits))
    want = filled((m, p.big1), SENTINEL)
    ggswf = _bootstrap_by_stages(eng, p, d_gates)
    eng.gate_ggsw(ggswf, runs, d_ct, m, LWE, want)
    eng.synchronize()                                                        # a device call only enqueues: the GGSWs must outlive the kernel that reads them
    buf, rows = guarded(m, p.big1)
    eng.gate_bits(d_gates, runs, d_ct, m, rows)
    eng.synchronize()
    got = host(rows)
    assert guards_intact(buf) and np.array_equal(got, host(want)), "%d words differ" % int((got != host(want)).sum())
    of_bit = np.repeat(np.array(valid, dtype=np.uint8), runs)
    assert client.decrypt_bits(got).tolist() == (bits * of_bit).tolist()
    h_out = np.empty((m, p.big1), dtype=np.uint64)                            # host arrays, and in place
    eng.gate_bits(host(d_gates), runs, host(d_ct), m, h_out)
    assert np.array_equal(h_out, got)
    eng.gate_bits(d_gates, runs, d_ct, m, d_ct)
    eng.synchronize()
    assert np.array_equal(host(d_ct), got)


def test_gate_packed_is_the_composition(toy, toy_server, tc):
    """2 GLWEs of Server.pack'ed bits under gates of 1 and 0, read back with Client.decrypt_packed"""
    p, eng = toy.params, toy_server.engine
    bits = np.random.default_rng(0x9AC).integers(0, 2, 2 * p.N).astype(np.uint8)
    packed = toy_server.pack(dev(tc.encrypt_bits(bits)))
    toy_server.synchronize()
    assert tuple(packed.shape) == (2, (p.k + 1) * p.N)
    d_gates = dev(tc.encrypt_bits(np.array([1, 0], dtype=np.uint8)))
    want = filled(packed.shape, SENTINEL)
    ggswf = _bootstrap_by_stages(eng, p, d_gates)
    eng.gate_ggsw(ggswf, [1, 1], packed, 2, GLWE, want)
    eng.synchronize()                                                        # the GGSWs must outlive the kernel that reads them
    buf, rows = guarded(2, (p.k + 1) * p.N)
    got = toy_server.gate_packed(packed, d_gates, out=rows)
    toy_server.synchronize()
    assert guards_intact(buf) and np.array_equal(host(got), host(want))
    dec = tc.decrypt_packed(host(got), 2 * p.N)
    assert dec[:p.N].tolist() == bits[:p.N].tolist() and not dec[p.N:].any()
    both = toy_server.gate_packed(packed, d_gates[:1])                        # one gate over both GLWEs, a new array
    toy_server.synchronize()
    assert np.array_equal(host(both)[0], host(got)[0]) and tc.decrypt_packed(host(both), 2 * p.N).tolist() == bits.tolist()
    with pytest.raises(ValueError):
        toy_server.gate_packed(packed, dev(tc.encrypt_bits(np.array([1, 0, 1], dtype=np.uint8))))      # 2 GLWEs under 3 gates


# ---- 4. the chunk seam of the gates' circuit bootstrap ---------------------------------------------------------------------------------------
def test_gates_beyond_one_chunk(toy, tc):
    """one gate more than the MAX_CHUNK_BITS a circuit bootstrap takes at a time, one bit each: the second chunk's one GGSW sits at the
    front of the workspace the first chunk's 32,768 have just left, and its workgroup must find it there"""
    import torch

    p, eng = toy.params, toy.engine()
    n = cs.MAX_CHUNK_BITS + 1
    valid = np.array([1, 0, 1, 1, 0, 0, 1], dtype=np.uint8)                   # period 7: gate 32,768 holds 1, gate 0 of the workspace too,
    bits = np.array([1, 1, 0, 1, 1], dtype=np.uint8)                          # gates 32,766 and 32,767 hold 1 and 0; bits of period 5
    idx = torch.arange(n, device="cuda")
    d_gates = settled(dev(tc.encrypt_bits(valid))[idx % 7].contiguous())
    d_ct = settled(dev(tc.encrypt_bits(bits))[idx % 5].contiguous())
    out = filled((n, p.big1), SENTINEL)
    eng.profile_reset()
    eng.gate_bits(d_gates, [1] * n, d_ct, n, out)
    prof = eng.profile_read()
    for stage in ("keyswitch", "blind_rotate", "pfpks", "vertical_packing"):
        assert (prof[stage]["launches"], prof[stage]["units"]) == (2, n), (stage, prof[stage])
    assert (prof["ggsw_fft"]["launches"], prof["ggsw_fft"]["units"]) == (2, n * (p.k + 1) ** 2)
    tail = slice(n - 3, n)                                                    # the last two gates of chunk 1 and the one of chunk 2, alone
    alone = filled((3, p.big1), SENTINEL)
    t_gates, t_ct = settled(d_gates[tail].contiguous()), settled(d_ct[tail].contiguous())
    eng.gate_bits(t_gates, [1, 1, 1], t_ct, 3, alone)
    eng.synchronize()
    assert np.array_equal(host(out[tail]), host(alone))
    head = filled((2, p.big1), SENTINEL)
    h_gates, h_ct = settled(d_gates[:2].contiguous()), settled(d_ct[:2].contiguous())
    eng.gate_bits(h_gates, [1, 1], h_ct, 2, head)
    eng.synchronize()
    assert np.array_equal(host(out[:2]), host(head))
    want = (valid[np.arange(n) % 7] * bits[np.arange(n) % 5])
    assert tc.decrypt_bits(host(out[n - 70:])).tolist() == want[n - 70:].tolist()
    assert not bool((out == SENTINEL).all(dim=1).any().item())                # every row was written


# ---- 5. the noise a gate adds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,gates,per_gate", [("toy", 64, 64), ("opt", 64, 8)])
def test_noise_of_a_gate_is_the_derived_one(request, which, gates, per_gate):
    """4,096 gated bits at PARAM_TOY and 512 at PARAM_OPT under gates of 1: the error against the input's own phase is held to
    gate_model.gate_variance; under gates of 0 the digit term alone (no rounding).  The ciphertexts of one gate share its GGSW's carried
    error, so where that leads the variance (gate_model.gate_shared_share) only the gates count as independent."""
    kit = _kit(request, which)
    p, eng, client = kit.params, kit.engine(), request.getfixturevalue("tc" if which == "toy" else "oc")
    model = nm.NoiseModel.of_client(kit.client)
    m = gates * per_gate
    bits = np.random.default_rng(0x901 + p.k).integers(0, 2, m).astype(np.uint8)
    ct = client.encrypt_bits(bits)
    _, ph_in = client.decrypt_bits(ct, return_phase=True)
    d_ct = dev(ct)
    for v in (1, 0):
        out = filled((m, p.big1), SENTINEL)
        d_gates = dev(client.encrypt_bits(np.full(gates, v, dtype=np.uint8)))
        eng.gate_bits(d_gates, [per_gate] * gates, d_ct, m, out)
        eng.synchronize()
        got, ph_out = client.decrypt_bits(host(out), return_phase=True)
        assert got.tolist() == (bits * v).tolist()
        digits, rounding, transform = gm.gate_terms(model, v)
        assert (rounding > 0) == (v == 1)
        n = gm.gate_independent(model, v, gates, per_gate)
        assert nm.rejects_doubling(n), (which, v, n)
        err = nm.signed(ph_out - ph_in * np.uint64(v))
        nm.assert_noise(err, digits + rounding + transform, n, "gate of %d, %s" % (v, which))
