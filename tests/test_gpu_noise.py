"""The HIP kernels against the noise budget (tests/noise_model.py), stage by stage and at both parameter sets: the k = 1 and k = 4
kernels are different templates.  The parity tests compare the kernels with the oracle word for word, and the oracle evaluates the same
expression tree; what a flaw the two share cannot leave alone is the noise.  Every case measures an error as a signed integer and hands
it to noise_model.assert_noise with the variance the model derives from the parameter set -- nothing here is compared with the oracle,
and no bound comes from what the kernels give.  test_noise_model_cpu.py asserts for every sample count used here that the band rejects
a doubled variance, and holds the oracle to the same model.

The sweeps are also the exhaustive table check of the engine's own LUT sets (host_tables.h::build_lutset_host): all 256 byte values
through LUTSET_SBOX, LUTSET_INV_SBOX, LUTSET_ENC_ROUND and LUTSET_DEC_MUL, decrypted and compared with aes_clear.  LUTSET_IDENTITY and
LUTSET_DEC_EQ_ROUND have no call of their own: the identity set is covered through the key expansion of one AES-256 key (163 of the
256 byte values, the most a clear search over 30,000 keys found), the equivalent-inverse set through one decryption of 16 blocks whose
round inputs hold all 256 values (asserted below)."""
import numpy as np
import pytest

import noise_model as nm
from aes_vectors import F1_KEY, F1_PT, block_bytes, key_words
from gpu_support import dev, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.server import gen_lut

pytestmark = pytest.mark.gpu

BOTH = pytest.mark.parametrize("which", ["toy", "opt"])
_models = {}


def model_of(kit):
    if kit.params.name not in _models:
        _models[kit.params.name] = nm.NoiseModel.of_client(kit.client)
    return _models[kit.params.name]


def _kit(request, which):
    kit = request.getfixturevalue(which)
    return kit, request.getfixturevalue(which + "_server"), request.getfixturevalue(which[0] + "c"), model_of(kit)


# ---- K1, K2, K3 ---------------------------------------------------------------------------------------------------------------------------
@BOTH
def test_k1(which, request):
    kit, _, c, M = _kit(request, which)
    p, m = kit.params, 4096
    x = c.encrypt_bits(np.random.default_rng(0x4B1).integers(0, 2, m).astype(np.uint8))
    out = np.zeros((m, p.n + 1), dtype=np.uint64)
    kit.engine().keyswitch_batch(x, out, m)
    _, ph_in = c.decrypt_bits(x, return_phase=True)
    assert nm.rejects_doubling(m)
    nm.assert_noise(nm.signed(c.phase_small(out) - ph_in), M.k1(), m, "K1 " + which)


def k2_outputs(kit, c, M, m, seed):
    """m honest small-key inputs (K1's and the modulus switch's noise from the model) through K2: (bits, outputs, rows to keep).  A row
    whose input phase lies within 6 sigma of the modulus switch from a decision boundary (2^62 either side of the message) is left out
    of the statistics, though not of the launch; with the model's noise that share is far below the 1 % asserted."""
    p = kit.params
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, m).astype(np.uint8)
    small, _ = nm.small_lwe(c.lwe_sk, bits, M.k1() + M.modswitch(), rng)
    off = nm.signed(c.phase_small(small) - (bits.astype(np.uint64) << np.uint64(63))).astype(np.float64)
    keep = 2.0 ** 62 - np.abs(off) >= 6.0 * np.sqrt(M.modswitch())
    assert (~keep).sum() <= m // 100, "%d of %d rows within 6 sigma of a decision boundary" % ((~keep).sum(), m)
    out = np.zeros((m, p.big1), dtype=np.uint64)
    kit.engine().cbs_pbs_batch(small, out, m)
    return bits, out, keep


@pytest.mark.parametrize("which,m", [("opt", 2100), ("toy", 300)])
def test_k2(which, m, request):
    """PARAM_OPT, 2,100 rows: two full generations of the paired kernel, every unit shape (test_gpu_k2_shapes.py names them)"""
    kit, _, c, M = _kit(request, which)
    bits, out, keep = k2_outputs(kit, c, M, m, 0x4B2)
    _, ph = c.decrypt_bits(out, return_phase=True)
    err = nm.signed(ph - (bits.astype(np.uint64) << np.uint64(64 - kit.params.cbs_base_log)))[keep]
    assert nm.rejects_doubling(err.size)
    nm.assert_noise(err, M.k2(), err.size, "K2 " + which)


@BOTH
def test_k3(which, request):
    kit, _, c, M = _kit(request, which)
    p, m = kit.params, 64
    bits, x, keep = k2_outputs(kit, c, M, m, 0x4B3)
    assert keep.all()
    out = np.zeros((m, p.k + 1, (p.k + 1) * p.N), dtype=np.uint64)
    kit.engine().pfpks_batch(x, out, m)
    e_k0, e_k, e_set, e_clear = nm.k3_errors(c, out, bits)
    assert nm.rejects_doubling(m)
    nm.assert_noise(e_k0, M.k3(p.k, 1), m, "K3 %s row k, coefficient 0" % which)
    nm.assert_noise(e_k, M.k3(p.k, 0), m, "K3 %s row k, other coefficients" % which)
    nm.assert_noise(e_set, M.k3(0, 1), m, "K3 %s rows j < k, key bit 1" % which)
    nm.assert_noise(e_clear, M.k3(0, 0), m, "K3 %s rows j < k, key bit 0" % which)


# ---- the WoPBS: every byte value through every exposed LUT set ----------------------------------------------------------------------------
S, IS, MUL = aes_clear.SBOX, aes_clear.INV_SBOX, aes_clear.gf_mul
SWEEPS = {
    "sbox": (False, False, [lambda x: S[x]]),
    "inv sbox": (True, False, [lambda x: IS[x]]),
    "many_sbox": (False, True, [lambda x, m=m: MUL(S[x], m) for m in (1, 2, 3)]),
    "many_sbox inv": (True, True, [lambda x, m=m: MUL(x, m) for m in (9, 11, 13, 14)]),
}


@BOTH
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_wopbs_sweep(which, name, request):
    kit, srv, c, M = _kit(request, which)
    inv, many, fs = SWEEPS[name]
    x = c.encrypt_bytes(np.arange(256))
    out = srv.many_sbox(x, inv=inv) if many else srv.sbox(x, inv=inv)[:, None]
    err, vals = nm.wopbs_error(c, out)
    assert vals.tolist() == [[f(v) for f in fs] for v in range(256)]
    n = M.wopbs_independent(256, 8)                                                    # 2,048 at PARAM_TOY, 256 at PARAM_OPT
    assert nm.rejects_doubling(n)
    nm.assert_noise(err, M.wopbs(8, np.arange(256))[:, None, None], n, "WoPBS %s, %s" % (which, name), left_out=M.wopbs_left_out())


def wide_outputs(srv, c, width, inputs, table=None, lut=None):
    """`inputs` values of `width` bits, 0 and 2^width - 1 among them, through one LUT: a random table whose every output row is
    non-constant (the default), or `lut` with its clear `table`: (errors [inputs][1][width], the inputs, the output words)"""
    rng = np.random.default_rng(width)
    if lut is None:
        table = rng.integers(0, 1 << width, 1 << width)
        lut = gen_lut(2, 1, 512, width, lambda v: int(table[v]))
    vals = rng.integers(0, 1 << width, inputs)
    vals[:2] = (0, (1 << width) - 1)
    bits = ((vals[:, None] >> np.arange(width)) & 1).astype(np.uint8)
    out = srv.many_wopbs_without_padding(c.encrypt_bits(bits), [lut])
    err, got = nm.wopbs_error(c, out)
    assert got[:, 0].tolist() == np.asarray(table)[vals].tolist()
    return err, vals, out


@pytest.mark.parametrize("width", [10, 12])
def test_wide_inputs(toy, toy_server, tc, width):
    """wider than log2 N: the CMUXes of the tree count, and the CMUX on the trivial LUT polynomials is the tree's first"""
    M = model_of(toy)
    err, vals, _ = wide_outputs(toy_server, tc, width, 32)
    n = M.wopbs_independent(32, width, width)
    assert n == 32 * width and nm.rejects_doubling(n)
    nm.assert_noise(err, M.wopbs(width, vals)[:, None, None], n, "WoPBS toy, %d bits" % width, left_out=M.wopbs_left_out())


@pytest.mark.parametrize("width", [10, 12, 16])
def test_wide_inputs_param_opt(opt, opt_server, oc, width):
    """The same at PARAM_OPT (cmux_level_kernel<5,15,3>), up to the 16 bits of the tag check: 64 inputs, all output rows of a random
    table.  The outputs of one input share its GGSWs, so the inputs are counted.  At 16 bits the 64 inputs need 2.7 GB of tree and the
    engine cuts the call at its 2 GiB bound: two chunks."""
    M = model_of(opt)
    err, vals, _ = wide_outputs(opt_server, oc, width, 64)
    n = M.wopbs_independent(64, width, width)
    assert n == 64 and err.shape == (64, 1, width) and nm.rejects_doubling(n)
    nm.assert_noise(err, M.wopbs(width, vals)[:, None, None], n, "WoPBS opt, %d bits" % width, left_out=M.wopbs_left_out())


def test_tag_lut_row_0_param_opt(opt, opt_server, oc):
    """The verdict of a tag check: output row 0 of the engine's 16-bit LUT (input == 0), the one term a gate's circuit bootstrap decides
    on.  Rows 1..15 of that LUT are constant zero, come out as exact zero ciphertexts and sit outside the model (NoiseModel.wopbs)."""
    import ccm

    M = model_of(opt)
    eq0 = ccm.tag_luts()[1]
    table = np.zeros(1 << 16, dtype=np.int64)
    table[0] = 1
    err, vals, out = wide_outputs(opt_server, oc, 16, 64, table=table, lut=eq0)
    assert out[:, :, 0].any(axis=-1).all() and not out[:, :, 1:].any()
    n = M.wopbs_independent(64, 1, 16)
    assert n == 64 and nm.rejects_doubling(n)
    nm.assert_noise(err[:, :, :1], M.wopbs(16, vals)[:, None, None], n, "WoPBS opt, tag LUT row 0", left_out=M.wopbs_left_out())


# ---- AES ----------------------------------------------------------------------------------------------------------------------------------
def test_aes_output_param_opt(opt, opt_server, oc, opt_rk128):
    """four blocks under the resident round keys: every output word is a two-term sum, a fresh S-Box output and a word of the last round
    key, which the four blocks share -- 128 independent sums of the second kind, the count the band is taken from"""
    M = model_of(opt)
    d_st = dev(np.stack([oc.encrypt_u128(v) for v in F1_PT]))
    opt_server.aes_encrypt(opt_rk128, d_st)
    opt_server.synchronize()
    out = host(d_st)
    want = [aes_clear.aes_encrypt_block(F1_KEY, v) for v in F1_PT]
    assert np.array_equal(oc.decrypt_bytes(out), block_bytes(want))
    err, _ = nm.wopbs_error(oc, out)
    # the two constants the other PARAM_OPT tests ask for, beside the derived ones
    assert np.abs(err).max() < 1 << 59, "max |noise| = 2^%.1f" % np.log2(float(np.abs(err).max()))
    assert np.abs(err).std() < 1 << 56
    assert nm.rejects_doubling(128)
    nm.assert_noise(err, nm.aes_output_variance(M, F1_KEY, want), 128, "AES output opt", left_out=2 * M.wopbs_left_out())


# AES-256: 208 expanded bytes, each the output of an identity WoPBS on its own value; 163 distinct values
KEY_256 = bytes.fromhex("17a56e720a5d2ac022f623e99f220e932ae16d4a6c3f97e4d0e05c7951ed820d")


@BOTH
def test_identity_set_through_the_key_expansion(which, request):
    kit, srv, c, M = _kit(request, which)
    want = key_words(aes_clear.expand_key(KEY_256))                                    # [15][16]
    assert len(set(want[2:].reshape(-1).tolist())) == 163
    rk = srv.aes_key_expansion(c.encrypt_aes_key(KEY_256))
    assert np.array_equal(c.decrypt_bytes(rk), want)
    err, _ = nm.wopbs_error(c, rk[2:])                                                 # rk[0], rk[1] are the key's own ciphertexts
    var = M.wopbs(8, want[2:].astype(np.int64))[:, :, None]
    n = M.wopbs_independent(208, 8)
    assert nm.rejects_doubling(n)
    nm.assert_noise(err, var, n, "key expansion " + which, left_out=M.wopbs_left_out())


def eq_inverse_round_inputs(key, ct):
    """the states FIPS-197 Fig. 15 hands to the rounds Nr-1 .. 1 (the equivalent-inverse LUT set's inputs), and the final round's"""
    dw = aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(key))
    nr = len(dw) - 1
    s = [a ^ b for a, b in zip(aes_clear._state(ct), dw[nr])]
    seen = []
    for rnd in range(nr - 1, 0, -1):
        seen.append(list(s))
        s = aes_clear._mix(aes_clear._inv_shift_rows([IS[b] for b in s]), (14, 11, 13, 9))
        s = [a ^ b for a, b in zip(s, dw[rnd])]
    return seen, s


def eq_inverse_blocks():
    """16 ciphertext blocks whose equivalent-inverse round inputs hold all 256 byte values, by clear search over random blocks"""
    for seed in range(64):
        rng = np.random.default_rng(0xE9 + seed)
        blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(16)]
        values = {b for ct in blocks for st in eq_inverse_round_inputs(F1_KEY, ct)[0] for b in st}
        if len(values) == 256:
            return blocks
    raise AssertionError("no 16 blocks found")


@BOTH
def test_equivalent_inverse_set_through_one_decryption(which, request):
    kit, srv, c, M = _kit(request, which)
    blocks = eq_inverse_blocks()
    pts = [aes_clear.aes_decrypt_block(F1_KEY, ct) for ct in blocks]
    assert [aes_clear.aes_decrypt_block_equivalent(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(F1_KEY)), ct) for ct in blocks] == pts
    rk = request.getfixturevalue("opt_rk128") if which == "opt" else dev(srv.aes_key_expansion(c.encrypt_aes_key(F1_KEY)))
    dw = srv.aes_decryption_round_keys(rk)
    d_st = dev(np.stack([c.encrypt_u128(ct) for ct in blocks]))
    srv.aes_decrypt_equivalent(dw, d_st)
    srv.synchronize()
    out = host(d_st)
    assert np.array_equal(c.decrypt_bytes(out), block_bytes(pts))
    # the last round: InvShiftRows(InvSubBytes) + w[0], and w[0] is the key's own ciphertext: one fresh WoPBS output per word, whose
    # input byte at the output's position p is SBOX[pt_p ^ key_p]
    last = np.array([[S[a ^ b] for a, b in zip(aes_clear._state(pt), F1_KEY)] for pt in pts], dtype=np.int64)
    assert all(aes_clear._inv_shift_rows(eq_inverse_round_inputs(F1_KEY, ct)[1]) == row.tolist() for ct, row in zip(blocks, last))
    err, _ = nm.wopbs_error(c, out)
    n = M.wopbs_independent(16 * 16, 8)
    assert nm.rejects_doubling(n)
    nm.assert_noise(err, M.wopbs(8, last)[:, :, None], n, "equivalent inverse " + which, left_out=M.wopbs_left_out())
