"""fheaes_pack_bits / fheaes_unpack_bits on the MI355X.  Every word comparison is exact (array_equal): the reference is built from what
existed before -- the oracle's packing key switch under key block k, a numpy fold, a numpy sample extraction (aes_model.py) --
and u64 wrapping sums give the same words in any order.  Then the round trip through the engine's own entry points at PARAM_OPT: a
128-block aes_ctr packed and decrypted, unpacked bytes through the S-Box, a block through aes_ctr, pack, unpack and the equivalent
inverse cipher; several contexts; host arrays against resident tensors; a reservation that forces chunks; the errors."""
import math

import numpy as np
import pytest

from aes_model import added_error, pack_sigma, ref_fold, ref_ks, ref_unpack
from aes_vectors import BASE, F1_PT, F5, MASK128
from gpu_support import dev, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes
from tfhe_aes_amd.server import ServerGroup

pytestmark = pytest.mark.gpu

TOY_M = (1, 7, 512, 513, 1541)
OPT_M = (513, 1100)


def _cases(kit, client, sizes, seed):
    """m -> (bits, their encryptions, the reference packing), all cut from ONE reference run over max(sizes) bits where that is the same
    thing: GLWE g of a packing depends on bits gN .. gN + N - 1 alone, so only a partly filled last GLWE needs a fold of its own"""
    top = max(sizes)
    bits = np.random.default_rng(seed).integers(0, 2, top).astype(np.uint8)
    lwe = client.encrypt_bits(bits)
    ks = ref_ks(kit, lwe)
    return {m: (bits[:m], lwe[:m], ref_fold(ks[:m], kit.params)) for m in sizes}


@pytest.fixture(scope="module")
def toy_cases(toy, tc):
    return _cases(toy, tc, TOY_M, 0x7AC)


@pytest.fixture(scope="module")
def opt_cases(opt, oc):
    return _cases(opt, oc, OPT_M, 0x0AC)


# ---- the words ------------------------------------------------------------------------------------------------------------------------------
def _check_pack_and_unpack(kit, server, client, cases, m):
    p = kit.params
    bits, lwe, want = cases[m]
    got = server.pack(lwe)
    assert got.dtype == np.uint64 and got.shape == ((m + p.N - 1) // p.N, (p.k + 1) * p.N) and got.size == server.engine.packed_words(m)
    assert np.array_equal(got, want), "%d packed words differ" % int((got != want).sum())
    assert np.array_equal(client.decrypt_packed(got, m), bits)
    back = server.unpack(got, m)
    assert back.shape == (m, p.big1)
    want_lwe = ref_unpack(want, m, p)
    assert np.array_equal(back, want_lwe), "%d unpacked words differ" % int((back != want_lwe).sum())
    assert np.array_equal(client.decrypt_bits(back), bits)


@pytest.mark.parametrize("m", TOY_M)
def test_toy_words_are_the_reference(toy, toy_server, tc, toy_cases, m):
    _check_pack_and_unpack(toy, toy_server, tc, toy_cases, m)


@pytest.mark.parametrize("m", OPT_M)
def test_param_opt_words_are_the_reference(opt, opt_server, oc, opt_cases, m):
    _check_pack_and_unpack(opt, opt_server, oc, opt_cases, m)


def test_shapes_follow_the_input(toy, toy_server, tc, toy_cases):
    """any [..., kN+1] array packs as its flattened bits; unpack gives the shape asked for"""
    _, lwe, want = toy_cases[1541]
    p = toy.params
    got = toy_server.pack(lwe[:1536].reshape(12, 16, 8, p.big1))
    assert np.array_equal(got, want[:3])
    assert toy_server.unpack(got, (12, 16, 8)).shape == (12, 16, 8, p.big1)
    assert np.array_equal(toy_server.unpack(got, (12, 16, 8)).reshape(-1, p.big1), ref_unpack(want, 1536, p))
    assert toy_server.pack(lwe[:0]).shape == (0, (p.k + 1) * p.N) and toy_server.unpack(got[:0], 0).shape == (0, p.big1)
    with pytest.raises(ValueError):
        toy_server.pack(lwe[:, :-1])
    with pytest.raises(ValueError):
        toy_server.unpack(got, 1537)


@pytest.mark.parametrize("which", ["toy", "opt"])
def test_host_arrays_and_resident_tensors_agree(toy, opt, toy_server, opt_server, toy_cases, opt_cases, which):
    server, cases, m = (toy_server, toy_cases, 1541) if which == "toy" else (opt_server, opt_cases, 513)
    _, lwe, want = cases[m]
    d_packed = server.pack(dev(lwe))
    d_back = server.unpack(d_packed, m)
    server.synchronize()
    assert d_packed.is_cuda and d_back.is_cuda
    assert np.array_equal(host(d_packed), want)
    assert np.array_equal(host(d_back), server.unpack(want, m))


def test_a_small_reservation_forces_chunks_and_the_words_stay(toy, toy_cases):
    """fheaes_reserve(256) sizes K3's workspace for 256 bits; a GGSW level is k+1 = 2 GLWEs per bit at PARAM_TOY, so packing finds room for
    one chunk of 512 bits and takes 1,541 bits in four: four launches of the matrix product, the same words"""
    _, lwe, want = toy_cases[1541]
    eng = _native.Engine(toy.params, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        eng.reserve(256)
        got = np.empty_like(want)
        eng.profile_reset()
        eng.pack_bits(lwe, 1541, got)
        prof = eng.profile_read()
        assert prof["pfpks"]["launches"] == 4 and prof["pfpks"]["units"] == 1541
        assert prof["linear"]["launches"] == 4 and prof["linear"]["units"] == 1541
        assert np.array_equal(got, want)
    finally:
        eng.close()


def test_server_group_of_two_contexts_gives_the_words_of_one(toy, toy_server, toy_cases):
    _, lwe, want = toy_cases[1541]
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        got = group.pack(lwe)
        assert np.array_equal(got, want)
        assert np.array_equal(group.unpack(got, 1541), toy_server.unpack(want, 1541))
        d_got = group.pack(dev(lwe[:512]))                           # one GLWE: the second context has nothing to do
        assert np.array_equal(host(d_got), want[:1])
    finally:
        for s in group.servers:
            s.engine.close()


# ---- PARAM_OPT, end to end ---------------------------------------------------------------------------------------------------------------
def test_param_opt_a_128_block_ctr_output_packs_into_32_glwes(opt, opt_server, opt_rk128, oc):
    """16,384 bits, the output of aes_ctr on 128 blocks with data: 268.6 MB become 655,360 bytes that decrypt to the AES-CTR plaintext,
    with an added error within 8 sigma of the parameter set's prediction, and the words are those of packing the 32 slices separately"""
    p, key, n = opt.params, F5[128][0], 128
    data = [(F1_PT[i % 4] + (i << 64)) & MASK128 for i in range(n)]
    d_ct = opt_server.aes_ctr(opt_rk128, BASE, 0, n, data=data)
    d_packed = opt_server.pack(d_ct)
    d_slices = [opt_server.pack(d_ct.reshape(-1, p.big1)[512 * g:512 * g + 512]) for g in range(32)]
    opt_server.synchronize()
    packed, ct = host(d_packed), host(d_ct)
    assert ct.nbytes == 268566528 and packed.nbytes == 655360 and packed.shape == (32, 2560)
    want = b"".join((k ^ d).to_bytes(16, "big") for k, d in zip(aes_clear.ctr_keystream(key, BASE, 0, n), data))
    assert oc.decrypt_packed_bytes(packed, 16 * n).tobytes() == want
    err = added_error(oc, packed, ct)
    sigma = pack_sigma(p)
    print("pack, 16,384 bits at PARAM_OPT: added error std 2^%.2f, max 2^%.2f = %.2f sigma (sigma 2^%.2f)" % (
        math.log2(err.std()), math.log2(np.abs(err).max()), np.abs(err).max() / sigma, math.log2(sigma)))
    assert np.abs(err).max() <= 8 * sigma
    assert np.array_equal(np.concatenate([host(s) for s in d_slices]), packed)


def test_param_opt_unpacked_bytes_are_valid_sbox_inputs(opt, opt_server, oc):
    vals = np.random.default_rng(0x5B0).integers(0, 256, 64).astype(np.uint8)
    ct = oc.encrypt_bytes(vals)
    back = opt_server.unpack(opt_server.pack(ct), (64, 8))
    assert np.array_equal(oc.decrypt_bytes(back), vals)
    out = opt_server.sbox(back, inv=False)
    assert np.array_equal(oc.decrypt_bytes(out), np.array([aes_clear.SBOX[v] for v in vals], dtype=np.uint8))


def test_param_opt_ctr_pack_unpack_then_the_equivalent_inverse_cipher(opt, opt_server, opt_rk128, oc):
    key = F5[128][0]
    d_ct = opt_server.aes_ctr(opt_rk128, BASE | 0x42, 0, 1, data=[F1_PT[2]])
    d_state = opt_server.unpack(opt_server.pack(d_ct), (1, 16, 8))
    d_dw = opt_server.aes_decryption_round_keys(opt_rk128)
    opt_server.aes_decrypt_equivalent(d_dw, d_state)
    opt_server.synchronize()
    block = aes_clear.ctr_keystream(key, BASE | 0x42, 0, 1)[0] ^ F1_PT[2]
    assert np.array_equal(oc.decrypt_bytes(host(d_ct))[0], np.array(u128_to_bytes(block), dtype=np.uint8))
    want = aes_clear.aes_decrypt_block(key, block)
    assert np.array_equal(oc.decrypt_bytes(host(d_state))[0], np.array(u128_to_bytes(want), dtype=np.uint8))


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors(toy, toy_cases):
    p = toy.params
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    _, lwe, _ = toy_cases[513]
    gw = (p.k + 1) * p.N
    for ms in (_native.HOST, _native.DEVICE):
        # overlapping buffers: one array, the other argument inside it
        buf = np.zeros(513 * p.big1 + 2 * gw, dtype=np.uint64)
        base = buf.ctypes.data
        assert lib.fheaes_pack_bits(h, base, 513, base + 8 * 100, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_pack_bits(h, base + 8 * gw, 513, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_unpack_bits(h, base, 513, base + 8 * (2 * gw - 1), ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_unpack_bits(h, base + 8 * 10, 513, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert not buf.any()
        # null pointers
        assert lib.fheaes_pack_bits(h, None, 1, base, ms) == -1 and lib.fheaes_pack_bits(h, base, 1, None, ms) == -1
        assert lib.fheaes_unpack_bits(h, None, 1, base, ms) == -1 and lib.fheaes_unpack_bits(h, base, 1, None, ms) == -1
        # m = 0 is fine and writes nothing
        out = np.full(gw, 0x5A5A, dtype=np.uint64)
        assert lib.fheaes_pack_bits(h, lwe.ctypes.data, 0, out.ctypes.data, ms) == 0
        assert lib.fheaes_unpack_bits(h, lwe.ctypes.data, 0, out.ctypes.data, ms) == 0
        assert (out == 0x5A5A).all()
    assert eng.packed_words(0) == 0 and eng.packed_words(1) == gw and eng.packed_words(512) == gw and eng.packed_words(513) == 2 * gw
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.pack_bits(lwe, 513, np.empty((2, gw), dtype=np.uint64))
        assert e.value.code == -2
        packed = np.arange(2 * gw, dtype=np.uint64).reshape(2, gw)            # unpacking needs no keys
        out = np.empty((513, p.big1), dtype=np.uint64)
        fresh.unpack_bits(packed, 513, out)
        assert np.array_equal(out, ref_unpack(packed, 513, p))
    finally:
        fresh.close()
