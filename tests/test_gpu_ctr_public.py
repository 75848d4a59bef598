"""Public blocks and CTR with a public nonce on the MI355X (fheaes_aes_encrypt_public_bits, fheaes_aes_ctr_bits): word for word against
Server.aes_encrypt on Client.trivial_bytes of the same blocks -- the parent's entry point is the reference, so every comparison is
array_equal --, the work really saved (blind-rotation units against fheaes_aes_public_plan), SP 800-38A F.5 end to end at PARAM_OPT,
128 consecutive counters at PARAM_OPT, several contexts, and the errors."""
from fractions import Fraction

import numpy as np
import pytest

from aes_model import noise
from aes_vectors import BASE, F1_PT, F5, F5_CTR, MASK128, NR, block_bytes, counters
from gpu_support import dev, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

_rng = np.random.default_rng(0x9B1C)
CASES = {
    "consecutive7": counters(BASE, 7),
    "wrap5": counters(BASE | 0xFD, 5),                                   # ..FD ..FE ..FF, then the low byte wraps
    "pairs": [BASE, BASE + 1, BASE, BASE + 1],                           # duplicate blocks stay shared through every round
    "random6": [int.from_bytes(_rng.bytes(16), "big") for _ in range(6)],
    "single": [0x3243F6A8885A308D313198A2E0370734],
}


def _trivial(c, blocks):
    return c.trivial_bytes([u128_to_bytes(b) for b in blocks])


def _xor_clear(c, words, data):
    """what folding clear data into ciphertext words means: bit << 63 added to the bodies"""
    return words + _trivial(c, data)


@pytest.fixture(scope="module")
def toy_rk(toy_server, tc):
    """round keys of the three SP 800-38A keys, expanded on the GPU"""
    return {bits: toy_server.aes_key_expansion(tc.encrypt_aes_key(F5[bits][0])) for bits in (128, 192, 256)}


# ---- PARAM_TOY: the words of aes_encrypt on the trivial state --------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_public_blocks_are_aes_encrypt_on_trivial_bytes(toy, toy_server, toy_rk, tc, bits, case):
    blocks, rk = CASES[case], toy_rk[bits]
    got = toy_server.aes_encrypt_public(rk, blocks)
    assert got.shape == (len(blocks), 16, 8, toy.params.big1) and got.dtype == np.uint64
    want = toy_server.aes_encrypt(rk, _trivial(tc, blocks))
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    key = F5[bits][0]
    assert np.array_equal(tc.decrypt_bytes(got), block_bytes([aes_clear.aes_encrypt_block(key, b) for b in blocks]))
    as_bytes = toy_server.aes_encrypt_public(rk, [b.to_bytes(16, "big") for b in blocks])
    assert np.array_equal(as_bytes, got)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_host_arrays_and_resident_tensors_agree(toy, toy_server, toy_rk, tc, bits):
    rk, blocks = toy_rk[bits], CASES["wrap5"]
    want = toy_server.aes_encrypt_public(rk, blocks)
    want_ctr = toy_server.aes_ctr(rk, blocks[0], 0, 5, data=F1_PT + [0])
    d_rk = dev(rk)
    d_out = toy_server.aes_encrypt_public(d_rk, blocks)
    d_ctr = toy_server.aes_ctr(d_rk, blocks[0], 0, 5, data=F1_PT + [0])
    toy_server.synchronize()
    assert d_out.is_cuda and tuple(d_out.shape) == want.shape
    assert np.array_equal(host(d_out), want)
    assert np.array_equal(host(d_ctr), want_ctr)


@pytest.mark.parametrize("bits", [128, 192, 256])
def test_toy_ctr_is_public_encryption_of_the_counter_blocks_plus_clear_data(toy, toy_server, toy_rk, tc, bits):
    key, rk = F5[bits][0], toy_rk[bits]
    iv = MASK128 - 2                                                          # the counter wraps mod 2^128 inside the batch
    blocks = counters(iv, 5)
    stream = toy_server.aes_ctr(rk, iv, 0, 5)
    assert np.array_equal(stream, toy_server.aes_encrypt_public(rk, blocks))
    assert np.array_equal(tc.decrypt_bytes(stream), block_bytes(aes_clear.ctr_keystream(key, iv, 0, 5)))
    data = F1_PT + [MASK128]
    ct = toy_server.aes_ctr(rk, iv, 0, 5, data=data)
    assert np.array_equal(ct, _xor_clear(tc, stream, data))
    assert np.array_equal(tc.decrypt_bytes(ct), block_bytes([k ^ d for k, d in zip(aes_clear.ctr_keystream(key, iv, 0, 5), data)]))
    # first_block continues the stream; iv as bytes, data as one bytes object
    tail = toy_server.aes_ctr(rk, iv.to_bytes(16, "big"), 3, 2, data=b"".join(d.to_bytes(16, "big") for d in data[3:]))
    assert np.array_equal(tail, ct[3:])
    assert np.array_equal(toy_server.aes_ctr(rk, iv - 7, 7, 5), stream)


def test_toy_work_done_is_the_plan_and_the_noise_level_is_five(toy, tc):
    """the blind-rotation units of a call against those of aes_encrypt on as many blocks are sum(plan) / (16 n Nr), exactly"""
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        for bits, blocks in ((128, CASES["consecutive7"]), (256, CASES["wrap5"]), (192, CASES["pairs"]), (128, CASES["random6"])):
            rk = srv.aes_key_expansion(tc.encrypt_aes_key(F5[bits][0]))
            n, plan = len(blocks), _native.aes_public_plan(blocks, bits)
            srv.engine.profile_enable(True)
            srv.engine.profile_reset()
            srv.aes_encrypt(rk, _trivial(tc, blocks))
            full = srv.engine.profile_read()["blind_rotate"]["units"]
            srv.engine.profile_reset()
            if blocks == counters(blocks[0], n):
                srv.aes_ctr(rk, blocks[0], 0, n)
            else:
                srv.aes_encrypt_public(rk, blocks)
            shared = srv.engine.profile_read()["blind_rotate"]["units"]
            srv.engine.profile_enable(False)
            assert full > 0 and shared > 0
            assert Fraction(shared, full) == Fraction(sum(plan), 16 * n * NR[bits]), (bits, plan, shared, full)
    finally:
        srv.engine.close()
    srv = Server(toy.keys, device=0)
    try:
        srv.aes_ctr(rk, BASE, 0, 3, data=F1_PT[:3])
        assert srv.engine.noise_level_seen() == (5, 5)                        # 4 WoPBS outputs + 1 round key, as aes_encrypt
    finally:
        srv.engine.close()


def test_toy_server_group_plans_each_shard(toy, toy_server, toy_rk, tc):
    rk, blocks = toy_rk[192], CASES["consecutive7"]
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        assert np.array_equal(group.aes_encrypt_public(rk, blocks), toy_server.aes_encrypt_public(rk, blocks))
        assert np.array_equal(group.aes_ctr(rk, BASE, 2, 5, data=F1_PT + [7]), toy_server.aes_ctr(rk, BASE, 2, 5, data=F1_PT + [7]))
    finally:
        for s in group.servers:
            s.engine.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors(toy, toy_server, toy_rk, tc):
    p = toy.params
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    rk = toy_rk[256]
    out = np.full((2, 16, 8, p.big1), 0x5A5A, dtype=np.uint64)
    blocks = _native.u128_pairs([1, 2])
    bp = blocks.ctypes.data_as(_native._u64p)
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_aes_encrypt_public_bits(h, rk.ctypes.data, 100, bp, 2, out.ctypes.data, ms) == -1
        assert b"key_bits" in lib.fheaes_last_error(h)
        assert lib.fheaes_aes_ctr_bits(h, rk.ctypes.data, 100, bp, 0, None, 2, out.ctypes.data, ms) == -1
        assert b"key_bits" in lib.fheaes_last_error(h)
        assert lib.fheaes_aes_encrypt_public_bits(h, None, 256, bp, 2, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_encrypt_public_bits(h, rk.ctypes.data, 256, None, 2, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_encrypt_public_bits(h, rk.ctypes.data, 256, bp, 2, None, ms) == -1
        assert lib.fheaes_aes_ctr_bits(h, None, 256, bp, 0, None, 2, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_ctr_bits(h, rk.ctypes.data, 256, None, 0, None, 2, out.ctypes.data, ms) == -1
        assert lib.fheaes_aes_ctr_bits(h, rk.ctypes.data, 256, bp, 0, None, 2, None, ms) == -1
        # n_blocks = 0 is fine and writes nothing
        assert lib.fheaes_aes_encrypt_public_bits(h, rk.ctypes.data, 256, bp, 0, out.ctypes.data, ms) == 0
        assert lib.fheaes_aes_ctr_bits(h, rk.ctypes.data, 256, bp, 0, None, 0, out.ctypes.data, ms) == 0
    assert (out == 0x5A5A).all()
    assert toy_server.aes_encrypt_public(rk, []).shape == (0, 16, 8, p.big1)
    assert toy_server.aes_ctr(rk, 5, 0, 0).shape == (0, 16, 8, p.big1)
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_encrypt_public_bits(rk, 256, [1], np.empty((1, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_ctr_bits(rk, 256, 1, 0, None, 1, np.empty((1, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()
    # what never reaches the library
    bad = np.zeros((12, 16, 8, p.big1), dtype=np.uint64)
    for call in (lambda: toy_server.aes_encrypt_public(bad, [1]), lambda: toy_server.aes_ctr(bad, 1, 0, 1),
                 lambda: toy_server.aes_encrypt_public(rk.reshape(15 * 16, 8, p.big1), [1]),
                 lambda: toy_server.aes_encrypt_public(rk, [1 << 128]), lambda: toy_server.aes_encrypt_public(rk, [bytes(15)]),
                 lambda: toy_server.aes_ctr(rk, 1 << 128, 0, 1), lambda: toy_server.aes_ctr(rk, 1, 0, 2, data=[1]),
                 lambda: toy_server.aes_ctr(rk, 1, 0, 2, data=bytes(31)), lambda: toy_server.aes_ctr(rk, 1, -1, 1),
                 lambda: toy_server.aes_encrypt_public(rk, [1], out=np.empty((2, 16, 8, p.big1), dtype=np.uint64))):
        with pytest.raises(ValueError):
            call()


# ---- PARAM_OPT ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 192, 256])
def test_param_opt_sp800_38a_f5_end_to_end(opt, opt_server, oc, bits):
    """F.5.1 / F.5.3 / F.5.5: the key expanded on the GPU, aes_ctr with the NIST plaintext as data, the client decrypts the NIST ciphertext"""
    key, first, last = F5[bits]
    rk = opt_server.aes_key_expansion(oc.encrypt_aes_key(key))
    assert rk.shape == (NR[bits] + 1, 16, 8, opt.params.big1)
    ct = opt_server.aes_ctr(rk, F5_CTR, 0, 4, data=F1_PT)
    got = oc.decrypt_bytes(ct)
    want = [k ^ p for k, p in zip(aes_clear.ctr_keystream(key, F5_CTR, 0, 4), F1_PT)]
    assert want[0] == first and want[3] == last
    assert np.array_equal(got, block_bytes(want))


def test_param_opt_128_aligned_blocks_are_aes_encrypt_on_the_trivial_state(opt, opt_server, opt_rk128, oc):
    """128 consecutive counters from ..00 on resident tensors: 17,051 byte-WoPBS instead of 20,480, the words of aes_encrypt, every block's
    plaintext right, and the noise of aes_encrypt's last round (one fresh WoPBS output plus one round key: the bounds of
    tests/test_gpu_aes_key_sizes.py)."""
    key, n = F5[128][0], 128
    blocks = counters(BASE, n)
    assert sum(_native.aes_public_plan(blocks)) == 17051
    d_out = opt_server.aes_ctr(opt_rk128, BASE, 0, n)
    d_ref = dev(_trivial(oc, blocks))
    opt_server.aes_encrypt(opt_rk128, d_ref)
    opt_server.synchronize()
    out, ref = host(d_out), host(d_ref)
    assert np.array_equal(out, ref), "%d words differ" % int((out != ref).sum())
    got = oc.decrypt_bytes(out)
    want = block_bytes(aes_clear.ctr_keystream(key, BASE, 0, n))
    wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
    assert not wrong, "blocks wrong: %s" % wrong
    err = np.abs(noise(oc, out))
    print("aes_ctr, 128 blocks: max |noise| = 2^%.2f, std = 2^%.2f" % (np.log2(float(err.max())), np.log2(float(err.std()))))
    assert err.max() < 1 << 59, "max |noise| = 2^%.1f" % np.log2(float(err.max()))
    assert err.std() < 1 << 56, "std = 2^%.1f" % np.log2(float(err.std()))


def test_param_opt_server_group_of_two_contexts_equals_one(opt, opt_server, opt_rk128, oc):
    """2 x 16 blocks on two contexts of one GPU: each plans its own shard; the words are those of one context planning all 32"""
    n = 32
    data = [(F1_PT[i % 4] + i) & MASK128 for i in range(n)]
    d_one = opt_server.aes_ctr(opt_rk128, BASE | 0xF0, 0, n, data=data)
    opt_server.synchronize()
    group = ServerGroup(opt.keys, devices=(0, 0))
    try:
        d_two = group.aes_ctr(opt_rk128, BASE | 0xF0, 0, n, data=data)
        assert np.array_equal(host(d_two), host(d_one))
    finally:
        for s in group.servers:
            s.engine.close()
    want = [k ^ d for k, d in zip(aes_clear.ctr_keystream(F5[128][0], BASE | 0xF0, 0, n), data)]
    assert np.array_equal(oc.decrypt_bytes(host(d_one)), block_bytes(want))
