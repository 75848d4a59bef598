"""The wire formats on the MI355X: fheaes_expand_lwe_seeded, fheaes_packed_mod_switch, fheaes_pack_bits_mod, fheaes_unpack_bits_mod and
the Python layer over them.  Every word comparison is array_equal against numpy and Python integers (tests/wire_formats.py,
SeededCiphertexts.expand()); device outputs sit between sentinel-filled guard rows.

The noise window of the PARAM_OPT test is the header's formula, not what the code gives: each of the 1 + h words of a phase moves uniformly
within +- 2^(63-w): std sqrt((1 + h) / 12) 2^(64-w), no error beyond (1 + h) 2^(63-w); the window 0.5 .. 2 on the standard deviation allows
for the mask errors that the coefficients of one GLWE share, the hard bound is the sharp check."""
import math

import numpy as np
import pytest

import wire_formats as wf
from aes_vectors import BASE, F1_PT, F5
from gpu_support import dev, guarded, guards_intact, host, oc, opt_rk128, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native, aes_clear
from tfhe_aes_amd.client import SeededCiphertexts, packed_mod_words, test_key as det_key
from tfhe_aes_amd.server import ServerGroup

pytestmark = pytest.mark.gpu

WIDTHS = (8, 10, 13, 16, 32, 64)


@pytest.fixture(scope="module")
def keyless():
    """contexts without keys, k = 1 and k = 4: expansion, the switch and the extraction need none"""
    engines = {1: _native.Engine(PARAM_TOY, device=0), 4: _native.Engine(PARAM_OPT, device=0)}
    yield engines
    for e in engines.values():
        e.close()


# ---- 1. expansion --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_bodies():
    return np.random.default_rng(0xB0D1).integers(0, 1 << 64, 1000, dtype=np.uint64)


@pytest.mark.parametrize("first", [0, 5, (1 << 32) - 3])
@pytest.mark.parametrize("m", [1, 7, 128, 1000])
def test_expansion_is_the_numpy_twin(toy_server, toy_bodies, m, first):
    p = PARAM_TOY
    sc = SeededCiphertexts(p, det_key(0xE8, 4, m), first, toy_bodies[:m])
    want = sc.expand()
    got = toy_server.expand(sc)                                                        # host arrays
    assert isinstance(got, np.ndarray) and got.dtype == np.uint64 and got.shape == (m, p.big1)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    buf, rows = guarded(m, p.big1)                                                     # a resident tensor between guard rows
    assert toy_server.expand(sc, out=rows) is rows
    toy_server.synchronize()
    assert np.array_equal(host(rows), want) and guards_intact(buf)


def test_expansion_at_k_4_and_resident_bodies(keyless):
    p, eng = PARAM_OPT, keyless[4]
    first = (1 << 32) - 1                                                              # ciphertexts 1 and 2 have a high nonce word
    sc = SeededCiphertexts(p, det_key(0xE8, 4, 77), first, np.random.default_rng(4).integers(0, 1 << 64, 3, dtype=np.uint64))
    want = sc.expand()
    buf, rows = guarded(3, p.big1)
    eng.expand_lwe_seeded(sc.mask_key, first, dev(sc.bodies), 3, rows)
    eng.synchronize()
    assert np.array_equal(host(rows), want) and guards_intact(buf)
    got = np.zeros((3, p.big1), dtype=np.uint64)
    eng.expand_lwe_seeded(sc.mask_key, first, sc.bodies, 3, got)
    assert np.array_equal(got, want)


def test_expansion_keeps_the_logical_shape(toy_server, tc):
    sc = tc.encrypt_bytes_seeded(list(range(40, 61)), first_index=(1 << 32) - 100)     # bodies [21][8]: 168 ciphertexts across 2^32
    want = sc.expand()
    assert np.array_equal(toy_server.expand(sc), want) and want.shape == (21, 8, PARAM_TOY.big1)
    assert np.array_equal(tc.decrypt_bytes(want), np.arange(40, 61))
    assert toy_server.expand(SeededCiphertexts(sc.params, sc.mask_key, 0, sc.bodies[:0])).shape == (0, 8, PARAM_TOY.big1)
    with pytest.raises(ValueError):
        toy_server.expand(SeededCiphertexts(PARAM_OPT, sc.mask_key, 0, sc.bodies))


# ---- 2. end to end at PARAM_TOY ---------------------------------------------------------------------------------------------------------------
def test_a_seeded_key_through_ctr_to_a_16_bit_packing(toy, toy_server, tc):
    key = F5[128][0]
    sc = tc.encrypt_aes_key_seeded(key)
    assert sc.nbytes == 1064
    d_key = toy_server.expand(sc, out=dev(np.zeros((16, 8, PARAM_TOY.big1), dtype=np.uint64)))
    uploaded = dev(sc.expand())                                                         # expanding on the host and uploading: the same words
    toy_server.synchronize()
    assert np.array_equal(host(d_key), host(uploaded))
    d_rk = toy_server.aes_key_expansion(d_key)
    data = [F1_PT[0], F1_PT[1]]
    d_ct = toy_server.aes_ctr(d_rk, BASE, 0, 2, data=data)
    d_packed = toy_server.pack(d_ct, width=16)
    toy_server.synchronize()
    packed = host(d_packed)
    assert packed.shape == (1, packed_mod_words(PARAM_TOY, 16)) and packed.nbytes == 2 * 512 * 2
    want = b"".join((ks ^ d).to_bytes(16, "big") for ks, d in zip(aes_clear.ctr_keystream(key, BASE, 0, 2), data))
    assert tc.decrypt_packed_bytes(packed, 32, width=16).tobytes() == want


# ---- 3. the switch and the extraction from fields -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def switched():
    """(k, w) -> (edge GLWEs, their switched form by the Python-integer packer)"""
    out = {}
    for k in (1, 4):
        for w in WIDTHS:
            glwe, _ = wf.edge_glwes(k, w)
            out[k, w] = (glwe, wf.switch_glwes(glwe, w))
    return out


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("w", WIDTHS)
def test_the_switch_on_the_edge_words(keyless, switched, k, w):
    eng = keyless[k]
    glwe, want = switched[k, w]
    assert eng.packed_words_mod(3 * 512, w) == want.size and eng.packed_words_mod(1, w) == want.shape[1]
    got = np.zeros_like(want)
    eng.packed_mod_switch(glwe, 3, w, got)                                             # host arrays
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    buf, rows = guarded(3, want.shape[1])
    eng.packed_mod_switch(dev(glwe), 3, w, rows)
    eng.synchronize()
    assert np.array_equal(host(rows), want) and guards_intact(buf)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("w", WIDTHS)
def test_extraction_from_the_fields_is_extraction_of_the_read_back_words(keyless, switched, k, w):
    eng = keyless[k]
    p = eng.params
    glwe, packed = switched[k, w]
    back = wf.read_back_glwes(packed, glwe.shape[1], w)
    assert np.array_equal(back, wf.round_words(glwe, w))
    want = np.zeros((1100, p.big1), dtype=np.uint64)
    eng.unpack_bits(back, 1100, want)                                                  # the parent's entry point on the read-back words
    d_packed = dev(packed)
    for m in (1, 511, 512, 513, 1100):
        g = (m + 511) // 512
        buf, rows = guarded(m, p.big1)
        eng.unpack_bits_mod(d_packed[:g], m, w, rows)
        eng.synchronize()
        assert np.array_equal(host(rows), want[:m]), "m = %d" % m
        assert guards_intact(buf)
    got = np.zeros((513, p.big1), dtype=np.uint64)
    eng.unpack_bits_mod(packed[:2], 513, w, got)                                       # host arrays
    assert np.array_equal(got, want[:513])


# ---- 4. fheaes_pack_bits_mod -------------------------------------------------------------------------------------------------------------------
PACK_M = (1, 512, 513, 1541)


@pytest.fixture(scope="module")
def toy_packed(toy, toy_server, tc):
    """1,541 encrypted bits and fheaes_pack_bits of their prefixes"""
    lwe = tc.encrypt_bits(np.random.default_rng(0x7AC).integers(0, 2, max(PACK_M)).astype(np.uint8))
    return lwe, {m: toy_server.pack(lwe[:m]) for m in PACK_M}


@pytest.mark.parametrize("w", [13, 16])
@pytest.mark.parametrize("m", PACK_M)
def test_pack_bits_mod_is_the_switch_of_pack_bits(toy_server, toy_packed, m, w):
    lwe, packed64 = toy_packed
    eng = toy_server.engine
    g = (m + 511) // 512
    want = np.zeros((g, packed_mod_words(PARAM_TOY, w)), dtype=np.uint64)
    eng.packed_mod_switch(packed64[m], g, w, want)
    assert np.array_equal(want, wf.switch_glwes(packed64[m], w))
    got = toy_server.pack(lwe[:m], width=w)                                            # host arrays
    assert got.shape == want.shape and np.array_equal(got, want)
    buf, rows = guarded(g, want.shape[1])
    toy_server.pack(dev(lwe[:m]), out=rows, width=w)
    toy_server.synchronize()
    assert np.array_equal(host(rows), want) and guards_intact(buf)
    assert np.array_equal(toy_server.pack(lwe[:m], width=64), packed64[m])            # 64: the words of fheaes_pack_bits


@pytest.mark.parametrize("w", [13, 16])
def test_pack_bits_mod_in_chunks(toy, toy_packed, w):
    """fheaes_reserve(256) leaves room for one chunk of 512 bits (tests/test_gpu_pack.py): 1,541 bits in four chunks, each switched after
    its fold"""
    lwe, packed64 = toy_packed
    eng = _native.Engine(toy.params, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        eng.reserve(256)
        got = np.zeros((4, packed_mod_words(PARAM_TOY, w)), dtype=np.uint64)
        eng.profile_reset()
        eng.pack_bits_mod(lwe, 1541, w, got)
        prof = eng.profile_read()
        assert prof["pfpks"]["launches"] == 4 and prof["pfpks"]["units"] == 1541
        assert np.array_equal(got, wf.switch_glwes(packed64[1541], w))
    finally:
        eng.close()


# ---- 5. PARAM_OPT ------------------------------------------------------------------------------------------------------------------------------
def test_param_opt_a_ctr_output_packed_at_16_bits(opt_server, opt_rk128, oc):
    key, n = F5[128][0], 4
    d_ct = opt_server.aes_ctr(opt_rk128, BASE, 0, n, data=F1_PT)
    d_p64, d_p16 = opt_server.pack(d_ct), opt_server.pack(d_ct, width=16)
    opt_server.synchronize()
    p64, p16 = host(d_p64), host(d_p16)
    assert p64.nbytes == 20480 and p16.nbytes == 5120
    want = b"".join((ks ^ d).to_bytes(16, "big") for ks, d in zip(aes_clear.ctr_keystream(key, BASE, 0, n), F1_PT))
    assert oc.decrypt_packed_bytes(p16, 16 * n, width=16).tobytes() == want            # all 512 bits
    _, ph64 = oc.decrypt_packed(p64, 512, return_phase=True)
    _, ph16 = oc.decrypt_packed(p16, 512, return_phase=True, width=16)
    err = (ph16 - ph64).astype(np.int64).astype(np.float64)
    h = int(oc.glwe_sk.sum())
    ratio = err.std() / wf.noise_std(h, 16)
    print("w = 16 at PARAM_OPT, h = %d: added error std 2^%.2f = %.3f of the formula, max 2^%.2f = %.3f of the hard bound" % (
        h, math.log2(err.std()), ratio, math.log2(np.abs(err).max()), np.abs(err).max() / wf.noise_bound(h, 16)))
    assert np.abs(err).max() <= wf.noise_bound(h, 16)
    assert 0.5 <= ratio <= 2
    d_back = opt_server.unpack(d_p16, (n, 16, 8), width=16)                            # and back: valid ciphertexts of the same bytes
    opt_server.synchronize()
    assert oc.decrypt_bytes(host(d_back)).tobytes() == want


# ---- 6. errors, groups -----------------------------------------------------------------------------------------------------------------------
def test_errors(toy, toy_packed):
    p = toy.params
    eng = toy.engine()
    lib, h = eng._lib, eng._h
    lwe, _ = toy_packed
    gw = (p.k + 1) * p.N
    key = np.zeros(8, dtype=np.uint32)
    kp = key.ctypes.data_as(_native._u32p)
    for ms in (_native.HOST, _native.DEVICE):
        buf = np.zeros(513 * p.big1 + 2 * gw, dtype=np.uint64)
        base = buf.ctypes.data
        for width in (7, 33, 63, 0, 65):
            assert lib.fheaes_packed_words_mod(h, 512, width) == 0
            assert lib.fheaes_packed_mod_switch(h, base, 1, width, base + 8 * gw, ms) == -1 and b"width" in lib.fheaes_last_error(h)
            assert lib.fheaes_pack_bits_mod(h, base, 1, width, base + 8 * p.big1, ms) == -1 and b"width" in lib.fheaes_last_error(h)
            assert lib.fheaes_unpack_bits_mod(h, base, 1, width, base + 8 * gw, ms) == -1 and b"width" in lib.fheaes_last_error(h)
        # overlapping buffers: one array, the other argument inside it
        assert lib.fheaes_pack_bits_mod(h, base, 513, 16, base + 8 * 100, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_pack_bits_mod(h, base + 8 * 100, 513, 16, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_unpack_bits_mod(h, base, 513, 16, base + 8 * (gw // 2 - 1), ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_unpack_bits_mod(h, base + 8 * 10, 513, 16, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_packed_mod_switch(h, base, 2, 16, base + 8 * (2 * gw - 1), ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_packed_mod_switch(h, base + 8, 2, 64, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_expand_lwe_seeded(h, kp, 0, base, 4, base + 8 * 3, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_expand_lwe_seeded(h, kp, 0, base + 8 * p.big1, 4, base, ms) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert not buf.any()
        # null pointers
        assert lib.fheaes_pack_bits_mod(h, None, 1, 16, base, ms) == -1 and lib.fheaes_pack_bits_mod(h, base, 1, 16, None, ms) == -1
        assert lib.fheaes_unpack_bits_mod(h, None, 1, 16, base, ms) == -1 and lib.fheaes_unpack_bits_mod(h, base, 1, 16, None, ms) == -1
        assert lib.fheaes_packed_mod_switch(h, None, 1, 16, base, ms) == -1 and lib.fheaes_packed_mod_switch(h, base, 1, 16, None, ms) == -1
        assert lib.fheaes_expand_lwe_seeded(h, None, 0, base, 1, base + 64, ms) == -1 and lib.fheaes_expand_lwe_seeded(h, kp, 0, None, 1, base, ms) == -1
        assert lib.fheaes_expand_lwe_seeded(h, kp, 0, base, 1, None, ms) == -1
        # nothing to do is fine and writes nothing
        out = np.full(gw, 0x5A5A, dtype=np.uint64)
        assert lib.fheaes_pack_bits_mod(h, lwe.ctypes.data, 0, 16, out.ctypes.data, ms) == 0
        assert lib.fheaes_unpack_bits_mod(h, lwe.ctypes.data, 0, 16, out.ctypes.data, ms) == 0
        assert lib.fheaes_packed_mod_switch(h, lwe.ctypes.data, 0, 16, out.ctypes.data, ms) == 0
        assert lib.fheaes_expand_lwe_seeded(h, kp, 0, lwe.ctypes.data, 0, out.ctypes.data, ms) == 0
        assert (out == 0x5A5A).all()
    assert eng.packed_words_mod(0, 16) == 0 and eng.packed_words_mod(513, 16) == 2 * gw // 4 and eng.packed_words_mod(513, 64) == eng.packed_words(513)
    fresh = _native.Engine(p, device=0)                                                # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.pack_bits_mod(lwe[:513], 513, 16, np.empty((2, gw // 4), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


def test_a_server_group_on_one_device_gives_the_words_of_a_server(toy, toy_server, toy_packed, tc):
    lwe, packed64 = toy_packed
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        want = toy_server.pack(lwe, width=16)
        got = group.pack(lwe, width=16)
        assert np.array_equal(got, want) and np.array_equal(want, wf.switch_glwes(packed64[1541], 16))
        assert np.array_equal(group.unpack(got, 1541, width=16), toy_server.unpack(want, 1541, width=16))
        sc = tc.encrypt_bits_seeded(np.arange(300) % 2, first_index=(1 << 32) - 7)
        assert np.array_equal(group.expand(sc), toy_server.expand(sc)) and np.array_equal(group.expand(sc), sc.expand())
        d = group.expand(SeededCiphertexts(sc.params, sc.mask_key, sc.first_index, dev(sc.bodies)))      # resident bodies, sharded
        assert d.is_cuda and np.array_equal(host(d), sc.expand())
    finally:
        for s in group.servers:
            s.engine.close()
