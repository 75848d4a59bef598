"""The two wire formats of include/fheaes.h on the CPU: seeded LWE ciphertexts (public mask key, first index, bodies) and packed GLWEs
modulus-switched to w bits per word.  All references are numpy and Python integers (tests/wire_formats.py, client.mask_words);
tests/test_gpu_wire_formats.py holds the engine to the same words.

The noise window of the switch is derived, not measured: each of the 1 + h words of a phase moves uniformly within +- 2^(63-w), so the
variance is (1 + h) 2^(2(64-w)) / 12 and no error exceeds (1 + h) 2^(63-w).  The coefficients of one GLWE share their mask errors, so a
sample standard deviation over a few GLWEs is noisier than 1 / sqrt(2n) suggests: the window is 0.5 .. 2, the hard bound is the sharp check."""
import ctypes

import numpy as np
import pytest

import wire_formats as wf
from aes_model import ref_fold, ref_ks
from gpu_support import tc  # noqa: F401
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native, client as cl
from tfhe_aes_amd.client import Client, SeededCiphertexts, load_ciphertexts, mask_words, read_back_packed, save_ciphertexts


# ---- seeded ciphertexts -------------------------------------------------------------------------------------------------------------------
def test_seeded_bits_expand_to_ciphertexts_of_the_bits(toy, tc):
    p = toy.params
    bits = np.random.default_rng(0x5EED).integers(0, 2, (5, 8)).astype(np.uint8)
    sc = tc.encrypt_bits_seeded(bits, first_index=5)
    assert isinstance(sc, SeededCiphertexts) and sc.bodies.shape == (5, 8) and sc.bodies.dtype == np.uint64 and sc.first_index == 5
    assert sc.mask_key.shape == (8,) and sc.mask_key.dtype == np.uint32
    assert sc.nbytes == 8 * 40 + 40
    lwe = sc.expand()
    assert lwe.shape == (5, 8, p.big1) and lwe.dtype == np.uint64
    got, phase = tc.decrypt_bits(lwe, return_phase=True)
    assert np.array_equal(got, bits)
    noise = (phase - (bits.astype(np.uint64) << np.uint64(63))).astype(np.int64)
    assert np.abs(noise).max() < 8 * p.glwe_noise_std * 2.0 ** 64                      # the noise of encrypt_bits, nothing else
    flat = lwe.reshape(40, p.big1)
    assert np.array_equal(flat[:, :p.big], mask_words(sc.mask_key, 6, 45, p.big)[5:])  # the stream of tag 6, offset by first_index
    assert np.array_equal(flat[:, :p.big], mask_words(sc.mask_key, cl.MASK_TAG_LWE, 40, p.big, first_ct=5))
    assert np.array_equal(flat[:, p.big], sc.bodies.reshape(-1))


def test_every_seeded_call_has_its_own_mask_key(toy):
    a = Client(params=toy.params)                                                      # os.urandom mode
    x, y = a.encrypt_bits_seeded(np.ones(3, dtype=np.uint8)), a.encrypt_bits_seeded(np.ones(3, dtype=np.uint8))
    assert not np.array_equal(x.mask_key, y.mask_key) and not np.array_equal(x.mask_key, a.mask_seed)
    assert np.array_equal(a.decrypt_bits(x.expand()), [1, 1, 1]) and np.array_equal(a.decrypt_bits(y.expand()), [1, 1, 1])


def test_the_deterministic_mode_reproduces(toy):
    def run():
        c = Client(params=toy.params, seed=0xD371)
        return c.encrypt_bytes_seeded([0x53, 0xA7]), c.encrypt_u128_seeded(0x0123456789ABCDEF0011223344556677)

    (a1, a2), (b1, b2) = run(), run()
    for x, y in ((a1, b1), (a2, b2)):
        assert np.array_equal(x.mask_key, y.mask_key) and np.array_equal(x.bodies, y.bodies) and x.first_index == y.first_index
    assert np.array_equal(a1.mask_key, cl.test_key(0xD371, 4, 1)) and np.array_equal(a2.mask_key, cl.test_key(0xD371, 4, 2))
    assert not np.array_equal(a1.mask_key, a2.mask_key)
    assert a1.bodies.shape == (2, 8) and a2.bodies.shape == (16, 8)


def test_the_four_seeded_methods_mirror_the_full_ones(toy, tc):
    assert np.array_equal(tc.decrypt_bytes(tc.encrypt_bytes_seeded([1, 0x80, 0xFF]).expand()), [1, 0x80, 0xFF])
    x = 0x00112233445566778899AABBCCDDEEFF
    assert tc.decrypt_u128(tc.encrypt_u128_seeded(x).expand()) == x
    for n in (16, 24, 32):
        key = bytes(range(7, 7 + n))
        sc = tc.encrypt_aes_key_seeded(key)
        assert sc.bodies.shape == (n, 8) and sc.nbytes == 64 * n + 40
        assert tc.decrypt_bytes(sc.expand()).tobytes() == key
    with pytest.raises(ValueError):
        tc.encrypt_aes_key_seeded(bytes(15))
    with pytest.raises(ValueError):
        tc.encrypt_bits_seeded(np.zeros(1, dtype=np.uint8), first_index=1 << 64)


def test_sizes_on_the_wire():
    """16,392 -> 8 bytes per input bit; one AES-128 key about 1 KB; 65,536 AES-128 keys 67.1 MB instead of 137.5 GB"""
    p = PARAM_OPT
    c = Client(params=p, seed=1)
    sc = c.encrypt_aes_key_seeded(bytes(16))
    full = sc.bodies.size * p.big1 * 8
    assert p.big1 * 8 == 16392 and sc.nbytes == 1064 and full == 2098176
    assert 65536 * full == 137506062336 and 65536 * sc.bodies.nbytes == 67108864
    assert cl.packed_mod_words(p, 16) * 8 * 32 == 163840 and cl.packed_mod_words(p, 64) * 8 * 32 == 655360


def test_the_c_client_takes_a_64_bit_first_index(toy, tc):
    """four ciphertexts from index 2^32 - 2 on: the last two have a nonzero high nonce word"""
    p, lib = toy.params, cl._load()
    first = (1 << 32) - 2
    enc_key, mask_key = cl.test_key(9, 3, 1), cl.test_key(9, 4, 1)
    bits = np.array([1, 0, 1, 1], dtype=np.uint8)
    bodies = np.zeros(4, dtype=np.uint64)
    lib.fheaes_client_encrypt_bits_seeded(ctypes.byref(tc._c), cl._u32(enc_key), cl._u32(mask_key), first, cl._u8(tc.glwe_sk), p.glwe_noise_std,
                                          cl._u8(bits), 4, cl._u64(bodies))
    masks = mask_words(mask_key, 6, 4, p.big, first_ct=first)
    for t, j in ((0, 0), (2, 0), (2, p.big - 1), (3, 17)):                             # numpy's stream is the C client's, at a 64-bit index
        assert int(masks[t, j]) == lib.fheaes_client_mask_word(cl._u32(mask_key), 6, first + t, j)
    assert not np.array_equal(masks[2], mask_words(mask_key, 6, 1, p.big, first_ct=0)[0])     # index 2^32 is not index 0
    sc = SeededCiphertexts(p, mask_key, first, bodies)
    assert np.array_equal(sc.expand()[:, :p.big], masks)
    assert np.array_equal(tc.decrypt_bits(sc.expand()), bits)
    # each ciphertext has its own streams, so neither the size of the call nor the number of threads enters
    for count in (1, 3):
        again = np.zeros(4, dtype=np.uint64)
        lib.fheaes_client_encrypt_bits_seeded(ctypes.byref(tc._c), cl._u32(enc_key), cl._u32(mask_key), first, cl._u8(tc.glwe_sk), p.glwe_noise_std,
                                              cl._u8(bits), count, cl._u64(again))
        assert np.array_equal(again[:count], bodies[:count]) and not again[count:].any()


def test_seeded_ciphertexts_save_and_load(toy, tc, tmp_path):
    sc = tc.encrypt_aes_key_seeded(bytes(range(16)), first_index=(1 << 40) + 3)
    path = tmp_path / "key.npz"
    sc.save(path)
    back = SeededCiphertexts.load(path, toy.params)
    assert back.first_index == sc.first_index and np.array_equal(back.mask_key, sc.mask_key) and np.array_equal(back.bodies, sc.bodies)
    assert back.bodies.shape == (16, 8) and np.array_equal(back.expand(), sc.expand())
    with pytest.raises(ValueError):
        SeededCiphertexts.load(path, PARAM_OPT)
    bad = tmp_path / "bad.npz"
    np.savez(bad, shape=cl._param_shape(toy.params), mask_key=np.zeros(7, dtype=np.uint32), first_index=np.zeros(1, dtype=np.uint64),
             bodies=np.zeros(3, dtype=np.uint64))
    with pytest.raises(ValueError):
        SeededCiphertexts.load(bad, toy.params)


# ---- the switch: rounding rule, layout, noise -------------------------------------------------------------------------------------------------
def test_the_rounding_rule_on_the_edge_words():
    for w in wf.WIDTHS:
        half = 1 << (63 - w)
        assert wf.mod_switch_word(0, w) == 0 and wf.mod_switch_word(wf.M64, w) == 0                    # the top rounds to 0 by wrapping
        assert wf.mod_switch_word(1 << 63, w) == 1 << (w - 1) and wf.mod_switch_word((1 << 63) - 1, w) == 1 << (w - 1)
        for j in (0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1):
            tie = (2 * j + 1) * half
            assert wf.mod_switch_word(tie - 1, w) == j                                                  # just below a tie: down
            assert wf.mod_switch_word(tie, w) == wf.mod_switch_word(tie + 1, w) == (j + 1) % (1 << w)   # a tie rounds up; the last wraps
        words = np.array(wf.edge_word_list(w), dtype=np.uint64)
        assert len(words) == 19
        assert [int(x) for x in wf.round_words(words, w)] == [wf.read_back_word(wf.mod_switch_word(int(x), w), w) for x in words]
    assert len(wf.edge_word_list(64)) == 4 and np.array_equal(wf.round_words(np.array([wf.M64], dtype=np.uint64), 64), [wf.M64])


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("w", wf.WIDTHS + (64,))
def test_the_edge_word_set_holds_its_classes(k, w):
    glwe, cls = wf.edge_glwes(k, w)
    runs = 3 * ((k + 1) * 2 + (1 if 64 % w else 0))          # copies of the word list: two per polynomial, one more on straddling fields
    n = len(wf.edge_word_list(w))
    assert glwe.shape == (3, (k + 1) * 512) and cls["placed"] == runs * n and cls["extremes"] == 4 * runs
    assert cls["first_of_polynomial"] == cls["last_of_polynomial"] == 3 * (k + 1) and cls["first_of_glwe"] == cls["last_of_glwe"] == 3
    if w == 64:
        assert n == 4 and cls["ties"] == 0
        return
    assert cls["ties"] == 5 * runs and cls["tie_neighbours"] == 10 * runs and cls["wrap_to_zero"] == 3 * runs and cls["wrap_last_of_glwe"] == 2
    if 64 % w:
        # w = 10 / 13: 4 of 32 / 12 of 64 consecutive fields lie across two words, so a run of 19 fields holds at least 2 / 3 of them,
        # and the extra copy puts EVERY word of the list on such a field, the three that wrap to 0 among them
        assert cls["straddling"] >= 3 * (19 + (2 if w == 10 else 3) * (k + 1) * 2) and cls["wrap_straddling"] >= 3 * 3
    else:
        assert cls["straddling"] == 0
    # the layout on the set: packer and read-back are inverse up to the rounding, and client.read_back_packed reads the same words
    params = PARAM_TOY if k == 1 else PARAM_OPT
    packed = wf.switch_glwes(glwe, w)
    assert packed.shape == (3, (k + 1) * 8 * w) and packed.shape[1] == cl.packed_mod_words(params, w)
    back = wf.read_back_glwes(packed, glwe.shape[1], w)
    assert np.array_equal(back, wf.round_words(glwe, w))
    assert np.array_equal(read_back_packed(packed, params, w), back)


@pytest.mark.parametrize("k", [1, 4])
def test_the_switch_adds_the_predicted_noise(k):
    params = PARAM_TOY if k == 1 else PARAM_OPT
    c = Client(params=params, seed=0x5717C4)                                   # a random binary key (no evaluation keys are generated)
    h = int(c.glwe_sk.sum())
    glwe = np.random.default_rng(0xA0 + k).integers(0, 1 << 64, (4, (k + 1) * 512), dtype=np.uint64)
    before = c.glwe_phase(glwe)
    for w in (10, 13, 16, 32):
        packed = wf.switch_glwes(glwe, w)
        after = c.glwe_phase(read_back_packed(packed, params, w))
        err = (after - before).astype(np.int64).reshape(-1).astype(np.float64)
        ratio, worst = err.std() / wf.noise_std(h, w), np.abs(err).max()
        print("k = %d, h = %d, w = %d: std / formula %.3f, max %.2f sigma, max / bound %.3f" % (k, h, w, ratio, worst / wf.noise_std(h, w),
                                                                                               worst / wf.noise_bound(h, w)))
        assert 0.5 <= ratio <= 2
        assert worst <= wf.noise_bound(h, w)


def test_param_opt_at_16_bits_is_inside_the_margin():
    h = 1024
    assert 51.1 < np.log2(wf.noise_std(h, 16)) < 51.3 and abs(np.log2(wf.noise_bound(h, 16)) - 57.0) < 0.01        # (1 + h) 2^47 = 2^57.001 < 2^58
    assert wf.noise_bound(2048, 16) < 1 << 59                                  # even a key of all ones stays below the WoPBS noise's max


def test_decrypt_packed_reads_the_switched_form(toy, tc):
    p, m = toy.params, 600
    bits = np.random.default_rng(0x16B).integers(0, 2, m).astype(np.uint8)
    packed64 = ref_fold(ref_ks(toy, tc.encrypt_bits(bits)), p)
    packed = wf.switch_glwes(packed64, 16)
    assert packed.shape == (2, cl.packed_mod_words(p, 16)) == (2, (p.k + 1) * 8 * 16)
    assert packed.nbytes * 4 == packed64.nbytes
    got, phase = tc.decrypt_packed(packed, m, return_phase=True, width=16)
    assert np.array_equal(got, bits)
    _, phase64 = tc.decrypt_packed(packed64, m, return_phase=True)
    h = int(tc.glwe_sk.sum())
    assert np.abs((phase - phase64).astype(np.int64)).max() <= wf.noise_bound(h, 16)
    assert np.array_equal(tc.decrypt_packed(packed64, m, width=64), bits)
    vals = np.random.default_rng(3).integers(0, 256, 70).astype(np.uint8)
    packed_b = wf.switch_glwes(ref_fold(ref_ks(toy, tc.encrypt_bytes(vals)), p), 16)
    assert np.array_equal(tc.decrypt_packed_bytes(packed_b, 70, width=16), vals)
    with pytest.raises(ValueError):
        tc.decrypt_packed(packed, m, width=13)                                 # the shape belongs to another width
    with pytest.raises(ValueError):
        tc.decrypt_packed(packed, m, width=7)


def test_switched_packed_save_and_load(toy, tmp_path):
    p = toy.params
    packed = wf.switch_glwes(np.random.default_rng(5).integers(0, 1 << 64, (2, (p.k + 1) * p.N), dtype=np.uint64), 13)
    path = tmp_path / "packed13.npz"
    save_ciphertexts(path, p, "packed_mod", packed, width=13)
    assert np.array_equal(load_ciphertexts(path, p, "packed_mod", width=13), packed)
    with pytest.raises(ValueError):
        load_ciphertexts(path, p, "packed_mod", width=16)                      # the wrong width
    with pytest.raises(ValueError):
        load_ciphertexts(path, p, "packed_mod")                                # no width
    with pytest.raises(ValueError):
        load_ciphertexts(path, p, "packed")                                    # the wrong kind
    with pytest.raises(ValueError):
        load_ciphertexts(path, PARAM_OPT, "packed_mod", width=13)
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "x.npz", p, "packed_mod", packed, width=16)   # the wrong shape for the width
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "x.npz", p, "packed_mod", packed, width=64)
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "x.npz", p, "packed", packed, width=13)


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fheaes_expand_lwe_seeded", "fheaes_packed_words_mod", "fheaes_packed_mod_switch", "fheaes_pack_bits_mod", "fheaes_unpack_bits_mod")


def test_the_five_symbols_are_exported_and_bound():
    lib = _native.load_library()
    for name in NEW_SYMBOLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES and hasattr(lib, name)
    blob = _native._build.ENGINE_SO.read_bytes()
    for kernel in (b"expand_lwe_kernel", b"mod_switch_pack_kernel", b"sample_extract_mod_kernel"):
        assert kernel in blob


def test_a_null_context_and_a_bad_width_are_errors():
    lib = _native.load_library()
    a, b = np.zeros(4096, dtype=np.uint64), np.zeros(4096, dtype=np.uint64)
    key = np.zeros(8, dtype=np.uint32)
    for width in (16, 64, 7, 33, 63, 0):
        assert lib.fheaes_packed_words_mod(None, 512, width) == 0
        assert lib.fheaes_packed_mod_switch(None, a.ctypes.data, 1, width, b.ctypes.data, _native.HOST) == -1
        assert lib.fheaes_pack_bits_mod(None, a.ctypes.data, 1, width, b.ctypes.data, _native.HOST) == -1
        assert lib.fheaes_unpack_bits_mod(None, a.ctypes.data, 1, width, b.ctypes.data, _native.HOST) == -1
    assert lib.fheaes_expand_lwe_seeded(None, key.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 0, a.ctypes.data, 1, b.ctypes.data, _native.HOST) == -1
    assert lib.fheaes_expand_lwe_seeded(None, None, 0, None, 0, None, _native.HOST) == -1
    assert not a.any() and not b.any()
