"""Packing N = 512 ciphertext bits into one GLWE ciphertext with the keys at hand (include/fheaes.h: fheaes_pack_bits,
fheaes_unpack_bits), on the CPU: the reference of the words (aes_model.py: ref_pack, ref_unpack), built from what already exists -- the
oracle's private functional packing key switch under key block k, a numpy fold and a numpy sample extraction -- decodes, adds the predicted noise and extracts to valid LWE
ciphertexts; the "packed" interchange kind; the three symbols and their NULL-context behaviour.  tests/test_gpu_pack.py holds the
engine to these words.

The noise bound (aes_model.pack_sigma) is computed from the parameter set, not from what the code gives:
    sigma^2 = N (kN+1) L (B^2 / 12) sigma_pfks^2  +  (kN/2 + 1) 2^(2R) / 12
B = 2^pfks_base_log, L = pfks_level, R = 64 - L pfks_base_log, sigma_pfks = pfks_noise_std 2^64: N rotated key switches, each a sum of
(kN+1) L digits (uniform in a range of width B) times fresh key noise, plus the rounding of the gadget to its 2^R grid against a binary
key of kN bits (half of them set) and the body.  The added error must stay within 8 sigma: over at most 2^15 samples a Gaussian
exceeds that with probability below 2^-30."""
import math

import numpy as np
import pytest

from aes_model import added_error, pack_sigma, ref_ks, ref_pack, ref_unpack
from gpu_support import tc  # noqa: F401
from tfhe_aes_amd import _native
from tfhe_aes_amd.client import load_ciphertexts, save_ciphertexts


# ---- PARAM_TOY ----------------------------------------------------------------------------------------------------------------------------
M = 600


@pytest.fixture(scope="module")
def packed600(toy, tc):
    bits = np.random.default_rng(0x9AC4).integers(0, 2, M).astype(np.uint8)
    lwe = tc.encrypt_bits(bits)
    return bits, lwe, ref_pack(toy, lwe)


def test_the_reference_key_switch_is_block_k_of_the_oracle(toy, packed600):
    _, lwe, _ = packed600
    assert np.array_equal(ref_ks(toy, lwe[:3]), toy.oracle.pfpks(lwe[:3])[:, toy.params.k])


def test_packed_reference_decrypts_to_the_bits(toy, tc, packed600):
    bits, _, packed = packed600
    p = toy.params
    assert packed.shape == (2, (p.k + 1) * p.N) and packed.dtype == np.uint64
    assert np.array_equal(tc.decrypt_packed(packed, M), bits)
    got, phase = tc.decrypt_packed(packed, M, return_phase=True)
    assert np.array_equal(got, bits) and phase.shape == (M,) and phase.dtype == np.uint64
    assert np.array_equal(phase, tc.glwe_phase(packed).reshape(-1)[:M])
    with pytest.raises(ValueError):
        tc.decrypt_packed(packed, 2 * p.N + 1)


def test_packed_bytes_decrypt(toy, tc):
    vals = np.random.default_rng(7).integers(0, 256, 70).astype(np.uint8)            # 560 bits: one full GLWE and a partly filled one
    packed = ref_pack(toy, tc.encrypt_bytes(vals))
    got = tc.decrypt_packed_bytes(packed, 70)
    assert got.dtype == np.uint8 and np.array_equal(got, vals)


def test_added_error_is_within_eight_sigma(toy, tc, packed600):
    _, lwe, packed = packed600
    sigma = pack_sigma(toy.params)
    assert 33.9 < math.log2(sigma) < 34.1                                             # 2^34.0 at PARAM_TOY
    err = added_error(tc, packed, lwe)
    print("added error: std 2^%.2f, max 2^%.2f = %.2f sigma (sigma 2^%.2f)" % (math.log2(err.std()), math.log2(np.abs(err).max()),
                                                                               np.abs(err).max() / sigma, math.log2(sigma)))
    assert np.abs(err).max() <= 8 * sigma


def test_param_opt_sigma():
    from tfhe_aes_amd import PARAM_OPT

    assert 33.4 < math.log2(pack_sigma(PARAM_OPT)) < 33.6                             # 2^33.5 at PARAM_OPT


def test_unused_coefficients_decode_to_zero(toy, tc, packed600):
    _, _, packed = packed600
    p = toy.params
    phase = tc.glwe_phase(packed).reshape(-1)[M:]
    assert phase.size == 2 * p.N - M == 424
    assert not ((phase + np.uint64(1 << 62)) >> np.uint64(63)).any()
    assert np.abs(phase.astype(np.int64)).max() <= 8 * pack_sigma(p)                  # encryptions of zero: the packing error alone


def test_extraction_of_the_reference_packing_decrypts_with_the_same_phases(toy, tc, packed600):
    bits, _, packed = packed600
    lwe = ref_unpack(packed, M, toy.params)
    assert lwe.shape == (M, toy.params.big1)
    got, phase = tc.decrypt_bits(lwe, return_phase=True)
    assert np.array_equal(got, bits)
    assert np.array_equal(phase, tc.decrypt_packed(packed, M, return_phase=True)[1])


def test_packed_save_and_load_round_trip(toy, packed600, tmp_path):
    from tfhe_aes_amd import PARAM_OPT

    _, lwe, packed = packed600
    path = tmp_path / "packed.npz"
    save_ciphertexts(path, toy.params, "packed", packed)
    back = load_ciphertexts(path, toy.params, "packed")
    assert back.dtype == np.uint64 and np.array_equal(back, packed)
    with pytest.raises(ValueError):
        load_ciphertexts(path, toy.params, "bytes")
    with pytest.raises(ValueError):
        load_ciphertexts(path, PARAM_OPT, "packed")
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "x.npz", toy.params, "packed", lwe)               # LWE words are not a packed array
    with pytest.raises(ValueError):
        save_ciphertexts(tmp_path / "x.npz", toy.params, "packed", packed[:, :-1])


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("fheaes_packed_words", "fheaes_pack_bits", "fheaes_unpack_bits")


def test_the_three_symbols_are_exported_and_bound():
    lib = _native.load_library()
    for name in NEW_SYMBOLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES and hasattr(lib, name)
    assert b"pack_fold_kernel" in _native._build.ENGINE_SO.read_bytes() and b"sample_extract_kernel" in _native._build.ENGINE_SO.read_bytes()


def test_a_null_context_is_an_error():
    lib = _native.load_library()
    a, b = np.zeros(4096, dtype=np.uint64), np.zeros(4096, dtype=np.uint64)
    assert lib.fheaes_pack_bits(None, a.ctypes.data, 1, b.ctypes.data, _native.HOST) == -1
    assert lib.fheaes_unpack_bits(None, a.ctypes.data, 1, b.ctypes.data, _native.HOST) == -1
    assert lib.fheaes_pack_bits(None, None, 0, None, _native.HOST) == -1
    assert lib.fheaes_packed_words(None, 512) == 0
