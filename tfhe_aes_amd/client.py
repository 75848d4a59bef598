"""Host-side ``Client``: key generation, per-bit encryption, decryption and verification.

Mirrors /root/reference/src/client/client.rs:59-218 (``Client::new``, ``client_encrypt``,
``client_decrypt_and_verify``, ``test_verify``) over flat ``uint64`` arrays instead of
tfhe-rs containers.  The heavy loops live in csrc/client.c (libfheaes_client.so).

Array conventions (see include/fheaes.h):
  byte  = [8][kN+1]   (block j = bit j, LSB first)
  state = [16][8][kN+1], byte index = 4*col + row, byte 0 = MSB of the u128 (client.rs:126-129)
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

from . import _build
from .params import PARAM_OPT, CParams, WopbsParameters

_lib = None


def _load():
    global _lib
    if _lib is None:
        path = _build.build_client()
        lib = ctypes.CDLL(str(path))
        u8p = ctypes.POINTER(ctypes.c_uint8)
        u64p = ctypes.POINTER(ctypes.c_uint64)
        pp = ctypes.POINTER(CParams)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.fheaes_client_gen_secret_keys.argtypes = [pp, u32p, u8p, u8p]
        lib.fheaes_client_gen_ksk.argtypes = [pp, u32p, u32p, u8p, u8p, ctypes.c_double, u64p]
        lib.fheaes_client_gen_bsk.argtypes = [pp, u32p, u32p, u8p, u8p, ctypes.c_double, u64p]
        lib.fheaes_client_gen_pfpksk.argtypes = [pp, u32p, u32p, u8p, ctypes.c_double, u64p]
        lib.fheaes_client_mask_word.argtypes = [u32p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
        lib.fheaes_client_mask_word.restype = ctypes.c_uint64
        lib.fheaes_client_chacha20_block.argtypes = [u32p, ctypes.c_uint32, u32p, u32p]
        lib.fheaes_client_chacha20_block.restype = None
        lib.fheaes_client_encrypt_bits.argtypes = [pp, u32p, u8p, ctypes.c_double, u8p, ctypes.c_uint64, u64p]
        lib.fheaes_client_encrypt_bits_seeded.argtypes = [pp, u32p, u32p, ctypes.c_uint64, u8p, ctypes.c_double, u8p, ctypes.c_uint64, u64p]
        lib.fheaes_client_decrypt_bits.argtypes = [pp, u8p, u64p, ctypes.c_uint64, u8p, u64p]
        lib.fheaes_client_phase_small.argtypes = [pp, u8p, u64p, ctypes.c_uint64, u64p]
        lib.fheaes_client_glwe_phase.argtypes = [pp, u8p, u64p, ctypes.c_uint64, u64p]
        for f in (lib.fheaes_client_gen_secret_keys, lib.fheaes_client_gen_ksk, lib.fheaes_client_gen_bsk,
                  lib.fheaes_client_gen_pfpksk, lib.fheaes_client_encrypt_bits, lib.fheaes_client_encrypt_bits_seeded, lib.fheaes_client_decrypt_bits,
                  lib.fheaes_client_phase_small, lib.fheaes_client_glwe_phase):
            f.restype = None
        _lib = lib
    return _lib


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u64(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


def _u32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def random_key() -> np.ndarray:
    """a fresh 256-bit ChaCha20 key from the OS"""
    return np.frombuffer(os.urandom(32), dtype=np.uint32).copy()


def test_key(seed: int, purpose: int, counter: int = 0) -> np.ndarray:
    """TEST-ONLY deterministic 256-bit key: (seed, "test", purpose, counter) -- 64 bits of entropy at most"""
    seed &= (1 << 64) - 1
    return np.array([seed & 0xFFFFFFFF, seed >> 32, 0x74736574, purpose & 0xFFFFFFFF, counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, 0, 0], dtype=np.uint32)


MASK_TAG_KSK, MASK_TAG_BSK, MASK_TAG_PFPKSK = 3, 4, 5          # csrc/client.c, csrc/kern_linear.h
MASK_TAG_LWE = 6                                               # seeded input ciphertexts (SeededCiphertexts, fheaes_expand_lwe_seeded)


def chacha20_blocks(key8: np.ndarray, counters: np.ndarray, nonce0: int, nonce1: np.ndarray, nonce2: np.ndarray) -> np.ndarray:
    """RFC 8439 block function, vectorised: one block per entry of `counters` / `nonce1` / `nonce2` (broadcast together);
    returns uint32 [..., 16].  The host-side twin of csrc/client.c::chacha20_block and kern_linear.h::fheaes_chacha20_block."""
    counters, nonce1, nonce2 = np.broadcast_arrays(np.asarray(counters, dtype=np.uint32), np.asarray(nonce1, dtype=np.uint32),
                                                   np.asarray(nonce2, dtype=np.uint32))
    shape = counters.shape
    init = [np.full(shape, c, dtype=np.uint32) for c in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)]
    init += [np.full(shape, int(k), dtype=np.uint32) for k in np.asarray(key8, dtype=np.uint32)]
    init += [counters.copy(), np.full(shape, nonce0 & 0xFFFFFFFF, dtype=np.uint32), nonce1.copy(), nonce2.copy()]
    x = [v.copy() for v in init]

    def rotl(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return np.stack([x[i] + init[i] for i in range(16)], axis=-1)


def mask_words(mask_key: np.ndarray, tag: int, n_cts: int, words_per_ct: int, first_ct: int = 0) -> np.ndarray:
    """The public mask stream of csrc/client.c in numpy: [n_cts][words_per_ct] uint64 -- 64-bit word j % 8 of ChaCha20 block
    j / 8 under (mask key, nonce = (tag, ct)), for the ciphertexts ct = first_ct .. first_ct + n_cts - 1 (a 64-bit index, wrapping).
    Host-side twin of the engine's expansion kernels."""
    blocks = (words_per_ct + 7) // 8
    out = np.empty((n_cts, blocks * 8), dtype=np.uint64)
    step = max(1, (1 << 21) // blocks)                                     # bound the temporaries
    for c0 in range(0, n_cts, step):
        with np.errstate(over="ignore"):
            ct = np.arange(c0, min(n_cts, c0 + step), dtype=np.uint64) + np.uint64(int(first_ct) & (2 ** 64 - 1))
        w = chacha20_blocks(mask_key, np.arange(blocks, dtype=np.uint32)[None, :], tag, (ct & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None],
                            (ct >> np.uint64(32)).astype(np.uint32)[:, None])      # [cts][blocks][16]
        out[c0:c0 + len(ct)] = np.ascontiguousarray(w).view(np.uint64).reshape(len(ct), blocks * 8)
    return out[:, :words_per_ct]


@dataclass
class SeededServerKeys:
    """The evaluation keys as (public mask seed, bodies): every mask word is regenerated from ``mask_seed`` (on the GPU by
    ``fheaes_upload_keys_seeded``, on the host by ``expand()``), so 0.19 GB travel instead of 1.04 GB at PARAM_OPT.
    Bodies: KSK [kN][ks_level] words; BSK [n][pbs_level][k+1][N]; PFPKSK [k+1][kN+1][pfks_level][N]."""
    params: WopbsParameters
    mask_seed: np.ndarray          # the PUBLIC 256-bit mask key, uint32[8]
    ksk_body: np.ndarray
    bsk_body: np.ndarray
    pfpksk_body: np.ndarray

    @property
    def nbytes(self) -> int:
        return 32 + self.ksk_body.nbytes + self.bsk_body.nbytes + self.pfpksk_body.nbytes

    def expand(self) -> "ServerKeys":
        p = self.params
        k, N, n = p.k, p.N, p.n
        ksk = np.empty((p.big * p.ks_level, n + 1), dtype=np.uint64)
        ksk[:, :n] = mask_words(self.mask_seed, MASK_TAG_KSK, p.big * p.ks_level, n)
        ksk[:, n] = self.ksk_body.reshape(-1)
        nb = p.n * p.pbs_level * (k + 1)
        bsk = np.empty((nb, (k + 1) * N), dtype=np.uint64)
        bsk[:, :k * N] = mask_words(self.mask_seed, MASK_TAG_BSK, nb, k * N)
        bsk[:, k * N:] = self.bsk_body.reshape(nb, N)
        npf = (k + 1) * p.big1 * p.pfks_level
        pf = np.empty((npf, (k + 1) * N), dtype=np.uint64)
        pf[:, :k * N] = mask_words(self.mask_seed, MASK_TAG_PFPKSK, npf, k * N)
        pf[:, k * N:] = self.pfpksk_body.reshape(npf, N)
        return ServerKeys(p, ksk.reshape(-1), bsk.reshape(-1), pf.reshape(-1), mask_seed=self.mask_seed)

    def save(self, path) -> None:
        np.savez(path, shape=_param_shape(self.params), mask_seed=np.asarray(self.mask_seed, dtype=np.uint32),
                 ksk_body=self.ksk_body, bsk_body=self.bsk_body, pfpksk_body=self.pfpksk_body)

    @staticmethod
    def load(path, params: WopbsParameters) -> "SeededServerKeys":
        with np.load(path, allow_pickle=False) as z:
            if list(map(int, z["shape"])) != list(map(int, _param_shape(params))):
                raise ValueError("key file was generated for a different parameter set")
            out = SeededServerKeys(params, z["mask_seed"].astype(np.uint32), z["ksk_body"].astype(np.uint64), z["bsk_body"].astype(np.uint64),
                                   z["pfpksk_body"].astype(np.uint64))
        k, N = params.k, params.N
        want = (params.big * params.ks_level, params.n * params.pbs_level * (k + 1) * N, (k + 1) * params.big1 * params.pfks_level * N)
        if (out.ksk_body.size, out.bsk_body.size, out.pfpksk_body.size) != want or out.mask_seed.size != 8:
            raise ValueError("key file has the wrong array sizes")
        return out


@dataclass
class SeededCiphertexts:
    """One-bit LWE ciphertexts as (public mask key, first index, bodies): ciphertext t of the flattened list is
    [mask(first_index + t) | bodies[t]], its kN mask words the public ChaCha20 stream under (mask_key, MASK_TAG_LWE, first_index + t)
    (include/fheaes.h, "wire formats"), regenerated on the GPU by ``Server.expand`` and on the host by ``expand()``: 8 bytes per bit
    travel instead of 8 (kN + 1).  ``bodies`` keeps the logical shape, e.g. [16][8] for an AES-128 key.

    The rule the sender keeps: a (mask_key, index) pair serves ONE ciphertext, under ONE secret key -- two bodies over one mask give
    the difference of their messages away.  ``Client.encrypt_*_seeded`` draws a fresh mask key for every call."""
    params: WopbsParameters
    mask_key: np.ndarray           # the PUBLIC 256-bit mask key, uint32[8]
    first_index: int               # index of the first ciphertext in the mask stream (uint64)
    bodies: np.ndarray             # uint64[...]

    @property
    def nbytes(self) -> int:
        return 32 + 8 + 8 * int(self.bodies.size)

    def expand(self) -> np.ndarray:
        """the full ciphertexts, bodies.shape + (kN+1,): the numpy twin of fheaes_expand_lwe_seeded"""
        p = self.params
        b = np.ascontiguousarray(self.bodies, dtype=np.uint64)
        out = np.empty((b.size, p.big1), dtype=np.uint64)
        out[:, :p.big] = mask_words(self.mask_key, MASK_TAG_LWE, b.size, p.big, first_ct=self.first_index)
        out[:, p.big] = b.reshape(-1)
        return out.reshape(b.shape + (p.big1,))

    def save(self, path) -> None:
        np.savez(path, shape=_param_shape(self.params), mask_key=np.asarray(self.mask_key, dtype=np.uint32),
                 first_index=np.array([int(self.first_index)], dtype=np.uint64), bodies=np.asarray(self.bodies, dtype=np.uint64))

    @staticmethod
    def load(path, params: WopbsParameters) -> "SeededCiphertexts":
        with np.load(path, allow_pickle=False) as z:
            if list(map(int, z["shape"])) != list(map(int, _param_shape(params))):
                raise ValueError("ciphertext file was produced for a different parameter set")
            mask_key, first, bodies = z["mask_key"], z["first_index"], z["bodies"]
        if mask_key.shape != (8,) or mask_key.dtype != np.uint32 or first.shape != (1,) or first.dtype != np.uint64 or bodies.dtype != np.uint64:
            raise ValueError("ciphertext file has the wrong array shapes (mask_key uint32[8], first_index uint64[1], bodies uint64[...])")
        return SeededCiphertexts(params, mask_key.copy(), int(first[0]), bodies.copy())


# ---- modulus-switched packed ciphertexts (include/fheaes.h, "wire formats") -------------------------------------------------------------
PACKED_WIDTHS = tuple(range(8, 33)) + (64,)


def _check_width(width: int) -> int:
    width = int(width)
    if width not in PACKED_WIDTHS:
        raise ValueError("width must be in 8..32, or 64 for the words as they are (got %d)" % width)
    return width


def packed_mod_words(params: WopbsParameters, width: int) -> int:
    """words of one packed GLWE at `width` bits per word: (k+1) N width / 64 = (k+1) 8 width"""
    return (params.k + 1) * params.N * _check_width(width) // 64


def read_back_packed(packed: np.ndarray, params: WopbsParameters, width: int) -> np.ndarray:
    """[G][(k+1) 8 width] switched GLWEs -> [G][(k+1)N] 64-bit words x' = v << (64 - width): field e of a GLWE sits at bits
    [e width, (e+1) width) of its little-endian bit string.  width 64: the words themselves."""
    width = _check_width(width)
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    if width == 64:
        return packed
    fields = (params.k + 1) * params.N
    if packed.ndim != 2 or packed.shape[1] != fields * width // 64:
        raise ValueError("a GLWE at width %d has %d words, got shape %s" % (width, fields * width // 64, packed.shape))
    bit = np.arange(fields, dtype=np.uint64) * np.uint64(width)
    word, off = (bit >> np.uint64(6)).astype(np.int64), bit & np.uint64(63)
    straddles = off + np.uint64(width) > np.uint64(64)                     # then off > 0
    v = packed[:, word] >> off
    nxt = packed[:, np.minimum(word + 1, packed.shape[1] - 1)]             # the last field ends with the last word and never straddles
    hi_shift = np.where(straddles, np.uint64(64) - off, np.uint64(0))
    v = v | np.where(straddles, nxt << hi_shift, np.uint64(0))
    return v << np.uint64(64 - width)


def _param_shape(p: WopbsParameters) -> np.ndarray:
    return np.array([p.lwe_dimension, p.glwe_dimension, p.polynomial_size, p.pbs_base_log, p.pbs_level, p.ks_base_log,
                     p.ks_level, p.pfks_base_log, p.pfks_level, p.cbs_base_log, p.cbs_level], dtype=np.uint32)


# ---- packed round keys (include/fheaes.h, "packed round keys") ------------------------------------------------------------------------
AES_ROUNDS = {128: 10, 192: 12, 256: 14}


def packed_key_glwes(params: WopbsParameters, key_bits: int) -> int:
    """G = ceil((Nr+1) 128 / N) GLWEs hold one key's round keys: 3 / 4 / 4 for AES-128 / 192 / 256 (fheaes_round_keys_packed_glwes)"""
    if key_bits not in AES_ROUNDS:
        raise ValueError("key_bits must be 128, 192 or 256, got %r" % (key_bits,))
    return -(-(AES_ROUNDS[key_bits] + 1) * 128 // params.N)


@dataclass
class PackedRoundKeys:
    """The round keys of n_keys AES keys of one size, packed: ``data`` is [n_keys][G][(k+1)N] words (a host array, or a resident tensor),
    slice i word for word ``Server.pack`` of key i's round keys [Nr+1][16][8][kN+1] -- bit round * 128 + byte * 8 + bit in GLWE t // N,
    coefficient t % N, every key on a GLWE boundary.  61,440 bytes per AES-128 key at PARAM_OPT against 23,079,936.  Every ``Server``
    method that takes round keys takes this in their place and reads the key words from it; ``prk[i]`` / ``prk[a:b]`` are stores of their
    own (views), ``PackedRoundKeys.concat`` joins stores.  Encryption and decryption round keys look alike: the caller knows which it holds."""
    params: WopbsParameters
    key_bits: int
    data: object                   # uint64 ndarray or int64 tensor, [n_keys][G][(k+1)N]

    def __post_init__(self):
        want = (packed_key_glwes(self.params, self.key_bits), (self.params.k + 1) * self.params.N)
        shape = tuple(int(d) for d in self.data.shape)
        if len(shape) != 3 or shape[0] < 1 or shape[1:] != want:
            raise ValueError("packed AES-%d round keys are [n_keys][%d][%d] words with n_keys >= 1, got shape %s" % ((self.key_bits,) + want + (shape,)))

    @property
    def n_keys(self) -> int:
        return int(self.data.shape[0])

    @property
    def nbytes(self) -> int:
        return 8 * self.n_keys * int(self.data.shape[1]) * int(self.data.shape[2])

    def __len__(self) -> int:
        return self.n_keys

    def __getitem__(self, i) -> "PackedRoundKeys":
        if isinstance(i, slice):
            if i.step not in (None, 1):
                raise ValueError("a slice of a packed store is a contiguous range of keys")
            return PackedRoundKeys(self.params, self.key_bits, self.data[i])
        i = int(i)
        if not -self.n_keys <= i < self.n_keys:
            raise IndexError("key %d of a store of %d" % (i, self.n_keys))
        i %= self.n_keys
        return PackedRoundKeys(self.params, self.key_bits, self.data[i:i + 1])

    @staticmethod
    def concat(stores) -> "PackedRoundKeys":
        """one store holding the keys of `stores` in order: same parameter set, key size and memory space"""
        stores = list(stores)
        if not stores:
            raise ValueError("nothing to concatenate")
        first = stores[0]
        if any(s.params != first.params or s.key_bits != first.key_bits for s in stores):
            raise ValueError("stores of one parameter set and one key size concatenate, keys of several sizes do not share a store")
        if all(isinstance(s.data, np.ndarray) for s in stores):
            return PackedRoundKeys(first.params, first.key_bits, np.concatenate([s.data for s in stores]))
        if any(isinstance(s.data, np.ndarray) for s in stores):
            raise ValueError("all stores must live in the same memory space")
        import torch

        return PackedRoundKeys(first.params, first.key_bits, torch.cat([s.data for s in stores]))


@dataclass
class ServerKeys:
    """What ``client_encrypt`` hands to ``Server::new`` (client.rs:143): the evaluation keys."""

    params: WopbsParameters
    ksk: np.ndarray      # [kN][ks_level][n+1]
    bsk: np.ndarray      # [n][pbs_level][k+1][k+1][N]   standard domain
    pfpksk: np.ndarray   # [k+1][kN+1][pfks_level][(k+1)N]
    mask_seed: np.ndarray | None = None   # the public 256-bit mask key when the masks follow the stream of csrc/client.c (keys made by Client)

    def compress(self) -> "SeededServerKeys":
        """(mask_seed, bodies): drops every mask word (they are a function of the public mask seed)"""
        if self.mask_seed is None:
            raise ValueError("these keys do not carry a mask seed (not generated by Client)")
        p = self.params
        k, N, n = p.k, p.N, p.n
        ksk_b = np.ascontiguousarray(self.ksk.reshape(-1, n + 1)[:, n]).reshape(p.big, p.ks_level)
        bsk_b = np.ascontiguousarray(self.bsk.reshape(-1, (k + 1) * N)[:, k * N:]).reshape(p.n, p.pbs_level, k + 1, N)
        pf_b = np.ascontiguousarray(self.pfpksk.reshape(-1, (k + 1) * N)[:, k * N:]).reshape(k + 1, p.big1, p.pfks_level, N)
        return SeededServerKeys(p, self.mask_seed, ksk_b, bsk_b, pf_b)

    # The reference never serialises anything; these two helpers exist so that keys produced
    # elsewhere can be fed to the engine.  Plain .npz of uint64 arrays (no pickle), layouts as in include/fheaes.h.
    def save(self, path) -> None:
        extra = {} if self.mask_seed is None else {"mask_seed": np.asarray(self.mask_seed, dtype=np.uint32).reshape(8)}
        np.savez(path, shape=_param_shape(self.params), ksk=self.ksk, bsk=self.bsk, pfpksk=self.pfpksk, **extra)

    @staticmethod
    def load(path, params: WopbsParameters) -> "ServerKeys":
        with np.load(path, allow_pickle=False) as z:
            want = [params.lwe_dimension, params.glwe_dimension, params.polynomial_size, params.pbs_base_log, params.pbs_level,
                    params.ks_base_log, params.ks_level, params.pfks_base_log, params.pfks_level, params.cbs_base_log, params.cbs_level]
            if list(map(int, z["shape"])) != want:
                raise ValueError("key file was generated for a different parameter set")
            seed = None
            if "mask_seed" in z.files:          # the public mask key travels with the keys: compress() still works after a round trip
                seed = z["mask_seed"]
                if seed.shape != (8,) or seed.dtype != np.uint32:
                    raise ValueError("key file has a malformed mask_seed (expected uint32[8])")
                seed = seed.copy()
            keys = ServerKeys(params, z["ksk"].astype(np.uint64), z["bsk"].astype(np.uint64), z["pfpksk"].astype(np.uint64), seed)
        if (keys.ksk.size, keys.bsk.size, keys.pfpksk.size) != (params.ksk_words, params.bsk_words, params.pfpksk_words):
            raise ValueError("key file has the wrong array sizes")
        return keys


# ---- ciphertext interchange --------------------------------------------------------------------------------
# The reference hands whole states across in memory (client_encrypt / client_decrypt_and_verify, client.rs:123-175) and never
# serialises them.  These helpers give encrypted states and round keys an on-disk / on-wire form so that inputs produced
# elsewhere can be fed to the engine: a plain .npz of uint64 words (no pickle) in the layout of include/fheaes.h, with the
# parameter set and the kind recorded and checked on load.
CIPHERTEXT_KINDS = {
    "state": (16, 8),           # [blocks][16 bytes][8 bits][kN+1]      Server::aes_encrypt / aes_decrypt / add_scalar
    "round_keys": (11, 16, 8),  # [11][16][8][kN+1]                     Server::aes_key_expansion output ([13] / [15]: AES-192 / AES-256)
    "bytes": (8,),              # [n][8][kN+1]                          sbox / many_sbox inputs
    "packed": (),               # [G][(k+1)N]                           Server.pack output: N bits per GLWE ciphertext
    "packed_mod": (),           # [G][(k+1) 8 width]                    Server.pack(width=w) output, 8 <= w <= 32: the width travels with the words
    "packed_round_keys": (),    # [n_keys][G][(k+1)N]                   a PackedRoundKeys store: the key size travels with the words
}


def _kind_tail(kind: str, params: WopbsParameters, width: int = 64) -> tuple:
    """the trailing axes of an array of this kind: LWE ciphertexts of kN+1 words, or (packed) GLWE ciphertexts of (k+1)N, (k+1) 8 width switched"""
    if kind == "packed_mod":
        return (packed_mod_words(params, width),)
    return CIPHERTEXT_KINDS[kind] + (((params.k + 1) * params.N,) if kind == "packed" else (params.big1,))


def _has_kind_shape(shape, kind: str, params: WopbsParameters, width: int = 64) -> bool:
    tail = _kind_tail(kind, params, width)
    if kind in ("packed", "packed_mod"):
        return len(shape) == 2 and shape[-1:] == tail
    if kind == "round_keys" and len(shape) >= 4 and shape[-4] in (13, 15):       # Nr + 1 round keys of AES-192 / AES-256
        return shape[-3:] == tail[1:]
    return shape[-len(tail):] == tail


def _kind_width(kind: str, width) -> int:
    """the width argument of save / load: the "packed_mod" kind needs one in 8..32, no other kind takes one"""
    if kind != "packed_mod":
        if width is not None:
            raise ValueError("only the 'packed_mod' kind has a width")
        return 64
    if width is None or _check_width(width) == 64:
        raise ValueError("the 'packed_mod' kind needs its width, 8..32 (64-bit words are the 'packed' kind)")
    return int(width)


def _save_packed_round_keys(path, params: WopbsParameters, prk) -> None:
    if not isinstance(prk, PackedRoundKeys) or not isinstance(prk.data, np.ndarray):
        raise ValueError("the 'packed_round_keys' kind saves a PackedRoundKeys on the host")
    if prk.params != params:
        raise ValueError("these keys were packed for %s, not %s" % (prk.params.name, params.name))
    np.savez(path, shape=_param_shape(params), kind=np.frombuffer(b"packed_round_keys".ljust(24, b"\0"), dtype=np.uint8),
             key_bits=np.array([prk.key_bits], dtype=np.uint32), words=np.ascontiguousarray(prk.data, dtype=np.uint64))


def save_ciphertexts(path, params: WopbsParameters, kind: str, words, width: int | None = None) -> None:
    """`words`: an array of the kind's shape; for "packed_round_keys" a PackedRoundKeys (its key size is recorded)"""
    if kind not in CIPHERTEXT_KINDS:
        raise ValueError("kind must be one of %s" % ", ".join(CIPHERTEXT_KINDS))
    if kind == "packed_round_keys":
        _kind_width(kind, width)
        return _save_packed_round_keys(path, params, words)
    w = _kind_width(kind, width)
    tail = _kind_tail(kind, params, w)
    a = np.ascontiguousarray(words, dtype=np.uint64)
    if not _has_kind_shape(a.shape, kind, params, w):
        raise ValueError("a %r array must end in shape %r, got %r" % (kind, tail, a.shape))
    extra = {"width": np.array([w], dtype=np.uint32)} if kind == "packed_mod" else {}
    np.savez(path, shape=_param_shape(params), kind=np.frombuffer(kind.encode().ljust(16, b"\0"), dtype=np.uint8), words=a, **extra)


def load_ciphertexts(path, params: WopbsParameters, kind: str, width: int | None = None, key_bits: int | None = None):
    """the array saved under `kind`; for "packed_round_keys" a PackedRoundKeys, and `key_bits` (if given) must be the recorded key size"""
    w = _kind_width(kind, width)
    if key_bits is not None and kind != "packed_round_keys":
        raise ValueError("only the 'packed_round_keys' kind has a key size")
    with np.load(path, allow_pickle=False) as z:
        if list(map(int, z["shape"])) != list(map(int, _param_shape(params))):
            raise ValueError("ciphertext file was produced for a different parameter set")
        got = bytes(z["kind"]).rstrip(b"\0").decode()
        if got != kind:
            raise ValueError("ciphertext file holds %r, expected %r" % (got, kind))
        if kind == "packed_round_keys":
            if "key_bits" not in z.files or z["key_bits"].shape != (1,):
                raise ValueError("ciphertext file does not record the key size of its packed round keys")
            have = int(z["key_bits"][0])
            if key_bits is not None and have != int(key_bits):
                raise ValueError("ciphertext file holds packed AES-%d round keys, expected AES-%d" % (have, int(key_bits)))
            return PackedRoundKeys(params, have, z["words"].astype(np.uint64))      # the shape is checked against the key size there
        if kind == "packed_mod" and ("width" not in z.files or z["width"].shape != (1,) or int(z["width"][0]) != w):
            raise ValueError("ciphertext file holds words of width %s, expected %d" % (int(z["width"][0]) if "width" in z.files else "?", w))
        a = z["words"].astype(np.uint64)
    if not _has_kind_shape(a.shape, kind, params, w):
        raise ValueError("ciphertext file has the wrong array shape")
    return a


def u128_to_bytes(x: int) -> list[int]:
    """state byte i = bits [8*(15-i), 8*(16-i)) of the u128 (client.rs:126-129)."""
    return [(x >> (8 * (15 - i))) & 0xFF for i in range(16)]


def bytes_to_u128(b) -> int:
    v = 0
    for i, x in enumerate(b):
        v |= int(x) << (8 * (15 - i))
    return v


class Client:
    """``Client::new`` (client.rs:70): generates the secret and evaluation keys.

    All randomness is ChaCha20 (csrc/client.c).  ``seed=None`` (the default, the counterpart of the reference's OS-seeded
    generators, client.rs:106-107): the 256-bit secret key-generation key, the 256-bit PUBLIC mask key and a fresh 256-bit key
    for every encryption call come from ``os.urandom``.  An explicit integer ``seed`` is the TEST-ONLY deterministic mode
    (golden vectors, parity tests, synthetic bench data): all keys derive from that one number (at most 64 bits of entropy)
    and encryption call i is reproducible -- two processes with the same seed then produce the same masks and noise, which
    is exactly what fixtures need and what real use must never do.

    The ``encrypt_*_seeded`` methods give the same encryptions as ``SeededCiphertexts`` (public mask key, first index, bodies).  The
    rule they keep: a (mask key, index) pair is used for one ciphertext only, under one secret key -- every seeded call draws a fresh
    mask key from ``os.urandom`` (test mode: ``test_key(seed, 4, call counter)``), the noise comes from the secret per-call key."""

    def __init__(self, number_of_outputs: int = 1, iv: int = 0, key: int = 0,
                 params: WopbsParameters = PARAM_OPT, seed: int | None = None):
        self.params = params
        self.number_of_outputs = number_of_outputs
        self.iv = iv
        self.key = key
        self.deterministic = seed is not None
        self.test_seed = int(seed) if seed is not None else None
        self.seed = test_key(self.test_seed, 1) if self.deterministic else random_key()          # SECRET
        self.mask_seed = test_key(self.test_seed, 2) if self.deterministic else random_key()     # PUBLIC: travels with seeded keys
        self._enc_counter = 0
        lib = _load()
        self._c = params.c_struct()
        self.lwe_sk = np.zeros(params.n, dtype=np.uint8)
        self.glwe_sk = np.zeros(params.big, dtype=np.uint8)
        lib.fheaes_client_gen_secret_keys(ctypes.byref(self._c), _u32(self.seed), _u8(self.lwe_sk), _u8(self.glwe_sk))
        self._server_keys = None

    # -- keys -----------------------------------------------------------------
    def server_keys(self) -> ServerKeys:
        """gen_keys_radix + WopbsKey::new_wopbs_key_only_for_wopbs (client.rs:106-107)."""
        if self._server_keys is None:
            p, lib = self.params, _load()
            ksk = np.empty(p.ksk_words, dtype=np.uint64)
            bsk = np.empty(p.bsk_words, dtype=np.uint64)
            pf = np.empty(p.pfpksk_words, dtype=np.uint64)
            lib.fheaes_client_gen_ksk(ctypes.byref(self._c), _u32(self.seed), _u32(self.mask_seed), _u8(self.lwe_sk), _u8(self.glwe_sk),
                                      p.lwe_noise_std, _u64(ksk))
            lib.fheaes_client_gen_bsk(ctypes.byref(self._c), _u32(self.seed), _u32(self.mask_seed), _u8(self.lwe_sk), _u8(self.glwe_sk),
                                      p.glwe_noise_std, _u64(bsk))
            lib.fheaes_client_gen_pfpksk(ctypes.byref(self._c), _u32(self.seed), _u32(self.mask_seed), _u8(self.glwe_sk), p.pfks_noise_std,
                                         _u64(pf))
            self._server_keys = ServerKeys(p, ksk, bsk, pf, mask_seed=self.mask_seed)
        return self._server_keys

    # -- encryption -----------------------------------------------------------
    def encrypt_bits(self, bits: np.ndarray) -> np.ndarray:
        """LWE encryptions (big key, glwe noise: EncryptionKeyChoice::Big) of an array of bits; adds a last axis kN+1."""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        out = np.empty(bits.shape + (self.params.big1,), dtype=np.uint64)
        self._enc_counter += 1
        enc_key = test_key(self.test_seed, 3, self._enc_counter) if self.deterministic else random_key()
        _load().fheaes_client_encrypt_bits(ctypes.byref(self._c), _u32(enc_key), _u8(self.glwe_sk),
                                           self.params.glwe_noise_std, _u8(bits), bits.size, _u64(out))
        return out

    def encrypt_bytes(self, values) -> np.ndarray:
        """cks.encrypt_without_padding per byte (client.rs:128): [len][8][kN+1]."""
        v = np.asarray(values, dtype=np.uint64).reshape(-1)
        bits = ((v[:, None] >> np.arange(8, dtype=np.uint64)[None, :]) & 1).astype(np.uint8)
        return self.encrypt_bits(bits)

    # The same four as (public mask key, first index, bodies): 8 bytes per bit on the wire instead of 8 (kN + 1).  A (mask key, index) pair
    # serves ONE ciphertext under ONE secret key, so every call draws a FRESH public mask key from os.urandom (deterministic test mode:
    # test_key(seed, 4, call counter)); the noise comes from the secret per-call key, as in encrypt_bits.  Server.expand regenerates the masks.
    def encrypt_bits_seeded(self, bits: np.ndarray, first_index: int = 0) -> SeededCiphertexts:
        """encrypt_bits in seeded form: bodies of the shape of `bits`; ciphertext t of the flattened list uses mask index first_index + t"""
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        first_index = int(first_index)
        if not 0 <= first_index < 1 << 64:
            raise ValueError("first_index is a uint64")
        bodies = np.empty(bits.shape, dtype=np.uint64)
        self._enc_counter += 1
        enc_key = test_key(self.test_seed, 3, self._enc_counter) if self.deterministic else random_key()        # SECRET
        mask_key = test_key(self.test_seed, 4, self._enc_counter) if self.deterministic else random_key()       # PUBLIC, this call only
        _load().fheaes_client_encrypt_bits_seeded(ctypes.byref(self._c), _u32(enc_key), _u32(mask_key), first_index, _u8(self.glwe_sk),
                                                  self.params.glwe_noise_std, _u8(bits), bits.size, _u64(bodies))
        return SeededCiphertexts(self.params, mask_key, first_index, bodies)

    def encrypt_bytes_seeded(self, values, first_index: int = 0) -> SeededCiphertexts:
        """encrypt_bytes in seeded form: bodies [len][8]"""
        v = np.asarray(values, dtype=np.uint64).reshape(-1)
        bits = ((v[:, None] >> np.arange(8, dtype=np.uint64)[None, :]) & 1).astype(np.uint8)
        return self.encrypt_bits_seeded(bits, first_index)

    def encrypt_u128_seeded(self, x: int, first_index: int = 0) -> SeededCiphertexts:
        """one AES state / key in seeded form: bodies [16][8]"""
        return self.encrypt_bytes_seeded(u128_to_bytes(x), first_index)

    def encrypt_aes_key_seeded(self, key: bytes, first_index: int = 0) -> SeededCiphertexts:
        """encrypt_aes_key in seeded form: bodies [len][8], 8 len(key) + 40 bytes in all (1,064 for AES-128 instead of 2 MB at PARAM_OPT)"""
        if len(key) not in (16, 24, 32):
            raise ValueError("an AES key has 16, 24 or 32 bytes, got %d" % len(key))
        return self.encrypt_bytes_seeded(list(key), first_index)

    def trivial_bytes(self, values) -> np.ndarray:
        """noise-free "encryptions" of PUBLIC bytes that anyone can write down: mask 0, body = bit << 63; [..., 8, kN+1] for values
        of shape [...].  A legal input wherever an encrypted byte is (a state of 16 n such bytes is what Server.aes_encrypt_public
        computes on, word for word)."""
        v = np.asarray(values, dtype=np.uint64)
        out = np.zeros(v.shape + (8, self.params.big1), dtype=np.uint64)
        out[..., self.params.big] = ((v[..., None] >> np.arange(8, dtype=np.uint64)) & np.uint64(1)) << np.uint64(63)
        return out

    def encrypt_u128(self, x: int) -> np.ndarray:
        """one AES state / key: [16][8][kN+1]"""
        return self.encrypt_bytes(u128_to_bytes(x))

    def encrypt_aes_key(self, key: bytes) -> np.ndarray:
        """an AES key of 16 / 24 / 32 bytes, in FIPS-197 order (byte 0 first): [len][8][kN+1], what Server.aes_key_expansion takes"""
        if len(key) not in (16, 24, 32):
            raise ValueError("an AES key has 16, 24 or 32 bytes, got %d" % len(key))
        return self.encrypt_bytes(list(key))

    def client_encrypt(self):
        """client.rs:123: (server keys, encrypted iv, encrypted key)."""
        return self.server_keys(), self.encrypt_u128(self.iv), self.encrypt_u128(self.key)

    # -- decryption -----------------------------------------------------------
    def decrypt_bits(self, lwe: np.ndarray, return_phase: bool = False):
        lwe = np.ascontiguousarray(lwe, dtype=np.uint64)
        assert lwe.shape[-1] == self.params.big1
        shape = lwe.shape[:-1]
        bits = np.empty(shape, dtype=np.uint8)
        phase = np.empty(shape, dtype=np.uint64)
        count = int(np.prod(shape)) if shape else 1
        _load().fheaes_client_decrypt_bits(ctypes.byref(self._c), _u8(self.glwe_sk), _u64(lwe), count, _u8(bits), _u64(phase))
        return (bits, phase) if return_phase else bits

    def decrypt_bytes(self, lwe: np.ndarray) -> np.ndarray:
        """[..., 8, kN+1] -> [...] byte values (decrypt_without_padding, client.rs:154)."""
        bits = self.decrypt_bits(lwe).astype(np.uint64)
        return (bits << np.arange(8, dtype=np.uint64)).sum(axis=-1).astype(np.uint8)

    def decrypt_u128(self, state: np.ndarray) -> int:
        return bytes_to_u128(self.decrypt_bytes(state).reshape(16))

    def phase_small(self, lwe_small: np.ndarray) -> np.ndarray:
        lwe_small = np.ascontiguousarray(lwe_small, dtype=np.uint64)
        shape = lwe_small.shape[:-1]
        out = np.empty(shape, dtype=np.uint64)
        _load().fheaes_client_phase_small(ctypes.byref(self._c), _u8(self.lwe_sk), _u64(lwe_small), out.size, _u64(out))
        return out

    def glwe_phase(self, glwe: np.ndarray) -> np.ndarray:
        """[..., (k+1)N] -> [..., N] phases B - sum A_m S_m"""
        glwe = np.ascontiguousarray(glwe, dtype=np.uint64)
        shape = glwe.shape[:-1]
        out = np.empty(shape + (self.params.N,), dtype=np.uint64)
        count = int(np.prod(shape)) if shape else 1
        _load().fheaes_client_glwe_phase(ctypes.byref(self._c), _u8(self.glwe_sk), _u64(glwe), count, _u64(out))
        return out

    def decrypt_packed(self, packed: np.ndarray, m: int, return_phase: bool = False, width: int = 64):
        """[G][(k+1)N] from Server.pack -> the m bits it holds (bit t: GLWE t // N, coefficient t % N), decoded like decrypt_bits
        (message at the MSB, rounded); with `return_phase` also the m phases B - sum A_j S_j of those coefficients.  `width` < 64: the
        modulus-switched form [G][(k+1) 8 width] of Server.pack(width=...), read back to 64-bit words first."""
        p = self.params
        packed = read_back_packed(packed, p, width)
        m = int(m)
        if packed.shape != ((m + p.N - 1) // p.N, (p.k + 1) * p.N):
            raise ValueError("%d bits are packed as [%d][%d] words, got shape %s" % (m, (m + p.N - 1) // p.N, (p.k + 1) * p.N, packed.shape))
        phase = self.glwe_phase(packed).reshape(-1)[:m]
        bits = ((phase + np.uint64(1 << 62)) >> np.uint64(63)).astype(np.uint8)
        return (bits, phase) if return_phase else bits

    def decrypt_packed_bytes(self, packed: np.ndarray, n_bytes: int, width: int = 64) -> np.ndarray:
        """the packed form of [n_bytes][8][kN+1] (states, blocks of states: any array of bytes) -> uint8[n_bytes]"""
        bits = self.decrypt_packed(packed, 8 * int(n_bytes), width=width).reshape(-1, 8).astype(np.uint64)
        return (bits << np.arange(8, dtype=np.uint64)).sum(axis=-1).astype(np.uint8)

    # -- verification (client.rs:147-216) --------------------------------------
    def client_decrypt_and_verify(self, states) -> None:
        """decrypt every CTR output block and compare with AES-128(key, iv + index)."""
        from .aes_clear import aes128_encrypt_block

        assert len(states) == self.number_of_outputs
        for index, st in enumerate(states):
            got = self.decrypt_u128(st)
            want = aes128_encrypt_block(self.key, (self.iv + index) & ((1 << 128) - 1))
            assert got == want, "block %d: FHE %032x != AES %032x" % (index, got, want)

    def test_verify(self, state_enc, state_dec) -> None:
        from .aes_clear import aes128_encrypt_block

        got = self.decrypt_u128(state_enc)
        want = aes128_encrypt_block(self.key, self.iv)
        assert got == want, "enc: FHE %032x != AES %032x" % (got, want)
        back = self.decrypt_u128(state_dec)
        assert back == self.iv, "dec: FHE %032x != %032x" % (back, self.iv)
