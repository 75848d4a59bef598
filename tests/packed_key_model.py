"""What the packed-round-key tests share: the numpy model of "key word from the packed form" (include/fheaes.h, "packed round keys"),
built on aes_model.ref_unpack, and the cases the GPU tests run.  A plain module like edge_words.py: imported by name, not collected.

A store is flat: key j holds G = ceil((Nr+1) 128 / N) GLWEs of (k+1)N words from word j G (k+1)N on, and bit
t = round * 128 + byte * 8 + bit of that key sits in GLWE t // N, coefficient t % N."""
import numpy as np

from aes_model import ref_unpack
from aes_vectors import BASE, F1_PT, MASK128, NR

# the blocks of test_gpu_multi_key.py
KOB = [0, 2, 1, 0, 2]                                   # 5 blocks over 3 keys
PTS = [BASE, 0, MASK128, 0x3243F6A8885A308D313198A2E0370734, BASE + 1]
PUBLIC_CASES = {"grouped": ([0, 0, 1, 1], [BASE, BASE + 1, BASE, BASE + 1]), "interleaved": ([0, 1, 1, 0], [BASE, BASE, BASE + 1, BASE + 1])}
STREAMS = [(0, BASE, 0, 3, None),                       # two streams under key 0 with different IVs,
           (0, BASE ^ (0xA5 << 64), 1, 2, F1_PT[:2]),   # one of them with data
           (2, BASE | 0xFE, 0, 3, None)]                # ..FE ..FF, then the low counter byte wraps


def aes_keys(bits, n=3):
    """n distinct clear AES keys of `bits` bits (the keys of test_gpu_multi_key.py)"""
    rng = np.random.default_rng(0xA5 + bits)
    return [rng.bytes(bits // 8) for _ in range(n)]


def key_glwes(p, key_bits):
    return -(-(NR[key_bits] + 1) * 128 // p.N)


def key_bit(rnd, byte, bit):
    return rnd * 128 + byte * 8 + bit


def key_lwe(store, key_bits, j, t, p):
    """the LWE ciphertext [kN+1] of bit t of key j, read from the flat words of a store: the GLWE found by the address arithmetic of the
    header, then ref_unpack's extraction of its coefficient t % N"""
    gw = (p.k + 1) * p.N
    flat = np.ascontiguousarray(store, dtype=np.uint64).reshape(-1)
    at = j * key_glwes(p, key_bits) * gw + (t // p.N) * gw
    i = t % p.N
    return ref_unpack(flat[at:at + gw].reshape(1, gw), i + 1, p)[i]


def key_word(store, key_bits, j, t, w, p):
    """word w of that ciphertext by the rule of the kernels' device function: body glwe[kN + i]; mask word w = pN + c is
    glwe[pN + ((i - c) & (N - 1))], negated when c > i"""
    N, gw = p.N, (p.k + 1) * p.N
    flat = np.ascontiguousarray(store, dtype=np.uint64).reshape(-1)
    glwe = flat[j * key_glwes(p, key_bits) * gw + (t // N) * gw:][:gw]
    i = t % N
    if w == p.k * N:
        return int(glwe[p.k * N + i])
    c = w % N
    v = int(glwe[(w - c) + ((i - c) & (N - 1))])
    return v if c <= i else (-v) % (1 << 64)
