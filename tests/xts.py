"""What the XTS tests share: the IEEE 1619 vectors as data, the multiplication by alpha^j in Python integers, the rows it gives, and
the composition of entry points older than fheaes_aes_xts_decrypt_bits that the call must equal word for word.  A plain module like
public_modes.py: imported by name, not collected."""
import numpy as np

from tfhe_aes_amd import aes_clear

h = bytes.fromhex
PT512 = bytes(range(256)) * 2
# IEEE 1619-2007 annex B: (key1, key2, data-unit number, plaintext, ciphertext or (its first bytes, its last bytes))
VECTORS = {
    1: (bytes(16), bytes(16), 0, bytes(32), h("917cf69ebd68b2ec9b9fe9a3eadda692cd43d2f59598ed858c02c2652fbf922e")),
    2: (h("11" * 16), h("22" * 16), 0x3333333333, h("44" * 32), h("c454185e6a16936e39334038acef838bfb186fff7480adc4289382ecd6d394f0")),
    3: (h("fffefdfcfbfaf9f8f7f6f5f4f3f2f1f0"), h("22" * 16), 0x3333333333, h("44" * 32),
        h("af85336b597afc1a900b2eb21ec949d292df4c047e0b21532186a5971a227a89")),
    4: (h("27182818284590452353602874713526"), h("31415926535897932384626433832795"), 0, PT512,
        (h("27a7479befa1d476489f308cd4cfa6e2a96e4bbe3208ff25287dd3819616e89c"), h("0a282df920147beabe421ee5319d0568"))),
    10: (h("2718281828459045235360287471352662497757247093699959574966967627"),
         h("3141592653589793238462643383279502884197169399375105820974944592"), 0xFF, PT512,
         (h("1c3b3a102f770386e4836c99e370cf9b"), h("c4f36ffda9fcea70b9c6e693e148c151"))),
}
SEGMENT, MAX_OFFSET = 120, 121
LUTSET_IDENTITY = 4


def matches(ciphertext: bytes, expected) -> bool:
    if isinstance(expected, bytes):
        return ciphertext == expected
    return ciphertext.startswith(expected[0]) and ciphertext.endswith(expected[1])


def mul_alpha(t: int, j: int) -> int:
    """t * alpha^j by j doublings in Python integers: bit d of t is degree d, x^128 = x^7 + x^2 + x + 1"""
    for _ in range(j):
        t <<= 1
        if t >> 128:
            t = (t & ((1 << 128) - 1)) ^ 0x87
    return t


def rows(j: int):
    """[128] sorted source bits of every output bit of the multiplication by alpha^j: column s of the map is alpha^j * x^s"""
    out = [[] for _ in range(128)]
    for s in range(128):
        v = mul_alpha(1 << s, j)
        for i in range(128):
            if (v >> i) & 1:
                out[i].append(s)
    return out


def np_tweaks(anchor, offsets):
    """anchor [128][kN+1] -> [len(offsets)][128][kN+1]: every row one wrapping uint64 sum of the anchor's rows"""
    out = np.zeros((len(offsets),) + anchor.shape, dtype=np.uint64)
    for t, j in enumerate(offsets):
        for i, src in enumerate(rows(j)):
            for s in src:
                out[t, i] += anchor[s]
    return out


def tweak_bytes(key2, sector, j):
    """the 16 bytes of T_j = E_K2(tweak block) * alpha^j"""
    t = int.from_bytes(aes_clear.aes_encrypt_block(key2, aes_clear.xts_tweak_block(sector)).to_bytes(16, "big"), "little")
    return list(mul_alpha(t, j).to_bytes(16, "little"))


def compose(srv, client, dw1, rk2, sectors, ciphertext, blocks_per_unit, first_block=0):
    """fheaes_aes_xts_decrypt_bits out of older calls and numpy, on host arrays: aes_encrypt_public of the tweak blocks, the identity
    WoPBS, the rows as wrapping sums, the identity WoPBS again chained through the anchors at 120, + trivial(C), aes_decrypt_equivalent,
    + T.  sectors: one data-unit number per unit from unit 0; ciphertext: bytes.  Returns (words [n][16][8][kN+1], the refreshed T)."""
    from oracle import oracle as orc

    lw = client.params.big1
    ident = list(orc.build_lutset(LUTSET_IDENTITY))
    refresh = lambda x: srv.many_wopbs_without_padding(np.ascontiguousarray(x).reshape(-1, 8, lw), ident)[:, 0].reshape(x.shape)
    n, bpu = len(ciphertext) // 16, blocks_per_unit
    blocks = [first_block + b for b in range(n)]
    units = sorted({g // bpu for g in blocks})
    e_k2 = srv.aes_encrypt_public(rk2, [aes_clear.xts_tweak_block(sectors[u]) for u in units])
    anchors = refresh(e_k2.reshape(len(units), 128, lw))
    tweak = {}
    for u, anchor in zip(units, anchors):
        mine = [g % bpu for g in blocks if g // bpu == u]
        for s in range(max(mine) // SEGMENT + 1):
            offsets = sorted({j % SEGMENT for j in mine if j // SEGMENT == s} | ({SEGMENT} if max(mine) // SEGMENT > s else set()))
            fresh = refresh(np_tweaks(anchor, offsets))
            for j, t in zip(offsets, fresh):
                if j < SEGMENT:
                    tweak[u * bpu + SEGMENT * s + j] = t
                else:
                    anchor = t
    T = np.stack([tweak[g] for g in blocks]).reshape(n, 16, 8, lw)
    state = client.trivial_bytes(np.frombuffer(ciphertext, dtype=np.uint8).reshape(n, 16)) + T
    srv.aes_decrypt_equivalent(dw1, state)
    return state + T, T
