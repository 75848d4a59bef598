"""What the CMAC tests share: the known answers as data (computed with aes_clear.aes_encrypt_block following SP 800-38B 6; the AES-128 /
192 / 256 sets are the examples of RFC 4493 4 and SP 800-38B D.1 - D.3), the subkey rows restated in Python integers, and the
compositions of older entry points that the CMAC calls must equal word for word.  A plain module like ccm.py: imported by name, not
collected."""
import numpy as np

import ccm
from tfhe_aes_amd import aes_clear

h = bytes.fromhex

MESSAGE = h("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51" "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
LENGTHS = (0, 16, 40, 64)

# key bits -> (key, K1, K2, the tag of the first 0, 16, 40 and 64 bytes of MESSAGE)
VECTORS = {
    128: (h("2b7e151628aed2a6abf7158809cf4f3c"), h("fbeed618357133667c85e08f7236a8de"), h("f7ddac306ae266ccf90bc11ee46d513b"),
          (h("bb1d6929e95937287fa37d129b756746"), h("070a16b46b4d4144f79bdd9dd04a287c"), h("dfa66747de9ae63030ca32611497c827"),
           h("51f0bebf7e3b9d92fc49741779363cfe"))),
    192: (h("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"), h("448a5b1c93514b273ee6439dd4daa296"), h("8914b63926a2964e7dcc873ba9b5452c"),
          (h("d17ddf46adaacde531cac483de7a9367"), h("9e99a7bf31e710900662f65e617c5184"), h("8a1de5be2eb31aad089a82e6ee908b0e"),
           h("a1d5df0eed790f794d77589659f39a11"))),
    256: (h("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"), h("cad1ed03299eedac2e9a99808621502f"),
          h("95a3da06533ddb585d3533010c42a0d9"),
          (h("028962f61b7bf89efc6b551f4667d983"), h("28a7023f452e8f82bd4bf28d8c37c35c"), h("aaf3d8f1de5640c232f5b169b9c911e6"),
           h("e1992190549f6ed5696a2c056c315410"))),
}
L_128 = h("7df76b0c1ab899b33e42f047b91b546f")


def degree(i):
    """the degree of state bit i (byte i // 8, bit i % 8 LSB first) of a CMAC block, a big-endian integer; its own inverse"""
    return 8 * (15 - i // 8) + i % 8


def double(v, times=1):
    """v * x^times in GF(2^128) mod x^128 + x^7 + x^2 + x + 1 on a Python integer whose bit d is degree d"""
    for _ in range(times):
        v <<= 1
        if v >> 128:
            v = (v ^ 0x87) & ((1 << 128) - 1)
    return v


def rows(which):
    """rows[i]: the sorted source bits of output bit i of L * x^(which + 1), from the doubling applied to the 128 unit vectors"""
    out = [[] for _ in range(128)]
    for src in range(128):
        image = double(1 << degree(src), which + 1)
        for i in range(128):
            if image >> degree(i) & 1:
                out[i].append(src)
    return out


def np_double(l):
    """fheaes_cmac_double in numpy: l [n_keys][128][kN+1] -> [n_keys][2][128][kN+1], wrapping sums over the rows above"""
    out = np.zeros((l.shape[0], 2) + l.shape[1:], dtype=np.uint64)
    for which in range(2):
        for i, srcs in enumerate(rows(which)):
            for s in srcs:
                out[:, which, i] += l[:, s]
    return out


def compose_subkeys(srv, client, rk, refresh_k=True):
    """fheaes_aes_cmac_subkeys_keyed out of older calls and fheaes_cmac_double, on host arrays: the public call on one zero block per key,
    the identity WoPBS XTS uses for its anchors, the gather, the identity WoPBS again (refresh_k False: left out, the raw subkeys).
    rk [n_keys][Nr+1][16][8][kN+1]; returns [n_keys][2][16][8][kN+1]"""
    from oracle import oracle as orc
    from xts import LUTSET_IDENTITY

    lw = client.params.big1
    n_keys = len(rk)
    ident = list(orc.build_lutset(LUTSET_IDENTITY))
    refresh = lambda x: np.ascontiguousarray(srv.many_wopbs_without_padding(np.ascontiguousarray(x).reshape(-1, 8, lw), ident)[:, 0]).reshape(x.shape)
    l = refresh(srv.aes_encrypt_public_keyed(rk, list(range(n_keys)), [0] * n_keys))
    raw = np.zeros((n_keys, 2, 16, 8, lw), dtype=np.uint64)
    srv.engine.cmac_double(l, n_keys, raw)
    return refresh(raw) if refresh_k else raw


def mac_streams(streams, subkeys):
    """CMAC streams (key_index, message) as ccm.compose_mac takes them: the padded blocks, the last one with its subkey as addend"""
    lw = subkeys.shape[-1]
    out = []
    for key_index, msg in streams:
        blocks, which = aes_clear.cmac_blocks(msg)
        enc = np.zeros((len(blocks), 16, 8, lw), dtype=np.uint64)
        enc[-1] = subkeys[key_index, which]
        out.append((key_index, blocks, enc, [0] * (len(blocks) - 1) + [16]))
    return out


def compose_verify(srv, client, rk, messages, subkeys):
    """aes_cmac_verify out of older calls: compose_mac over mac_streams, diff = X + trivial(tag) on 8t rows, the two WoPBS of ccm.tag_luts"""
    lw = client.params.big1
    n = len(messages)
    x = ccm.compose_mac(srv, client, rk, mac_streams([m[:2] for m in messages], subkeys))
    diff = np.zeros((n, 128, lw), dtype=np.uint64)
    for s, (_, _, tag) in enumerate(messages):
        t = len(tag)
        full = x[s] + client.trivial_bytes(list(tag) + [0] * (16 - t))
        diff[s, :8 * t] = full.reshape(128, lw)[:8 * t]
    ne0, eq0 = ccm.tag_luts()
    w1 = srv.many_wopbs_without_padding(diff.reshape(16 * n, 8, lw), [ne0])
    w2 = srv.many_wopbs_without_padding(np.ascontiguousarray(w1[:, 0, 0, :]).reshape(n, 16, lw), [eq0])
    return np.ascontiguousarray(w2[:, 0, 0, :])
