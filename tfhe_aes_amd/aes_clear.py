"""Clear-text AES (FIPS-197: 128-, 192- and 256-bit keys) and the S-Box LUT functions of the path.

Stands in for (a) the RustCrypto ``aes`` crate the reference verifies against
(/root/reference/src/client/client.rs:166-171) and (b) the reference's tables and GF(2^8)
helpers (src/tables/table.rs, src/server/sbox/sbox.rs:20-42).  Tables are derived from the
field definition (inverse in GF(2^8) mod x^8+x^4+x^3+x+1, then the FIPS-197 affine map), not
copied; tests pin them against FIPS-197 values.  The reference is AES-128 only; the other two key sizes are pinned by the
vectors of FIPS-197 appendices A and C and of SP 800-38A (tests/test_aes_key_sizes_cpu.py).
"""
from __future__ import annotations


def gf_mul(a: int, b: int) -> int:
    r = 0
    for _ in range(8):
        if b & 1:
            r ^= a
        hi = a & 0x80
        a = (a << 1) & 0xFF
        if hi:
            a ^= 0x1B
        b >>= 1
    return r


def _make_tables():
    sbox = [0] * 256
    inv = [0] * 256
    for x in range(256):
        y = 0
        if x:
            for c in range(1, 256):
                if gf_mul(x, c) == 1:
                    y = c
                    break
        s = v = y
        for _ in range(4):
            v = ((v << 1) | (v >> 7)) & 0xFF
            s ^= v
        s ^= 0x63
        sbox[x] = s
        inv[s] = x
    return tuple(sbox), tuple(inv)


SBOX, INV_SBOX = _make_tables()
RCON = (0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80, 0x1B, 0x36)


def mul2(x): return gf_mul(x, 2)
def mul3(x): return gf_mul(x, 3)
def mul9(x): return gf_mul(x, 9)
def mul11(x): return gf_mul(x, 11)
def mul13(x): return gf_mul(x, 13)
def mul14(x): return gf_mul(x, 14)


def expand_key(key):
    """FIPS-197 section 5.2.  `key`: 16 / 24 / 32 `bytes` (AES-128 / 192 / 256), or an int, which is a 128-bit key with byte 0 the
    most significant.  Returns the Nr + 1 = 11 / 13 / 15 round keys of 16 bytes."""
    kb = list(key) if isinstance(key, (bytes, bytearray)) else [(key >> (8 * (15 - i))) & 0xFF for i in range(16)]
    if len(kb) not in (16, 24, 32):
        raise ValueError("an AES key has 16, 24 or 32 bytes, got %d" % len(kb))
    nk = len(kb) // 4
    nr = nk + 6
    w = [kb[4 * i:4 * i + 4] for i in range(nk)]
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = t[1:] + t[:1]
            t = [SBOX[b] for b in t]
            t[0] ^= RCON[i // nk - 1]
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(nr + 1)]


def _shift_rows(s):
    return [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]


def _inv_shift_rows(s):
    return [s[4 * ((c - r) % 4) + r] for c in range(4) for r in range(4)]


def _mix(s, m):
    out = []
    for c in range(4):
        col = s[4 * c:4 * c + 4]
        for r in range(4):
            v = 0
            for j in range(4):
                v ^= gf_mul(col[j], m[(j - r) % 4])
            out.append(v)
    return out


def _state(block: int):
    return [(block >> (8 * (15 - i))) & 0xFF for i in range(16)]


def _u128(s) -> int:
    return sum(b << (8 * (15 - i)) for i, b in enumerate(s))


def aes_encrypt_block(key, block: int) -> int:
    """FIPS-197 Fig. 5 for a key of 16 / 24 / 32 bytes (or a 128-bit int, as expand_key); the block is a u128, byte 0 = MSB"""
    rk = expand_key(key)
    nr = len(rk) - 1
    s = [a ^ b for a, b in zip(_state(block), rk[0])]
    for rnd in range(1, nr):
        s = _mix(_shift_rows([SBOX[b] for b in s]), (2, 3, 1, 1))
        s = [a ^ b for a, b in zip(s, rk[rnd])]
    s = _shift_rows([SBOX[b] for b in s])
    return _u128(a ^ b for a, b in zip(s, rk[nr]))


def counter_block(iv: int, i: int, counter_bits: int = 128) -> int:
    """counter block i of SP 800-38A appendix B.1: the low counter_bits bits of iv incremented i times mod 2^counter_bits, the bits above
    them unchanged (counter_bits = 32: inc32 of SP 800-38D)"""
    if counter_bits not in (32, 128):
        raise ValueError("counter_bits must be 32 or 128, got %r" % (counter_bits,))
    m = 1 << counter_bits
    return (iv & ~(m - 1)) | ((iv + i) & (m - 1))


def ctr_keystream(key, iv: int, first_block: int, n_blocks: int, counter_bits: int = 128) -> list[int]:
    """SP 800-38A CTR: keystream block i = E_K((iv + first_block + i) mod 2^128), i < n_blocks, as u128 (byte 0 = MSB); counter_bits = 32:
    only the low 32 bits of iv count (the counter field of GCM)"""
    return [aes_encrypt_block(key, counter_block(iv, first_block + i, counter_bits)) for i in range(n_blocks)]


def gcm_keystream(key, iv: bytes, first_block: int, n_blocks: int) -> list[int]:
    """SP 800-38D GCTR for a 96-bit IV: J0 = iv || 00000001, keystream block i (for data block first_block + i) = E_K(inc32^(first_block +
    i + 1)(J0)); E_K(J0) itself masks the tag and is not part of it.  GHASH and the tag are not computed here."""
    if len(iv) != 12:
        raise ValueError("a 12-byte IV is expected (other lengths derive J0 with GHASH), got %d bytes" % len(iv))
    j0 = int.from_bytes(bytes(iv) + b"\x00\x00\x00\x01", "big")
    return ctr_keystream(key, j0, first_block + 1, n_blocks, counter_bits=32)


def ctr_streams(keys, streams) -> list[int]:
    """several SP 800-38A CTR streams under several keys, as Server.aes_ctr_streams takes them: `streams` is a list of
    (key_index, iv, first_block, n_blocks, data_or_None), data a list of n_blocks u128; returns the streams' blocks concatenated in order,
    keystream ^ data (data None: the keystream)"""
    out = []
    for key_index, iv, first_block, n_blocks, data in streams:
        ks = ctr_keystream(keys[key_index], iv, first_block, n_blocks)
        out += ks if data is None else [k ^ d for k, d in zip(ks, data)]
    return out


def aes_decrypt_block(key, block: int) -> int:
    """FIPS-197 Fig. 12, the inverse cipher, in the order Server::aes_decrypt takes it (AddRoundKey before InvMixColumns)"""
    rk = expand_key(key)
    nr = len(rk) - 1
    s = [a ^ b for a, b in zip(_state(block), rk[nr])]
    for rnd in range(nr - 1, 0, -1):
        s = [INV_SBOX[b] for b in _inv_shift_rows(s)]
        s = [a ^ b for a, b in zip(s, rk[rnd])]
        s = _mix(s, (14, 11, 13, 9))
    s = [INV_SBOX[b] for b in _inv_shift_rows(s)]
    return _u128(a ^ b for a, b in zip(s, rk[0]))


def cbc_decrypt(key, iv: int, ciphertext) -> list[int]:
    """SP 800-38A CBC decryption: P_i = D_K(C_i) ^ C_{i-1}, C_{-1} = iv; blocks as u128"""
    ciphertext = list(ciphertext)
    return [aes_decrypt_block(key, c) ^ prev for c, prev in zip(ciphertext, [iv] + ciphertext[:-1])]


def cfb128_decrypt(key, iv: int, ciphertext) -> list[int]:
    """SP 800-38A CFB-128 decryption: P_i = E_K(C_{i-1}) ^ C_i, C_{-1} = iv; blocks as u128"""
    ciphertext = list(ciphertext)
    return [aes_encrypt_block(key, prev) ^ c for c, prev in zip(ciphertext, [iv] + ciphertext[:-1])]


def xts_tweak_block(sector: int) -> int:
    """the 16-byte tweak block of IEEE 1619 for data-unit number `sector`, as a u128 with byte 0 the most significant: the number is written
    little-endian, so its least significant byte is byte 0"""
    if not 0 <= sector < 1 << 128:
        raise ValueError("a data-unit number is a 128-bit value")
    return int.from_bytes(sector.to_bytes(16, "little"), "big")


def xts_mul_alpha(t: int, j: int = 1) -> int:
    """t * alpha^j in GF(2^128) mod x^128 + x^7 + x^2 + x + 1, t the little-endian reading of the block (bit b of byte p = degree 8p + b)"""
    for _ in range(j):
        t <<= 1
        if t >> 128:
            t = (t & ((1 << 128) - 1)) ^ 0x87
    return t


def _xts(key1, key2, sector: int, data: bytes, first_block: int, cipher) -> bytes:
    if len(key1) != len(key2) or len(key1) not in (16, 32):
        raise ValueError("XTS-AES takes two keys of 16 or of 32 bytes")
    if len(data) % 16:
        raise ValueError("whole 16-byte blocks are expected (ciphertext stealing is not offered), got %d bytes" % len(data))
    t = int.from_bytes(aes_encrypt_block(key2, xts_tweak_block(sector)).to_bytes(16, "big"), "little")
    t = xts_mul_alpha(t, first_block)
    out = bytearray()
    for i in range(0, len(data), 16):
        mask = int.from_bytes(t.to_bytes(16, "little"), "big")
        out += (cipher(key1, int.from_bytes(data[i:i + 16], "big") ^ mask) ^ mask).to_bytes(16, "big")
        t = xts_mul_alpha(t)
    return bytes(out)


def xts_encrypt(key1, key2, sector: int, data: bytes, first_block: int = 0) -> bytes:
    """IEEE 1619 XTS-AES encryption of ONE data unit (whole blocks): C_j = E_K1(P_j ^ T_j) ^ T_j, T_j = E_K2(tweak) * alpha^j; `data` starts
    at block first_block of the unit"""
    return _xts(key1, key2, sector, data, first_block, aes_encrypt_block)


def xts_decrypt(key1, key2, sector: int, data: bytes, first_block: int = 0) -> bytes:
    """IEEE 1619 XTS-AES decryption of one data unit: P_j = D_K1(C_j ^ T_j) ^ T_j; first_block continues a stream inside the unit"""
    return _xts(key1, key2, sector, data, first_block, aes_decrypt_block)


def cbc_mac(key, blocks, init: int = 0) -> int:
    """the raw CBC-MAC chain X_{i+1} = E_K(X_i ^ B_i) from X_0 = init over u128 blocks; no blocks: init"""
    x = init
    for b in blocks:
        x = aes_encrypt_block(key, x ^ b)
    return x


CCM_TAG_LENGTHS = (4, 6, 8, 10, 12, 14, 16)


def ccm_blocks(nonce: bytes, aad: bytes, payload_len: int, tag_len: int):
    """SP 800-38C A.2 / A.3 formatting -> (B0, the encoded and zero-padded AAD blocks, the counter blocks Ctr_0 .. Ctr_m), all u128 with
    byte 0 the most significant; m = ceil(payload_len / 16).  q = 15 - len(nonce), nonce of 7 .. 13 bytes, tag_len in 4, 6, .., 16; the
    AAD length takes 2 bytes below 0xFF00, else FF FE and 4 bytes (the 10-byte form for 2^32 bytes and more is refused)"""
    nonce, aad = bytes(nonce), bytes(aad)
    if not 7 <= len(nonce) <= 13:
        raise ValueError("a CCM nonce has 7 to 13 bytes, got %d" % len(nonce))
    if tag_len not in CCM_TAG_LENGTHS:
        raise ValueError("a CCM tag has 4, 6, .., 16 bytes, got %r" % (tag_len,))
    q = 15 - len(nonce)
    if payload_len < 0 or payload_len >> (8 * q):
        raise ValueError("a payload of %d bytes does not fit the %d-byte length field" % (payload_len, q))
    if len(aad) >= 1 << 32:
        raise ValueError("the 10-byte AAD length form (2^32 bytes and more) is not offered")
    b0 = bytes([64 * (len(aad) > 0) + 8 * ((tag_len - 2) // 2) + (q - 1)]) + nonce + payload_len.to_bytes(q, "big")
    enc = b""
    if aad:
        enc = len(aad).to_bytes(2, "big") if len(aad) < 0xFF00 else b"\xff\xfe" + len(aad).to_bytes(4, "big")
        enc += aad
        enc += bytes(-len(enc) % 16)
    m = (payload_len + 15) // 16
    ctr = [int.from_bytes(bytes([q - 1]) + nonce + i.to_bytes(q, "big"), "big") for i in range(m + 1)]
    return int.from_bytes(b0, "big"), [int.from_bytes(enc[i:i + 16], "big") for i in range(0, len(enc), 16)], ctr


def _ccm_tag(key, b0: int, aad_blocks, payload: bytes, s0: int, tag_len: int) -> bytes:
    padded = payload + bytes(-len(payload) % 16)
    x = cbc_mac(key, [b0] + list(aad_blocks) + [int.from_bytes(padded[i:i + 16], "big") for i in range(0, len(padded), 16)])
    return (x ^ s0).to_bytes(16, "big")[:tag_len]


def _ccm_ctr(key, ctr, data: bytes) -> bytes:
    out = bytearray()
    for i in range(0, len(data), 16):
        ks = aes_encrypt_block(key, ctr[1 + i // 16]).to_bytes(16, "big")
        out += bytes(a ^ b for a, b in zip(data[i:i + 16], ks))
    return bytes(out)


def ccm_encrypt(key, nonce: bytes, aad: bytes, payload: bytes, tag_len: int) -> bytes:
    """SP 800-38C 6.1 (RFC 3610): ciphertext || tag, the tag MSB_t(X_last ^ E_K(Ctr_0))"""
    payload = bytes(payload)
    b0, aad_blocks, ctr = ccm_blocks(nonce, aad, len(payload), tag_len)
    return _ccm_ctr(key, ctr, payload) + _ccm_tag(key, b0, aad_blocks, payload, aes_encrypt_block(key, ctr[0]), tag_len)


def ccm_decrypt(key, nonce: bytes, aad: bytes, ciphertext_and_tag: bytes, tag_len: int):
    """SP 800-38C 6.2: the payload, or None where the tag does not verify"""
    data = bytes(ciphertext_and_tag)
    if tag_len not in CCM_TAG_LENGTHS or len(data) < tag_len:
        raise ValueError("ciphertext || tag is shorter than its tag of %r bytes" % (tag_len,))
    ct, tag = data[:-tag_len], data[-tag_len:]
    b0, aad_blocks, ctr = ccm_blocks(nonce, aad, len(ct), tag_len)
    payload = _ccm_ctr(key, ctr, ct)
    return payload if _ccm_tag(key, b0, aad_blocks, payload, aes_encrypt_block(key, ctr[0]), tag_len) == tag else None


def _cmac_double(v: int) -> int:
    """v * x in GF(2^128) mod x^128 + x^7 + x^2 + x + 1, the block a big-endian integer (SP 800-38B 6.1: shift left, R_128 = 0x87)"""
    v <<= 1
    return (v ^ 0x87) & ((1 << 128) - 1) if v >> 128 else v


def cmac_subkeys(key):
    """SP 800-38B 6.1 (RFC 4493 2.3): (K1, K2) = (L x, L x^2), L = E_K(0^128), as u128"""
    k1 = _cmac_double(aes_encrypt_block(key, 0))
    return k1, _cmac_double(k1)


def cmac_blocks(msg: bytes):
    """SP 800-38B 6.2 -> (blocks, which): the n = max(1, ceil(len / 16)) u128 blocks of a message (byte 0 most significant) and the subkey
    its last block takes -- 0 (K1) for a whole last block, 1 (K2) for one padded with 0x80 00..; the empty message is the one block
    0x80 00.. with K2"""
    msg = bytes(msg)
    which = 0 if msg and len(msg) % 16 == 0 else 1
    if which:
        msg += b"\x80" + bytes(-(len(msg) + 1) % 16)
    return [int.from_bytes(msg[i:i + 16], "big") for i in range(0, len(msg), 16)], which


def cmac(key, msg: bytes, tag_len: int = 16) -> bytes:
    """AES-CMAC (SP 800-38B 6.2, RFC 4493) for any of the three key sizes: MSB_tag_len of the CBC-MAC whose last block also gets its subkey"""
    if not 1 <= tag_len <= 16:
        raise ValueError("a CMAC tag has 1 to 16 bytes, got %r" % (tag_len,))
    blocks, which = cmac_blocks(msg)
    blocks[-1] ^= cmac_subkeys(key)[which]
    return cbc_mac(key, blocks).to_bytes(16, "big")[:tag_len]


def cmac_verify(key, msg: bytes, tag: bytes) -> bool:
    """SP 800-38B 6.3: whether `tag` is the first len(tag) bytes of the CMAC of msg"""
    tag = bytes(tag)
    return 1 <= len(tag) <= 16 and cmac(key, msg, len(tag)) == tag


KW_ICV = 0xA6A6A6A6A6A6A6A6      # RFC 3394 2.2.3.1: the default initial value, the integrity check of the unwrap


def _kw_semiblocks(data: bytes, lo: int, what: str):
    data = bytes(data)
    if len(data) % 8 or not lo <= len(data) // 8 <= lo + 6:
        raise ValueError("%s has %d..%d bytes in whole semiblocks of 8, got %d" % (what, 8 * lo, 8 * (lo + 6), len(data)))
    return [int.from_bytes(data[i:i + 8], "big") for i in range(0, len(data), 8)]


def key_wrap(kek, data: bytes) -> bytes:
    """AES Key Wrap (RFC 3394 2.2.1, SP 800-38F KW) of a payload of n = 2..8 semiblocks of 8 bytes under a KEK of 16 / 24 / 32 bytes:
    8 (n + 1) bytes.  For j = 0..5, i = 1..n: B = E_KEK(A | R[i]); A = MSB64(B) ^ (n j + i); R[i] = LSB64(B)"""
    r = [KW_ICV] + _kw_semiblocks(data, 2, "a payload to wrap")
    n = len(r) - 1
    for j in range(6):
        for i in range(1, n + 1):
            b = aes_encrypt_block(kek, (r[0] << 64) | r[i])
            r[0], r[i] = (b >> 64) ^ (n * j + i), b & ((1 << 64) - 1)
    return b"".join(v.to_bytes(8, "big") for v in r)


def key_unwrap(kek, wrapped: bytes):
    """AES Key Unwrap (RFC 3394 2.2.2) -> (ok, data): the n = len / 8 - 1 payload semiblocks, and whether A came out as A6A6A6A6A6A6A6A6.
    The payload is returned either way -- Server.aes_key_unwrap does not gate it on `valid` either.  For j = 5..0, i = n..1:
    B = D_KEK((A ^ (n j + i)) | R[i]); A = MSB64(B); R[i] = LSB64(B)"""
    r = _kw_semiblocks(wrapped, 3, "a wrapped key")
    n = len(r) - 1
    for j in range(5, -1, -1):
        for i in range(n, 0, -1):
            b = aes_decrypt_block(kek, ((r[0] ^ (n * j + i)) << 64) | r[i])
            r[0], r[i] = b >> 64, b & ((1 << 64) - 1)
    return r[0] == KW_ICV, b"".join(v.to_bytes(8, "big") for v in r[1:])


def aes128_encrypt_block(key: int, block: int) -> int:
    return aes_encrypt_block(key, block)


def aes128_decrypt_block(key: int, block: int) -> int:
    return aes_decrypt_block(key, block)


def inv_mix_columns_round_keys(expanded):
    """the equivalent inverse cipher's round keys (FIPS-197 section 5.3.5): dw[0] = w[0], dw[Nr] = w[Nr], dw[r] = InvMixColumns(w[r])"""
    nr = len(expanded) - 1
    return [list(expanded[0])] + [_mix(list(expanded[r]), (14, 11, 13, 9)) for r in range(1, nr)] + [list(expanded[nr])]


def aes_decrypt_block_equivalent(dw, block: int) -> int:
    """FIPS-197 Fig. 15 with the Nr + 1 round keys of inv_mix_columns_round_keys: InvSubBytes, InvShiftRows, InvMixColumns, AddRoundKey"""
    nr = len(dw) - 1
    s = [a ^ b for a, b in zip(_state(block), dw[nr])]
    for rnd in range(nr - 1, 0, -1):
        s = _mix(_inv_shift_rows([INV_SBOX[b] for b in s]), (14, 11, 13, 9))
        s = [a ^ b for a, b in zip(s, dw[rnd])]
    s = _inv_shift_rows([INV_SBOX[b] for b in s])
    return _u128(a ^ b for a, b in zip(s, dw[0]))


def aes128_decrypt_block_equivalent(dw, block: int) -> int:
    return aes_decrypt_block_equivalent(dw, block)
