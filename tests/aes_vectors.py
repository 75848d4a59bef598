"""The clear constants the AES tests share, and the helpers that only rearrange them: FIPS-197 appendices A and C, SP 800-38A F.1 and
F.5, the counter blocks of the public / CTR tests.  A plain module like edge_words.py: imported by name, not collected."""
import numpy as np

from tfhe_aes_amd.client import Client, u128_to_bytes

# FIPS-197 appendix C.1 / C.2 / C.3: key 00 01 02 .., one plaintext
FIPS_C_PT = 0x00112233445566778899AABBCCDDEEFF
FIPS_C = {128: (bytes(range(16)), 0x69C4E0D86A7B0430D8CDB78070B4C55A),
          192: (bytes(range(24)), 0xDDA97CA4864CDFE06EAF70A0EC0D7191),
          256: (bytes(range(32)), 0x8EA2B7CA516745BFEAFC49904B496089)}
# C.1 again as integers, for the entry points that take a 128-bit key as one
FIPS_C1_KEY = 0x000102030405060708090A0B0C0D0E0F
FIPS_C1_PT = FIPS_C_PT
FIPS_C1_CT = FIPS_C[128][1]
# FIPS-197 appendix A.2 / A.3 (key expansion; the last word) and SP 800-38A F.1.3 / F.1.5 (ECB, first block) with the same keys
A2_KEY = bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b")
A3_KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
SP800_PT = 0x6BC1BEE22E409F96E93D7E117393172A

NR = {128: 10, 192: 12, 256: 14}

MASK128 = (1 << 128) - 1
BASE = 0x00112233445566778899AABBCCDDEE00             # sixteen distinct bytes, the low one 00
F5_CTR = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
F1_KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")
F1_PT = [0x6BC1BEE22E409F96E93D7E117393172A, 0xAE2D8A571E03AC9C9EB76FAC45AF8E51, 0x30C81C46A35CE411E5FBC1191A0A52EF,
         0xF69F2445DF4F9B17AD2B417BE66C3710]
# SP 800-38A F.5.1 / F.5.3 / F.5.5: key, first and last ciphertext block
F5 = {128: (F1_KEY, 0x874D6191B620E3261BEF6864990DB6CE, 0x1E031DDA2FBE03D1792170A0F3009CEE),
      192: (A2_KEY, 0x1ABC932417521CA24F2B0459FE7E6E0B, 0x4F78A7F6D29809585A97DAEC58C6B050),
      256: (A3_KEY, 0x601EC313775789A5B7A7F504BBF3D228, 0xDFC9C58DB67AADA613C2DD08457941A6)}


def counters(start, n):
    return [(start + i) & MASK128 for i in range(n)]


def key_words(rk):
    """round keys as lists of 16 ints -> what the client decrypts from [Nr+1][16][8][kN+1]"""
    return np.array(rk, dtype=np.uint8)


def block_bytes(values):
    """128-bit integers -> what the client decrypts from [n][16][8][kN+1]"""
    return np.array([u128_to_bytes(v) for v in values], dtype=np.uint8)


def own_client(kit):
    """a Client with the kit's secret key but its own encryption counter: the session client's sequence of encryptions, which the
    other test files run on, stays as it was"""
    return Client(1, kit.client.iv, kit.client.key, params=kit.params, seed=kit.client.test_seed)
