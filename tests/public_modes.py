"""What the tests of the public-ciphertext modes share (CBC, CFB-128, the 32-bit counter of GCM, public blocks through the equivalent
inverse cipher): the clear vectors of SP 800-38A F.2 / F.3 and SP 800-38D test case 3, the sharing rule of the decryption direction
restated from include/fheaes.h, and the shared schedule built on it with the CPU oracle's WoPBS.  A plain module like aes_model.py:
imported by name, not collected."""
import numpy as np

from aes_model import DEC_MULS, INV_MC
from aes_vectors import A2_KEY, A3_KEY, F1_KEY, F1_PT
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.client import u128_to_bytes

IV = int.from_bytes(bytes(range(16)), "big")                       # SP 800-38A F.2 / F.3: 000102..0f
# SP 800-38A F.2.2 / F.2.4 / F.2.6 (CBC decryption): key, first and last ciphertext block; the plaintext is F1_PT
CBC = {128: (F1_KEY, 0x7649ABAC8119B246CEE98E9B12E9197D, 0x3FF1CAA1681FAC09120ECA307586E1A7),
       192: (A2_KEY, 0x4F021DB243BC633D7178183A9FA071E8, 0x08B0E27988598881D920A9E64F5615CD),
       256: (A3_KEY, 0xF58C4C04D6E5F1BA779EABFB5F7BFBD6, 0xB2EB05E2C39BE9FCDA6C19078C6A9D1B)}
# SP 800-38A F.3.14 (CFB128-AES128 decryption)
CFB128 = (F1_KEY, 0x3B3FD92EB72DAD20333449F8E83CFB4A, 0xC04B05357C5D1C0EEAC4C66F9FF7F2E6)
# SP 800-38D test case 3 (the GCM specification's AES-128 case with a 96-bit IV and four whole blocks)
GCM_KEY = bytes.fromhex("feffe9928665731c6d6a8f9467308308")
GCM_IV = bytes.fromhex("cafebabefacedbaddecaf888")
GCM_PT = [0xD9313225F88406E5A55909C5AFF5269A, 0x86A7A9531534F7DA2E4C303D8A318A72, 0x1C3C0C95956809532FCF0E2449A6B525,
          0xB16AEDF5AA0DE657BA637B391AAFD255]
GCM_CT_FIRST, GCM_CT_LAST = 0x42831EC2217774244B7221B784D0D49C, 0x1BA30B396A0AAC973D58E091473F5985
GCM_EK_J0 = 0x3247184B3C4F69A44DBCD22887BBB418
GCM_J0 = int.from_bytes(GCM_IV + b"\x00\x00\x00\x01", "big")


def cbc_encrypt(key, iv, plaintext):
    """SP 800-38A CBC encryption in the clear (serial): what produces the ciphertexts the tests decrypt"""
    out, prev = [], iv
    for p in plaintext:
        prev = aes_clear.aes_encrypt_block(key, p ^ prev)
        out.append(prev)
    return out


def cfb128_encrypt(key, iv, plaintext):
    out, prev = [], iv
    for p in plaintext:
        prev = aes_clear.aes_encrypt_block(key, prev) ^ p
        out.append(prev)
    return out


def cbc_ct(bits):
    """the four ciphertext blocks of F.2.1 / F.2.3 / F.2.5"""
    return cbc_encrypt(CBC[bits][0], IV, F1_PT)


def inc32(block, i):
    """SP 800-38D inc32, i times: the low 32 bits count mod 2^32, the upper 96 stay"""
    return (block >> 32 << 32) | ((block + i) & 0xFFFFFFFF)


# the four sources of position p = 4 col + row in the decryption direction (InvShiftRows folded into InvMixColumns): row j of column col - j
DEC_SOURCES = [[4 * ((col - j) % 4) + j for j in range(4)] for col in range(4) for _ in range(4)]


def rule_dec(blocks, nr, key_of_block=None):
    """the sharing rule of the decryption direction restated: the id of a round-1 input is (key, position, byte), of a later one (position,
    the ids of its four sources); returns (distinct ids per round, the ids of every round)"""
    keys = key_of_block if key_of_block is not None else [0] * len(blocks)
    ids = [[(k, p, v) for p, v in enumerate(u128_to_bytes(b))] for b, k in zip(blocks, keys)]
    counts, all_ids = [], []
    for _ in range(nr):
        number = {}
        ids = [[number.setdefault(i, len(number)) for i in blk] for blk in ids]
        counts.append(len(number))
        all_ids.append(ids)
        ids = [[(p,) + tuple(blk[s] for s in DEC_SOURCES[p]) for p in range(16)] for blk in ids]
    return counts, all_ids


def shared_decrypt(model, dw, trivial, blocks, data=None):
    """the equivalent inverse cipher on public blocks with one WoPBS per distinct S-Box input: pools and index tables from rule_dec(), the
    WoPBS from the oracle, numpy wrapping sums for the linear layers.  dw [Nr+1][16][8][kN+1]; trivial, data (trivial ciphertexts of the
    clear data, or None) [n][16][8][kN+1]; returns (the same shape, byte-WoPBS evaluated)."""
    nr = dw.shape[0] - 1
    counts, ids = rule_dec(blocks, nr)
    n = len(blocks)
    pool = np.zeros((counts[0],) + dw.shape[2:], dtype=np.uint64)
    for b in range(n):
        for p in range(16):
            pool[ids[0][b][p]] = dw[nr, p] + trivial[b, p]
    evaluated = 0
    for r in range(1, nr + 1):
        y = model.O.wopbs_batch(pool, model.dec_eq_round if r < nr else model.inv_sbox)      # [pool][L][8][kN+1]
        evaluated += len(pool)
        if r == nr:
            break
        pool = np.zeros((counts[r],) + dw.shape[2:], dtype=np.uint64)
        done = set()
        for b in range(n):
            for p in range(16):
                u = ids[r][b][p]
                if u not in done:                                            # InvMixColumns row p % 4 over the LUTs {9, 11, 13, 14} InvS
                    done.add(u)
                    for j, s in enumerate(DEC_SOURCES[p]):
                        pool[u] += y[ids[r - 1][b][s], DEC_MULS.index(INV_MC[p % 4][j])]
                    pool[u] += dw[nr - r, p]
    out = np.empty_like(trivial)
    for b in range(n):
        for col in range(4):
            for row in range(4):
                out[b, 4 * col + row] = y[ids[nr - 1][b][4 * ((col - row) % 4) + row], 0] + dw[0, 4 * col + row]
    return (out if data is None else out + data), evaluated
