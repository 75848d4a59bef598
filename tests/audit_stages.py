"""What the tests of the key switches' audit share (test_audit_stages_cpu.py without a GPU, test_gpu_audit_stages.py on one): the shapes,
the launch sizes of the clean calls, and a numpy model of the plain form (kern_audit.h, keyswitch_plain_kernel).  A plain module like
audit_model.py: imported by name, not collected.

The model follows the kernel, not the reference: it cuts the key into the balanced byte planes in B-fragment order that keybytes_kernel
leaves on the device (zero padded to whole K steps of 64 rows and whole tiles of 16 columns), recombines the key words from the planes,
takes digits for rows below Q = n_in levels and columns below ncols only, and adds the body term.  edge_words.keyswitch_plain / pfpks_plain
are the references it is pinned against; they never see a byte plane."""
import numpy as np

import audit_calls as ac
import edge_words as ew

KSTEP, COLTILE = 64, 16
STAGES = ("keyswitch", "blind_rotate", "pfpks")
KS, K2, PF = STAGES
STAGE_NO = {KS: 0, K2: 1, PF: 2}                       # FHEAES_STAGE_*
ROW_COUNTS = (1, 127, 128, 129)                        # one row; the product kernel's 128-ciphertext workgroup tile and its seam
ROWS_MAX = max(ROW_COUNTS)
K1_SMALL_N = (1, 15, 16, 63, 64)                       # n + 1 columns on both sides of a 16- and of a 64-column tile
SEED = 0x5EED57A6E5
MASK = 1 << 40


def row_words(p, stage, block=-1):
    """the words a launch writes for one row: K1 n + 1; K3 the k + 1 key blocks, or one"""
    if stage == KS:
        return p.n + 1
    return (p.k + 1 if block < 0 else 1) * (p.k + 1) * p.N


# ---- the clean calls: case of workspace_state.CASES -> the rows of every launch of each audited stage, on a fresh context -----------------
def _cbs(rows):
    return {KS: rows, K2: rows, PF: rows}


CLEAN_CALLS = {
    "aes_encrypt": _cbs(ac.launch_list("aes_encrypt")),                  # 2 blocks: ten WoPBS over 256 bits
    "wopbs_8_bits_shared_luts": _cbs(ac.launch_list("wopbs_8_bits_shared_luts")),
    "gate": _cbs(ac.launch_list("gate")),
    "pack_unpack_513": {KS: [], K2: [], PF: [513]},                      # key block k alone, one chunk
    "pack_unpack_round_keys": {KS: [], K2: [], PF: [2 * 11 * 128]},      # two keys of 1,408 bits in one chunk
    "k1_keyswitch": {KS: [3], K2: [], PF: []},
    "k3_pfpks": {KS: [], K2: [], PF: [3]},
}


def window_k1_rows(n_blocks: int, steps: int, window: int) -> list[int]:
    """rows of every K1 launch of `steps` WoPBS over n_blocks blocks cut into windows: K2 and K3 run once per window
    (audit_calls.window_launch_rows), K1 once per segment -- a window that straddles two steps switches the blocks of either step by
    themselves (aes_schedule.h)"""
    total, out = steps * n_blocks, []
    for i0 in range(0, total, window):
        i1 = min(i0 + window, total)
        cut = (i0 // n_blocks + 1) * n_blocks
        out += [128 * (i1 - i0)] if cut >= i1 else [128 * (cut - i0), 128 * (i1 - cut)]
    return out


def counters_after(launches, rows):
    """(launches, rows_checked) an audit of `rows` rows has counted after launches of these sizes"""
    return len(launches), sum(min(rows, m) for m in launches)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def balanced_planes(x):
    """edge_words.balanced_bytes over an array: int8 [8] + x.shape"""
    x = np.asarray(x, dtype=np.uint64)
    out = np.empty((8,) + x.shape, dtype=np.int8)
    carry = np.zeros(x.shape, dtype=np.uint64)
    for j in range(8):
        v = ((x >> np.uint64(8 * j)) & np.uint64(0xFF)) + carry
        carry = (v >= 128).astype(np.uint64)
        out[j] = (v & np.uint64(0xFF)).astype(np.uint8).view(np.int8)
    return out


def key_fragments(key):
    """key [nz][Q][ncols] uint64 -> int8 [nz][ksteps][coltiles][8][64][16], keybytes_kernel's image: lane l of (kstep, column tile C,
    plane j) holds byte j of column 16 C + l % 16 in rows 64 kstep + 16 (l // 16) + e, e < 16; zero beyond Q rows and ncols columns"""
    key = np.asarray(key, dtype=np.uint64)
    nz, Q, ncols = key.shape
    ksteps, coltiles = -(-Q // KSTEP), -(-ncols // COLTILE)
    padded = np.zeros((nz, ksteps * KSTEP, coltiles * COLTILE), dtype=np.uint64)
    padded[:, :Q, :ncols] = key
    planes = balanced_planes(padded)                                              # [8][nz][rows][cols]
    # rows = (kstep, quarter, e), cols = (C, c): lane = 16 quarter + c
    planes = planes.reshape(8, nz, ksteps, 4, 16, coltiles, COLTILE)
    return np.ascontiguousarray(planes.transpose(1, 2, 5, 0, 3, 6, 4).reshape(nz, ksteps, coltiles, 8, 64, 16))


def fragment_words(frag, Q, ncols):
    """the key words the plain form recombines: [nz][Q][ncols] uint64 = sum_j plane_j 2^(8j), rows and columns bounded"""
    nz, ksteps, coltiles = frag.shape[:3]
    planes = frag.reshape(nz, ksteps, coltiles, 8, 4, COLTILE, 16).transpose(3, 0, 1, 4, 6, 2, 5).reshape(8, nz, ksteps * KSTEP, coltiles * COLTILE)
    words = np.zeros(planes.shape[1:], dtype=np.uint64)
    for j in range(8):
        words += planes[j].astype(np.int64).view(np.uint64) << np.uint64(8 * j)
    return words[:, :Q, :ncols]


def plain_model(x, frag, gadget, n_in, ncols, body=None):
    """x [m][words] -> [m][nz][ncols]: out = -sum_{i < n_in, l} digit_l(x[i]) KEY[i levels + l], + x[body[0]] in column body[1]"""
    b, level = gadget
    x = np.asarray(x, dtype=np.uint64)
    key = fragment_words(frag, n_in * level, ncols)
    d = ew.digits_of_rows(x[:, :n_in], b, level).astype(np.uint64)
    out = np.stack([np.uint64(0) - d @ key[z] for z in range(key.shape[0])], axis=1)
    if body is not None:
        out[:, :, body[1]] += x[:, body[0], None]
    return out


def k1_model(x, ksk, p):
    """[m][n+1]"""
    frag = key_fragments(np.asarray(ksk, dtype=np.uint64).reshape(1, p.big * p.ks_level, p.n + 1))
    return plain_model(x, frag, ew.gadget(p, "K1"), p.big, p.n + 1, body=(p.big, p.n))[:, 0]


def k3_model(x, key_blocks, p, c0=0, c1=None):
    """key_blocks [nz][(kN+1) levels][(k+1)N] (any choice of key blocks) -> [m][nz][c1 - c0]: columns c0 .. c1 - 1 only, c0 a multiple of 16"""
    key = np.asarray(key_blocks, dtype=np.uint64)
    c1 = key.shape[2] if c1 is None else c1
    assert c0 % COLTILE == 0
    return plain_model(x, key_fragments(key[:, :, c0:c1]), ew.gadget(p, "K3"), p.big1, c1 - c0)


def drop_carry(frag, plane):
    """the can-fail mutant: the byte plane as if the carry out of a negative byte below it had been lost, so every such word is off by
    2^(8 plane)"""
    frag = frag.copy()
    below = frag[:, :, :, plane - 1].astype(np.int16)
    frag[:, :, :, plane] = (frag[:, :, :, plane].astype(np.int16) - (below < 0)).astype(np.int8)
    return frag
