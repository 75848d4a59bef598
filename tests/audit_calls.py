"""What the audit's call tests share (test_gpu_audit_calls.py on the GPU, test_audit_calls_cpu.py without one): which cases of
workspace_state.CASES launch a blind rotation at all, the launch sizes m_i of the cases whose schedule follows from a plan function, and
what an audit of `rows` rows must then have counted.  A helper module like chunk_seams.py: no test, no fixture, no call into the engine
beyond the host-only plan functions.

All four callers of launch_cbs_pbs are modelled by the rule their host code states:

  fheaes_cbs_pbs_batch   one launch of the m rows it is given
  wopbs_dev              chunks of MAX_CHUNK_BITS // bits inputs (chunk_seams.wopbs_chunks), one launch of inputs x bits rows per chunk
  aes_run_dev            without a window one WoPBS over 16 n bytes per step; with a window w the steps x n block-rounds cut into launches
                         of w blocks = 128 w rows, the last one shorter (chunk_seams.window_launches counts them, this module sizes them)
  gate_call              chunks of MAX_CHUNK_BITS gates, one launch of that many rows per chunk
"""
import chunk_seams as cs
from tfhe_aes_amd import _native

SEED = 0x5EED0A0D17
MASK = 1 << 62                                         # into a body word: the phase moves by a quarter turn, so K3 .. K5 see another bit
RECORDS, MAX_ROWS = _native.AUDIT_RECORDS, _native.AUDIT_MAX_ROWS
STEPS = {"encrypt": 10, "decrypt": 19, "decrypt_equivalent": 10}          # WoPBS per AES-128 block: Nr, 2 Nr - 1, Nr

# the cases that never reach launch_cbs_pbs: an audit that counts anything there is a bug
NO_K2 = ("k1_keyswitch", "k3_pfpks", "k4_forward_fourier", "k5_vertical_packing", "pack_unpack_round_keys", "pack_unpack_513",
         "pack_unpack_513_width16", "expand_seeded")


def launches_k2(case) -> bool:
    """by the table alone: the case grows K1's and K2's outputs (a WoPBS, a window or a bootstrapped gate ran), or it calls the K2 stage
    entry point itself, which writes into the caller's buffer"""
    return {"ws_small", "ws_pbs"} <= set(case.uses) or "fheaes_cbs_pbs_batch" in case.entry


def wopbs_launch_rows(n_inputs: int, bits: int, n_luts: int = 1, k1: int = 2) -> list[int]:
    """rows of every blind-rotation launch of one wopbs_dev: chunk_seams.wopbs_chunks, with the sizes"""
    chunk = max(1, cs.MAX_CHUNK_BITS // bits)
    if bits > 9:
        chunk = max(1, min(chunk, (2 << 30) // (n_luts * bits * (1 << (bits - 9)) * k1 * cs.N * 8)))
    return [min(chunk, n_inputs - i0) * bits for i0 in range(0, n_inputs, chunk)]


def window_launch_rows(n_blocks: int, steps: int, window: int) -> list[int]:
    """rows of every blind-rotation launch of `steps` WoPBS over n_blocks blocks: window 0 one WoPBS over 16 n bytes per step, else the
    stream of steps x n block-rounds cut every `window` blocks (clamped to n, as aes_context_window does)"""
    if window == 0:
        return [m for _ in range(steps) for m in wopbs_launch_rows(16 * n_blocks, 8)]
    w, total = min(window, n_blocks), steps * n_blocks
    return [128 * min(w, total - i0) for i0 in range(0, total, w)]


def gate_launch_rows(n_gates: int) -> list[int]:
    return [min(cs.MAX_CHUNK_BITS, n_gates - g0) for g0 in range(0, n_gates, cs.MAX_CHUNK_BITS)]


def launch_list(name: str, inputs=None, window: int = 0):
    """the m_i of case `name` of workspace_state.CASES at PARAM_TOY, in launch order; None: no plan function gives them.  `inputs`: what
    the case's build returned (the public call's pools depend on its blocks); `window`: the forced window of the block ciphers"""
    if name in NO_K2:
        return []
    if name == "k2_cbs_pbs":
        return [3]
    if name == "gate_ggsw":
        return [2]                                     # the stage call on the two gate bits
    if name.startswith("wopbs_"):
        return wopbs_launch_rows(3, int(name.split("_")[1]))
    if name.startswith(("sbox", "many_sbox")):
        return wopbs_launch_rows(3, 8)
    for direction, steps in sorted(STEPS.items(), key=lambda kv: -len(kv[0])):
        for form, n in (("", 2), ("_keyed", 3), ("_keyed_packed", 3)):
            if name == "aes_%s%s" % (direction, form):
                return window_launch_rows(n, steps, window)
    if name == "aes_encrypt_public":
        return [m for u in _native.aes_public_plan(inputs["blocks"]) for m in wopbs_launch_rows(u, 8)]
    if name in ("gate", "gate_packed"):
        return gate_launch_rows(2)
    return None


def has_launch_list(name: str) -> bool:
    return name == "aes_encrypt_public" or launch_list(name) is not None


def rows_checked(launches, rows: int) -> int:
    """what fheaes_audit_read's rows_checked must be after these launches: S = min(rows, m) each"""
    return sum(min(rows, m) for m in launches)


def largest_pool_launches(plan):
    """(8 x the largest entry of a public plan, the indices of the rounds with that pool): with min_bits at the first, exactly those rounds
    are audited"""
    top = max(plan)
    return 8 * top, [r for r, u in enumerate(plan) if u == top]


def cap_hooks(n_launches: int = 17):
    """(row, word) of the hook of launch j of the record-cap test: r_j = 5 j, word j"""
    return [(5 * j, j) for j in range(n_launches)]
