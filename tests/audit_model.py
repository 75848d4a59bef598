"""A Python-integer model of fheaes_audit_rows (include/fheaes.h, "audit"): which rows of a blind-rotation launch the audit re-runs.
A plain module like xts.py: imported by name, not collected."""

MASK = (1 << 64) - 1
MAX_ROWS = 256


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def mix(seed: int, launch: int, s: int) -> int:
    return splitmix64((splitmix64((seed + launch) & MASK) + s) & MASK)


def strata(m: int, rows: int) -> list[tuple[int, int]]:
    """the S = min(rows, m) strata [lo, hi) of a launch of m rows"""
    S = min(rows, m)
    return [(s * m // S, (s + 1) * m // S) for s in range(S)]


def audit_rows(seed: int, launch: int, m: int, rows: int) -> list[int]:
    """sample s: its stratum's start + mix(seed, launch, s) mod the stratum's length"""
    assert m >= 1 and 1 <= rows <= MAX_ROWS
    return [lo + mix(seed, launch, s) % (hi - lo) for s, (lo, hi) in enumerate(strata(m, rows))]


def caught_run_length(m: int, rows: int) -> int:
    """2 ceil(m / S) - 1: a run of this many consecutive rows holds a whole stratum wherever it starts"""
    S = min(rows, m)
    return 2 * -(-m // S) - 1
