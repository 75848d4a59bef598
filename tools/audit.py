"""What the audit of the blind rotation costs (fheaes_audit_set), in one process at PARAM_OPT on one GPU, on resident
device tensors: aes_encrypt on 128 blocks with the audit

  off        the default;
  rows64     64 sampled rows of every blind-rotation launch re-run through the latency form and compared on the device;
  rows256    256 rows, the most: one latency-form workgroup per CU.

The three settings ALTERNATE inside one timed loop (wall clock around the call and a synchronize; --warmup rounds, then the median of
--steps); every block of each is decrypted with the client key and compared with FIPS-197 arithmetic, the three outputs word for word, and
one further call each runs with the per-stage profile on, after which the audit's counters are read (they are that call's alone: the
job's reset is a fheaes_audit_set).

The yardstick, measured in the same process: what one audit of S rows adds to a launch is a latency-form launch of S rows and the two small
kernels around it, so a blind-rotation launch of S rows with the audit on S rows (every row sampled: the launch, the gather, the same launch
again, the compare) minus the same launch with the audit off.  The prediction for a setting is the `off` time + (audited launches) x that;
measured / predicted is held to 1.03.  Nobody had measured the latency form behind a full paired launch before this tool: the overhead
itself is reported, not bounded.  Prints one JSON line (--out: also written there).

    python tools/audit.py [--steps 5] [--warmup 1] [--out FILE]
"""
from __future__ import annotations

import statistics
import sys

import numpy as np
import torch

import measure
from measure import block_bytes, host, to_dev
from tfhe_aes_amd import PARAM_OPT, aes_clear

KEY = 0x2B7E151628AED2A6ABF7158809CF4F3C
IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
MASK128 = (1 << 128) - 1
SEED = 0xA0D175EED
BLOCKS = 128
SETTINGS = (("off", 0), ("rows64", 64), ("rows256", 256))
UNIT_REPS = 10                          # back-to-back launches per timed step of the yardstick


def audit_unit_costs(eng, p, steps: int) -> dict:
    """per S: median ms of a blind-rotation launch of S rows with the audit off (`cbs_pbs_ms`) and with the audit on all S rows; their
    difference is what one audit of S rows adds (`audit_ms`), and what exceeds a second launch in it the two small kernels"""
    rng = np.random.default_rng(0)
    out = {}
    for _, S in SETTINGS[1:]:
        small = to_dev(rng.integers(0, 1 << 64, (S, p.n + 1), dtype=np.uint64))
        res = torch.empty((S, p.big1), dtype=torch.int64, device="cuda")

        def run():
            for _ in range(UNIT_REPS):
                eng.cbs_pbs_batch(small, res, S)

        jobs = {"plain": (run, lambda: eng.audit_set(0)), "audited": (run, lambda S=S: eng.audit_set(S, 0, SEED))}
        ts = measure.wall(eng, jobs, 1, steps)
        plain, audited = (1000 * statistics.median(ts[k]) / UNIT_REPS for k in ("plain", "audited"))
        out[S] = {"cbs_pbs_ms": round(plain, 4), "audited_ms": round(audited, 4), "audit_ms": round(audited - plain, 4),
                  "small_kernels_ms": round(audited - 2 * plain, 4), "kernel": eng.k2_plan(S)["kernel"]}
    eng.audit_set(0)
    return out


def main() -> int:
    args = measure.arg_parser().parse_args()
    p, n = PARAM_OPT, BLOCKS

    client, eng = measure.session(0xAE50001, IV, KEY)
    d_rk = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ek = to_dev(client.encrypt_u128(KEY))
    eng.aes_key_expansion(d_ek, d_rk)
    eng.synchronize()
    all_ok = bool(np.array_equal(client.decrypt_bytes(host(d_rk)), np.array(aes_clear.expand_key(KEY), dtype=np.uint8)))
    eng.reserve(n * 128)

    unit = audit_unit_costs(eng, p, args.steps)

    pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
    want = block_bytes([aes_clear.aes128_encrypt_block(KEY, v) for v in pts])
    d_in = to_dev(np.stack([client.encrypt_u128(v) for v in pts]))
    # a state per setting, so that each one's words outlast the other's calls; the reset of a job also makes its setting the engine's
    # (fheaes_audit_set synchronises and zeroes the counters, outside the timed interval)
    st = {name: torch.empty_like(d_in) for name, _ in SETTINGS}
    jobs = {}
    for name, rows in SETTINGS:
        def run(name=name):
            eng.aes_encrypt(d_rk, st[name], n)

        def reset(name=name, rows=rows):
            eng.audit_set(rows, 0, SEED)
            st[name].copy_(d_in)

        jobs[name] = (run, reset)
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: measure.progress("audit", "step %d / %d: %.1f s" % (i, of, s)))
    words = {name: host(st[name]) for name in jobs}                    # read before the profiled calls overwrite them
    results = {}
    for name, rows in SETTINGS:
        prof = measure.profiled(eng, *jobs[name])
        counters = eng.audit_read()
        got = client.decrypt_bytes(words[name])
        wrong = [b for b in range(n) if not np.array_equal(got[b], want[b])]
        results[name] = {"rows": rows, **measure.row(times[name], n), "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                         "k2_launches": prof["blind_rotate"]["launches"], "k2_units": prof["blind_rotate"]["units"],
                         "audit": {"launches": counters["launches"], "rows_checked": counters["rows_checked"], "rows_wrong": counters["rows_wrong"]},
                         "stages_ms": measure.stage_ms(prof)}
        all_ok = all_ok and not wrong and counters["rows_wrong"] == 0 and counters["launches"] == (prof["blind_rotate"]["launches"] if rows else 0)
    eng.audit_set(0)
    same_words = all(np.array_equal(words["off"], words[name]) for name in words)
    all_ok = all_ok and same_words

    off = results["off"]["ms_median"]
    checks = {}
    for name, rows in SETTINGS[1:]:
        r = results[name]
        predicted = off + r["audit"]["launches"] * unit[rows]["audit_ms"]
        checks[name] = {**measure.check(r["ms_median"], predicted, 1.03), "overhead_percent": round(100 * (r["ms_median"] / off - 1), 3),
                        "predicted_overhead_percent": round(100 * (predicted / off - 1), 3),
                        "k2_stage_growth_ms": round(r["stages_ms"]["blind_rotate"] - results["off"]["stages_ms"]["blind_rotate"], 3)}
    line = {**measure.header("audit", args), "blocks": n, "all_verified": all_ok, "same_words": same_words,
            "audit_unit": {str(S): v for S, v in unit.items()}, "settings": results, "checks": checks,
            "note": "aes_encrypt on 128 blocks; off / rows64 / rows256 alternate inside one timed loop on resident tensors (call + synchronize), median "
                    "of the timed steps; stages_ms and the audit's counters from one further profiled call each; audit_unit: a blind-rotation launch of "
                    "S rows with the audit on all S rows minus the same launch with the audit off, %d back-to-back launches per timed step, same "
                    "process; predicted = off + audited launches x audit_unit.audit_ms, bound 1.03 on measured / predicted" % UNIT_REPS}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, all(c["within_bound"] for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
