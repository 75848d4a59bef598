"""What the audit of the key switches costs next to the blind rotation's (fheaes_audit_stage_set), in one process at
PARAM_OPT on one GPU, on resident device tensors: aes_encrypt on 128 blocks with the audit

  off        the default;
  k2_64      64 sampled rows of every blind-rotation launch (tools/audit.py's rows64);
  all_64     64 rows of every K1, K2 and K3 launch;
  all_256    256 rows of each, the most.

The settings ALTERNATE inside one timed loop (wall clock around the call and a synchronize; --warmup rounds, then the median of --steps);
every block of each is decrypted with the client key and compared with FIPS-197 arithmetic, the outputs word for word, and one further call
each runs with the per-stage profile on, after which the stages' counters are read.  --parent LIB: a build of the parent commit's library;
its engine gets the same keys and its `off` call alternates in the same loop, and the branch's `off` is held to 1.03 of it.

The yardstick of the key switches, measured in the same process: the plain form alone (fheaes_audit_plain_batch) on 64 and on 256 rows
inside a 16,384-row input, per stage, K3 over all key blocks as the circuit bootstrap launches it.  The prediction for a setting is the
`off` time + per stage (audited launches) x that, the blind rotation's unit being tools/audit.py's (a launch of S rows audited on all S
minus the same launch unaudited); measured / predicted is held to 1.03, the project's bound for a prediction made of older calls.  The
overhead itself is reported, not bounded: nobody had measured the plain form before this tool.  Prints one JSON line (--out: also written).

    python tools/audit_stages.py [--steps 5] [--warmup 1] [--parent LIB] [--out FILE]
"""
from __future__ import annotations

import statistics
import sys

import numpy as np
import torch

import audit
import measure
from measure import block_bytes, host, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.client import Client

KEY, IV, MASK128, SEED, BLOCKS = audit.KEY, audit.IV, audit.MASK128, audit.SEED, audit.BLOCKS
KS, K2, PF = _native.AUDIT_STAGES
SETTINGS = (("off", 0, ()), ("k2_64", 64, (K2,)), ("all_64", 64, _native.AUDIT_STAGES), ("all_256", 256, _native.AUDIT_STAGES))
INPUT_ROWS = 16384
UNIT_REPS = 10


def set_audit(eng, rows: int, stages) -> None:
    for s in _native.AUDIT_STAGES:
        eng.audit_stage_set(s, rows if s in stages else 0, 0, SEED)


def plain_unit_costs(eng, p, steps: int) -> dict:
    """{stage: {S: median ms of the plain form on S rows in the middle of a 16,384-row input}}"""
    x = to_dev(np.random.default_rng(1).integers(0, 1 << 64, (INPUT_ROWS, p.big1), dtype=np.uint64))
    words = {KS: p.n + 1, PF: (p.k + 1) ** 2 * p.N}
    out = {}
    for stage in (KS, PF):
        res = torch.empty((256, words[stage]), dtype=torch.int64, device="cuda")
        jobs = {}
        for S in (64, 256):
            rows = x[INPUT_ROWS // 2:INPUT_ROWS // 2 + S]

            def run(stage=stage, rows=rows, S=S):
                for _ in range(UNIT_REPS):
                    eng.audit_plain_batch(stage, rows, res, S)

            jobs[S] = (run, lambda: None)
        ts = measure.wall(eng, jobs, 1, steps)
        out[stage] = {S: round(1000 * statistics.median(ts[S]) / UNIT_REPS, 4) for S in jobs}
    return out


def main() -> int:
    ap = measure.arg_parser()
    ap.add_argument("--parent", default=None, help="libfheaes.so built from the parent commit")
    args = ap.parse_args()
    p, n = PARAM_OPT, BLOCKS

    client = Client(1, IV, KEY, params=p, seed=0xAE50001)
    keys = client.server_keys()
    engines = {"branch": _native.Engine(p, device=0)}
    if args.parent:
        engines["parent"] = _native.Engine(p, device=0, library=args.parent)
    d_ek = to_dev(client.encrypt_u128(KEY))
    d_rk = {}
    all_ok = True
    for name, e in engines.items():
        e.upload_keys(keys.ksk, keys.bsk, keys.pfpksk)
        d_rk[name] = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
        e.aes_key_expansion(d_ek, d_rk[name])
        e.synchronize()
        all_ok = all_ok and bool(np.array_equal(client.decrypt_bytes(host(d_rk[name])), np.array(aes_clear.expand_key(KEY), dtype=np.uint8)))
        e.reserve(n * 128)
    eng = engines["branch"]

    k2_unit = audit.audit_unit_costs(eng, p, args.steps)
    plain_unit = plain_unit_costs(eng, p, args.steps)
    unit_ms = {S: {KS: plain_unit[KS][S], K2: k2_unit[S]["audit_ms"], PF: plain_unit[PF][S]} for S in (64, 256)}

    pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
    want = block_bytes([aes_clear.aes128_encrypt_block(KEY, v) for v in pts])
    d_in = to_dev(np.stack([client.encrypt_u128(v) for v in pts]))
    names = [s[0] for s in SETTINGS] + (["parent_off"] if args.parent else [])
    st = {name: torch.empty_like(d_in) for name in names}
    jobs = {}
    for name, rows, stages in SETTINGS:
        def run(name=name):
            eng.aes_encrypt(d_rk["branch"], st[name], n)

        def reset(name=name, rows=rows, stages=stages):
            set_audit(eng, rows, stages)
            st[name].copy_(d_in)

        jobs[name] = (run, reset)
    if args.parent:
        # measure.wall synchronises `eng` after every run; the parent's engine synchronises itself inside its job
        def run_parent():
            engines["parent"].aes_encrypt(d_rk["parent"], st["parent_off"], n)
            engines["parent"].synchronize()

        jobs["parent_off"] = (run_parent, lambda: st["parent_off"].copy_(d_in))
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: measure.progress("audit_stages", "step %d / %d: %.1f s" % (i, of, s)))
    words = {name: host(st[name]) for name in jobs}

    results = {}
    for name, rows, stages in SETTINGS:
        prof = measure.profiled(eng, *jobs[name])
        counters = {s: eng.audit_stage_read(s) for s in _native.AUDIT_STAGES}
        got = client.decrypt_bytes(words[name])
        wrong = [b for b in range(n) if not np.array_equal(got[b], want[b])]
        results[name] = {"rows": rows, "stages": list(stages), **measure.row(times[name], n), "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                         "launches": {s: prof[s]["launches"] for s in _native.AUDIT_STAGES},
                         "audit": {s: {k: int(c[k]) for k in ("launches", "rows_checked", "rows_wrong")} for s, c in counters.items()},
                         "stages_ms": measure.stage_ms(prof)}
        for s, c in counters.items():
            all_ok = all_ok and c["rows_wrong"] == 0 and c["launches"] == (prof[s]["launches"] if s in stages and rows else 0)
        all_ok = all_ok and not wrong
    set_audit(eng, 0, ())
    if args.parent:
        got = client.decrypt_bytes(words["parent_off"])
        wrong = [b for b in range(n) if not np.array_equal(got[b], want[b])]
        results["parent_off"] = {**measure.row(times["parent_off"], n), "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                                 "version": engines["parent"]._lib.fheaes_version().decode()}
        all_ok = all_ok and not wrong
    same_words = all(np.array_equal(words["off"], words[name]) for name in words)
    all_ok = all_ok and same_words

    off = results["off"]["ms_median"]
    checks = {}
    for name, rows, stages in SETTINGS[1:]:
        r = results[name]
        added = {s: round(r["audit"][s]["launches"] * unit_ms[rows][s], 3) for s in stages}
        predicted = off + sum(added.values())
        checks[name] = {**measure.check(r["ms_median"], predicted, 1.03), "overhead_percent": round(100 * (r["ms_median"] / off - 1), 3),
                        "predicted_overhead_percent": round(100 * (predicted / off - 1), 3), "predicted_added_ms": added,
                        "stage_growth_ms": {s: round(r["stages_ms"][s] - results["off"]["stages_ms"][s], 3) for s in _native.AUDIT_STAGES}}
    if args.parent:
        checks["off_against_parent"] = measure.check(off, results["parent_off"]["ms_median"], 1.03)
    line = {**measure.header("audit_stages", args), "blocks": n, "all_verified": all_ok, "same_words": same_words,
            "plain_unit_ms": {s: {str(S): v for S, v in d.items()} for s, d in plain_unit.items()},
            "k2_audit_unit": {str(S): v for S, v in k2_unit.items()}, "settings": results, "checks": checks,
            "note": "aes_encrypt on 128 blocks; the settings%s alternate inside one timed loop on resident tensors (call + synchronize), median of the "
                    "timed steps; stages_ms and the counters from one further profiled call each; plain_unit_ms: fheaes_audit_plain_batch on S rows "
                    "inside a 16,384-row input, %d back-to-back calls per timed step; k2_audit_unit as tools/audit.py; predicted = off + per stage "
                    "audited launches x unit, bound 1.03 on measured / predicted%s"
                    % (" and the parent library's unaudited call" if args.parent else "", UNIT_REPS,
                       "; off_against_parent: this library's off against the parent's, bound 1.03" if args.parent else "")}
    measure.emit(line, args.out)
    for e in engines.values():
        e.close()
    return measure.exit_code(all_ok, all(c["within_bound"] for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
