"""The block ciphers with and without their rounds rolled over windows of blocks (fheaes_aes_set_window), in one
process at PARAM_OPT on one GPU, on resident device tensors:

  off    FHEAES_AES_WINDOW_OFF: one WoPBS per round, every blind-rotation launch ends in a partly filled generation;
  auto   the default: windows of whole six-ciphertext generations (fheaes_aes_context_window), one partial generation per call.

For aes_encrypt at 128 and 32 blocks and aes_decrypt at 32 blocks the two settings ALTERNATE inside one timed loop (wall clock around
the call and a synchronize; --warmup rounds, then the median of --steps), every block of both is decrypted with the client key and
compared with FIPS-197 arithmetic and the two outputs word for word, and one further call each runs with the per-stage profile on
(fheaes_profile_read; HIP events around every launch, so kept out of the timed calls).

The cost of a six-ciphertext generation (g6) and of the four-ciphertext tail generation (g4) are measured in the same process from
blind-rotation launches of 1,024, 4,096 and 16,384 bits (= 1 x g4', 2 g6 + g4, 10 g6 + g4): g6 = (t16384 - t4096) / 8, g4 = t4096 - 2 g6.
Rolling turns the 128-block step's 100 g6 + 10 g4 into 106 g6 + 1 g4, so the blind-rotation stage must shrink by 9 g4 - 6 g6; the line
says whether it shrank by at least 0.8 of that (the power-capped clock moves with the mix of generations) and whether the sum of all
other stages grew by no more than the spread of the `off` runs.  Prints one JSON line (--out: also written there).

    python tools/aes_windows.py [--steps 5] [--warmup 1] [--out FILE]
"""
from __future__ import annotations

import statistics
import sys

import numpy as np
import torch

import measure
from measure import block_bytes, host, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear

KEY = 0x2B7E151628AED2A6ABF7158809CF4F3C
IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
MASK128 = (1 << 128) - 1
SETTINGS = (("off", _native.AES_WINDOW_OFF), ("auto", 0))
SHAPES = (("aes_encrypt", 128, 10), ("aes_encrypt", 32, 10), ("aes_decrypt", 32, 19))


def k2_generation_costs(eng: _native.Engine, p, launches: int) -> dict:
    """median ms of `launches` blind-rotation launches (after one warm-up) per size on the schedule without windows, and g6, g4 from them"""
    rng = np.random.default_rng(0)
    ms = {}
    for m in (1024, 4096, 16384):
        small = to_dev(rng.integers(0, 1 << 64, (m, p.n + 1), dtype=np.uint64))
        out = torch.empty((m, p.big1), dtype=torch.int64, device="cuda")
        ts = measure.wall(eng, {m: (lambda: eng.cbs_pbs_batch(small, out, m), lambda: None)}, 1, launches)[m]      # a loop per size
        ms[m] = 1000 * statistics.median(ts)
    g6 = (ms[16384] - ms[4096]) / 8
    g4 = ms[4096] - 2 * g6
    return {"ms_per_launch": {str(m): round(v, 3) for m, v in ms.items()}, "g6_ms": round(g6, 3), "g4_ms": round(g4, 3),
            "kernel": eng.k2_plan(16384)["kernel"]}


def main() -> int:
    args = measure.arg_parser().parse_args()
    p = PARAM_OPT

    client, eng = measure.session(0xAE50001, IV, KEY)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    d_rk = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ek = to_dev(client.encrypt_u128(KEY))
    eng.aes_key_expansion(d_ek, d_rk)
    eng.synchronize()
    all_ok = bool(np.array_equal(client.decrypt_bytes(host(d_rk)), np.array(aes_clear.expand_key(KEY), dtype=np.uint8)))
    eng.reserve(128 * 128)

    eng.aes_set_window(_native.AES_WINDOW_OFF)
    gen = k2_generation_costs(eng, p, args.steps)
    eng.aes_set_window(0)

    results = {}
    for cipher, n, steps in SHAPES:
        pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
        cts = [aes_clear.aes128_encrypt_block(KEY, v) for v in pts]
        clear_in, clear_out = (pts, cts) if cipher == "aes_encrypt" else (cts, pts)
        want = block_bytes(clear_out)
        d_in = to_dev(np.stack([client.encrypt_u128(v) for v in clear_in]))
        fn = getattr(eng, cipher)
        plan = _native.aes_window_plan(n, steps, cus, p.k)
        row = {"plan_at_%d_cus" % cus: plan}
        # a state per setting, so that each one's words outlast the other's calls; the reset of a job also makes its setting the engine's.
        # off / auto alternate inside one loop: both settings see the same clock drift
        st = {name: torch.empty_like(d_in) for name, _ in SETTINGS}
        jobs = {}
        for name, setting in SETTINGS:
            def run(name=name):
                fn(d_rk, st[name], n)

            def reset(name=name, setting=setting):
                eng.aes_set_window(setting)
                st[name].copy_(d_in)

            jobs[name] = (run, reset)
        times = measure.wall(eng, jobs, args.warmup, args.steps)
        words = {name: host(st[name]) for name in jobs}                # read before the profiled calls overwrite them
        for name in jobs:
            prof = measure.profiled(eng, *jobs[name])
            window = eng.aes_window(n, steps)
            got = client.decrypt_bytes(words[name])
            wrong = [b for b in range(n) if not np.array_equal(got[b], want[b])]
            row[name] = {"window_blocks": window, **measure.row(times[name], n),
                         "blocks_verified": n - len(wrong), "wrong_blocks": wrong, "k2_launches": prof["blind_rotate"]["launches"],
                         "stages_ms": measure.stage_ms(prof),
                         "other_stages_ms": round(sum(v["ms"] for k, v in prof.items() if k != "blind_rotate"), 3)}
            all_ok = all_ok and not wrong
        eng.aes_set_window(0)
        row["same_words"] = bool(np.array_equal(words["off"], words["auto"]))
        row["gain"] = round(1 - row["auto"]["ms_median"] / row["off"]["ms_median"], 5)
        row["k2_stage_reduction_ms"] = round(row["off"]["stages_ms"]["blind_rotate"] - row["auto"]["stages_ms"]["blind_rotate"], 3)
        row["other_stages_growth_ms"] = round(row["auto"]["other_stages_ms"] - row["off"]["other_stages_ms"], 3)
        row["off_spread_ms"] = round(1000 * max(times["off"]) - 1000 * min(times["off"]), 3)
        all_ok = all_ok and row["same_words"]
        results["%s_%d" % (cipher, n)] = row
        del d_in, st

    head = results["aes_encrypt_128"]
    predicted = 9 * gen["g4_ms"] - 6 * gen["g6_ms"]
    checks = {"predicted_k2_reduction_ms": round(predicted, 3), "required_k2_reduction_ms": round(0.8 * predicted, 3),
              "measured_k2_reduction_ms": head["k2_stage_reduction_ms"],
              "k2_reduction_ok": head["k2_stage_reduction_ms"] >= 0.8 * predicted,
              "other_stages_ok": head["other_stages_growth_ms"] <= head["off_spread_ms"]}
    line = {**measure.header("aes_windows", args), "cu_count": cus, "all_verified": all_ok, "k2_generations": gen, "shapes": results, "checks": checks,
            "note": "off / auto alternate inside one timed loop on resident tensors (call + synchronize), median of the timed steps; stages_ms "
                    "from one further profiled call each (HIP events around every launch); g6 = (t16384 - t4096) / 8, g4 = t4096 - 2 g6 from "
                    "blind-rotation launches in the same process; checks are for aes_encrypt at 128 blocks: the blind-rotation stage must shrink "
                    "by at least 0.8 x (9 g4 - 6 g6), the other stages together may grow by no more than the spread of the off runs"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok)


if __name__ == "__main__":
    sys.exit(main())
