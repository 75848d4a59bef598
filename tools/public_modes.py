"""The public-ciphertext modes against the entry points they are built from, at PARAM_OPT on one GPU, resident tensors, AES-128:

  cbc                  aes_cbc_decrypt of n random ciphertext blocks           (the equivalent inverse cipher on pools, 4 LUTs per entry)
  eq_round_by_round    aes_decrypt_equivalent on the uploaded trivial state, the round window turned off (fheaes_aes_set_window): the
                       yardstick, since the public path is not windowed
  eq_windowed          the same call with the context's automatic window       (reported, no bound)
  ctr32                aes_ctr(counter_bits=32), n counters that do not wrap
  ctr128               aes_ctr on the same counter blocks

One process, one context; every job runs once in every step of ONE timed loop, its reset (outside the timed interval) restoring its
state and setting the window it runs under; the median of --steps steps after --warmup.  Every block of every output is decrypted with
the client key and compared with aes_clear: a wrong block makes the tool exit 1.

    T(cbc) <= 1.03 T(eq_round_by_round) sum(plan) / (16 n Nr)        and        T(ctr32) <= 1.03 T(ctr128)

1.03 is the margin every earlier entry point of this kind was given against a prediction from older entry points.  `checks` in the output
records prediction, measurement, ratio and whether the bound holds; a missed bound makes the tool exit 2.

    python tools/public_modes.py [--blocks 128] [--steps 5] [--warmup 1] [--out profiles/public_modes.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import block_bytes, host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.client import u128_to_bytes

KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")           # SP 800-38A F.1.1
IV = 0x000102030405060708090A0B0C0D0E0F
ICB = 0xCAFEBABEFACEDBADDECAF88800000002                           # SP 800-38D test case 3: the first data block's counter
NR = 10
TOOL = "public_modes"


def main() -> int:
    args = measure.arg_parser(blocks="128").parse_args()
    n = int(args.blocks)
    p = PARAM_OPT
    client, eng = measure.session(0xAE50001, IV, int.from_bytes(KEY, "big"))

    d_rk = torch.empty((NR + 1, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    eng.aes_key_expansion_bits(to_dev(client.encrypt_aes_key(KEY)), 128, d_rk)
    d_dw = torch.empty_like(d_rk)
    eng.aes_decryption_round_keys(d_rk, d_dw)
    eng.synchronize()
    eng.reserve(n * 128)

    rng = np.random.default_rng(0xCBC)
    ct = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    counters = [ICB + i for i in range(n)]
    plan = _native.aes_decrypt_public_plan(ct)
    d_trivial = to_dev(client.trivial_bytes([u128_to_bytes(b) for b in ct]))
    out = {k: torch.empty((n, 16, 8, p.big1), dtype=torch.int64, device="cuda") for k in ("cbc", "eq_round_by_round", "eq_windowed", "ctr32", "ctr128")}

    def state(name, window):
        def reset():
            out[name].copy_(d_trivial)
            eng.aes_set_window(window)
        return reset

    plain = lambda: eng.aes_set_window(_native.AES_WINDOW_OFF)  # noqa: E731
    dec = block_bytes([aes_clear.aes_decrypt_block(KEY, b) for b in ct])
    ks = block_bytes([aes_clear.aes_encrypt_block(KEY, b) for b in counters])
    # name -> (run, reset, the blocks the output must decrypt to)
    jobs = {
        "cbc": (lambda: eng.aes_cbc_decrypt_bits(d_dw, 128, IV, ct, out["cbc"]), plain, block_bytes(aes_clear.cbc_decrypt(KEY, IV, ct))),
        "eq_round_by_round": (lambda: eng.aes_decrypt_equivalent_bits(d_dw, 128, out["eq_round_by_round"], n),
                              state("eq_round_by_round", _native.AES_WINDOW_OFF), dec),
        "eq_windowed": (lambda: eng.aes_decrypt_equivalent_bits(d_dw, 128, out["eq_windowed"], n), state("eq_windowed", 0), dec),
        "ctr32": (lambda: eng.aes_ctr_bits(d_rk, 128, ICB, 0, None, n, out["ctr32"], counter_bits=32), plain, ks),
        "ctr128": (lambda: eng.aes_ctr_bits(d_rk, 128, ICB, 0, None, n, out["ctr128"]), plain, ks),
    }
    times = measure.wall(eng, {k: j[:2] for k, j in jobs.items()}, args.warmup, args.steps,
                         on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    all_ok, rows = True, {}
    for k, (run, reset, want) in jobs.items():
        row = measure.row(times[k], n)
        got = client.decrypt_bytes(host(out[k]))
        wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
        all_ok = all_ok and not wrong
        row.update({"blocks_verified": n - len(wrong), "wrong_blocks": wrong})
        prof = measure.profiled(eng, run, reset)
        row["stages_ms"] = measure.stage_ms(prof)
        row["stages_units"] = {s: v["units"] for s, v in prof.items()}
        rows[k] = row
        progress(TOOL, "%s, %d blocks: %.1f ms" % (k, n, row["ms_median"]))
    same_words = bool(torch.equal(out["cbc"], out["eq_round_by_round"] + to_dev(client.trivial_bytes([u128_to_bytes(b) for b in [IV] + ct[:-1]])))
                      and torch.equal(out["ctr32"], out["ctr128"]))
    all_ok = all_ok and same_words

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    share = sum(plan) / (16 * n * NR)
    checks = {"cbc": {"byte_wopbs": sum(plan), "share_of_16_n_Nr": round(share, 6), **measure.check(T("cbc"), T("eq_round_by_round") * share, 1.03)},
              "ctr32": measure.check(T("ctr32"), T("ctr128"), 1.03),
              "cbc_against_windowed_aes_decrypt_equivalent": measure.check(T("cbc"), T("eq_windowed") * share, None)}
    for name, c in checks.items():
        progress(TOOL, "%s: %.1f ms, predicted %.1f ms, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    line = {**measure.header(TOOL, args), "blocks": n, "all_verified": all_ok, "same_words_as_the_older_entry_points": same_words, "checks": checks,
            "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one "
                    "loop; cbc is predicted from aes_decrypt_equivalent with the round window off times sum(plan) / (16 n Nr), ctr32 from aes_ctr "
                    "on the same counter blocks; the comparison with the windowed aes_decrypt_equivalent has no bound"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
