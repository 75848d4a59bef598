"""XTS-AES decryption against the entry points it is built from, at PARAM_OPT on one GPU, resident tensors, AES-128, 4 data units of 32
blocks (4 x 512 bytes):

  xts          aes_xts_decrypt of the 128 ciphertext blocks
  eq           aes_decrypt_equivalent on 128 blocks (the uploaded trivial state of the ciphertext), the context's automatic window, as
               the call's own cipher runs
  public4      aes_encrypt_public of the 4 tweak blocks
  ident64      the identity many_wopbs_without_padding on 64 bytes   (the 4 anchors)
  ident2048    the identity many_wopbs_without_padding on 2,048 bytes (the 128 tweaks)

One process, one context; every job runs once in every step of ONE timed loop (measure.wall), the median of --steps steps after --warmup.
Every block of every output is decrypted with the client key and compared with aes_clear: a wrong block makes the tool exit 1.

    (a)  T(xts) <= 1.03 (T(eq) + T(public4) + T(ident64) + T(ident2048))

1.03 is the margin every earlier entry point of this kind was given against a prediction from older entry points.

    (b)  bit_rows_kernel<XtsRows> over 128 tweak blocks (fheaes_xts_tweaks, 4 units x 32 offsets) against gather_add_kernel with a four-term table
         and no key over the same number of output bytes (fheaes_inv_mix_columns_batch on 128 blocks), device events around --reps
         calls of each, alternating; bound 1.5.

Also in the record: the stage split of the call and the byte-WoPBS of fheaes_aes_xts_plan next to the profile's units.  A missed bound
makes the tool exit 2.

    python tools/xts.py [--steps 5] [--warmup 1] [--reps 20] [--out profiles/xts.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear

KEY1 = bytes.fromhex("27182818284590452353602874713526")          # IEEE 1619 vector 4
KEY2 = bytes.fromhex("31415926535897932384626433832795")
SECTOR, UNITS, BPU, NR = 0x3333333333, 4, 32, 10
TOOL = "xts"


def main() -> int:
    args = measure.arg_parser(reps=20).parse_args()
    p, n = PARAM_OPT, UNITS * BPU
    client, eng = measure.session(0xAE50001)

    def expanded(key):
        d = torch.empty((NR + 1, 16, 8, p.big1), dtype=torch.int64, device="cuda")
        eng.aes_key_expansion_bits(to_dev(client.encrypt_aes_key(key)), 128, d)
        return d

    d_rk1, d_rk2 = expanded(KEY1), expanded(KEY2)
    d_dw1 = torch.empty_like(d_rk1)
    eng.aes_decryption_round_keys(d_rk1, d_dw1)
    eng.synchronize()
    eng.reserve(n * 128)

    pt = np.random.default_rng(0x1619).bytes(16 * n)
    ct = b"".join(aes_clear.xts_encrypt(KEY1, KEY2, SECTOR + u, pt[512 * u:512 * (u + 1)]) for u in range(UNITS))
    ct_blocks = [ct[16 * i:16 * i + 16] for i in range(n)]
    tweaks = [aes_clear.xts_tweak_block(SECTOR + u) for u in range(UNITS)]
    d_trivial = to_dev(client.trivial_bytes(np.frombuffer(ct, dtype=np.uint8).reshape(n, 16)))
    d_ident = to_dev(_native.gen_lut(8, np.arange(256))[None])
    state = lambda blocks: torch.empty((blocks, 16, 8, p.big1), dtype=torch.int64, device="cuda")  # noqa: E731
    out = {"xts": state(n), "eq": state(n), "public4": state(UNITS), "ident64": state(UNITS), "ident2048": state(n)}
    eng.aes_encrypt_public_bits(d_rk2, 128, tweaks, out["public4"])
    eng.synchronize()
    d_e = out["public4"].clone()                                     # E_K2(tweak): the input of the 64-byte refresh
    torch.cuda.synchronize()

    nothing = lambda: None  # noqa: E731
    rows16 = lambda b: np.frombuffer(b, dtype=np.uint8).reshape(-1, 16)  # noqa: E731
    e_clear = measure.block_bytes([aes_clear.aes_encrypt_block(KEY2, t) for t in tweaks])
    # name -> (run, reset, the bytes the output must decrypt to)
    jobs = {
        "xts": (lambda: eng.aes_xts_decrypt_bits(d_dw1, d_rk2, 128, tweaks, BPU, 0, ct_blocks, out["xts"]), nothing, rows16(pt)),
        "eq": (lambda: eng.aes_decrypt_equivalent_bits(d_dw1, 128, out["eq"], n), lambda: out["eq"].copy_(d_trivial),
               measure.block_bytes([aes_clear.aes_decrypt_block(KEY1, int.from_bytes(b, "big")) for b in ct_blocks])),
        "public4": (lambda: eng.aes_encrypt_public_bits(d_rk2, 128, tweaks, out["public4"]), nothing, e_clear),
        "ident64": (lambda: eng.wopbs_batch(d_e.view(-1, 8, p.big1), 16 * UNITS, 8, d_ident, 1, False, out["ident64"]), nothing, e_clear),
        "ident2048": (lambda: eng.wopbs_batch(d_trivial.view(-1, 8, p.big1), 16 * n, 8, d_ident, 1, False, out["ident2048"]), nothing, rows16(ct)),
    }
    times = measure.wall(eng, {k: j[:2] for k, j in jobs.items()}, args.warmup, args.steps,
                         on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    all_ok, rows = True, {}
    for k, (run, reset, want) in jobs.items():
        blocks = len(want)
        row = measure.row(times[k], blocks)
        got = client.decrypt_bytes(host(out[k]))
        wrong = [i for i in range(blocks) if not np.array_equal(got[i], want[i])]
        all_ok = all_ok and not wrong
        row.update({"blocks_verified": blocks - len(wrong), "wrong_blocks": wrong})
        prof = measure.profiled(eng, run, reset)
        row["stages_ms"] = measure.stage_ms(prof)
        row["stages_units"] = {s: v["units"] for s, v in prof.items()}
        row["stages_launches"] = {s: v["launches"] for s, v in prof.items()}
        rows[k] = row
        progress(TOOL, "%s, %d blocks: %.1f ms" % (k, blocks, row["ms_median"]))

    # (b) the tweak kernel alone: 4 units x 32 offsets from the refreshed anchors, checked against the rows of fheaes_xts_tweak_row
    d_anchor = out["ident64"].view(UNITS, 128, p.big1)
    d_tw = torch.empty((UNITS, BPU, 128, p.big1), dtype=torch.int64, device="cuda")
    d_mul = torch.empty((n, 16, 4, 8, p.big1), dtype=torch.int64, device="cuda")
    eng.many_sbox(d_trivial.view(-1, 8, p.big1), 16 * n, True, d_mul)
    d_mix = torch.empty((n, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    ev = measure.events(eng, {"tweaks": lambda: eng.xts_tweaks(d_anchor, UNITS, 0, BPU, d_tw), "gather": lambda: eng.inv_mix_columns_batch(d_mul, n, d_mix)},
                        args.warmup, args.steps, args.reps)
    ms = ev["tweaks"]
    mixed = client.decrypt_bytes(host(d_mix))
    all_ok = all_ok and all(mixed[i].tolist() == aes_clear._mix(list(ct_blocks[i]), (14, 11, 13, 9)) for i in range(n))
    a, t = host(d_anchor), host(d_tw)
    for u, j in ((0, 0), (1, 7), (UNITS - 1, BPU - 1)):
        want = np.stack([sum((a[u, s] for s in _native.xts_tweak_row(j, i)), np.zeros(p.big1, dtype=np.uint64)) for i in range(128)])
        all_ok = all_ok and np.array_equal(t[u, j], want)
    tweak_ms = float(np.median(ms))
    gather_ms = float(np.median(ev["gather"]))
    out_bytes = UNITS * BPU * 128 * p.big1 * 8

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    plan = _native.aes_xts_plan(UNITS, BPU, 0, n, 128)
    public_bytes = sum(_native.aes_public_plan(tweaks, 128))
    checks = {"xts": measure.check(T("xts"), T("eq") + T("public4") + T("ident64") + T("ident2048"), 1.03),
              "tweak_kernel_against_the_four_term_gather": {**measure.check(tweak_ms, gather_ms, 1.5), "output_bytes": out_bytes,
                                                            "tweak_kernel_GB_per_s_written": round(out_bytes / tweak_ms / 1e6, 1),
                                                            "ms_all": [round(v, 4) for v in ms],
                                                            "gather_ms_all": [round(v, 4) for v in ev["gather"]]}}
    for name, c in checks.items():
        progress(TOOL, "%s: %.3f ms, predicted %.3f ms, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    units = rows["xts"]["stages_units"]["blind_rotate"]
    line = {**measure.header(TOOL, args), "blocks": n, "units": UNITS, "blocks_per_unit": BPU, "all_verified": bool(all_ok), "checks": checks,
            "plan": {**plan, "tweak_blocks_public_bytes": public_bytes,
                     "byte_wopbs": plan["tweak_refresh_bytes"] + plan["cipher_bytes"] + public_bytes, "profile_blind_rotate_bits": units,
                     "profile_bits_are_8_x_byte_wopbs": units == 8 * (plan["tweak_refresh_bytes"] + plan["cipher_bytes"] + public_bytes)},
            "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one "
                    "loop; xts is predicted from aes_decrypt_equivalent on 128 blocks + aes_encrypt_public on the 4 tweak blocks + the identity "
                    "WoPBS on 64 and on 2,048 bytes; the tweak kernel and the four-term gather without a key (fheaes_inv_mix_columns_batch on 128 "
                    "blocks, as many output bytes) are timed with device events around --reps calls of each, alternating"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(bool(all_ok), all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
