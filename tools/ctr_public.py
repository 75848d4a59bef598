"""CTR with a public nonce against the ways to the same blocks that the engine had before, at PARAM_OPT on one GPU, resident tensors:

  ctr_aligned          aes_ctr, n consecutive counters from ..00          (one S-Box evaluation per DISTINCT input of the batch)
  ctr_fa               aes_ctr, n consecutive counters from ..FA          (the low byte wraps inside the batch)
  public_no_sharing    aes_encrypt_public on n blocks that share nothing  (every position draws its n bytes without replacement)
  aes_encrypt          aes_encrypt on a resident encrypted state          (the yardstick: 16 n S-Boxes in every round)
  reference_iteration  add_scalar + aes_encrypt on n copies of an encrypted IV   (the reference's CTR iteration, main.rs:59-61)

for AES-128 / 192 / 256 at 128 and 32 blocks, plus aes_decryption_round_keys at AES-128 (two 1,152-bit WoPBS).  One process; every
variant of every size runs once in every step of ONE timed loop, so a drift of the clocks meets all of them alike; the median of
--steps steps after --warmup.  Every block of every output is decrypted with the client key and compared with aes_clear: a wrong block
makes the tool exit 1.  One further call per variant runs with the per-stage profile on (HIP events around every launch, so kept out of
the timed calls) and records milliseconds and fheaes_profile_read units per stage.

The time of aes_ctr on 128 aligned AES-128 blocks was derived before it was measured: eight full rounds, a
4,192-bit round that costs what a 4,096-bit one does, a 1,144-bit round that costs what a 1,152-bit WoPBS does.  All three are entry
points that existed before, measured here in the same loop:

    P = 0.8 T(aes_encrypt, 128 blocks) + 0.1 T(aes_encrypt, 32 blocks) + 0.5 T(aes_decryption_round_keys)
    T(ctr_aligned, 128 blocks, AES-128) <= 1.03 P           and           T(public_no_sharing, 128) <= 1.03 T(aes_encrypt, 128)

`check` in the output records prediction, measurement, ratio and whether the bound holds; a missed bound makes the tool exit 2.

    python tools/ctr_public.py [--blocks 128,32] [--steps 5] [--warmup 1] [--out profiles/ctr_public.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import block_bytes, host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear

# SP 800-38A F.1.1 / F.1.3 / F.1.5
KEYS = {128: bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"),
        192: bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"),
        256: bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")}
NR = {128: 10, 192: 12, 256: 14}
SIZES = (128, 192, 256)
IV = 0x00112233445566778899AABBCCDDEE00
MASK128 = (1 << 128) - 1
VARIANTS = ("ctr_aligned", "ctr_fa", "public_no_sharing", "aes_encrypt", "reference_iteration")
TOOL = "ctr_public"


def main() -> int:
    args = measure.arg_parser(blocks="128,32").parse_args()
    batch_sizes = [int(x) for x in args.blocks.split(",")]
    p = PARAM_OPT

    client, eng = measure.session(0xAE50001, IV, int.from_bytes(KEYS[128], "big"))

    d_rk, d_dw = {}, None
    for bits in SIZES:
        d_ek = to_dev(client.encrypt_aes_key(KEYS[bits]))
        d_rk[bits] = torch.empty((NR[bits] + 1, 16, 8, p.big1), dtype=torch.int64, device="cuda")
        eng.aes_key_expansion_bits(d_ek, bits, d_rk[bits])
        eng.synchronize()
    d_dw = torch.empty_like(d_rk[128])
    eng.reserve(max(batch_sizes) * 128)

    # ---- the measurements: name -> (run, reset, output tensor, the blocks it must decrypt to per key size) ----
    jobs = {}
    rng = np.random.default_rng(0xC7A)
    enc_iv = client.encrypt_u128(IV)
    for n in batch_sizes:
        aligned = [(IV + i) & MASK128 for i in range(n)]
        fa = [((IV | 0xFA) + i) & MASK128 for i in range(n)]
        cols = np.stack([rng.permutation(256)[:n] for _ in range(16)], axis=1)
        apart = [int.from_bytes(bytes(int(v) for v in row), "big") for row in cols]
        d_state = to_dev(np.stack([client.encrypt_u128(v) for v in aligned]))
        d_ivs = to_dev(np.stack([enc_iv] * n))
        for bits in SIZES:
            rk = d_rk[bits]
            out = {v: torch.empty((n, 16, 8, p.big1), dtype=torch.int64, device="cuda") for v in VARIANTS}
            key = KEYS[bits]

            def enc(blocks, key=key):
                return block_bytes([aes_clear.aes_encrypt_block(key, b) for b in blocks])

            def ref_iter(rk=rk, bits=bits, st=out["reference_iteration"], n=n):
                eng.add_scalar(st, n, range(n))
                eng.aes_encrypt_bits(rk, bits, st, n)

            nothing = lambda: None  # noqa: E731
            jobs[("ctr_aligned", n, bits)] = (lambda rk=rk, bits=bits, o=out["ctr_aligned"], n=n: eng.aes_ctr_bits(rk, bits, IV, 0, None, n, o),
                                              nothing, out["ctr_aligned"], enc(aligned), aligned)
            jobs[("ctr_fa", n, bits)] = (lambda rk=rk, bits=bits, o=out["ctr_fa"], n=n: eng.aes_ctr_bits(rk, bits, IV | 0xFA, 0, None, n, o),
                                         nothing, out["ctr_fa"], enc(fa), fa)
            jobs[("public_no_sharing", n, bits)] = (lambda rk=rk, bits=bits, o=out["public_no_sharing"], b=apart: eng.aes_encrypt_public_bits(rk, bits, b, o),
                                                    nothing, out["public_no_sharing"], enc(apart), apart)
            jobs[("aes_encrypt", n, bits)] = (lambda rk=rk, bits=bits, o=out["aes_encrypt"], n=n: eng.aes_encrypt_bits(rk, bits, o, n),
                                              lambda o=out["aes_encrypt"], s=d_state: o.copy_(s), out["aes_encrypt"], enc(aligned), None)
            jobs[("reference_iteration", n, bits)] = (ref_iter, lambda o=out["reference_iteration"], s=d_ivs: o.copy_(s),
                                                      out["reference_iteration"], enc(aligned), None)
    jobs[("aes_decryption_round_keys", 0, 128)] = (lambda: eng.aes_decryption_round_keys(d_rk[128], d_dw), lambda: None, d_dw, None, None)

    # ---- one timed loop, every job once per step ----
    times = measure.wall(eng, {k: j[:2] for k, j in jobs.items()}, args.warmup, args.steps,
                         on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    # ---- verify every block of every output, then one profiled call each ----
    all_ok = True
    rows = {}
    for k, (run, reset, out, want, public_blocks) in jobs.items():
        name, n, bits = k
        if want is None:                                             # the round-key conversion
            row = measure.row(times[k])
            ok = bool(np.array_equal(client.decrypt_bytes(host(out)),
                                     np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(KEYS[128])), dtype=np.uint8)))
            row["verified"] = ok
            all_ok = all_ok and ok
        else:
            row = measure.row(times[k], n)
            got = client.decrypt_bytes(host(out))
            wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
            all_ok = all_ok and not wrong
            row.update({"blocks_verified": n - len(wrong), "wrong_blocks": wrong})
            plan = _native.aes_public_plan(public_blocks, bits) if public_blocks is not None else [16 * n] * NR[bits]
            row["bit_cbs"] = 8 * sum(plan) + (143 * n if name == "reference_iteration" else 0)     # add_scalar: 143 bit-CBS per block
            row["byte_wopbs_rounds_1_2"] = plan[:2]
        prof = measure.profiled(eng, run, reset)
        row["stages_ms"] = measure.stage_ms(prof)
        row["stages_units"] = {s: v["units"] for s, v in prof.items()}
        rows.setdefault(name, {}).setdefault(str(n), {})[str(bits)] = row
        progress(TOOL, "%s, %d blocks, AES-%d: %.1f ms" % (name, n, bits, row["ms_median"]))

    check = None
    if 128 in batch_sizes and 32 in batch_sizes:
        T = lambda name, n: rows[name][str(n)]["128"]["ms_median"]  # noqa: E731
        proxy = {"aes_encrypt_128_blocks_ms": T("aes_encrypt", 128), "aes_encrypt_32_blocks_ms": T("aes_encrypt", 32),
                 "aes_decryption_round_keys_ms": T("aes_decryption_round_keys", 0)}
        pred = 0.8 * T("aes_encrypt", 128) + 0.1 * T("aes_encrypt", 32) + 0.5 * T("aes_decryption_round_keys", 0)
        check = {"proxies": proxy, **measure.check(T("ctr_aligned", 128), pred, 1.03),
                 "no_sharing_ms": T("public_no_sharing", 128), "no_sharing_ratio_to_aes_encrypt": round(T("public_no_sharing", 128) / T("aes_encrypt", 128), 4),
                 "no_sharing_within_bound": bool(T("public_no_sharing", 128) <= 1.03 * T("aes_encrypt", 128)),
                 "share_of_aes_encrypt": round(T("ctr_aligned", 128) / T("aes_encrypt", 128), 4),
                 "share_of_reference_iteration": round(T("ctr_aligned", 128) / T("reference_iteration", 128), 4)}
        progress(TOOL, "aes_ctr 128 aligned: %.1f ms, predicted %.1f ms, ratio %.4f; no sharing / aes_encrypt %.4f" % (
            check["measured_ms"], pred, check["ratio"], check["no_sharing_ratio_to_aes_encrypt"]))

    line = {**measure.header(TOOL, args), "all_verified": all_ok, "check": check, "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps; every variant of every size "
                    "runs once in every step of one loop; rows are variants[name][blocks][key bits]; stages_ms / stages_units "
                    "(fheaes_profile_read: bits for the five WoPBS stages, blocks for the linear layers) from one further profiled call; "
                    "bit_cbs = bit circuit bootstraps of the call (8 x fheaes_aes_public_plan; 128 n per round for aes_encrypt; add_scalar 143 n)"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, check is None or (check["within_bound"] and check["no_sharing_within_bound"]))


if __name__ == "__main__":
    sys.exit(main())
