"""The two homomorphic AES decryptions side by side at PARAM_OPT on one GPU, on resident device tensors:

  aes_decrypt             the reference's schedule (server.rs:67-105): INV_SBOX WoPBS + 4-LUT InvMixColumns WoPBS per round,
                          19 x 128 = 2,432 bit circuit bootstraps per block;
  aes_decrypt_equivalent  the equivalent inverse cipher (FIPS-197 section 5.3.5): one WoPBS per round with the composed
                          {9, 11, 13, 14} * InvS tables, 10 x 128 = 1,280 per block, after a once-per-key round-key conversion
                          (aes_decryption_round_keys: 2 x 1,152 bit circuit bootstraps).

For each batch size: warm-up, then the median of --steps timed calls (wall clock around the call and a synchronize), every block of
both paths decrypted with the client key and compared with FIPS-197 arithmetic, and one further call with the per-stage profile on
(fheaes_profile_read; HIP events around every launch, so kept out of the timed calls).  Prints one JSON line (--out: also written there).

    python tools/decrypt_paths.py [--blocks 32,128] [--steps 5] [--warmup 1] [--out FILE]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, to_dev
from tfhe_aes_amd import PARAM_OPT, aes_clear

KEY = 0x2B7E151628AED2A6ABF7158809CF4F3C
IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
MASK128 = (1 << 128) - 1


def main() -> int:
    args = measure.arg_parser(blocks="32,128").parse_args()
    sizes = [int(x) for x in args.blocks.split(",")]
    p = PARAM_OPT

    client, eng = measure.session(0xAE50001, IV, KEY)
    d_rk = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ek = to_dev(client.encrypt_u128(KEY))
    eng.aes_key_expansion(d_ek, d_rk)
    eng.synchronize()
    rk_ok = np.array_equal(client.decrypt_bytes(host(d_rk)), np.array(aes_clear.expand_key(KEY), dtype=np.uint8))

    # ---- the round-key conversion, once per AES key ----
    d_dw = torch.empty_like(d_rk)

    def convert():
        eng.aes_decryption_round_keys(d_rk, d_dw)

    conv_s = measure.wall(eng, {"conversion": (convert, lambda: None)}, args.warmup, args.steps)["conversion"]
    dw_ok = np.array_equal(client.decrypt_bytes(host(d_dw)),
                           np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(KEY)), dtype=np.uint8))
    conversion = {**measure.row(conv_s), "bit_cbs": 2 * 9 * 16 * 8, "verified_vs_fips197": dw_ok,
                  "stages_ms": measure.stage_ms(measure.profiled(eng, convert))}

    results = {}
    all_ok = rk_ok and dw_ok
    for n in sizes:
        pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
        want = measure.block_bytes(pts)
        d_in = to_dev(np.stack([client.encrypt_u128(aes_clear.aes128_encrypt_block(KEY, v)) for v in pts]))
        eng.reserve(n * 128)
        row = {}
        words = {}
        for name, fn, keys_d, bit_cbs in (("aes_decrypt", eng.aes_decrypt, d_rk, 19 * 128),
                                           ("aes_decrypt_equivalent", eng.aes_decrypt_equivalent, d_dw, 10 * 128)):
            st = torch.empty_like(d_in)

            def run(fn=fn, keys_d=keys_d, st=st):
                fn(keys_d, st, n)

            def reset(st=st):
                st.copy_(d_in)

            ts = measure.wall(eng, {name: (run, reset)}, args.warmup, args.steps)[name]      # a loop per path, not alternating
            got = client.decrypt_bytes(host(st))
            wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
            words[name] = got
            row[name] = {**measure.row(ts, n), "bit_cbs_per_block": bit_cbs, "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                         "stages_ms": measure.stage_ms(measure.profiled(eng, run, reset))}
            all_ok = all_ok and not wrong
        row["same_plaintexts"] = bool(np.array_equal(words["aes_decrypt"], words["aes_decrypt_equivalent"]))
        row["speedup"] = round(row["aes_decrypt"]["ms_median"] / row["aes_decrypt_equivalent"]["ms_median"], 3)
        all_ok = all_ok and row["same_plaintexts"]
        results[str(n)] = row
        del d_in

    line = {**measure.header("decrypt_paths", args), "round_keys_verified": rk_ok, "all_verified": all_ok,
            "conversion": conversion, "blocks": results,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps; stages_ms from one further "
                    "profiled call (HIP events around every launch); speedup = aes_decrypt ms / aes_decrypt_equivalent ms"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok)


if __name__ == "__main__":
    sys.exit(main())
