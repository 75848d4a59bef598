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

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tfhe_aes_amd import PARAM_OPT, _build, _native, aes_clear  # noqa: E402
from tfhe_aes_amd.client import Client  # noqa: E402

KEY = 0x2B7E151628AED2A6ABF7158809CF4F3C
IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
MASK128 = (1 << 128) - 1


def to_dev(a: np.ndarray) -> torch.Tensor:
    d = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


def host(d: torch.Tensor) -> np.ndarray:
    return d.cpu().numpy().view(np.uint64)


def stage_ms(eng: _native.Engine, run) -> dict:
    """one call of `run` with the per-stage profile on: {stage: ms}"""
    eng.profile_enable(True)
    eng.profile_reset()
    run()
    prof = eng.profile_read()
    eng.profile_enable(False)
    return {k: round(v["ms"], 3) for k, v in prof.items()}


def timed(eng: _native.Engine, run, reset, warmup: int, steps: int) -> list[float]:
    out = []
    for i in range(warmup + steps):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        eng.synchronize()
        if i >= warmup:
            out.append(time.perf_counter() - t0)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="32,128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(x) for x in args.blocks.split(",")]
    p = PARAM_OPT

    client = Client(1, IV, KEY, params=p, seed=0xAE50001)
    keys = client.server_keys()
    eng = _native.Engine(p, device=0)
    eng.upload_keys(keys.ksk, keys.bsk, keys.pfpksk)
    del keys
    d_rk = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ek = to_dev(client.encrypt_u128(KEY))
    eng.aes_key_expansion(d_ek, d_rk)
    eng.synchronize()
    rk_ok = np.array_equal(client.decrypt_bytes(host(d_rk)), np.array(aes_clear.expand_key(KEY), dtype=np.uint8))

    # ---- the round-key conversion, once per AES key ----
    d_dw = torch.empty_like(d_rk)
    conv_s = timed(eng, lambda: eng.aes_decryption_round_keys(d_rk, d_dw), lambda: None, args.warmup, args.steps)
    dw_ok = np.array_equal(client.decrypt_bytes(host(d_dw)),
                           np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(KEY)), dtype=np.uint8))
    conversion = {"ms_median": round(1000 * statistics.median(conv_s), 3), "ms_all": [round(1000 * t, 3) for t in conv_s],
                  "bit_cbs": 2 * 9 * 16 * 8, "verified_vs_fips197": dw_ok,
                  "stages_ms": stage_ms(eng, lambda: eng.aes_decryption_round_keys(d_rk, d_dw))}

    results = {}
    all_ok = rk_ok and dw_ok
    for n in sizes:
        pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
        want = np.array([[(v >> (8 * (15 - b))) & 0xFF for b in range(16)] for v in pts], dtype=np.uint8)
        d_in = to_dev(np.stack([client.encrypt_u128(aes_clear.aes128_encrypt_block(KEY, v)) for v in pts]))
        eng.reserve(n * 128)
        row = {}
        words = {}
        for name, fn, keys_d, bit_cbs in (("aes_decrypt", eng.aes_decrypt, d_rk, 19 * 128),
                                           ("aes_decrypt_equivalent", eng.aes_decrypt_equivalent, d_dw, 10 * 128)):
            st = torch.empty_like(d_in)

            def run(fn=fn, keys_d=keys_d, st=st):
                fn(keys_d, st, n)

            ts = timed(eng, run, lambda st=st: st.copy_(d_in), args.warmup, args.steps)
            out = host(st)
            got = client.decrypt_bytes(out)
            wrong = [i for i in range(n) if not np.array_equal(got[i], want[i])]
            words[name] = got
            st.copy_(d_in)
            torch.cuda.synchronize()
            med = statistics.median(ts)
            row[name] = {"blocks_per_s": round(n / med, 2), "ms_median": round(1000 * med, 3), "ms_all": [round(1000 * t, 3) for t in ts],
                         "bit_cbs_per_block": bit_cbs, "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                         "stages_ms": stage_ms(eng, run)}
            all_ok = all_ok and not wrong
        row["same_plaintexts"] = bool(np.array_equal(words["aes_decrypt"], words["aes_decrypt_equivalent"]))
        row["speedup"] = round(row["aes_decrypt"]["ms_median"] / row["aes_decrypt_equivalent"]["ms_median"], 3)
        all_ok = all_ok and row["same_plaintexts"]
        results[str(n)] = row
        del d_in

    line = {"tool": "decrypt_paths", "params": p.name, "version": _native.load_library().fheaes_version().decode(),
            "engine_src_sha256": _build.engine_source_hash(), "device": torch.cuda.get_device_name(0),
            "steps": args.steps, "warmup": args.warmup, "round_keys_verified": rk_ok, "all_verified": all_ok,
            "conversion": conversion, "blocks": results,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps; stages_ms from one further "
                    "profiled call (HIP events around every launch); speedup = aes_decrypt ms / aes_decrypt_equivalent ms"}
    text = json.dumps(line)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    eng.close()
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
