"""The two wire formats (include/fheaes.h: seeded input ciphertexts, packed words switched to 16 bits) against entry points the engine had
before, at PARAM_OPT on one GPU, one process, resident tensors: 16,384 bits = 128 AES-128 keys in, 128 blocks out.

Three ratios, each against an existing entry point measured in the same loop, never against the new code:

  expand        T(fheaes_expand_lwe_seeded, 16,384 bits) / T(fheaes_unpack_bits, 16,384 bits)      accepted up to 6
                both write the same 268.6 MB; by instruction count the ChaCha20 work is one to two times the store time.
  pack_mod      T(fheaes_pack_bits_mod, width 16) / T(fheaes_pack_bits)                            bound 1.05
                one more launch over 655 KB against 3.7 ms; the margin is the run-to-run spread of one binary.
  unpack_mod    T(fheaes_unpack_bits_mod, width 16) / T(fheaes_unpack_bits)                        bound 1.5
                field extraction adds shifts to a store-bound kernel; the reads shrink.

All five calls run on a torch stream handed to the engine (fheaes_set_stream), each timed by a pair of device events around --reps
back-to-back calls; every step of ONE loop times all five, so a drift of the clocks meets them alike; the median of --steps steps after
--warmup.  Reported without a bound: the wall time of one FHEAES_HOST call on the 128 expanded keys (fheaes_pack_bits: the engine uploads
268.6 MB, packs, returns 655 KB) against their 131 KB of bodies copied to the device, expanded there and packed by the same entry point
on resident words, and the sizes.  The expanded words are compared with SeededCiphertexts.expand() and
decrypted, the 16-bit packing with the rounding rule applied to fheaes_pack_bits' words, the extraction with fheaes_unpack_bits of the
read-back words: a wrong result makes the tool exit 1, a missed bound exit 2.

    python tools/wire_formats.py [--steps 5] [--warmup 1] [--reps 10] [--out profiles/wire_formats.json]
"""
from __future__ import annotations

import statistics
import sys
import time

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT
from tfhe_aes_amd.client import read_back_packed

N_KEYS = 128
WIDTH = 16
BOUNDS = {"expand": 6.0, "pack_mod": 1.05, "unpack_mod": 1.5}
TOOL = "wire_formats"


def main() -> int:
    args = measure.arg_parser(reps=10).parse_args()
    p = PARAM_OPT
    m = N_KEYS * 128
    gw, glwes = (p.k + 1) * p.N, m // p.N
    gw_mod = gw * WIDTH // 64

    client, eng = measure.session(0xAE50001)
    eng.reserve(m)

    rng = np.random.default_rng(0x31BE)
    aes_keys = rng.integers(0, 256, (N_KEYS, 16)).astype(np.uint8)
    seeded = client.encrypt_bytes_seeded(aes_keys.reshape(-1))               # bodies [2048][8]: 128 AES-128 keys
    t0 = time.perf_counter()
    full = seeded.expand()
    progress(TOOL, "numpy expansion of %d ciphertexts: %.1f s" % (m, time.perf_counter() - t0))

    d_bodies = to_dev(seeded.bodies)
    d_lwe = torch.empty((m, p.big1), dtype=torch.int64, device="cuda")
    d_back = torch.empty((m, p.big1), dtype=torch.int64, device="cuda")
    d_back_mod = torch.empty((m, p.big1), dtype=torch.int64, device="cuda")
    d_p64 = torch.empty((glwes, gw), dtype=torch.int64, device="cuda")
    d_p16 = torch.empty((glwes, gw_mod), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    # ---- reported, no bound: the two ways in, wall clock, through the engine ----
    # expanded: one FHEAES_HOST call on the expanded ciphertexts (fheaes_pack_bits: the engine stages the 268.6 MB to the device, packs,
    # copies 655 KB back); seeded: the bodies to the device, fheaes_expand_lwe_seeded, the same pack on resident words, 655 KB back.
    # Both end with the same packed words on the host; the device's share of either is the `pack` / `expand` time measured below.
    wall = {"host_call_on_expanded": [], "seeded_expand_then_device_call": []}
    full_flat = np.ascontiguousarray(full.reshape(m, p.big1))
    p64_host = np.zeros((glwes, gw), dtype=np.uint64)
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        eng.pack_bits(full_flat, m, p64_host)                                # FHEAES_HOST: returns when the words are in p64_host
        t1 = time.perf_counter()
        d_b = to_dev(seeded.bodies)
        eng.expand_lwe_seeded(seeded.mask_key, seeded.first_index, d_b, m, d_lwe)
        eng.pack_bits(d_lwe, m, d_p64)
        eng.synchronize()
        p64_seeded = host(d_p64)
        t2 = time.perf_counter()
        if i >= args.warmup:
            wall["host_call_on_expanded"].append(t1 - t0)
            wall["seeded_expand_then_device_call"].append(t2 - t1)
        progress(TOOL, "way in, step %d of %d: host call on the expanded words %.4f s, seeded %.4f s" % (i + 1, args.warmup + args.steps, t1 - t0, t2 - t1))
    ok_expand = bool(np.array_equal(host(d_lwe), full_flat)) and bool(np.array_equal(p64_host, p64_seeded)) and \
        client.decrypt_bytes(host(d_lwe).reshape(-1, 8, p.big1)).tobytes() == aes_keys.tobytes()
    del full, full_flat

    # ---- verification of the switched packing ----
    eng.pack_bits(d_lwe, m, d_p64)
    eng.pack_bits_mod(d_lwe, m, WIDTH, d_p16)
    eng.unpack_bits_mod(d_p16, m, WIDTH, d_back_mod)
    eng.synchronize()
    p64, p16 = host(d_p64), host(d_p16)
    with np.errstate(over="ignore"):
        rounded = ((p64 + np.uint64(1 << (63 - WIDTH))) >> np.uint64(64 - WIDTH)) << np.uint64(64 - WIDTH)
    ok_pack = bool(np.array_equal(read_back_packed(p16, p, WIDTH), rounded)) and \
        client.decrypt_packed_bytes(p16, N_KEYS * 16, width=WIDTH).tobytes() == aes_keys.tobytes()
    eng.unpack_bits(to_dev(rounded), m, d_back)
    eng.synchronize()
    ok_unpack = bool(torch.equal(d_back, d_back_mod))
    _, ph64 = client.decrypt_packed(p64, m, return_phase=True)
    _, ph16 = client.decrypt_packed(p16, m, return_phase=True, width=WIDTH)
    err = (ph16 - ph64).astype(np.int64).astype(np.float64)
    h = int(client.glwe_sk.sum())
    formula_std, bound = ((1 + h) / 12.0) ** 0.5 * 2.0 ** (64 - WIDTH), (1 + h) * 2.0 ** (63 - WIDTH)
    ok_noise = bool(np.abs(err).max() <= bound)
    progress(TOOL, "verified: expansion %s, packing at %d bits %s, extraction %s, hard noise bound %s" % (ok_expand, WIDTH, ok_pack, ok_unpack, ok_noise))

    # ---- the bounded measurements: device events on a stream the engine shares with torch ----
    jobs = {"unpack": lambda: eng.unpack_bits(d_p64, m, d_back),
            "expand": lambda: eng.expand_lwe_seeded(seeded.mask_key, seeded.first_index, d_bodies, m, d_lwe),
            "unpack_mod": lambda: eng.unpack_bits_mod(d_p16, m, WIDTH, d_back_mod),
            "pack": lambda: eng.pack_bits(d_lwe, m, d_p64),
            "pack_mod": lambda: eng.pack_bits_mod(d_lwe, m, WIDTH, d_p16)}
    times = measure.events(eng, jobs, args.warmup, args.steps, args.reps, on_step=lambda i, of, last: progress(
        TOOL, "step %d of %d: %s" % (i, of, ", ".join("%s %.4f ms" % kv for kv in last.items()))))
    ok_after = bool(np.array_equal(host(d_p16), p16)) and bool(np.array_equal(host(d_p64), p64))

    med = {k: statistics.median(v) for k, v in times.items()}
    ratios = {"expand": med["expand"] / med["unpack"], "pack_mod": med["pack_mod"] / med["pack"], "unpack_mod": med["unpack_mod"] / med["unpack"]}
    lwe_bytes = m * p.big1 * 8
    check = {k + "_ratio": round(v, 4) for k, v in ratios.items()}
    check.update({k + "_bound": BOUNDS[k] for k in ratios})
    check.update({k + "_within_bound": bool(ratios[k] <= BOUNDS[k]) for k in ratios})
    all_ok = ok_expand and ok_pack and ok_unpack and ok_noise and ok_after
    line = {**measure.header(TOOL, args), "bits": m, "width": WIDTH, "reps": args.reps, "all_verified": all_ok, "check": check,
            "ms": {k: round(v, 4) for k, v in med.items()}, "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
            "expand_tb_per_s": round(lwe_bytes / (med["expand"] * 1e-3) / 1e12, 3), "unpack_tb_per_s": round(lwe_bytes / (med["unpack"] * 1e-3) / 1e12, 3),
            "noise": {"h": h, "std_over_formula": round(float(err.std() / formula_std), 4), "max_over_hard_bound": round(float(np.abs(err).max() / bound), 4),
                      "std_log2": round(float(np.log2(err.std())), 2), "max_log2": round(float(np.log2(np.abs(err).max())), 2)},
            "way_in": {"expanded_bytes": lwe_bytes, "seeded_bytes": seeded.nbytes, "size_ratio": round(lwe_bytes / seeded.nbytes, 1),
                       "host_call_on_expanded_s": round(statistics.median(wall["host_call_on_expanded"]), 5),
                       "seeded_expand_then_device_call_s": round(statistics.median(wall["seeded_expand_then_device_call"]), 5),
                       "host_call_on_expanded_s_all": [round(t, 5) for t in wall["host_call_on_expanded"]],
                       "seeded_expand_then_device_call_s_all": [round(t, 5) for t in wall["seeded_expand_then_device_call"]]},
            "way_out": {"packed_bytes": glwes * gw * 8, "packed_mod_bytes": glwes * gw_mod * 8, "lwe_bytes": lwe_bytes},
            "sizes_65536_aes128_keys": {"expanded_bytes": 65536 * 128 * p.big1 * 8, "seeded_body_bytes": 65536 * 128 * 8},
            "note": "unpack / expand / unpack_mod / pack / pack_mod: device events around `reps` back-to-back calls on resident tensors, per call, "
                    "median of the timed steps, all five in every step of one loop; ratios against the existing entry point of the same bytes "
                    "(expand, unpack_mod: fheaes_unpack_bits; pack_mod: fheaes_pack_bits); way_in: wall clock of one FHEAES_HOST fheaes_pack_bits on the "
                    "expanded ciphertexts of 128 AES-128 keys (the engine's own upload of 268.6 MB, the pack, 655 KB back) against their "
                    "bodies copied to the device + fheaes_expand_lwe_seeded + the same pack on resident words + 655 KB back; noise: the error the "
                    "16-bit switch adds to the 16,384 phases against (1 + h) 2^(2(64-w)) / 12 and (1 + h) 2^(63-w)"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, all(check[k + "_within_bound"] for k in ratios))


if __name__ == "__main__":
    sys.exit(main())
