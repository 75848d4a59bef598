"""Packing ciphertext bits into GLWEs (fheaes_pack_bits / fheaes_unpack_bits) against entry points the engine had before, at PARAM_OPT on
one GPU, one process, resident tensors: 16,384 bits, the output of a 128-block aes_ctr.

Two bounds, both against existing entry points measured in the same process, never against the new code:

  pack     T(pack, 16,384 bits) <= 0.30 T(fheaes_pfpks_batch, 16,384 bits)
           one of the k+1 = 5 key blocks is 0.20 of K3's matrix product; the digit planes do not shrink with the number of blocks; the
           fold reads 335 MB once.
  unpack   T(unpack, 16,384 bits) <= 2 x (its bytes: 20,480 read per GLWE, 16,392 written per bit) / (bytes per second of the linear
           stage of a 128-block aes_encrypt: fheaes_profile_read(FHEAES_STAGE_LINEAR) against the 13.2 GB its layers move)
           the factor 2: extraction reads with a reversed stride.

pack, unpack and fheaes_pfpks_batch run on a torch stream handed to the engine (fheaes_set_stream), each timed by a pair of device events
around --reps back-to-back calls; every step of ONE loop times all three, so a drift of the clocks meets them alike; the median of
--steps steps after --warmup.  Reported without a bound: the wall time of a FHEAES_HOST aes_ctr of 128 blocks (268.6 MB come back over
PCIe), of a FHEAES_DEVICE aes_ctr + pack + a host copy of the 655,360 packed bytes, and the two sizes.  The packed words are decrypted
with the client key and compared with the AES-CTR plaintext, the unpacked words with the LWE words numpy extracts: a wrong result makes
the tool exit 1, a missed bound exit 2.

    python tools/pack_bits.py [--steps 5] [--warmup 1] [--reps 10] [--out profiles/pack_bits.json]
"""
from __future__ import annotations

import statistics
import sys
import time

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, aes_clear

KEY = bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c")           # SP 800-38A F.1.1
IV = 0x00112233445566778899AABBCCDDEE00
N_BLOCKS = 128
TOOL = "pack_bits"


def main() -> int:
    args = measure.arg_parser(reps=10).parse_args()
    p = PARAM_OPT
    m = N_BLOCKS * 128
    gw, glwes = (p.k + 1) * p.N, m // p.N

    client, eng = measure.session(0xAE50001, IV, int.from_bytes(KEY, "big"))
    eng.reserve(m)

    rng = np.random.default_rng(0x9AC4)
    data = [int.from_bytes(rng.bytes(16), "big") for _ in range(N_BLOCKS)]
    plain = b"".join((k ^ d).to_bytes(16, "big") for k, d in zip(aes_clear.ctr_keystream(KEY, IV, 0, N_BLOCKS), data))

    d_rk = torch.empty((11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    eng.aes_key_expansion_bits(to_dev(client.encrypt_aes_key(KEY)), 128, d_rk)
    eng.synchronize()
    d_ct = torch.empty((N_BLOCKS, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_packed = torch.empty((glwes, gw), dtype=torch.int64, device="cuda")
    d_back = torch.empty((m, p.big1), dtype=torch.int64, device="cuda")
    d_ggsw = torch.empty((m, p.k + 1, gw), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    # ---- reported, no bound: the two ways out of the engine, wall clock ----
    h_rk = host(d_rk)
    h_ct = np.empty((N_BLOCKS, 16, 8, p.big1), dtype=np.uint64)
    wall = {"host_aes_ctr": [], "device_aes_ctr_pack_copy": []}
    h_packed = None
    for i in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        eng.aes_ctr_bits(h_rk, 128, IV, 0, data, N_BLOCKS, h_ct)
        t1 = time.perf_counter()
        eng.aes_ctr_bits(d_rk, 128, IV, 0, data, N_BLOCKS, d_ct)
        eng.pack_bits(d_ct, m, d_packed)
        eng.synchronize()
        h_packed = host(d_packed)
        t2 = time.perf_counter()
        if i >= args.warmup:
            wall["host_aes_ctr"].append(t1 - t0)
            wall["device_aes_ctr_pack_copy"].append(t2 - t1)
        progress(TOOL, "way out, step %d of %d: host %.3f s, device + pack + copy %.3f s" % (i + 1, args.warmup + args.steps, t1 - t0, t2 - t1))

    # ---- verification ----
    ok_pack = client.decrypt_packed_bytes(h_packed, 16 * N_BLOCKS).tobytes() == plain
    ok_host = client.decrypt_bytes(h_ct).tobytes() == plain and bool(np.array_equal(h_ct, host(d_ct)))
    eng.unpack_bits(d_packed, m, d_back)
    eng.synchronize()
    back = host(d_back)
    glwe = h_packed.reshape(glwes, p.k + 1, p.N)
    c = np.arange(p.N)
    ok_unpack = client.decrypt_bytes(back.reshape(N_BLOCKS, 16, 8, p.big1)).tobytes() == plain
    with np.errstate(over="ignore"):
        for t in rng.integers(0, m, 64):                           # 64 bits word for word against numpy's extraction
            g, i = divmod(int(t), p.N)
            a = glwe[g, :p.k][:, (i - c) % p.N]
            a[:, i + 1:] = np.uint64(0) - a[:, i + 1:]
            ok_unpack = ok_unpack and bool(np.array_equal(back[t, :p.big], a.reshape(-1))) and back[t, p.big] == glwe[g, p.k, i]
    progress(TOOL, "verified: packed %s, host aes_ctr %s, unpacked %s" % (ok_pack, ok_host, ok_unpack))

    # ---- the linear stage's rate: one profiled 128-block aes_encrypt ----
    d_state = d_ct.clone()
    torch.cuda.synchronize()
    prof = measure.profiled(eng, lambda: eng.aes_encrypt_bits(d_rk, 128, d_state, N_BLOCKS))
    state_bytes = N_BLOCKS * 16 * 8 * p.big1 * 8
    # initial AddRoundKey (read + write), nine MixColumns layers (four terms read + one write; the round key stays in cache), the last
    # round's ShiftRows + AddRoundKey (one term read + one write)
    linear_bytes = (2 + 9 * 5 + 2) * state_bytes
    linear_ms = prof["linear"]["ms"]
    linear_rate = linear_bytes / (linear_ms * 1e-3)
    unpack_bytes = glwes * gw * 8 + m * p.big1 * 8
    unpack_bound_ms = 2 * unpack_bytes / linear_rate * 1e3
    del d_state

    # ---- the bounded measurements: device events on a stream the engine shares with torch ----
    jobs = {"pack": lambda: eng.pack_bits(d_ct, m, d_packed),
            "unpack": lambda: eng.unpack_bits(d_packed, m, d_back),
            "pfpks_batch": lambda: eng.pfpks_batch(d_ct, d_ggsw, m)}
    times = measure.events(eng, jobs, args.warmup, args.steps, args.reps, on_step=lambda i, of, last: progress(
        TOOL, "step %d of %d: %s" % (i, of, ", ".join("%s %.3f ms" % kv for kv in last.items()))))
    ok_after = bool(np.array_equal(host(d_packed), h_packed)) and bool(np.array_equal(host(d_back), back))

    # per-stage split of one profiled pack and one profiled unpack
    prof_pack = measure.profiled(eng, jobs["pack"])
    prof_unpack = measure.profiled(eng, jobs["unpack"])
    launched = lambda prof: measure.stage_ms({s: v for s, v in prof.items() if v["launches"]}, 4)  # noqa: E731

    med = {k: statistics.median(v) for k, v in times.items()}
    pack_ratio = med["pack"] / med["pfpks_batch"]
    unpack_ratio = med["unpack"] / unpack_bound_ms * 2            # against ONE times the bytes at the linear stage's rate
    check = {"pack_ms": round(med["pack"], 4), "pfpks_batch_ms": round(med["pfpks_batch"], 4), "pack_ratio": round(pack_ratio, 4), "pack_bound": 0.30,
             "pack_within_bound": bool(pack_ratio <= 0.30),
             "unpack_ms": round(med["unpack"], 4), "unpack_bytes": unpack_bytes, "linear_stage_ms": round(linear_ms, 3), "linear_stage_bytes": linear_bytes,
             "linear_stage_tb_per_s": round(linear_rate / 1e12, 3), "unpack_tb_per_s": round(unpack_bytes / (med["unpack"] * 1e-3) / 1e12, 3),
             "unpack_ratio": round(unpack_ratio, 4), "unpack_bound": 2.0, "unpack_within_bound": bool(unpack_ratio <= 2.0)}
    all_ok = ok_pack and ok_host and ok_unpack and ok_after
    line = {**measure.header(TOOL, args), "bits": m, "reps": args.reps, "all_verified": all_ok, "check": check,
            "ms_all": {k: [round(t, 4) for t in v] for k, v in times.items()},
            "pack_stages_ms": launched(prof_pack), "unpack_stages_ms": launched(prof_unpack),
            "fold_tb_per_s": round(m * gw * 8 / (prof_pack["linear"]["ms"] * 1e-3) / 1e12, 3),
            "way_out": {"lwe_bytes": state_bytes, "packed_bytes": glwes * gw * 8, "size_ratio": round(state_bytes / (glwes * gw * 8), 1),
                        "host_aes_ctr_s": round(statistics.median(wall["host_aes_ctr"]), 4),
                        "device_aes_ctr_pack_copy_s": round(statistics.median(wall["device_aes_ctr_pack_copy"]), 4),
                        "host_aes_ctr_s_all": [round(t, 4) for t in wall["host_aes_ctr"]],
                        "device_aes_ctr_pack_copy_s_all": [round(t, 4) for t in wall["device_aes_ctr_pack_copy"]]},
            "note": "pack / unpack / pfpks_batch: device events around `reps` back-to-back calls on resident tensors, per call, median of the timed "
                    "steps, all three in every step of one loop; unpack_ratio = unpack time over the time of its bytes at the linear stage's rate "
                    "(bound 2); pack_stages_ms / unpack_stages_ms: fheaes_profile_read of one further profiled call (fold: its memset and "
                    "pack_fold_kernel under `linear`); way_out: wall clock, a host aes_ctr of 128 blocks against device aes_ctr + pack + "
                    "a host copy of the packed bytes"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, check["pack_within_bound"] and check["unpack_within_bound"])


if __name__ == "__main__":
    sys.exit(main())
