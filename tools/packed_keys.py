"""Packed round keys against the LWE form the engine had before, at PARAM_OPT, AES-128, one GPU, one process, resident tensors.  Every
quantity runs once in every step of ONE timed loop, so the two forms of a call alternate and a drift of the clocks meets them alike; the
median of --steps steps after --warmup.  Every output block is decrypted with the client key and compared with aes_clear: a wrong one
makes the tool exit 1.  The yardstick of every check is an entry point that existed before, timed in the same loop:

  keyed cipher   T(aes_encrypt_keyed, 128 blocks as 8 keys x 16, from a packed store) against the same call from LWE keys   [<= 1.03 x]
                 with the linear stage's milliseconds of both from one further profiled call each                           [reported]
  streams        T(aes_ctr_streams, 8 keys x 16 consecutive counters, from a packed store) against the call from LWE keys   [<= 1.03 x]
  packing        T(pack_round_keys, 32 keys: 45,056 bits) against T(aes_key_expansion_many) of the same 32 keys              [<= 0.05 x]
  memory         bytes per key in both forms, and the largest store of either form that the device's free memory would hold  [reported]

The bounds were written down before anything was timed: 1.03 is the project's bound for the keyed calls (tools/multi_key.py; the linear
layers are 0.15 % of such a call, so anything above it means the key read is wrong, not slow), and packing should cost about 1.2 % of
the expansion (45,056 bits at 3.72 ms per 16,384 against 838 ms); 5 % leaves a factor of four for the per-key fold and small chunks.
`checks` records yardstick, measurement, ratio and whether each bound holds; a missed bound makes the tool exit 2.

    python tools/packed_keys.py [--steps 5] [--warmup 1] [--commit ID] [--out profiles/packed_keys.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import block_bytes, check, host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, aes_clear
from tfhe_aes_amd.client import Client
from tfhe_aes_amd.server import Server

BASE = 0x00112233445566778899AABBCCDDEE00
N_KEYS = 32                     # keys expanded and packed
BOUND = 1.03
PACK_BOUND = 0.05
TOOL = "packed_keys"


def main() -> int:
    ap = measure.arg_parser()
    ap.add_argument("--commit", default=None, help="what the measured tree is (default: git rev-parse HEAD + working tree)")
    args = ap.parse_args()
    p = PARAM_OPT
    rng = np.random.default_rng(0x3A17)
    aes_keys = [rng.bytes(16) for _ in range(N_KEYS)]

    client = Client(1, BASE, int.from_bytes(aes_keys[0], "big"), params=p, seed=0xAE50003)
    srv = Server(client.server_keys(), device=0)            # not measure.session: everything is timed through the Server
    eng = srv.engine
    eng.reserve(128 * 128)
    empty = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")  # noqa: E731

    d_ek = to_dev(np.stack([client.encrypt_aes_key(k) for k in aes_keys]))                   # [32][16][8][kN+1]
    d_rk = srv.aes_key_expansion_many(d_ek)                                                  # [32][11][16][8][kN+1]
    prk = srv.pack_round_keys(d_rk)                                                          # [32][3][(k+1)N]
    eng.synchronize()
    lwe_key_bytes, packed_key_bytes = d_rk[0].numel() * 8, prk.nbytes // N_KEYS
    rk8, prk8 = d_rk[:8], prk[:8]

    # ---- the jobs: name -> (run, reset, verify) ----
    jobs = {}
    nothing = lambda: None  # noqa: E731
    n_blocks, kob = 128, [b // 16 for b in range(128)]                                       # 8 keys x 16 blocks
    pts = [(BASE + 0x0101 * i) & ((1 << 128) - 1) for i in range(n_blocks)]
    want_enc = block_bytes([aes_clear.aes_encrypt_block(aes_keys[k], v) for k, v in zip(kob, pts)])
    d_state = to_dev(np.stack([client.encrypt_u128(v) for v in pts]))
    d_lwe, d_pk = torch.empty_like(d_state), torch.empty_like(d_state)
    jobs["aes_encrypt_keyed/8x16 lwe"] = (lambda: srv.aes_encrypt_keyed(rk8, kob, d_lwe), lambda: d_lwe.copy_(d_state),
                                          lambda: np.array_equal(client.decrypt_bytes(host(d_lwe)), want_enc))
    jobs["aes_encrypt_keyed/8x16 packed"] = (lambda: srv.aes_encrypt_keyed(prk8, kob, d_pk), lambda: d_pk.copy_(d_state),
                                             lambda: np.array_equal(client.decrypt_bytes(host(d_pk)), want_enc))

    streams = [(k, BASE, 0, 16, None) for k in range(8)]
    want_streams = block_bytes(aes_clear.ctr_streams(aes_keys, streams))
    d_str_lwe, d_str_pk = empty(128, 16, 8, p.big1), empty(128, 16, 8, p.big1)
    jobs["aes_ctr_streams/8x16 lwe"] = (lambda: srv.aes_ctr_streams(rk8, streams, out=d_str_lwe), nothing,
                                        lambda: np.array_equal(client.decrypt_bytes(host(d_str_lwe)), want_streams))
    jobs["aes_ctr_streams/8x16 packed"] = (lambda: srv.aes_ctr_streams(prk8, streams, out=d_str_pk), nothing,
                                           lambda: np.array_equal(client.decrypt_bytes(host(d_str_pk)), want_streams))

    rk_words = lambda k: np.array(aes_clear.expand_key(k), dtype=np.uint8)  # noqa: E731
    d_rk_again, d_packed_again = torch.empty_like(d_rk), torch.empty_like(prk.data)
    jobs["aes_key_expansion_many/%d" % N_KEYS] = (
        lambda: srv.aes_key_expansion_many(d_ek, out=d_rk_again), nothing,
        lambda: all(np.array_equal(client.decrypt_bytes(host(d_rk_again[i])), rk_words(aes_keys[i])) for i in range(N_KEYS)))
    # the packed keys are read by the client straight from the GLWEs: 1,408 bits a key
    jobs["pack_round_keys/%d" % N_KEYS] = (
        lambda: srv.pack_round_keys(d_rk, out=d_packed_again), nothing,
        lambda: all(np.array_equal(client.decrypt_packed_bytes(host(d_packed_again[i]), 11 * 16).reshape(11, 16), rk_words(aes_keys[i]))
                    for i in range(N_KEYS)))

    # ---- one timed loop, every job once per step ----
    times = measure.wall(eng, {k: j[:2] for k, j in jobs.items()}, args.warmup, args.steps,
                         on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    all_ok = True
    rows = {}
    for k, (run, reset, verify) in jobs.items():
        rows[k] = measure.row(times[k])
        rows[k]["verified"] = bool(verify())
        all_ok = all_ok and rows[k]["verified"]
        progress(TOOL, "%s: %.2f ms verified=%s" % (k, rows[k]["ms_median"], rows[k]["verified"]))
    same = bool(torch.equal(d_packed_again, prk.data))                                       # packing is deterministic: the timed call wrote the store again
    all_ok = all_ok and same
    T = lambda k: rows[k]["ms_median"]  # noqa: E731

    # the stage split of both forms of every timed pair: one further profiled call each (HIP events around every launch, so kept out of the timed calls)
    for k in jobs:
        rows[k]["stages_ms"] = measure.stage_ms(measure.profiled(eng, *jobs[k][:2]))

    checks = {
        "aes_encrypt_keyed_8x16_packed_vs_lwe": check(T("aes_encrypt_keyed/8x16 packed"), T("aes_encrypt_keyed/8x16 lwe"), BOUND),
        "aes_ctr_streams_8x16_packed_vs_lwe": check(T("aes_ctr_streams/8x16 packed"), T("aes_ctr_streams/8x16 lwe"), BOUND),
        "pack_round_keys_%d_vs_key_expansion_%d" % (N_KEYS, N_KEYS): check(T("pack_round_keys/%d" % N_KEYS), T("aes_key_expansion_many/%d" % N_KEYS), PACK_BOUND),
    }
    for name, c in checks.items():
        progress(TOOL, "%s: %.2f / %.2f ms = %.4f (bound %.2f: %s)" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"], c["bound"],
                                                                      "ok" if c["within_bound"] else "MISSED"))

    # what the device would hold: free memory with nothing of this tool's on it but the context and its keys
    del d_rk, d_rk_again, rk8, d_lwe, d_pk, d_str_lwe, d_str_pk, d_state, d_ek
    torch.cuda.empty_cache()
    free_bytes, total_bytes = torch.cuda.mem_get_info(0)
    memory = {"lwe_bytes_per_key": lwe_key_bytes, "packed_bytes_per_key": packed_key_bytes, "ratio": round(lwe_key_bytes / packed_key_bytes, 1),
              "device_free_bytes": free_bytes, "device_total_bytes": total_bytes,
              "keys_in_free_memory_lwe": free_bytes // lwe_key_bytes, "keys_in_free_memory_packed": free_bytes // packed_key_bytes,
              "bytes_of_65536_keys_packed": 65536 * packed_key_bytes, "bytes_of_65536_keys_lwe": 65536 * lwe_key_bytes}
    progress(TOOL, "per key %d B in LWE form, %d B packed (%.1f x); %d B free hold %d keys in LWE form, %d packed" % (
        lwe_key_bytes, packed_key_bytes, memory["ratio"], free_bytes, memory["keys_in_free_memory_lwe"], memory["keys_in_free_memory_packed"]))

    line = {**measure.header(TOOL, args), "commit": args.commit or measure.commit_id(),
            "k2_kernels": {str(bits): eng.k2_plan(bits)["kernel"] for bits in (32 * N_KEYS, 8 * 248, 8 * 608, 128 * 128)},
            "all_verified": all_ok, "repacked_store_is_the_same_words": same, "checks": checks, "memory": memory, "rows": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, AES-128; every row runs once in every "
                    "step of one loop, the two forms of a call one after the other; checks: measured against the call on the LWE form (or the key "
                    "expansion) timed in the same loop; stages_ms from one further profiled call of each row; memory: free device memory once the "
                    "tool's own tensors are released (the context, its keys and workspaces stay)"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
