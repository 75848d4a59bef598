"""Many AES keys under one FHE key against the single-key entry points the engine had before, at PARAM_OPT, AES-128, one GPU, one process,
resident tensors.  Every quantity runs once in every step of ONE timed loop (a drift of the clocks meets all of them alike); the median
of --steps steps after --warmup.  Every output is decrypted with the client key and compared with aes_clear: a wrong one makes the tool
exit 1.  The yardsticks are entry points that existed before, timed in the same loop, never the new calls against themselves:

  key expansion      T(aes_key_expansion_batch, n keys), n in {1, 8, 32}, against n x T(aes_key_expansion)                  [reported]
                     and against  P(n) = 40 T(identity WoPBS of 4n bytes) + 10 T(sbox of 4n bytes)                          [<= 1.03 P(n)]
  round-key conv.    T(aes_decryption_round_keys_batch, 14 keys: 16,128 bits) against 14 x T(aes_decryption_round_keys)      [reported]
                     and against  T(many_sbox inv of 2,016 bytes) + T(identity WoPBS of 2,016 bytes)                         [reported]
  keyed cipher       T(aes_encrypt_keyed, 128 blocks as 8 keys x 16) against T(aes_encrypt, 128 blocks)                     [<= 1.03 x]
                     with the linear stage's time and bytes/s of both from one further profiled call
  streams            T(aes_ctr_streams, 8 keys x 16 consecutive counters) against the prediction from its plan,
                     T(many_sbox of 248 bytes) + T(many_sbox of 608 bytes) + 7 T(many_sbox of 2,048 bytes) + T(sbox of 2,048 bytes)  [<= 1.03 x]
                     and against eight separate 16-block aes_ctr calls                                                      [reported]

The predictions were written down before anything was timed.  `checks` in the output records prediction, measurement,
ratio and whether each bound holds; a missed bound makes the tool exit 2.  The blind-rotation kernel of every launch size involved is
recorded from fheaes_k2_context_plan.

    python tools/multi_key.py [--steps 5] [--warmup 1] [--commit ID] [--out profiles/multi_key.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import block_bytes, check, host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.client import Client
from tfhe_aes_amd.server import Server, ctr_stream_blocks

BASE = 0x00112233445566778899AABBCCDDEE00
KX_N = (1, 8, 32)               # keys per batched expansion
CONV_N = 14                     # 14 x 1,152 = 16,128 bits
BOUND = 1.03
TOOL = "multi_key"


def main() -> int:
    ap = measure.arg_parser()
    ap.add_argument("--commit", default=None, help="what the measured tree is (default: git rev-parse HEAD + working tree)")
    args = ap.parse_args()
    p = PARAM_OPT
    rng = np.random.default_rng(0x3A17)
    aes_keys = [rng.bytes(16) for _ in range(max(KX_N))]

    client = Client(1, BASE, int.from_bytes(aes_keys[0], "big"), params=p, seed=0xAE50002)
    srv = Server(client.server_keys(), device=0)            # not measure.session: aes_ctr and aes_ctr_streams are timed through the Server
    eng = srv.engine
    eng.reserve(128 * 128)
    empty = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")  # noqa: E731

    d_ek = to_dev(np.stack([client.encrypt_aes_key(k) for k in aes_keys]))                   # [32][16][8][kN+1]
    d_rk = empty(max(KX_N), 11, 16, 8, p.big1)                                               # the keys everything below runs under
    eng.aes_key_expansion_batch(d_ek, 128, max(KX_N), d_rk)
    eng.synchronize()
    ident = to_dev(_native.gen_lut(8, np.arange(256, dtype=np.uint64))[None, None])           # [1][1][8][512]

    # ---- the jobs: name -> (run, reset, verify) ----
    jobs = {}
    nothing = lambda: None  # noqa: E731
    rk_words = lambda k: np.array(aes_clear.expand_key(k), dtype=np.uint8)  # noqa: E731
    dw_words = lambda k: np.array(aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(k)), dtype=np.uint8)  # noqa: E731

    d_rk1 = empty(11, 16, 8, p.big1)
    jobs["aes_key_expansion"] = (lambda: eng.aes_key_expansion_bits(d_ek[0], 128, d_rk1), nothing,
                                 lambda: np.array_equal(client.decrypt_bytes(host(d_rk1)), rk_words(aes_keys[0])))
    for n in KX_N:
        out = empty(n, 11, 16, 8, p.big1)
        jobs["aes_key_expansion_batch/%d" % n] = (
            lambda n=n, out=out: eng.aes_key_expansion_batch(d_ek[:n], 128, n, out), nothing,
            lambda n=n, out=out: all(np.array_equal(client.decrypt_bytes(host(out[i])), rk_words(aes_keys[i])) for i in range(n)))
    # the WoPBS the predictions are made of, on bytes of the expanded keys (a WoPBS takes the same time whatever its input says)
    flat = d_rk.reshape(-1, 8, p.big1)
    wopbs_sizes = sorted({4 * n for n in KX_N} | {CONV_N * 144, 248, 608, 2048})
    scratch_in = {m: flat[:m].clone() for m in wopbs_sizes}
    scratch_out = empty(max(wopbs_sizes), 4, 8, p.big1)
    for m in (4 * n for n in KX_N):
        jobs["identity_wopbs/%d" % m] = (lambda m=m: eng.wopbs_batch(scratch_in[m], m, 8, ident, 1, False, scratch_out), nothing, None)
        jobs["sbox/%d" % m] = (lambda m=m: eng.sbox(scratch_in[m], m, False), nothing, None)
    m = CONV_N * 144
    jobs["identity_wopbs/%d" % m] = (lambda m=m: eng.wopbs_batch(scratch_in[m], m, 8, ident, 1, False, scratch_out), nothing, None)
    jobs["many_sbox_inv/%d" % m] = (lambda m=m: eng.many_sbox(scratch_in[m], m, True, scratch_out), nothing, None)
    for m in (248, 608, 2048):
        jobs["many_sbox/%d" % m] = (lambda m=m: eng.many_sbox(scratch_in[m], m, False, scratch_out), nothing, None)
    jobs["sbox/2048"] = (lambda: eng.sbox(scratch_in[2048], 2048, False), nothing, None)

    d_dw1, d_dwb = empty(11, 16, 8, p.big1), empty(CONV_N, 11, 16, 8, p.big1)
    jobs["aes_decryption_round_keys"] = (lambda: eng.aes_decryption_round_keys_bits(d_rk[0], 128, d_dw1), nothing,
                                         lambda: np.array_equal(client.decrypt_bytes(host(d_dw1)), dw_words(aes_keys[0])))
    jobs["aes_decryption_round_keys_batch/%d" % CONV_N] = (
        lambda: eng.aes_decryption_round_keys_batch(d_rk[:CONV_N], 128, CONV_N, d_dwb), nothing,
        lambda: all(np.array_equal(client.decrypt_bytes(host(d_dwb[i])), dw_words(aes_keys[i])) for i in range(CONV_N)))

    n_blocks, kob = 128, [b // 16 for b in range(128)]                                       # 8 keys x 16 blocks
    pts = [(BASE + 0x0101 * i) & ((1 << 128) - 1) for i in range(n_blocks)]
    d_state = to_dev(np.stack([client.encrypt_u128(v) for v in pts]))
    d_enc1, d_enck = torch.empty_like(d_state), torch.empty_like(d_state)
    jobs["aes_encrypt/128"] = (lambda: eng.aes_encrypt_bits(d_rk[0], 128, d_enc1, n_blocks), lambda: d_enc1.copy_(d_state),
                               lambda: np.array_equal(client.decrypt_bytes(host(d_enc1)), block_bytes([aes_clear.aes_encrypt_block(aes_keys[0], v) for v in pts])))
    jobs["aes_encrypt_keyed/8x16"] = (lambda: eng.aes_encrypt_keyed(d_rk[:8], 128, 8, kob, d_enck, n_blocks), lambda: d_enck.copy_(d_state),
                                      lambda: np.array_equal(client.decrypt_bytes(host(d_enck)),
                                                             block_bytes([aes_clear.aes_encrypt_block(aes_keys[k], v) for k, v in zip(kob, pts)])))

    streams = [(k, BASE, 0, 16, None) for k in range(8)]
    d_str, d_sep = empty(128, 16, 8, p.big1), empty(128, 16, 8, p.big1)
    want_streams = block_bytes(aes_clear.ctr_streams(aes_keys, streams))

    def separate():
        for k in range(8):
            srv.aes_ctr(d_rk[k], BASE, 0, 16, out=d_sep[16 * k:16 * k + 16])

    jobs["aes_ctr_streams/8x16"] = (lambda: srv.aes_ctr_streams(d_rk[:8], streams, out=d_str), nothing,
                                    lambda: np.array_equal(client.decrypt_bytes(host(d_str)), want_streams))
    jobs["aes_ctr/8 calls of 16"] = (separate, nothing, lambda: np.array_equal(client.decrypt_bytes(host(d_sep)), want_streams))
    stream_keys, stream_blocks, _ = ctr_stream_blocks(streams)
    plan = _native.aes_public_plan_keyed(stream_blocks, stream_keys, 8, 128)
    assert plan == [248, 608] + [2048] * 8, plan

    # ---- one timed loop, every job once per step ----
    times = measure.wall(eng, {k: j[:2] for k, j in jobs.items()}, args.warmup, args.steps,
                         on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    all_ok = True
    rows = {}
    for k, (run, reset, verify) in jobs.items():
        rows[k] = measure.row(times[k])
        if verify is not None:
            rows[k]["verified"] = bool(verify())
            all_ok = all_ok and rows[k]["verified"]
        progress(TOOL, "%s: %.2f ms%s" % (k, rows[k]["ms_median"], "" if verify is None else " verified=%s" % rows[k]["verified"]))
    T = lambda k: rows[k]["ms_median"]  # noqa: E731

    # the linear stage of the two 128-block encryptions: one further profiled call each (HIP events around every launch, so kept out of the timed calls).
    # Bytes as DESIGN.md section 7 counts them for gather_add_kernel's 4.2 TB/s: the state read and written by AddRoundKey (2 rows per byte),
    # 4 WoPBS outputs read and a byte written by each of the 9 MixColumns layers (5), 1 + 1 by the last: 49 x the state; the round-key rows
    # on top of that are 16 rows per layer for one key (cache) and up to one set per block for the keyed call
    linear_bytes = 49 * 16 * n_blocks * 8 * p.big1 * 8
    for k in ("aes_encrypt/128", "aes_encrypt_keyed/8x16"):
        prof = measure.profiled(eng, *jobs[k][:2])
        rows[k]["stages_ms"] = measure.stage_ms(prof)
        rows[k]["linear_bytes"] = linear_bytes
        rows[k]["linear_TB_per_s"] = round(linear_bytes / (prof["linear"]["ms"] * 1e-3) / 1e12, 3)

    checks = {}
    for n in KX_N:
        b = "aes_key_expansion_batch/%d" % n
        checks["key_expansion_%d_vs_prediction" % n] = check(T(b), 40 * T("identity_wopbs/%d" % (4 * n)) + 10 * T("sbox/%d" % (4 * n)), BOUND)
        checks["key_expansion_%d_vs_%d_single_calls" % (n, n)] = check(T(b), n * T("aes_key_expansion"), None)
    b, m = "aes_decryption_round_keys_batch/%d" % CONV_N, CONV_N * 144
    checks["round_key_conversion_%d_vs_prediction" % CONV_N] = check(T(b), T("many_sbox_inv/%d" % m) + T("identity_wopbs/%d" % m), None)
    checks["round_key_conversion_%d_vs_%d_single_calls" % (CONV_N, CONV_N)] = check(T(b), CONV_N * T("aes_decryption_round_keys"), None)
    checks["aes_encrypt_keyed_8x16_vs_aes_encrypt_128"] = check(T("aes_encrypt_keyed/8x16"), T("aes_encrypt/128"), BOUND)
    checks["aes_ctr_streams_8x16_vs_prediction"] = check(T("aes_ctr_streams/8x16"),
                                                         T("many_sbox/248") + T("many_sbox/608") + 7 * T("many_sbox/2048") + T("sbox/2048"), BOUND)
    checks["aes_ctr_streams_8x16_vs_8_aes_ctr_calls"] = check(T("aes_ctr_streams/8x16"), T("aes_ctr/8 calls of 16"), None)
    for name, c in checks.items():
        progress(TOOL, "%s: %.2f / %.2f ms = %.4f%s" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"],
                                                   "" if c["bound"] is None else " (bound %.2f: %s)" % (c["bound"], "ok" if c["within_bound"] else "MISSED")))

    launch_bits = sorted({32 * n for n in KX_N} | {CONV_N * 1152, 128 * 128, 8 * 248, 8 * 608})
    line = {**measure.header(TOOL, args), "commit": args.commit or measure.commit_id(),
            "k2_kernels": {str(bits): eng.k2_plan(bits)["kernel"] for bits in launch_bits}, "streams_plan": plan,
            "all_verified": all_ok, "checks": checks, "rows": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, AES-128; every row runs once in every "
                    "step of one loop; checks: measured against a yardstick made of entry points that existed before (bound null: reported only); "
                    "k2_kernels: fheaes_k2_context_plan's kernel per blind-rotation launch size in bits; linear_TB_per_s from one further profiled call"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok, all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
