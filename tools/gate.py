"""The gate -- ciphertexts times an encrypted `valid` bit -- against what it replaces and what it is built from, at PARAM_OPT on one
GPU, resident tensors.  The data is the README's CCM example: 64 messages of 32 bytes under 8 AES-128 keys, every second one with a
flipped tag bit, so 16,384 plaintext bits under 64 `valid` bits of both values.

  (a)  gate_bits of the 16,384 bits under the 64 gates against the composition DESIGN.md named until now: a 9-bit
       many_wopbs_without_padding per byte with `valid` as the ninth input (LUT: the byte if bit 8 is set, else 0), 2,048 inputs.  The
       9-bit inputs are put together once, outside the timed call.  The only condition: gate_bits is faster.
  (b)  the same gate_bits call against a prediction from entry points that stand alone: fheaes_keyswitch_batch, fheaes_cbs_pbs_batch,
       fheaes_pfpks_batch and fheaes_forward_fourier_batch on the 64 bits, plus fheaes_gate_ggsw on their GGSWs.  Bound 1.03; the words
       of the two routes are compared with array_equal.
  (c)  gate_kernel against K5, per external product: fheaes_gate_ggsw (LWE form) on the 16,384 bits against
       fheaes_vertical_packing_batch on 2,048 eight-bit inputs with one LUT -- 16,384 outputs of 8 products each -- divided by 8.
       Device events around --reps calls of each, alternating.  No bound: the gate reads and writes an LWE ciphertext per product and K5
       does not; the ratio and the bytes moved per product are recorded.
  (d)  Server.aes_ccm_decrypt(gate=True) against gate=False on the 64 messages; the difference is to be compared with (a).

One process, one context; the jobs of (a) and (b) run once in every step of one timed loop (measure.wall), those of (d) in another; the
median of --steps steps after --warmup.  Every output is decrypted with the client key and compared.  A wrong bit makes the tool exit 1,
a missed condition 2.

    python tools/gate.py [--steps 5] [--warmup 1] [--reps 20] [--out profiles/gate.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.client import Client
from tfhe_aes_amd.server import Server

N_KEYS, N_MSG, AAD_BYTES, PAYLOAD_BYTES, TAG_BYTES = 8, 64, 8, 32, 8
TOOL = "gate"


def main() -> int:
    args = measure.arg_parser(reps=20).parse_args()
    p, n = PARAM_OPT, N_MSG
    k1 = p.k + 1
    client = Client(1, 0, 0, params=p, seed=0xAE56A7E)
    srv = Server(client.server_keys(), device=0)
    eng = srv.engine
    rng = np.random.default_rng(0x6A7E)
    keys = [rng.bytes(16) for _ in range(N_KEYS)]
    d_rk = srv.aes_key_expansion_many(to_dev(np.stack([client.encrypt_aes_key(k) for k in keys])))
    eng.synchronize()
    eng.reserve(4 * n * 128)

    clear = [(i % N_KEYS, rng.bytes(12), rng.bytes(AAD_BYTES), rng.bytes(PAYLOAD_BYTES)) for i in range(n)]
    messages = []
    for i, (k, nonce, aad, payload) in enumerate(clear):
        out = aes_clear.ccm_encrypt(keys[k], nonce, aad, payload, TAG_BYTES)
        tag = out[-TAG_BYTES:]
        if i % 2:                                                             # every second message is forged: one tag bit
            tag = tag[:-1] + bytes([tag[-1] ^ 1])
        messages.append((k, nonce, aad, out[:-TAG_BYTES], tag))
    want_valid = [1 - i % 2 for i in range(n)]
    payloads = np.frombuffer(b"".join(c[3] for c in clear), dtype=np.uint8).reshape(n, PAYLOAD_BYTES)
    gated = payloads * np.array(want_valid, dtype=np.uint8)[:, None]
    n_bytes, m = n * PAYLOAD_BYTES, n * PAYLOAD_BYTES * 8
    runs = [PAYLOAD_BYTES * 8] * n
    plan = _native.gate_plan(runs, p.k)

    # the data of (a), (b), (c): the ungated plaintext and `valid` of one call
    d_pt, d_valid, at = srv.aes_ccm_decrypt(d_rk, messages)
    srv.synchronize()
    assert at == list(range(0, 2 * n + 1, 2))
    verified = {"ccm_ungated": np.array_equal(client.decrypt_bytes(host(d_pt)).reshape(n, PAYLOAD_BYTES), payloads)
                and client.decrypt_bits(host(d_valid)).tolist() == want_valid}
    d_bytes = d_pt.view(n_bytes, 8, p.big1)
    d_in9 = torch.empty((n_bytes, 9, p.big1), dtype=torch.int64, device="cuda")
    d_in9[:, :8] = d_bytes
    d_in9[:, 8] = d_valid[torch.arange(n_bytes, device="cuda") // PAYLOAD_BYTES]
    x = np.arange(512)
    d_lut9 = to_dev(_native.gen_lut(9, np.where(x >> 8, x & 0xFF, 0).astype(np.uint64))[None])
    d_ident = to_dev(_native.gen_lut(8, np.arange(256, dtype=np.uint64))[None])
    torch.cuda.synchronize()

    new = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")  # noqa: E731
    d_gate, d_gate2, d_w9 = new(m, p.big1), new(m, p.big1), new(n_bytes, 1, 9, p.big1)
    d_small, d_pbs, d_rows = new(n, p.n + 1), new(n, p.big1), new(n, k1, k1 * p.N)
    d_ggswf = torch.empty((n, 1, k1, k1, 256, 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    nothing = lambda: None  # noqa: E731
    jobs = {
        "gate_bits": (lambda: eng.gate_bits(d_valid, runs, d_pt, m, d_gate), nothing),
        "wopbs9": (lambda: eng.wopbs_batch(d_in9, n_bytes, 9, d_lut9, 1, False, d_w9), nothing),
        "keyswitch64": (lambda: eng.keyswitch_batch(d_valid, d_small, n), nothing),
        "cbs_pbs64": (lambda: eng.cbs_pbs_batch(d_small, d_pbs, n, 1), nothing),
        "pfpks64": (lambda: eng.pfpks_batch(d_pbs, d_rows, n), nothing),
        "forward_fourier64": (lambda: eng.forward_fourier_batch(d_rows, d_ggswf, n * k1 * k1), nothing),
        "gate_ggsw": (lambda: eng.gate_ggsw(d_ggswf, runs, d_pt, m, _native.GATE_LWE, d_gate2), nothing),
    }
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.2f s" % (i, of, s)))
    bytes_of = lambda d: client.decrypt_bytes(host(d).reshape(n_bytes, 8, p.big1)).reshape(n, PAYLOAD_BYTES)  # noqa: E731
    verified["gate_bits"] = np.array_equal(bytes_of(d_gate), gated)
    verified["wopbs9"] = np.array_equal(client.decrypt_bytes(host(d_w9[:, 0, :8].contiguous())).reshape(n, PAYLOAD_BYTES), gated)
    verified["gate_ggsw"] = bool(torch.equal(d_gate, d_gate2))                # the two routes of (b): the same words
    for name in ("keyswitch64", "cbs_pbs64", "pfpks64", "forward_fourier64"):
        verified[name] = verified["gate_ggsw"]                               # their outputs are what gate_ggsw read

    rows = {}
    for name, (run, reset) in jobs.items():
        row = measure.row(times[name])
        prof = measure.profiled(eng, run, reset)
        row["verified"] = bool(verified[name])
        row["stages_ms"] = measure.stage_ms(prof)
        row["stages_units"] = {s: v["units"] for s, v in prof.items()}
        row["stages_launches"] = {s: v["launches"] for s, v in prof.items()}
        rows[name] = row
        progress(TOOL, "%s: %.3f ms" % (name, row["ms_median"]))

    # (c) gate_kernel against K5 per external product: the GGSWs of all 16,384 plaintext bits, by the stage calls
    d_small_all, d_pbs_all = new(m, p.n + 1), new(m, p.big1)
    d_rows_all = new(m, k1, k1 * p.N)
    d_ggswf_all = torch.empty((m, 1, k1, k1, 256, 2), dtype=torch.float64, device="cuda")
    d_vp = new(n_bytes, 1, 8, p.big1)
    torch.cuda.synchronize()
    flat = d_pt.view(m, p.big1)
    eng.keyswitch_batch(flat, d_small_all, m)
    eng.cbs_pbs_batch(d_small_all, d_pbs_all, m, 1)
    eng.pfpks_batch(d_pbs_all, d_rows_all, m)
    eng.forward_fourier_batch(d_rows_all, d_ggswf_all, m * k1 * k1)
    eng.vertical_packing_batch(d_ggswf_all, n_bytes, 8, d_ident, 1, False, d_vp)
    eng.synchronize()
    del d_rows_all, d_pbs_all, d_small_all
    verified["vertical_packing"] = np.array_equal(client.decrypt_bytes(host(d_vp[:, 0].contiguous())).reshape(n, PAYLOAD_BYTES), payloads)
    ev = measure.events(eng, {"gate_ggsw": lambda: eng.gate_ggsw(d_ggswf, runs, d_pt, m, _native.GATE_LWE, d_gate2),
                              "vertical_packing": lambda: eng.vertical_packing_batch(d_ggswf_all, n_bytes, 8, d_ident, 1, False, d_vp)},
                        args.warmup, args.steps, args.reps)
    gate_ms, vp_ms = float(np.median(ev["gate_ggsw"])), float(np.median(ev["vertical_packing"]))
    ggsw_bytes, lwe_bytes, R = k1 * k1 * p.N * 8, p.big1 * 8, plan["instances_per_workgroup"]
    per_product = {
        "gate_kernel": {"lwe_read": lwe_bytes, "lwe_written": lwe_bytes, "ggsw_from_hbm": round(n * ggsw_bytes / m, 1),
                        "ggsw_through_the_caches": round(ggsw_bytes / R, 1)},
        "vertical_packing_kernel": {"lut_read": p.N * 8 / 8, "lwe_written": lwe_bytes / 8, "ggsw_from_hbm": ggsw_bytes / 8,
                                    "ggsw_through_the_caches": round(ggsw_bytes / R, 1)},
    }
    del d_ggswf_all

    # (d) the CCM call with and without the gate
    d_pt2, d_ok2, d_pt3, d_ok3 = new(2 * n, 16, 8, p.big1), new(n, p.big1), new(2 * n, 16, 8, p.big1), new(n, p.big1)
    torch.cuda.synchronize()
    ccm_jobs = {"ccm": (lambda: srv.aes_ccm_decrypt(d_rk, messages, out=d_pt2, valid_out=d_ok2), nothing),
                "ccm_gated": (lambda: srv.aes_ccm_decrypt(d_rk, messages, out=d_pt3, valid_out=d_ok3, gate=True), nothing)}
    ccm_times = measure.wall(eng, ccm_jobs, args.warmup, args.steps, on_step=lambda i, of, s: progress(TOOL, "ccm step %d of %d: %.1f s" % (i, of, s)))
    verified["ccm"] = bool(torch.equal(d_pt2, d_pt)) and bool(torch.equal(d_ok2, d_valid))
    verified["ccm_gated"] = (np.array_equal(client.decrypt_bytes(host(d_pt3)).reshape(n, PAYLOAD_BYTES), gated) and bool(torch.equal(d_ok3, d_valid))
                             and bool(torch.equal(d_pt3.view(m, p.big1), d_gate)))
    for name in ccm_jobs:
        rows[name] = {**measure.row(ccm_times[name]), "verified": bool(verified[name])}
        progress(TOOL, "%s: %.1f ms" % (name, rows[name]["ms_median"]))
    all_ok = all(verified.values())

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    predicted = T("keyswitch64") + T("cbs_pbs64") + T("pfpks64") + T("forward_fourier64") + T("gate_ggsw")
    checks = {
        "a_gate_bits_against_the_9_bit_wopbs": {**measure.check(T("gate_bits"), T("wopbs9"), 1.0), "wopbs9_over_gate_bits": round(T("wopbs9") / T("gate_bits"), 2),
                                                 "circuit_bootstraps": {"gate_bits": n, "wopbs9": 9 * n_bytes}},
        "b_gate_bits_against_its_parts": measure.check(T("gate_bits"), predicted, 1.03),
        "c_gate_kernel_against_k5_per_product": {**measure.check(gate_ms / m * 1e3, vp_ms / (8 * m) * 1e3, None), "unit": "microseconds per external product",
                                                 "gate_ggsw_ms": round(gate_ms, 4), "vertical_packing_ms": round(vp_ms, 4), "products": {"gate": m, "k5": 8 * m},
                                                 "bytes_per_product": per_product, "ms_all": [round(v, 4) for v in ev["gate_ggsw"]],
                                                 "vertical_packing_ms_all": [round(v, 4) for v in ev["vertical_packing"]]},
        "d_ccm_gated_against_ungated": {"ccm_ms": T("ccm"), "ccm_gated_ms": T("ccm_gated"), "difference_ms": round(T("ccm_gated") - T("ccm"), 3),
                                        "gate_bits_ms": T("gate_bits"), "ratio": round(T("ccm_gated") / T("ccm"), 5)},
    }
    for name in ("a_gate_bits_against_the_9_bit_wopbs", "b_gate_bits_against_its_parts", "c_gate_kernel_against_k5_per_product"):
        c = checks[name]
        progress(TOOL, "%s: %.3f against %.3f, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    progress(TOOL, "d: %r" % (checks["d_ccm_gated_against_ungated"],))
    line = {**measure.header(TOOL, args), "messages": n, "keys": N_KEYS, "payload_bytes": PAYLOAD_BYTES, "gated_bits": m, "gates": n, "plan": plan,
            "all_verified": bool(all_ok), "verified": {k: bool(v) for k, v in verified.items()}, "checks": checks, "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one loop "
                    "(the CCM pair in a loop of its own); (c) is device events around --reps calls of each, alternating, in microseconds per external "
                    "product: gate_ggsw / 16,384 against vertical_packing_batch / 131,072; (a) passes when gate_bits is faster than the 9-bit WoPBS"}
    measure.emit(line, args.out)
    eng.close()
    ok_bounds = checks["a_gate_bits_against_the_9_bit_wopbs"]["within_bound"] and checks["b_gate_bits_against_its_parts"]["within_bound"]
    return measure.exit_code(bool(all_ok), bool(ok_bounds))


if __name__ == "__main__":
    sys.exit(main())
