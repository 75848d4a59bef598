"""AES key unwrap (RFC 3394) against the entry points it is built from, at PARAM_OPT on one GPU, resident tensors: 64 wrapped AES-128
keys (n = 2 semiblocks, 24 bytes each) under 4 AES-128 KEKs, so 12 passes of the equivalent inverse cipher over 64 blocks, the identity
WoPBS on the 1,024 bytes of the unwrapped keys and the two WoPBS of the tag check:

  unwrap     aes_kw_unwrap_keyed of the 64 wrapped keys
  dec64      aes_decrypt_equivalent_keyed on 64 blocks under the 4 KEKs: ONE step (the call runs 12)
  ident1024  many_wopbs_without_padding, 8 bits, the identity, on 1,024 bytes                  (the refresh of the keys)
  ne0        many_wopbs_without_padding, 8 bits, one LUT (byte != 0), on 1,024 bytes            (the first WoPBS of the tag check)
  eq0        many_wopbs_without_padding, 16 bits, one LUT (input == 0), on 64 inputs            (the second)

One process, one context; every job runs once in every step of ONE timed loop (measure.wall), the median of --steps steps after --warmup.
The unwrapped keys and `valid` are decrypted with the client key and checked both ways: the payloads and all 1 on the call as it is, and
0 on exactly the keys a second, untimed call has a bit flipped in; the other jobs' outputs are decrypted and compared with aes_clear.  A
wrong bit makes the tool exit 1.

    (a)  T(unwrap) <= 1.03 (12 T(dec64) + T(ident1024) + T(ne0) + T(eq0))

1.03 is the margin every composed call here was given against a prediction from older entry points; what the call adds is 13 K6 launches
of well under a millisecond.

    (b)  one shuffle of kw_link_kernel over 64 keys (fheaes_kw_link, step 1) against fheaes_mac_link over 64 slots without an encrypted
         addend: both write 128 rows per key or slot; device events around --reps calls of each, alternating; bound 1.5.

A missed bound makes the tool exit 2.

    python tools/keywrap.py [--steps 5] [--warmup 1] [--reps 20] [--out profiles/key_unwrap.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear

N_KEKS, N_KEYS, SEMIBLOCKS, STEPS_OF_CHAIN = 4, 64, 2, 12
TOOL = "keywrap"


def main() -> int:
    args = measure.arg_parser(reps=20).parse_args()
    p, n = PARAM_OPT, N_KEYS
    client, eng = measure.session(0xAE53394)
    rng = np.random.default_rng(0x3394)
    keks = [rng.bytes(16) for _ in range(N_KEKS)]
    d_rk = torch.empty((N_KEKS, 11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_dw = torch.empty_like(d_rk)
    eng.aes_key_expansion_batch(to_dev(np.stack([client.encrypt_aes_key(k) for k in keks])), 128, N_KEKS, d_rk)
    eng.aes_decryption_round_keys_batch(d_rk, 128, N_KEKS, d_dw)
    eng.synchronize()
    eng.reserve(4 * n * 128)

    kek_of = [i % N_KEKS for i in range(n)]
    payloads = [rng.bytes(8 * SEMIBLOCKS) for _ in range(n)]
    wrapped = [aes_clear.key_wrap(keks[k], d) for k, d in zip(kek_of, payloads)]
    plan = _native.aes_kw_plan(128, SEMIBLOCKS, n)
    assert plan == {"steps": STEPS_OF_CHAIN, "cipher_blocks": STEPS_OF_CHAIN * n, "byte_wopbs": 160 * STEPS_OF_CHAIN * n + 16 * n + 16 * n}

    step_blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    d_step0 = to_dev(client.trivial_bytes(measure.block_bytes(step_blocks)))
    ident_bytes = rng.integers(0, 256, 16 * n).astype(np.uint8)
    d_ident_in = to_dev(client.trivial_bytes(ident_bytes))
    ne0_bytes = rng.integers(0, 4, 16 * n).astype(np.uint8)                   # a quarter of them 0
    eq0_values = rng.integers(0, 2, n).astype(np.uint64) * rng.integers(1, 1 << 16, n).astype(np.uint64)
    d_ne0_in = to_dev(client.trivial_bytes(ne0_bytes))
    eq0_bits = ((eq0_values[:, None] >> np.arange(16, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    d_eq0_in = to_dev(client.trivial_bytes(eq0_bits)[:, :, 0, :])             # bit 0 of a trivial byte: [n][16][kN+1]
    d_ident = to_dev(_native.gen_lut(8, np.arange(256, dtype=np.uint64))[None])
    d_ne0 = to_dev(_native.gen_lut(8, (np.arange(256) != 0).astype(np.uint64))[None])
    d_eq0 = to_dev(_native.gen_lut(16, (np.arange(1 << 16) == 0).astype(np.uint64))[None])

    d_keys = torch.empty((n, 8 * SEMIBLOCKS, 8, p.big1), dtype=torch.int64, device="cuda")
    d_valid = torch.empty((n, p.big1), dtype=torch.int64, device="cuda")
    d_step = torch.empty((n, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ident_out = torch.empty((16 * n, 1, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ne0_out = torch.empty((16 * n, 1, 8, p.big1), dtype=torch.int64, device="cuda")
    d_eq0_out = torch.empty((n, 1, 16, p.big1), dtype=torch.int64, device="cuda")

    def unwrap(w, keys, valid):
        eng.aes_kw_unwrap_keyed(d_dw, 128, N_KEKS, kek_of, SEMIBLOCKS, w, keys, valid)

    nothing = lambda: None  # noqa: E731
    jobs = {
        "unwrap": (lambda: unwrap(wrapped, d_keys, d_valid), nothing),
        "dec64": (lambda: eng.aes_decrypt_equivalent_keyed(d_dw, 128, N_KEKS, kek_of, d_step, n), lambda: d_step.copy_(d_step0)),
        "ident1024": (lambda: eng.wopbs_batch(d_ident_in, 16 * n, 8, d_ident, 1, False, d_ident_out), nothing),
        "ne0": (lambda: eng.wopbs_batch(d_ne0_in, 16 * n, 8, d_ne0, 1, False, d_ne0_out), nothing),
        "eq0": (lambda: eng.wopbs_batch(d_eq0_in, n, 16, d_eq0, 1, False, d_eq0_out), nothing),
    }
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    # every output decrypted and compared
    valid = client.decrypt_bits(host(d_valid)).tolist()
    got_keys = [bytes(k.tolist()) for k in client.decrypt_bytes(host(d_keys))]
    verified = {"unwrap": valid == [1] * n and got_keys == payloads,
                "dec64": np.array_equal(client.decrypt_bytes(host(d_step)),
                                        measure.block_bytes([aes_clear.aes_decrypt_block(keks[k], b) for k, b in zip(kek_of, step_blocks)])),
                "ident1024": client.decrypt_bytes(host(d_ident_out)).reshape(-1).tolist() == ident_bytes.tolist(),
                "ne0": client.decrypt_bits(host(d_ne0_out))[:, 0, 0].tolist() == (ne0_bytes != 0).astype(int).tolist(),
                "eq0": client.decrypt_bits(host(d_eq0_out))[:, 0, 0].tolist() == (eq0_values == 0).astype(int).tolist()}
    # `valid` the other way: a bit of C[0] flipped in every fourth key, a bit of C[2] in every fourth from 2 on
    bad = list(wrapped)
    for i in range(0, n, 4):
        bad[i] = bad[i][:5] + bytes([bad[i][5] ^ 0x04]) + bad[i][6:]
    for i in range(2, n, 4):
        bad[i] = bad[i][:-1] + bytes([bad[i][-1] ^ 0x80])
    d_keys2, d_valid2 = torch.empty_like(d_keys), torch.empty_like(d_valid)
    unwrap(bad, d_keys2, d_valid2)
    eng.synchronize()
    valid_bad = client.decrypt_bits(host(d_valid2)).tolist()
    want_bad = [aes_clear.key_unwrap(keks[k], w) for k, w in zip(kek_of, bad)]
    verified["unwrap_rejects"] = (valid_bad == [0 if i % 2 == 0 else 1 for i in range(n)] == [int(ok) for ok, _ in want_bad]
                                  and [bytes(k.tolist()) for k in client.decrypt_bytes(host(d_keys2))] == [d for _, d in want_bad])
    all_ok = all(verified.values())

    rows = {}
    for k, (run, reset) in jobs.items():
        row = measure.row(times[k])
        prof = measure.profiled(eng, run, reset)
        row["verified"] = bool(verified[k])
        row["stages_ms"] = measure.stage_ms(prof)
        row["stages_units"] = {s: v["units"] for s, v in prof.items()}
        row["stages_launches"] = {s: v["launches"] for s, v in prof.items()}
        rows[k] = row
        progress(TOOL, "%s: %.1f ms" % (k, row["ms_median"]))

    # (b) one shuffle of the unwrap link against one CBC-MAC link of public blocks: 128 rows written per key or slot
    d_state = to_dev(client.trivial_bytes(measure.block_bytes(step_blocks)))
    d_regs = to_dev(client.trivial_bytes(np.frombuffer(b"".join(payloads), dtype=np.uint8).reshape(n, 8 * SEMIBLOCKS)))
    d_mac = to_dev(client.trivial_bytes(measure.block_bytes(step_blocks)))
    clear = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    eng.kw_link(d_state, d_regs, SEMIBLOCKS, 1)                               # i_0 = 2 -> i_1 = 1, t_1 = 11
    eng.mac_link(d_mac, False, None, None, None, None, clear)
    eng.synchronize()
    want_state = [((b >> 64) ^ 11) << 64 | int.from_bytes(d[:8], "big") for b, d in zip(step_blocks, payloads)]
    want_regs = [d[:8] + (b & ((1 << 64) - 1)).to_bytes(8, "big") for b, d in zip(step_blocks, payloads)]
    want_mac = [b ^ int.from_bytes(bytes(c.tolist()), "big") for b, c in zip(step_blocks, clear)]
    all_ok = (all_ok and np.array_equal(client.decrypt_bytes(host(d_state)), measure.block_bytes(want_state))
              and [bytes(k.tolist()) for k in client.decrypt_bytes(host(d_regs))] == want_regs
              and np.array_equal(client.decrypt_bytes(host(d_mac)), measure.block_bytes(want_mac)))
    ev = measure.events(eng, {"kw_link": lambda: eng.kw_link(d_state, d_regs, SEMIBLOCKS, 1),
                              "mac_link": lambda: eng.mac_link(d_mac, False, None, None, None, None, clear)}, args.warmup, args.steps, args.reps)
    kw_ms, mac_ms = float(np.median(ev["kw_link"])), float(np.median(ev["mac_link"]))
    out_bytes = n * 128 * p.big1 * 8

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    predicted = STEPS_OF_CHAIN * T("dec64") + T("ident1024") + T("ne0") + T("eq0")
    checks = {"unwrap": measure.check(T("unwrap"), predicted, 1.03),
              "kw_link_against_mac_link": {**measure.check(kw_ms, mac_ms, 1.5), "written_bytes": out_bytes,
                                           "kw_link_GB_per_s_written": round(out_bytes / kw_ms / 1e6, 1),
                                           "ms_all": [round(v, 4) for v in ev["kw_link"]], "mac_link_ms_all": [round(v, 4) for v in ev["mac_link"]]}}
    for name, c in checks.items():
        progress(TOOL, "%s: %.3f ms, predicted %.3f ms, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    line = {**measure.header(TOOL, args), "wrapped_keys": n, "keks": N_KEKS, "semiblocks": SEMIBLOCKS, "kek_bits": 128,
            "all_verified": bool(all_ok), "valid_on_the_keys_as_sent": valid.count(1), "valid_after_flipped_bits": valid_bad.count(1),
            "checks": checks, "plan": plan, "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one loop; "
                    "unwrap is predicted from 12 x aes_decrypt_equivalent_keyed on 64 blocks + the identity WoPBS on 1,024 bytes + the two WoPBS of the "
                    "tag check; one shuffle of kw_link_kernel (64 keys) and one mac_link_kernel launch without an encrypted addend (64 slots) write 128 "
                    "rows per key or slot and are timed with device events around --reps calls of each, alternating"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(bool(all_ok), all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
