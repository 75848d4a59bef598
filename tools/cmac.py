"""AES-CMAC verification against the entry points it is built from, at PARAM_OPT on one GPU, resident tensors, AES-128: 64 messages of 48
bytes (three whole blocks, so K1) under 8 keys with 8-byte tags, the subkeys derived inside the call, so a public call on 8 zero blocks,
two identity WoPBS, a chain of 3 steps over 64 streams and the two WoPBS of the tag check:

  cmac_verify  aes_cmac_keyed of the 64 messages with their tags, subkeys NULL
  public8      aes_public_keyed on 8 zero blocks, one per key                                   (L before its refresh)
  ident128     many_wopbs_without_padding, 8 bits, the identity, on 128 bytes                   (the refresh of L)
  ident256     the same on 256 bytes                                                            (the refresh of K1 and K2)
  keyed64      aes_encrypt_keyed on 64 blocks under the 8 keys: ONE chain step (the call runs 3)
  ne0          many_wopbs_without_padding, 8 bits, one LUT (byte != 0), on 1,024 bytes          (the first WoPBS of the tag check)
  eq0          many_wopbs_without_padding, 16 bits, one LUT (input == 0), on 64 inputs          (the second)

One process, one context; every job runs once in every step of ONE timed loop (measure.wall), the median of --steps steps after --warmup.
`valid` is decrypted with the client key and checked both ways: all 1 on the call as it is, and 0 on exactly the messages whose tag or
message a second, untimed call has a bit flipped in; the other jobs' outputs are decrypted and compared with aes_clear.  A wrong bit
makes the tool exit 1.

    (a)  T(cmac_verify) <= 1.03 (T(public8) + T(ident128) + T(ident256) + 3 T(keyed64) + T(ne0) + T(eq0))

1.03 is the margin every composed call here was given against a prediction from older entry points; what the call adds is K6 launches
of well under a millisecond.

    (b)  bit_rows_kernel<CmacRows> on 64 keys (fheaes_cmac_double: 128 blocks out) against bit_rows_kernel<XtsRows> on 64 units and offsets 1 and 2
         (fheaes_xts_tweaks: 128 blocks out, the same rows in the other byte order), device events around --reps calls of each,
         alternating; bound 1.5.

A missed bound makes the tool exit 2.

    python tools/cmac.py [--steps 5] [--warmup 1] [--reps 20] [--out profiles/cmac.json]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.server import cmac_args

N_KEYS, N_MSG, MESSAGE_BYTES, TAG_BYTES, STEPS_OF_CHAIN, DOUBLE_KEYS = 8, 64, 48, 8, 3, 64
TOOL = "cmac"


def main() -> int:
    args = measure.arg_parser(reps=20).parse_args()
    p, n = PARAM_OPT, N_MSG
    client, eng = measure.session(0xAE5C3AC)
    rng = np.random.default_rng(0x38B)
    keys = [rng.bytes(16) for _ in range(N_KEYS)]
    d_rk = torch.empty((N_KEYS, 11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    eng.aes_key_expansion_batch(to_dev(np.stack([client.encrypt_aes_key(k) for k in keys])), 128, N_KEYS, d_rk)
    eng.synchronize()
    eng.reserve(4 * n * 128)

    messages = []
    for i in range(n):
        msg = rng.bytes(MESSAGE_BYTES)
        messages.append((i % N_KEYS, msg, aes_clear.cmac(keys[i % N_KEYS], msg, TAG_BYTES)))
    a = cmac_args(messages)
    plan = _native.aes_cmac_plan(a["message_bytes"])
    assert plan == {"steps": STEPS_OF_CHAIN, "chained_blocks": STEPS_OF_CHAIN * n, "padded_streams": 0}

    step_keys = [m[0] for m in messages]
    step_blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    d_step0 = to_dev(client.trivial_bytes(measure.block_bytes(step_blocks)))
    ident_bytes = rng.integers(0, 256, 256).astype(np.uint8)
    d_ident_in = to_dev(client.trivial_bytes(ident_bytes))
    ne0_bytes = rng.integers(0, 4, 16 * n).astype(np.uint8)                   # a quarter of them 0
    eq0_values = rng.integers(0, 2, n).astype(np.uint64) * rng.integers(1, 1 << 16, n).astype(np.uint64)
    d_ne0_in = to_dev(client.trivial_bytes(ne0_bytes))
    eq0_bits = ((eq0_values[:, None] >> np.arange(16, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    d_eq0_in = to_dev(client.trivial_bytes(eq0_bits)[:, :, 0, :])             # bit 0 of a trivial byte: [n][16][kN+1]
    d_ident = to_dev(_native.gen_lut(8, np.arange(256, dtype=np.uint64))[None])
    d_ne0 = to_dev(_native.gen_lut(8, (np.arange(256) != 0).astype(np.uint64))[None])
    d_eq0 = to_dev(_native.gen_lut(16, (np.arange(1 << 16) == 0).astype(np.uint64))[None])

    blocks = lambda k: torch.empty((k, 16, 8, p.big1), dtype=torch.int64, device="cuda")  # noqa: E731
    d_valid = torch.empty((n, p.big1), dtype=torch.int64, device="cuda")
    d_pub, d_step = blocks(N_KEYS), blocks(n)
    d_ident_out = torch.empty((256, 1, 8, p.big1), dtype=torch.int64, device="cuda")
    d_ne0_out = torch.empty((16 * n, 1, 8, p.big1), dtype=torch.int64, device="cuda")
    d_eq0_out = torch.empty((n, 1, 16, p.big1), dtype=torch.int64, device="cuda")

    def cmac_call(x, valid):
        eng.aes_cmac_keyed(d_rk, 128, N_KEYS, None, x["key_of_stream"], x["message_bytes"], x["data"], x["tags"], x["tag_bytes"], None, valid)

    nothing = lambda: None  # noqa: E731
    jobs = {
        "cmac_verify": (lambda: cmac_call(a, d_valid), nothing),
        "public8": (lambda: eng.aes_public_keyed(d_rk, 128, N_KEYS, list(range(N_KEYS)), [0] * N_KEYS, None, d_pub), nothing),
        "ident128": (lambda: eng.wopbs_batch(d_ident_in[:128], 128, 8, d_ident, 1, False, d_ident_out[:128]), nothing),
        "ident256": (lambda: eng.wopbs_batch(d_ident_in, 256, 8, d_ident, 1, False, d_ident_out), nothing),
        "keyed64": (lambda: eng.aes_encrypt_keyed(d_rk, 128, N_KEYS, step_keys, d_step, n), lambda: d_step.copy_(d_step0)),
        "ne0": (lambda: eng.wopbs_batch(d_ne0_in, 16 * n, 8, d_ne0, 1, False, d_ne0_out), nothing),
        "eq0": (lambda: eng.wopbs_batch(d_eq0_in, n, 16, d_eq0, 1, False, d_eq0_out), nothing),
    }
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    # every output decrypted and compared
    valid = client.decrypt_bits(host(d_valid)).tolist()
    ident_ok = client.decrypt_bytes(host(d_ident_out)).reshape(-1).tolist() == ident_bytes.tolist()
    verified = {"cmac_verify": valid == [1] * n,
                "public8": np.array_equal(client.decrypt_bytes(host(d_pub)), measure.block_bytes([aes_clear.aes_encrypt_block(k, 0) for k in keys])),
                "ident128": ident_ok, "ident256": ident_ok,
                "keyed64": np.array_equal(client.decrypt_bytes(host(d_step)),
                                          measure.block_bytes([aes_clear.aes_encrypt_block(keys[k], b) for k, b in zip(step_keys, step_blocks)])),
                "ne0": client.decrypt_bits(host(d_ne0_out))[:, 0, 0].tolist() == (ne0_bytes != 0).astype(int).tolist(),
                "eq0": client.decrypt_bits(host(d_eq0_out))[:, 0, 0].tolist() == (eq0_values == 0).astype(int).tolist()}
    # `valid` the other way: the last tag bit flipped in every fourth message, a message bit in every fourth from 2 on
    bad = list(messages)
    for i in range(0, n, 4):
        k, msg, tag = bad[i]
        bad[i] = (k, msg, tag[:-1] + bytes([tag[-1] ^ 1]))
    for i in range(2, n, 4):
        k, msg, tag = bad[i]
        bad[i] = (k, msg[:20] + bytes([msg[20] ^ 0x40]) + msg[21:], tag)
    d_valid2 = torch.empty_like(d_valid)
    cmac_call(cmac_args(bad), d_valid2)
    eng.synchronize()
    valid_bad = client.decrypt_bits(host(d_valid2)).tolist()
    verified["cmac_rejects"] = valid_bad == [0 if i % 2 == 0 else 1 for i in range(n)]
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

    # (b) the subkey gather against the XTS tweak gather: 64 blocks in, 128 blocks out
    m = DOUBLE_KEYS
    values = [int.from_bytes(rng.bytes(16), "big") | (1 << 127) for _ in range(m)]          # every one is reduced
    d_l = to_dev(client.trivial_bytes(measure.block_bytes(values))).view(m, 128, p.big1)
    d_sub = torch.empty((m, 2, 128, p.big1), dtype=torch.int64, device="cuda")
    d_twk = torch.empty((m, 2, 128, p.big1), dtype=torch.int64, device="cuda")
    eng.cmac_double(d_l, m, d_sub)
    eng.synchronize()
    dbl = lambda v: ((v << 1) ^ (0x87 if v >> 127 else 0)) & ((1 << 128) - 1)  # noqa: E731
    want = [w for v in values for w in (dbl(v), dbl(dbl(v)))]
    all_ok = all_ok and np.array_equal(client.decrypt_bytes(host(d_sub).reshape(2 * m, 16, 8, p.big1)), measure.block_bytes(want))
    ev = measure.events(eng, {"double": lambda: eng.cmac_double(d_l, m, d_sub), "tweaks": lambda: eng.xts_tweaks(d_l, m, 1, 2, d_twk)},
                        args.warmup, args.steps, args.reps)
    double_ms, tweaks_ms = float(np.median(ev["double"])), float(np.median(ev["tweaks"]))
    out_bytes = 2 * m * 128 * p.big1 * 8

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    predicted = T("public8") + T("ident128") + T("ident256") + STEPS_OF_CHAIN * T("keyed64") + T("ne0") + T("eq0")
    checks = {"cmac_verify": measure.check(T("cmac_verify"), predicted, 1.03),
              "subkey_gather_against_the_xts_tweak_gather": {**measure.check(double_ms, tweaks_ms, 1.5), "output_bytes": out_bytes,
                                                             "subkey_gather_GB_per_s_written": round(out_bytes / double_ms / 1e6, 1),
                                                             "ms_all": [round(v, 4) for v in ev["double"]],
                                                             "tweaks_ms_all": [round(v, 4) for v in ev["tweaks"]]}}
    for name, c in checks.items():
        progress(TOOL, "%s: %.3f ms, predicted %.3f ms, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    line = {**measure.header(TOOL, args), "messages": n, "keys": N_KEYS, "message_bytes": MESSAGE_BYTES, "tag_bytes": TAG_BYTES,
            "all_verified": bool(all_ok), "valid_on_the_messages_as_sent": valid.count(1), "valid_after_flipped_bits": valid_bad.count(1),
            "checks": checks, "plan": plan, "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one loop; "
                    "cmac_verify (subkeys derived in the call) is predicted from aes_public_keyed on 8 zero blocks + the identity WoPBS on 128 and on 256 "
                    "bytes + 3 x aes_encrypt_keyed on 64 blocks + the two WoPBS of the tag check; the subkey gather (64 keys) and the XTS tweak gather (64 "
                    "units, offsets 1 and 2) write 128 blocks each and are timed with device events around --reps calls of each, alternating"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(bool(all_ok), all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
