"""AES-CCM decryption with its tag check against the entry points it is built from, at PARAM_OPT on one GPU, resident tensors, AES-128:
64 messages under 8 keys, each with 8 bytes of AAD (one block), 32 bytes of payload (two blocks) and an 8-byte tag, so 256 public
blocks (B0, Ctr_0, Ctr_1, Ctr_2 per message) and a chain of 3 steps over 64 streams:

  ccm          aes_ccm_open_keyed of the 64 messages
  public256    aes_public_keyed on the call's 256 public blocks with its data
  keyed64      aes_encrypt_keyed on 64 blocks under the 8 keys: ONE chain step (the call runs 3)
  ne0          many_wopbs_without_padding, 8 bits, one LUT (byte != 0), on 1,024 bytes     (the first WoPBS of the tag check)
  eq0          many_wopbs_without_padding, 16 bits, one LUT (input == 0), on 64 inputs      (the second)

One process, one context; every job runs once in every step of ONE timed loop (measure.wall), the median of --steps steps after --warmup.
Every message's plaintext is decrypted with the client key and compared with aes_clear, and `valid` is checked both ways: all 1 on the
call as it is, and 0 on exactly the messages whose tag or ciphertext a second, untimed call has a bit flipped in.  A wrong block or bit
makes the tool exit 1.

    (a)  T(ccm) <= 1.03 (T(public256) + 3 T(keyed64) + T(ne0) + T(eq0))

1.03 is the margin every composed call here was given against a prediction from older entry points; what the call adds is K6 launches
of well under a millisecond.

    (b)  mac_link_kernel over 64 slots with an encrypted addend (fheaes_mac_link) against xts_whiten_kernel over 64 blocks in place
         (fheaes_xts_whiten): as many output bytes and the same reads per word, device events around --reps calls of each,
         alternating; bound 1.5.

A missed bound makes the tool exit 2.

    python tools/ccm.py [--steps 5] [--warmup 1] [--reps 20] [--out profiles/ccm.json]

--host-path: instead of all that, the HOST side of two small calls at PARAM_TOY, where the kernels take so little that the entry point's own
work shows: Server.aes_ctr on 4 blocks and Server.aes_cbc_mac_streams on 3 streams of 2 blocks, resident tensors, measure.wall.  --lib PATH
loads that libfheaes.so instead of the tree's, so that two builds can be run in alternating processes of one call and compared.

    python tools/ccm.py --host-path [--lib path/to/libfheaes.so] [--steps 50] [--warmup 5]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import host, progress, to_dev
from tfhe_aes_amd import PARAM_OPT, _native, aes_clear
from tfhe_aes_amd.server import ccm_args

N_KEYS, N_MSG, AAD_BYTES, PAYLOAD_BYTES, TAG_BYTES, STEPS_OF_CHAIN = 8, 64, 8, 32, 8, 3
TOOL = "ccm"


def host_path(args) -> int:
    from tfhe_aes_amd import PARAM_TOY
    from tfhe_aes_amd.client import Client
    from tfhe_aes_amd.server import Server

    client = Client(1, 0, 0, params=PARAM_TOY, seed=0xC0DE)
    server = Server(client.server_keys(), device=0, engine=_native.Engine(PARAM_TOY, device=0, library=args.lib))
    key = bytes(range(16))
    d_rk = server.aes_key_expansion(to_dev(client.encrypt_aes_key(key)))
    server.synchronize()
    streams = [(0, [17 * s + i for i in range(2)]) for s in range(3)]
    got = {}
    nothing = lambda: None  # noqa: E731
    jobs = {"aes_ctr_4_blocks": (lambda: got.update(ctr=server.aes_ctr(d_rk, 5, 0, 4)), nothing),
            "aes_cbc_mac_3_streams_of_2_blocks": (lambda: got.update(mac=server.aes_cbc_mac_streams(d_rk, streams)), nothing)}
    times = measure.wall(server.engine, jobs, args.warmup, args.steps)
    ok = np.array_equal(client.decrypt_bytes(host(got["ctr"])), measure.block_bytes([aes_clear.aes_encrypt_block(key, 5 + i) for i in range(4)]))
    for s, (_, blocks) in enumerate(streams):
        x = 0
        for b in blocks:
            x = aes_clear.aes_encrypt_block(key, x ^ b)
        ok = ok and np.array_equal(client.decrypt_bytes(host(got["mac"][s])), measure.block_bytes([x])[0])
    line = {"tool": TOOL, "mode": "host-path", "params": PARAM_TOY.name, "lib": args.lib or "the tree's", "version": server.engine._lib.fheaes_version().decode(),
            "steps": args.steps, "warmup": args.warmup, "all_verified": bool(ok), "variants": {k: measure.row(t) for k, t in times.items()}}
    measure.emit(line, args.out)
    return measure.exit_code(bool(ok))


def main() -> int:
    ap = measure.arg_parser(reps=20)
    ap.add_argument("--host-path", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.host_path:
        return host_path(args)
    p, n = PARAM_OPT, N_MSG
    client, eng = measure.session(0xAE5CC01)
    rng = np.random.default_rng(0x38C)
    keys = [rng.bytes(16) for _ in range(N_KEYS)]
    d_rk = torch.empty((N_KEYS, 11, 16, 8, p.big1), dtype=torch.int64, device="cuda")
    eng.aes_key_expansion_batch(to_dev(np.stack([client.encrypt_aes_key(k) for k in keys])), 128, N_KEYS, d_rk)
    eng.synchronize()
    eng.reserve(4 * n * 128)

    clear = [(i % N_KEYS, rng.bytes(12), rng.bytes(AAD_BYTES), rng.bytes(PAYLOAD_BYTES)) for i in range(n)]
    messages = []
    for k, nonce, aad, payload in clear:
        out = aes_clear.ccm_encrypt(keys[k], nonce, aad, payload, TAG_BYTES)
        messages.append((k, nonce, aad, out[:-TAG_BYTES], out[-TAG_BYTES:]))
    a = ccm_args(messages)
    total = a["block_of_message"][-1]
    plan = _native.aes_mac_plan([h - 1 + (b + 15) // 16 for h, b in zip(a["head_blocks"], a["payload_bytes"])], [(b + 15) // 16 for b in a["payload_bytes"]])
    assert plan["steps"] == STEPS_OF_CHAIN and plan["n_active"] == [n] * STEPS_OF_CHAIN and plan["public_blocks"] == 4 * n

    # the call's public batch, as one older call takes it
    pub_keys, pub_blocks, pub_data, pub_want = [], [], [], []
    for k, nonce, aad, ct, tag in messages:
        b0, _, ctr = aes_clear.ccm_blocks(nonce, aad, len(ct), len(tag))
        pub_keys += [k] * 4
        pub_blocks += [b0] + ctr
        pub_data += [0, 0] + [int.from_bytes(ct[i:i + 16], "big") for i in (0, 16)]
        pub_want += [aes_clear.aes_encrypt_block(keys[k], b) ^ d for b, d in zip(pub_blocks[-4:], pub_data[-4:])]
    step_keys = [m[0] for m in messages]
    step_blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    d_step0 = to_dev(client.trivial_bytes(measure.block_bytes(step_blocks)))
    ne0_bytes = rng.integers(0, 4, 16 * n).astype(np.uint8)                   # a quarter of them 0
    eq0_values = rng.integers(0, 2, n).astype(np.uint64) * rng.integers(1, 1 << 16, n).astype(np.uint64)
    d_ne0_in = to_dev(client.trivial_bytes(ne0_bytes))
    eq0_bits = ((eq0_values[:, None] >> np.arange(16, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    d_eq0_in = to_dev(client.trivial_bytes(eq0_bits)[:, :, 0, :])             # bit 0 of a trivial byte: [n][16][kN+1]
    d_ne0 = to_dev(_native.gen_lut(8, (np.arange(256) != 0).astype(np.uint64))[None])
    d_eq0 = to_dev(_native.gen_lut(16, (np.arange(1 << 16) == 0).astype(np.uint64))[None])

    blocks = lambda k: torch.empty((k, 16, 8, p.big1), dtype=torch.int64, device="cuda")  # noqa: E731
    d_pt, d_valid = blocks(total), torch.empty((n, p.big1), dtype=torch.int64, device="cuda")
    d_pub, d_step = blocks(4 * n), blocks(n)
    d_ne0_out = torch.empty((16 * n, 1, 8, p.big1), dtype=torch.int64, device="cuda")
    d_eq0_out = torch.empty((n, 1, 16, p.big1), dtype=torch.int64, device="cuda")

    def ccm_call(x, pt, valid):
        eng.aes_ccm_open_keyed(d_rk, 128, N_KEYS, x["key_of_stream"], x["head_blocks"], x["head"], x["ctr0"], x["payload_bytes"], x["ciphertext"], x["tags"],
                               x["tag_bytes"], pt, valid)

    nothing = lambda: None  # noqa: E731
    jobs = {
        "ccm": (lambda: ccm_call(a, d_pt, d_valid), nothing),
        "public256": (lambda: eng.aes_public_keyed(d_rk, 128, N_KEYS, pub_keys, pub_blocks, pub_data, d_pub), nothing),
        "keyed64": (lambda: eng.aes_encrypt_keyed(d_rk, 128, N_KEYS, step_keys, d_step, n), lambda: d_step.copy_(d_step0)),
        "ne0": (lambda: eng.wopbs_batch(d_ne0_in, 16 * n, 8, d_ne0, 1, False, d_ne0_out), nothing),
        "eq0": (lambda: eng.wopbs_batch(d_eq0_in, n, 16, d_eq0, 1, False, d_eq0_out), nothing),
    }
    times = measure.wall(eng, jobs, args.warmup, args.steps, on_step=lambda i, of, s: progress(TOOL, "step %d of %d: %.1f s" % (i, of, s)))

    # every output decrypted and compared
    payloads = client.decrypt_bytes(host(d_pt)).reshape(n, PAYLOAD_BYTES)
    wrong = [i for i in range(n) if bytes(payloads[i].tolist()) != clear[i][3]]
    valid = client.decrypt_bits(host(d_valid)).tolist()
    verified = {"ccm": not wrong and valid == [1] * n,
                "public256": np.array_equal(client.decrypt_bytes(host(d_pub)), measure.block_bytes(pub_want)),
                "keyed64": np.array_equal(client.decrypt_bytes(host(d_step)),
                                          measure.block_bytes([aes_clear.aes_encrypt_block(keys[k], b) for k, b in zip(step_keys, step_blocks)])),
                "ne0": client.decrypt_bits(host(d_ne0_out))[:, 0, 0].tolist() == (ne0_bytes != 0).astype(int).tolist(),
                "eq0": client.decrypt_bits(host(d_eq0_out))[:, 0, 0].tolist() == (eq0_values == 0).astype(int).tolist()}
    # `valid` the other way: a tag bit flipped in every fourth message, a ciphertext bit in every fourth from 2 on
    bad = list(messages)
    for i in range(0, n, 4):
        k, nonce, aad, ct, tag = bad[i]
        bad[i] = (k, nonce, aad, ct, tag[:-1] + bytes([tag[-1] ^ 1]))
    for i in range(2, n, 4):
        k, nonce, aad, ct, tag = bad[i]
        bad[i] = (k, nonce, aad, ct[:20] + bytes([ct[20] ^ 0x40]) + ct[21:], tag)
    d_pt2, d_valid2 = torch.empty_like(d_pt), torch.empty_like(d_valid)
    ccm_call(ccm_args(bad), d_pt2, d_valid2)
    eng.synchronize()
    valid_bad = client.decrypt_bits(host(d_valid2)).tolist()
    verified["ccm_rejects"] = valid_bad == [0 if i % 2 == 0 else 1 for i in range(n)]
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

    # (b) the link kernel against the XTS whitening: 64 blocks out, the state and one more block in per word, in place
    d_state, d_other = blocks(n), blocks(n)
    d_state.copy_(d_pub[:n]); d_other.copy_(d_pub[n:2 * n])
    torch.cuda.synchronize()
    before = host(d_state[:2]) + host(d_other[:2])
    ident, sixteen, zeros = list(range(n)), [16] * n, np.zeros((n, 16), dtype=np.uint8)
    eng.mac_link(d_state, False, None, d_other, ident, sixteen, zeros)
    eng.synchronize()
    all_ok = all_ok and np.array_equal(host(d_state[:2]), before)
    ev = measure.events(eng, {"link": lambda: eng.mac_link(d_state, False, None, d_other, ident, sixteen, zeros),
                              "whiten": lambda: eng.xts_whiten(d_state, d_state, d_other, ident, zeros)}, args.warmup, args.steps, args.reps)
    link_ms, whiten_ms = float(np.median(ev["link"])), float(np.median(ev["whiten"]))
    out_bytes = n * 128 * p.big1 * 8

    T = lambda name: rows[name]["ms_median"]  # noqa: E731
    checks = {"ccm": measure.check(T("ccm"), T("public256") + STEPS_OF_CHAIN * T("keyed64") + T("ne0") + T("eq0"), 1.03),
              "link_kernel_against_the_xts_whitening": {**measure.check(link_ms, whiten_ms, 1.5), "output_bytes": out_bytes,
                                                        "link_kernel_GB_per_s_written": round(out_bytes / link_ms / 1e6, 1),
                                                        "ms_all": [round(v, 4) for v in ev["link"]], "whiten_ms_all": [round(v, 4) for v in ev["whiten"]]}}
    for name, c in checks.items():
        progress(TOOL, "%s: %.3f ms, predicted %.3f ms, ratio %.4f" % (name, c["measured_ms"], c["predicted_ms"], c["ratio"]))
    line = {**measure.header(TOOL, args), "messages": n, "keys": N_KEYS, "aad_bytes": AAD_BYTES, "payload_bytes": PAYLOAD_BYTES, "tag_bytes": TAG_BYTES,
            "all_verified": bool(all_ok), "valid_on_the_messages_as_sent": valid.count(1), "valid_after_flipped_bits": valid_bad.count(1),
            "checks": checks, "plan": plan, "variants": rows,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, every job once in every step of one loop; ccm is "
                    "predicted from aes_public_keyed on its 256 public blocks + 3 x aes_encrypt_keyed on 64 blocks + the two WoPBS of the tag check; the link "
                    "kernel and the XTS whitening (64 blocks in place, one more block read per word) are timed with device events around --reps calls of "
                    "each, alternating"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(bool(all_ok), all(c["within_bound"] is not False for c in checks.values()))


if __name__ == "__main__":
    sys.exit(main())
