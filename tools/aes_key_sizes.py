"""The three FIPS-197 key sizes side by side at PARAM_OPT on one GPU, on resident device tensors:

  AES-128  Nr = 10 rounds  fheaes_aes_key_expansion / _encrypt / _decrypt / _decryption_round_keys / _decrypt_equivalent
  AES-192  Nr = 12         the five fheaes_aes_*_bits entry points with key_bits = 192
  AES-256  Nr = 14         ... with key_bits = 256

Per key size: the time of the key expansion (a chain of 40 / 46 / 52 new words, 50 / 54 / 65 dependent 32-bit WoPBS with the SubWords)
and of the round-key conversion of the equivalent inverse cipher (recorded without a target), and for each batch size blocks/s of aes_encrypt, aes_decrypt_equivalent (Nr x 128 bit circuit bootstraps per
block each) and aes_decrypt ((2 Nr - 1) x 128).  Every round is the same launch sequence whatever Nr is, so the time of a call should be
Nr / 10 (aes_decrypt: (2 Nr - 1) / 19) times that of the AES-128 entry point measured in the same process: `ratio_to_128`, `expected`
and `within_3_percent` record it.  The key sizes ALTERNATE inside the timed loop (step i runs 128, 192, 256 one after the other), so a
drift of the clocks meets all three alike.

Warm-up, then the median of --steps timed calls (wall clock around the call and a synchronize); every block of every output is
decrypted with the client key and compared with FIPS-197 arithmetic (aes_clear): a wrong block makes the tool exit 1.  One further call
per measurement runs with the per-stage profile on (HIP events around every launch, so kept out of the timed calls).  Prints one JSON
line (--out: also written there).

    python tools/aes_key_sizes.py [--blocks 32,128] [--steps 5] [--warmup 1] [--out FILE]
"""
from __future__ import annotations

import sys

import numpy as np
import torch

import measure
from measure import block_bytes, host, to_dev
from tfhe_aes_amd import PARAM_OPT, aes_clear

# FIPS-197 appendix A.1 / A.2 / A.3
KEYS = {128: bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"),
        192: bytes.fromhex("8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b"),
        256: bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")}
NR = {128: 10, 192: 12, 256: 14}
SIZES = (128, 192, 256)
IV = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
MASK128 = (1 << 128) - 1


def ratios(rows: dict, expected: dict) -> None:
    """adds ratio_to_128 / expected / within_3_percent to the rows of one measurement, {key size: row with ms_median}"""
    base = rows[128]["ms_median"]
    for bits, row in rows.items():
        row["ratio_to_128"] = round(row["ms_median"] / base, 4)
        if expected is not None:
            row["expected"] = round(expected[bits], 4)
            row["within_3_percent"] = bool(abs(row["ratio_to_128"] / expected[bits] - 1) <= 0.03)


def main() -> int:
    args = measure.arg_parser(blocks="32,128").parse_args()
    batch_sizes = [int(x) for x in args.blocks.split(",")]
    p = PARAM_OPT

    client, eng = measure.session(0xAE50001, IV, int.from_bytes(KEYS[128], "big"))

    # the entry points: AES-128 through the ones without a key-size argument (the yardstick), the others through *_bits
    def entry(name, bits):
        if bits == 128:
            return getattr(eng, name)
        fn = getattr(eng, name + "_bits")
        return lambda keys_d, *rest: fn(keys_d, bits, *rest)

    all_ok = True
    d_ek = {bits: to_dev(client.encrypt_aes_key(KEYS[bits])) for bits in SIZES}
    d_rk = {bits: torch.empty((NR[bits] + 1, 16, 8, p.big1), dtype=torch.int64, device="cuda") for bits in SIZES}
    d_dw = {bits: torch.empty_like(d_rk[bits]) for bits in SIZES}
    clear_rk = {bits: aes_clear.expand_key(KEYS[bits]) for bits in SIZES}

    # ---- once per AES key: the expansion and the conversion to the equivalent inverse cipher's round keys ----
    # every step of a loop runs the three key sizes one after the other
    per_key = {}
    for name, src, dst, want in (
            ("key_expansion", d_ek, d_rk, clear_rk),
            ("decryption_round_keys", d_rk, d_dw, {b: aes_clear.inv_mix_columns_round_keys(clear_rk[b]) for b in SIZES})):
        jobs = {b: ((lambda b=b: entry("aes_" + name, b)(src[b], dst[b])), lambda: None) for b in SIZES}
        ts = measure.wall(eng, jobs, args.warmup, args.steps)
        rows = {}
        for b in SIZES:
            ok = bool(np.array_equal(client.decrypt_bytes(host(dst[b])), np.array(want[b], dtype=np.uint8)))
            all_ok = all_ok and ok
            rows[b] = {**measure.row(ts[b]), "verified_vs_fips197": ok, "stages_ms": measure.stage_ms(measure.profiled(eng, jobs[b][0]))}
            if name == "key_expansion":
                nk = NR[b] - 6
                rows[b]["new_words"] = 4 * (NR[b] + 1) - nk
                # the chain: one identity WoPBS per new word and one S-Box WoPBS per SubWord, 32 bits each, every one waiting for the last
                rows[b]["dependent_wopbs"] = rows[b]["new_words"] + sum(1 for i in range(nk, 4 * (NR[b] + 1)) if i % nk == 0 or (nk > 6 and i % nk == 4))
                rows[b]["bit_cbs"] = 32 * rows[b]["dependent_wopbs"]
            else:
                rows[b]["bit_cbs"] = 2 * (NR[b] - 1) * 128
        ratios(rows, None)                  # recorded without a target: neither is a multiple of one round
        per_key[name] = {str(b): rows[b] for b in SIZES}
        measure.progress("aes_key_sizes", "%s: %s ms" % (name, " / ".join("%.1f" % rows[b]["ms_median"] for b in SIZES)))

    # ---- per batch size: the three block operations ----
    results = {}
    for n in batch_sizes:
        pts = [(IV + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
        want_pt = block_bytes(pts)
        want_ct = {b: block_bytes([aes_clear.aes_encrypt_block(KEYS[b], v) for v in pts]) for b in SIZES}
        d_pt = to_dev(np.stack([client.encrypt_u128(v) for v in pts]))
        d_ct = {b: to_dev(np.stack([client.encrypt_bytes(row) for row in want_ct[b]])) for b in SIZES}
        eng.reserve(n * 128)
        st = {b: torch.empty_like(d_pt) for b in SIZES}
        row_n = {}
        for name, keys_d, inputs, want, per_block in (
                ("aes_encrypt", d_rk, {b: d_pt for b in SIZES}, want_ct, lambda nr: nr * 128),
                ("aes_decrypt_equivalent", d_dw, d_ct, {b: want_pt for b in SIZES}, lambda nr: nr * 128),
                ("aes_decrypt", d_rk, d_ct, {b: want_pt for b in SIZES}, lambda nr: (2 * nr - 1) * 128)):
            jobs = {b: ((lambda b=b: entry(name, b)(keys_d[b], st[b], n)), (lambda b=b: st[b].copy_(inputs[b]))) for b in SIZES}
            ts = measure.wall(eng, jobs, args.warmup, args.steps)
            rows = {}
            for b in SIZES:
                got = client.decrypt_bytes(host(st[b]))
                wrong = [i for i in range(n) if not np.array_equal(got[i], want[b][i])]
                all_ok = all_ok and not wrong
                rows[b] = {**measure.row(ts[b], n), "bit_cbs_per_block": per_block(NR[b]), "blocks_verified": n - len(wrong), "wrong_blocks": wrong,
                           "stages_ms": measure.stage_ms(measure.profiled(eng, *jobs[b]))}
            ratios(rows, {b: per_block(NR[b]) / per_block(10) for b in SIZES})
            row_n[name] = {str(b): rows[b] for b in SIZES}
            measure.progress("aes_key_sizes", "%d blocks, %s: %s blocks/s, ratios %s" % (
                n, name, " / ".join("%.2f" % rows[b]["blocks_per_s"] for b in SIZES), " / ".join("%.3f" % rows[b]["ratio_to_128"] for b in SIZES)))
        results[str(n)] = row_n
        del d_pt, d_ct, st

    line = {**measure.header("aes_key_sizes", args), "all_verified": all_ok,
            "key_expansion": per_key["key_expansion"], "decryption_round_keys": per_key["decryption_round_keys"], "blocks": results,
            "note": "wall clock per call on resident tensors (call + synchronize), median of the timed steps, the key sizes alternating "
                    "inside every step; AES-128 runs through the entry points without a key-size argument; ratio_to_128 = ms_median / "
                    "ms_median of AES-128 in this run, expected = Nr / 10 (aes_decrypt: (2 Nr - 1) / 19), none for the two once-per-key operations; "
                    "stages_ms from one further profiled call (HIP events around every launch)"}
    measure.emit(line, args.out)
    eng.close()
    return measure.exit_code(all_ok)


if __name__ == "__main__":
    sys.exit(main())
