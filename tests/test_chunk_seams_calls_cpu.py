"""The shapes of test_gpu_chunk_seams_calls.py without a GPU: the conditions that keep its tests from silently becoming one-chunk tests.
Every figure is derived in chunk_seams.py (part G) by restating the engine's rule in plain Python and is held here to the host-only plan
entry points (fheaes_aes_cmac_plan, fheaes_aes_mac_plan, fheaes_aes_public_plan_keyed, fheaes_aes_kw_plan, fheaes_gate_plan) and to the
hand counts.  Each shape is shown to cross its seam, and the shape one smaller not to."""
import numpy as np

import chunk_seams as cs
import keywrap
from tfhe_aes_amd import PARAM_TOY, _native, aes_clear


def _launches(parts):
    return {name: v[0] for name, v in parts.items()}


# ---- the constants ---------------------------------------------------------------------------------------------------------------------------
def test_gate_constants_are_the_plans():
    assert PARAM_TOY.k == 1 and _native.gate_plan([1], PARAM_TOY.k) == {"workgroups": 1, "instances_per_workgroup": cs.GATE_R}
    assert _native.gate_plan([1], 4)["instances_per_workgroup"] == 3
    assert cs.GATE_MAX_GRID == 65536 and cs.GATE_ROW_PERIOD == 7 and cs.GATE_R % cs.GATE_ROW_PERIOD and cs.GATE_ROW_PERIOD % 2
    for runs in ([1], [0], [8, 9, 0, 17], [0, 0, 1], cs.GATE_GRID_RUNS, cs.gate_boot_runs(), cs.gate_packed_runs()):
        assert cs.gate_workgroups(runs) == len(cs.gate_table(runs)) == _native.gate_plan(runs, PARAM_TOY.k)["workgroups"], runs[:4]
    assert cs.gate_workgroups([7, 0, 4], 3) == _native.gate_plan([7, 0, 4], 4)["workgroups"] == 5


# ---- A. CMAC subkeys of 257 keys --------------------------------------------------------------------------------------------------------------
def _subkey_plan(m):
    return _native.aes_public_plan_keyed([0] * m, list(range(m)), m)


def test_257_keys_put_one_key_behind_every_seam_of_the_subkey_call():
    m = cs.CMAC_KEYS
    assert m == cs.SLOTS_PER_PASS + 1 == cs.CHUNK_BYTES // 16 + 1 and cs.CMAC_VECTOR_KEY == m - 1 and set(cs.CMAC_KEYS_ALONE) == {0, 127, 128, 255, 256}
    plan = _subkey_plan(m)
    assert plan == [16 * m] * 10 and 16 * m == 4112 > cs.CHUNK_BYTES            # zero blocks under distinct keys share nothing, round 1 included
    parts = cs.cmac_keyswitch(plan, m, [])
    assert _launches(parts) == {"chain": 0, "public_rounds": 20, "refresh_l": 2, "refresh_k": 3}
    assert 16 * m - cs.CHUNK_BYTES == 16 and 32 * m - 2 * cs.CHUNK_BYTES == 32    # key 256 alone in the last chunk of both refreshes
    assert 256 * m == 65792                                                     # workgroups of bit_rows_kernel<CmacRows>
    one_less = cs.cmac_keyswitch(_subkey_plan(m - 1), m - 1, [])
    assert _launches(one_less) == {"chain": 0, "public_rounds": 10, "refresh_l": 1, "refresh_k": 2}


# ---- B. CMAC over 257 streams -----------------------------------------------------------------------------------------------------------------
def test_cmac_streams_name_257_of_259_keys_and_reach_subkey_513():
    n = cs.CMAC_STREAMS
    keys = [cs.cmac_key_of_stream(s) for s in range(n)]
    named = sorted(set(keys))
    assert len(named) == n == cs.CMAC_STORE_KEYS - 2 and not set(cs.CMAC_UNNAMED) & set(named) and keys != sorted(keys)
    at = {k: i for i, k in enumerate(named)}                                    # the compaction of the keys a call names
    assert any(at[k] != k for k in named) and at[cs.CMAC_STORE_KEYS - 1] == 256 and at[4] == 4 and at[6] == 5 and at[131] == 129
    lens = [cs.cmac_message_bytes(s) for s in range(n)]
    b = [2 * at[keys[s]] + (0 if lens[s] and lens[s] % 16 == 0 else 1) for s in range(n)]
    assert max(b) == 513 and len(set(b)) == n and sum(1 for v in b if v > 511) == 1      # one stream a key; key 258's stream takes its K2
    assert len({keys[s] for s in cs.CALL_ALONE}) == 4


def test_cmac_lengths_tags_and_live_prefixes():
    n = cs.CMAC_STREAMS
    lens = [cs.cmac_message_bytes(s) for s in range(n)]
    assert (lens[0], lens[255], lens[256], lens[100]) == (48, 0, 48, 17) and lens[2] == 16 and 0 < lens[1] < 16
    assert all(v == 16 for s, v in enumerate(lens) if s % 2 == 0 and s not in cs.CMAC_LENGTHS)
    assert all(0 < v < 16 for s, v in enumerate(lens) if s % 2 == 1 and s not in cs.CMAC_LENGTHS)
    assert {cs.cmac_tag_bytes(s) for s in range(n)} == set(range(4, 17))
    blocks = cs.cmac_chain_blocks()
    plan = _native.aes_cmac_plan(lens)
    assert plan == {"steps": 3, "chained_blocks": sum(blocks), "padded_streams": sum(1 for v in lens if v == 0 or v % 16)}
    assert _native.aes_mac_plan(blocks)["n_active"] == cs.live_prefixes(blocks) == [257, 3, 2]
    assert cs.live_prefixes(blocks[:256]) == [256, 2, 1]                        # 256 streams: the first pass fits one chunk


def test_cmac_keyswitch_counts():
    n, n_active = cs.CMAC_STREAMS, cs.live_prefixes(cs.cmac_chain_blocks())
    plan = _subkey_plan(n)
    verify = cs.cmac_keyswitch(plan, n, n_active, n)
    assert _launches(verify) == {"chain": 20 + 10 + 10, "public_rounds": 20, "refresh_l": 2, "refresh_k": 3, "tag_bytes": 2, "tag_tree": 3}
    assert cs.total(verify)[0] == 70
    assert cs.total(cs.cmac_keyswitch(plan, n, n_active))[0] == 65              # the call that returns the tags
    assert cs.total(cs.cmac_keyswitch(None, 0, n_active, n))[0] == 45           # with the caller's subkeys
    assert cs.total(verify)[1] == 8 * (10 * 16 * n + 16 * n + 32 * n + 10 * 16 * sum(n_active) + 16 * n) + 16 * n
    small = cs.cmac_keyswitch(_subkey_plan(256), 256, [256, 2, 1], 256)
    assert _launches(small) == {"chain": 30, "public_rounds": 10, "refresh_l": 1, "refresh_k": 2, "tag_bytes": 1, "tag_tree": 2}


def test_the_rejected_streams_and_keys_are_not_periodic_in_128_or_256():
    # key 256 of the unwrap is valid like key 0 (it holds the RFC vector): there the KEK and the payload are what differs across 256
    for bad, n, shifts in ((cs.CMAC_BAD, cs.CMAC_STREAMS, (128, 256)), (cs.KW_BAD, cs.KW_KEYS, (128,))):
        assert {1, 127, 129, 255} <= set(bad) and 0 not in bad
        pattern = [i in bad for i in range(n)]
        for shift in shifts:
            assert any(pattern[i] != pattern[i - shift] for i in range(shift, n))
            assert any(pattern[i] != pattern[i % shift] for i in range(n))
    assert 256 in cs.CMAC_BAD and cs.CMAC_BAD_MESSAGE == 256 and cs.cmac_message_bytes(256) > 0 and len(cs.CMAC_BAD) == 11
    assert 256 not in cs.KW_BAD and len(cs.KW_BAD) == 10 and cs.KW_WRONG_KEK not in cs.KW_BAD


# ---- C. key unwrap of 257 keys ------------------------------------------------------------------------------------------------------------------
def test_kw_shape_crosses_the_link_the_cipher_and_the_refresh():
    n_keys, n = cs.KW_KEYS, cs.KW_SEMIBLOCKS
    kek = cs.kw_kek_of_key()
    assert len(kek) == n_keys and set(kek) == {0, 1, 2} and kek[256] == 0 and kek[0] != 0 and kek[255] != 0 and kek[127] != kek[128]
    assert all(kek[j] != kek[j - 128] for j in range(128, 256))
    assert (4 * n_keys, (4 * n_keys + 31) // 32 * 32) == (1028, 1056)          # the KEK table the wrapped bytes lie behind
    assert n_keys == cs.SLOTS_PER_PASS + 1 and 8 * n * n_keys == 4112 and 8 * n * n_keys - cs.CHUNK_BYTES == 8 * n
    parts = cs.kw_keyswitch()
    assert _launches(parts) == {"cipher": 12 * 10 * 2, "refresh": 2, "tag_bytes": 2, "tag_tree": 3} and cs.total(parts)[0] == 247
    plan = _native.aes_kw_plan(128, n, n_keys)
    assert plan["steps"] == 6 * n == 12 and plan["cipher_blocks"] == 12 * n_keys
    assert 8 * plan["byte_wopbs"] == parts["cipher"][1] + parts["refresh"][1] + parts["tag_bytes"][1]
    less = cs.kw_keyswitch(n_keys - 1)
    assert _launches(less) == {"cipher": 120, "refresh": 1, "tag_bytes": 1, "tag_tree": 2}
    # in windows of 200 blocks: 10 x 257 block-rounds a pass are 13 windows, all but the first across two steps or from a block above 0
    windowed = cs.kw_keyswitch(window=cs.WINDOW)
    k2, k1 = cs.window_launches(n_keys, 10, cs.WINDOW)
    assert (k2, k1) == (13, 22) and windowed["cipher"] == (12 * 22, parts["cipher"][1]) and cs.kw_keyswitch(1, window=cs.WINDOW)["cipher"][0] == 120


def test_the_numpy_key_wrap_is_aes_clears():
    """keywrap.wrap_many makes the 257 blobs of the GPU test (3,084 block encryptions) in numpy; here it is aes_clear.key_wrap"""
    rng = np.random.default_rng(0xC9)
    for size in (16, 24, 32):
        keys = [rng.bytes(size) for _ in range(5)]
        blocks = [rng.bytes(16) for _ in range(5)]
        got = keywrap.np_encrypt_blocks([aes_clear.expand_key(k) for k in keys], [list(b) for b in blocks])
        want = [aes_clear.aes_encrypt_block(k, int.from_bytes(b, "big")) for k, b in zip(keys, blocks)]
        assert [int.from_bytes(bytes(g.tolist()), "big") for g in got] == want
    for name in keywrap.VECTORS:
        kek, payload, wrapped = keywrap.vector(name)
        assert keywrap.wrap_many([kek], [0], [payload]) == [wrapped], name
    keks = [rng.bytes(16) for _ in range(3)]
    for n in (2, 3, 8):
        payloads, kek_of = [rng.bytes(8 * n) for _ in range(7)], [0, 2, 1, 1, 0, 2, 2]
        assert keywrap.wrap_many(keks, kek_of, payloads) == [aes_clear.key_wrap(keks[k], d) for k, d in zip(kek_of, payloads)]


# ---- D. the gate kernel behind GATE_MAX_GRID ------------------------------------------------------------------------------------------------------
def test_gate_grid_runs_put_a_ragged_workgroup_first_in_the_second_launch():
    runs = cs.GATE_GRID_RUNS
    assert runs == [8 * 65536 + 3, 0, 9, 1] and sum(runs) == 524301
    assert _native.gate_plan(runs, 1)["workgroups"] == cs.gate_workgroups(runs) == 65540 and cs.gate_launches(runs) == [2]
    tab = cs.gate_table(runs)
    assert tab[65535] == (8 * 65535, 0, 8) and tab[65536] == (8 * 65536, 0, 3)   # the first workgroup of the second launch: gate 0's ragged last
    assert tab[65537:] == [(8 * 65536 + 3, 2, 8), (8 * 65536 + 11, 2, 1), (8 * 65536 + 12, 3, 1)]
    # one instance fewer in gate 0: still 65,540 workgroups in two launches, the same workgroup leading the second with 2 instances
    fewer = [runs[0] - 1] + runs[1:]
    assert _native.gate_plan(fewer, 1)["workgroups"] == 65540 and cs.gate_table(fewer)[65536] == (8 * 65536, 0, 2)
    # the cut itself: 65,536 workgroups are one launch, one instance more a second one
    assert cs.gate_launches([8 * 65536]) == [1] and cs.gate_launches([8 * 65536 + 1]) == [2]
    assert cs.gate_launches([8 * 65533, 0, 9, 1]) == [1] and cs.gate_workgroups([8 * 65533, 0, 9, 1]) == 65536
    assert len({i % 8 for i in range(0, 56, 7)}) == 8                             # a row period of 7 meets every slot of a workgroup


# ---- E. both gate seams in one bootstrapped call ---------------------------------------------------------------------------------------------------
def test_gate_boot_runs_cross_the_chunk_and_the_grid_cut_inside_chunk_1():
    runs, chunk = cs.gate_boot_runs(), cs.MAX_CHUNK_BITS
    assert len(runs) == chunk + 1 == 32769 and runs[0] == 8 * 32771 and runs[-4:] == [1, 1, 0, 9] and set(runs[1:-4]) == {1}
    per_chunk = [cs.gate_workgroups(runs[:chunk]), cs.gate_workgroups(runs[chunk:])]
    assert per_chunk == [32771 + 32766, 2] == [65537, 2] and cs.gate_launches(runs, chunk=chunk) == [2, 1]
    assert _native.gate_plan(runs, 1)["workgroups"] == 65539
    tab = cs.gate_table(runs, chunk=chunk)
    assert tab[65535][1:] == (32765, 1) and tab[65536][1:] == (32766, 1)         # the grid cut inside chunk 1: between gates 32,765 and 32,766
    assert tab[65537:] == [(sum(runs) - 9, 0, 8), (sum(runs) - 1, 0, 1)]          # chunk 2: two workgroups, both naming gate 0 of the workspace
    # 8 instances fewer in gate 0: chunk 1 is one launch of exactly 65,536 workgroups
    less = cs.gate_boot_runs(cs.GATE_BOOT_HEAD - 8)
    assert cs.gate_workgroups(less[:chunk]) == 65536 and cs.gate_launches(less, chunk=chunk) == [1, 1]
    assert cs.gate_launches(runs[:chunk], chunk=chunk) == [2]                     # and one gate fewer is one chunk
    packed = cs.gate_packed_runs()
    assert len(packed) == 32769 and packed[-3:] == [1, 0, 2] and sum(packed) == 32769 and cs.gate_launches(packed, chunk=chunk) == [1, 1]
    assert cs.gate_table(packed, chunk=chunk)[-2:] == [(32766, 32766, 1), (32767, 0, 2)]
