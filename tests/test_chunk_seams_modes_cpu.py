"""The shapes of test_gpu_chunk_seams_modes.py without a GPU: the conditions that keep its tests from silently becoming one-chunk tests.
Every figure is derived in chunk_seams.py by restating the engine's rule in plain Python and is held here to the host-only plan entry
points (fheaes_aes_xts_plan, fheaes_aes_mac_plan, fheaes_aes_public_plan_keyed, fheaes_xts_tweak_row) and to the hand counts."""
import chunk_seams as cs
import xts
from tfhe_aes_amd import PARAM_TOY, _native, aes_clear


def test_pass_and_chunk_constants():
    assert cs.BIG1_TOY == PARAM_TOY.big1 and cs.N == PARAM_TOY.N and PARAM_TOY.k == 1
    assert cs.slots_per_pass(cs.BIG1_TOY) == cs.SLOTS_PER_PASS == 256
    assert cs.slots_per_pass(4 * 512 + 1) == 256 and cs.slots_per_pass(9) == 16384 // 5        # 64 workgroups in x from 128 words a bit on
    assert cs.TWEAK_ROWS_PER_PASS == 8192 and cs.TAG_TREE_CHUNK == 128 and cs.TAG_BYTE_CHUNK == 256
    assert cs.WHITEN_BLOCKS == cs.LINK_SLOTS == 257 and cs.LINK_ENC == 259
    tab = cs.whiten_table()
    assert tab[256] not in (tab[0], tab[255]) and tab != sorted(tab)
    src, eb = cs.link_tables()
    assert (src[256], src[0], src[255]) == (0, 258, cs.MAC_NONE) and eb[256] == 5 and set(eb) == {0, 1, 5, 15, 16}
    assert all(v == cs.MAC_NONE or v < cs.LINK_ENC for v in src)


def test_wopbs_chunks_is_the_rule_of_the_older_seams():
    assert cs.wopbs_chunks(cs.PER_INPUT_N, cs.PER_INPUT_BITS, 1, 2) == 2 and cs.wopbs_chunks(cs.PER_INPUT_CHUNK, cs.PER_INPUT_BITS, 1, 2) == 1
    assert cs.wopbs_chunks(cs.TREE_N, cs.TREE_BITS, cs.TREE_LUTS, 2) == 2 and cs.wopbs_chunks(cs.TREE_CHUNK, cs.TREE_BITS, cs.TREE_LUTS, 2) == 1
    assert cs.wopbs_chunks(0, 8, 1, 2) == 0 and cs.wopbs_chunks(1, 16, 64, 5) == 1               # never less than one input a chunk


def test_the_two_tag_wopbs_of_257_messages_take_2_and_3_chunks():
    at = lambda n: (cs.wopbs_chunks(16 * n, 8, 1, PARAM_TOY.k + 1), cs.wopbs_chunks(n, 16, 1, PARAM_TOY.k + 1))
    assert at(cs.CCM_MESSAGES) == (2, 3) and at(256) == (1, 2)
    assert cs.CCM_MESSAGES == cs.TAG_BYTE_CHUNK + 1 == 2 * cs.TAG_TREE_CHUNK + 1


def test_68_units_of_122_offsets_are_the_first_to_pass_the_grid_cap():
    assert 67 * 122 * 128 < 1 << 20 <= 68 * 122 * 128
    assert (cs.TWEAK_UNITS, cs.TWEAK_OFFSETS) == (68, 122) and cs.TWEAK_OFFSETS == xts.MAX_OFFSET + 1
    assert cs.TWEAK_BLOCKS == 8296 and cs.TWEAK_BLOCKS * 128 == 1061888 and cs.TWEAK_SEAM == (67, 18)


def test_tweak_rows_17_to_19_are_the_rows_of_the_device_reference():
    for j in (17, 18, 19):
        want = xts.rows(j)
        for i in range(128):
            assert sorted(_native.xts_tweak_row(j, i)) == want[i], (j, i)


def test_xts_shape_crosses_the_plan_refresh_and_whitening_seams():
    pl = _native.aes_xts_plan(len(cs.XTS_SECTORS), cs.XTS_BPU, cs.XTS_FIRST, cs.XTS_BLOCKS)
    assert pl["segments"] == 2 and pl["tweak_refresh_bytes"] == 16 * 374
    units, rows = cs.xts_segment_rows()
    assert (units, rows) == (4, [1 + 242 + 121, 1 + 4 + 1]) and 16 * (units + sum(rows)) == pl["tweak_refresh_bytes"]
    assert 16 * rows[0] == 5824 > cs.CHUNK_BYTES >= 16 * rows[1]
    assert cs.XTS_BLOCKS > cs.SLOTS_PER_PASS and len(set(cs.XTS_SECTORS)) == 4
    assert (cs.XTS_FIRST + cs.XTS_BLOCKS - 1) // cs.XTS_BPU == 3 and (cs.XTS_FIRST + cs.XTS_BLOCKS - 1) % cs.XTS_BPU == 120
    parts = cs.xts_keyswitch(_native.aes_public_plan([aes_clear.xts_tweak_block(v) for v in cs.XTS_SECTORS]))
    assert [parts[k][0] for k in ("public_rounds", "refresh", "cipher")] == [10, 1 + 2 + 1, 10 * 2] and cs.total(parts)[0] == 34
    for bpu, first, n in ((256, 0, 512), (256, 119, 256), (123, 119, 4), (1, 5, 9)):           # the rule against the plan on other shapes
        units, rows = cs.xts_segment_rows(bpu, first, n)
        pl = _native.aes_xts_plan((first + n + bpu - 1) // bpu, bpu, first, n)
        assert (len(rows), 16 * (units + sum(rows))) == (pl["segments"], pl["tweak_refresh_bytes"])


def test_ccm_chain_lengths_give_the_live_prefixes_the_gpu_test_relies_on():
    lengths, payload = cs.ccm_stream_blocks()
    assert {i: lengths[i] for i in cs.CCM_LONG} == {0: 2, 127: 6, 128: 3, 255: 3, 256: 3} and sum(lengths) == 17 and sum(payload) == 8
    plan = _native.aes_mac_plan(lengths, payload)
    assert plan["n_active"] == cs.live_prefixes(lengths) == [5, 5, 4, 1, 1, 1]
    assert plan["public_blocks"] == 2 * cs.CCM_MESSAGES + 8 == 522 and 16 * plan["public_blocks"] > 2 * cs.CHUNK_BYTES
    assert cs.chain_keyswitch(plan["n_active"]) == (60, 8 * 16 * 10 * 17)
    assert {i: cs.CCM_LONG[i][1] % 16 for i in (128, 256)} == {128: 5, 256: 5}                  # a partial last block at 128 and 256
    assert sorted(t for _, _, t in cs.CCM_LONG.values()) == [4, 8, 10, 16, 16]
    keys = [cs.ccm_shape(i)[0] for i in range(cs.CCM_MESSAGES)]
    assert len({keys[0], keys[128], keys[256]}) == 3 and set(keys) == {0, 1, 2}
    assert all(keys[i] != keys[i - 128] for i in range(128, cs.CCM_MESSAGES)) and keys[256] != keys[0]     # the key changes across both seams


def test_the_rejected_positions_are_not_periodic_in_128_or_256():
    bad = set(cs.CCM_BAD)
    assert {1, 127, 129, 255, 256} <= bad and all(i in bad for i in range(37, cs.CCM_MESSAGES, 37)) and len(bad) == 11
    pattern = [i in bad for i in range(cs.CCM_MESSAGES)]
    for shift in (128, 256):
        assert any(pattern[i] != pattern[i - shift] for i in range(shift, cs.CCM_MESSAGES))
        assert any(pattern[i] != pattern[i % shift] for i in range(cs.CCM_MESSAGES))


def test_mac_streams_shrink_from_256_live_streams_to_2():
    lengths = cs.mac_lengths()
    assert len(lengths) == 257 and (lengths[0], lengths[1], lengths[255], lengths[256]) == (3, 1, 0, 3)
    assert _native.aes_mac_plan(lengths)["n_active"] == cs.live_prefixes(lengths) == [256, 2, 2]
    assert cs.chain_keyswitch([256, 2, 2]) == (30, 8 * 16 * 10 * 260)


def test_keyed_public_pools_are_one_chunk_in_round_1_and_two_from_round_2_on():
    blocks, kob, data = cs.public_keyed_blocks()
    assert len(blocks) == len(data) == cs.PUBLIC_BLOCKS and set(kob) == {0, 1, 2}
    assert len({kob[b] for b in cs.PUBLIC_ALONE}) > 1 and kob[255] != kob[256]
    first = len({(k, p, (b >> (8 * (15 - p))) & 0xFF) for b, k in zip(blocks, kob) for p in range(16)})
    for plan in (_native.aes_public_plan_keyed(blocks, kob, cs.PUBLIC_KEYS), _native.aes_decrypt_public_plan_keyed(blocks, kob, cs.PUBLIC_KEYS)):
        assert plan == [first] + [16 * cs.PUBLIC_BLOCKS] * 9 and first <= cs.CHUNK_BYTES < 16 * cs.PUBLIC_BLOCKS
        assert sum(cs.byte_wopbs(v)[0] for v in plan) == 1 + 2 * 9
