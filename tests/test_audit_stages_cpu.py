"""The audit of the key switches without a GPU: the four entry points' place in the header, the library and the binding and their
bad-argument codes, the Python side's choice of stages, and the numpy model of the plain form (audit_stages.py) pinned against
edge_words.keyswitch_plain / pfpks_plain and against the oracle at PARAM_TOY and PARAM_EDGE.  The model is the plain kernel's arithmetic
restated: balanced byte planes in B-fragment order, recombined, rows and columns bounded, the body term added -- so a wrong plane order, a
lost carry or a missing bound shows here before any kernel runs."""
import ctypes
import re

import numpy as np
import pytest

import audit_stages as st
import edge_words as ew
from edge_words import PARAM_EDGE
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_TOY, _build, _native, server

NAMES = ("fheaes_audit_stage_set", "fheaes_audit_stage_read", "fheaes_audit_stage_debug", "fheaes_audit_plain_batch")
M = 6


def header_text():
    return re.sub(r"/\*.*?\*/", "", (_build.ROOT / "include" / "fheaes.h").read_text(), flags=re.S)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_four_names_are_declared_exported_and_bound():
    text, lib = header_text(), _native.load_library()
    for name in NAMES:
        assert name in _native.SIGNATURES and name in _native.header_symbols() and hasattr(lib, name)
        args = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, text).group(1)
        assert len(args.split(",")) == len(_native.SIGNATURES[name][1]), name
        assert "memspace" not in args, name                    # three are configuration; the hook takes device pointers only and stages nothing
    for method in ("audit_stage_set", "audit_stage_read", "audit_stage_debug", "audit_plain_batch"):
        assert callable(getattr(_native.Engine, method))
    assert _native.AUDIT_STAGES == st.STAGES and [_native.STAGES.index(s) for s in st.STAGES] == [st.STAGE_NO[s] for s in st.STAGES] == [0, 1, 2]
    for s, no in st.STAGE_NO.items():
        assert re.search(r"#define\s+FHEAES_STAGE_%s\s+%d\b" % ({"keyswitch": "KEYSWITCH", "blind_rotate": "BLIND_ROTATE", "pfpks": "PFPKS"}[s], no), text)


def test_a_null_context_is_refused_by_each():
    lib = _native.load_library()
    u64 = ctypes.c_uint64
    a, b, c, n = u64(), u64(), u64(), u64()
    rec = (u64 * (5 * _native.AUDIT_RECORDS))()
    buf = (u64 * 8)()
    for stage in (0, 1, 2, 3, -1):
        for rows in (0, 1, 256, 257):
            assert lib.fheaes_audit_stage_set(None, stage, rows, 0, 1) == -1
        assert lib.fheaes_audit_stage_read(None, stage, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), rec, _native.AUDIT_RECORDS, ctypes.byref(n)) == -1
        assert lib.fheaes_audit_stage_read(None, stage, None, None, None, None, 0, None) == -1
        assert lib.fheaes_audit_stage_debug(None, stage, 0, 0, 1) == -1
        for block in (-1, 0):
            assert lib.fheaes_audit_plain_batch(None, stage, buf, 1, block, buf) == -1
    assert (a.value, b.value, c.value, n.value) == (0, 0, 0, 0)


# ---- the Python side ------------------------------------------------------------------------------------------------------------------------
class FakeEngine:
    def __init__(self):
        self.calls = []

    def audit_set(self, *a):
        self.calls.append(("audit_set",) + a)

    def audit_stage_set(self, *a):
        self.calls.append(("audit_stage_set",) + a)


def fake_server():
    srv = server.Server.__new__(server.Server)
    srv.engine, srv._audit_stages = FakeEngine(), ()
    return srv


def test_the_default_audit_makes_exactly_the_blind_rotation_s_call():
    srv = fake_server()
    srv.audit(rows=32, min_bits=5, seed=7)
    srv.audit(rows=0)
    assert [c[:3] for c in srv.engine.calls] == [("audit_set", 32, 5), ("audit_set", 0, 0)] and srv.engine.calls[0][3] == 7
    assert srv._audit_stages == ()


def test_stages_are_passed_on_in_the_order_they_run_and_turned_off_again():
    srv = fake_server()
    srv.audit(rows=64, seed=9, stages=("pfpks", "keyswitch", "blind_rotate"))
    assert srv.engine.calls == [("audit_set", 64, 0, 9), ("audit_stage_set", "keyswitch", 64, 0, 9), ("audit_stage_set", "pfpks", 64, 0, 9)]
    assert srv._audit_stages == st.STAGES
    del srv.engine.calls[:]
    srv.audit(rows=16, seed=9, stages=("pfpks",))                                  # the stages no longer named go off
    assert srv.engine.calls == [("audit_set", 0, 0, 9), ("audit_stage_set", "keyswitch", 0, 0, 9), ("audit_stage_set", "pfpks", 16, 0, 9)]
    assert srv._audit_stages == ("pfpks",)
    del srv.engine.calls[:]
    srv.audit(rows=0)
    assert [c[:3] for c in srv.engine.calls] == [("audit_set", 0, 0), ("audit_stage_set", "pfpks", 0)] and srv._audit_stages == ()
    with pytest.raises(ValueError):
        srv.audit(stages=("linear",))


def test_audit_mismatch_names_its_stage_and_keeps_the_blind_rotation_s_message():
    rec = server.AuditRecord(3, 17, 5, 0x10, 0x30)
    report = server.AuditReport(4, 256, 1, [rec])
    old = server.AuditMismatch(report)
    assert old.stage == "blind_rotate" and str(old).endswith(
        "the audit found 1 wrong rows in 256 checked over 4 launches; first: launch 3 row 17 word 5, 0x0000000000000010 for 0x0000000000000030")
    new = server.AuditMismatch(report, "pfpks", {"pfpks": report})
    assert new.stage == "pfpks" and "of stage pfpks found 1 wrong rows" in str(new) and new.records == [rec] and new.reports == {"pfpks": report}


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def test_balanced_planes_are_edge_words_balanced_bytes():
    words = [ew.KEY_M128, ew.KEY_P127, ew.KEY_ALT, *ew.EXTREMES, 0x80, 0x7F, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFFFFFFFFFFFF80]
    words += np.random.default_rng(0xBA1).integers(0, 1 << 64, 200, dtype=np.uint64).tolist()
    planes = st.balanced_planes(np.array(words, dtype=np.uint64))
    for i, w in enumerate(words):
        assert planes[:, i].tolist() == ew.balanced_bytes(w), hex(w)
    assert planes[:, 0].tolist() == [-128] * 8                                    # the carry that runs through all eight bytes


def test_fragments_are_padded_and_recombine_to_the_key():
    key = ew.key_words("mixture", (2, 70, 25))                                    # 70 rows: two K steps; 25 columns: two tiles
    frag = st.key_fragments(key)
    assert frag.shape == (2, 2, 2, 8, 64, 16) and frag.dtype == np.int8
    assert np.array_equal(st.fragment_words(frag, 70, 25), key)
    full = st.fragment_words(frag, 128, 32)
    assert not full[:, 70:].any() and not full[:, :, 25:].any()
    # lane l of (kstep 1, tile 1): column 16 + l % 16, rows 64 + 16 (l // 16) + e
    lane, e = 16 * 0 + 8, 5
    assert frag[1, 1, 1, :, lane, e].tolist() == ew.balanced_bytes(int(key[1, 64 + e, 16 + 8]))


def _inputs(p, stage):
    x, _ = ew.ks_inputs(p, stage, 16)
    return np.ascontiguousarray(x[[0, 3, 5, 6, 14, 15]])                           # full rows of four edge words, two mixed rows


@pytest.mark.parametrize("pattern", ["mixture", "m128"])
def test_model_is_the_plain_product_and_the_oracle_at_param_toy(pattern):
    p = PARAM_TOY
    ksk = ew.key_words(pattern, (p.big, p.ks_level, p.n + 1))
    pf = ew.key_words(pattern, (p.k + 1, p.big1, p.pfks_level, (p.k + 1) * p.N), seed=0x6E8)
    o = orc.Oracle(p, ksk, np.zeros(p.bsk_words, dtype=np.uint64), pf)
    x1, x3 = _inputs(p, "K1"), _inputs(p, "K3")
    got1 = st.k1_model(x1, ksk, p)
    assert got1.shape == (M, p.n + 1) and np.array_equal(got1, ew.keyswitch_plain(x1, ksk, p)) and np.array_equal(got1, o.keyswitch(x1))
    blocks = pf.reshape(p.k + 1, p.big1 * p.pfks_level, (p.k + 1) * p.N)
    got3 = st.k3_model(x3, blocks, p)
    assert got3.shape == (M, p.k + 1, (p.k + 1) * p.N)
    assert np.array_equal(got3, ew.pfpks_plain(x3, pf, p)) and np.array_equal(got3, o.pfpks(x3))
    # one key block alone, as pack's launch takes it
    assert np.array_equal(st.k3_model(x3, blocks[p.k:], p)[:, 0], got3[:, p.k])


@pytest.mark.parametrize("n", st.K1_SMALL_N + (PARAM_EDGE.n,))
def test_k1_model_bounds_its_columns_at_every_tile_edge(n):
    import dataclasses

    p = dataclasses.replace(PARAM_EDGE, name="PARAM_EDGE_N%d" % n, lwe_dimension=n)
    ksk = ew.key_words("mixture", (p.big, p.ks_level, p.n + 1), seed=0x6E7 + n)
    x = _inputs(p, "K1")
    got = st.k1_model(x, ksk, p)
    assert got.shape == (M, n + 1) and np.array_equal(got, ew.keyswitch_plain(x, ksk, p))
    o = orc.Oracle(p, ksk, np.zeros(p.bsk_words, dtype=np.uint64), np.zeros(1, dtype=np.uint64))
    assert np.array_equal(got, o.keyswitch(x))


def test_k3_model_at_param_edge_on_the_first_and_last_columns_of_two_key_blocks():
    """12,800 columns and Q = 6,147 rows (96 K steps and 3 rows): key blocks 0 and k, columns 0..63 and the last 16; the key holds the
    word whose carry runs through all eight bytes everywhere and the mixture in its first 48 columns"""
    p = PARAM_EDGE
    k1, gsz = p.k + 1, (p.k + 1) * p.N
    pf = ew.key_words("m128", (k1, p.big1, p.pfks_level, gsz))
    pf[..., :48] = ew.key_words("mixture", (k1, p.big1, p.pfks_level, 48), seed=0x6E9)
    x = _inputs(p, "K3")[:2]
    want = ew.pfpks_plain(x, pf, p)
    assert np.array_equal(want, orc.Oracle(p, np.zeros(1, dtype=np.uint64), np.zeros(p.bsk_words, dtype=np.uint64), pf).pfpks(x))
    blocks = pf.reshape(k1, p.big1 * p.pfks_level, gsz)[[0, p.k]]
    assert p.big1 * p.pfks_level == 6147 and 6147 % st.KSTEP == 3
    assert np.array_equal(st.k3_model(x, blocks, p, 0, 64), want[:, [0, p.k], :64])
    assert np.array_equal(st.k3_model(x, blocks, p, gsz - 16, gsz), want[:, [0, p.k], gsz - 16:])


def test_can_fail_a_lost_carry_of_one_byte_plane_is_seen():
    p = PARAM_TOY
    ksk = ew.key_words("mixture", (p.big, p.ks_level, p.n + 1))
    x = _inputs(p, "K1")
    frag = st.key_fragments(ksk.reshape(1, p.big * p.ks_level, p.n + 1))
    args = (ew.gadget(p, "K1"), p.big, p.n + 1)
    want = ew.keyswitch_plain(x, ksk, p)[:, None]
    assert np.array_equal(st.plain_model(x, frag, *args, body=(p.big, p.n)), want)
    for plane in (1, 7):
        assert not np.array_equal(st.plain_model(x, st.drop_carry(frag, plane), *args, body=(p.big, p.n)), want)
    assert not np.array_equal(st.plain_model(x, frag, *args), want)                # and so is a missing body term


def test_clean_call_table_counts():
    assert st.CLEAN_CALLS["aes_encrypt"][st.K2] == [256] * 10 and st.CLEAN_CALLS["gate"][st.KS] == [2]
    assert st.counters_after([256] * 10, 1) == (10, 10) and st.counters_after([513], 256) == (1, 256) and st.counters_after([3, 2816], 256) == (2, 259)
    # K1 runs once per segment of a window: 5 blocks in windows of 2 straddle a step in every fifth window
    k1 = st.window_k1_rows(5, 10, 2)
    assert len(k1) == 30 and sum(k1) == 50 * 128 and k1[:4] == [256, 256, 128, 128] and st.window_k1_rows(4, 10, 2) == [256] * 20
    assert st.window_k1_rows(5, 10, 3)[-1] == 256 and sum(st.window_k1_rows(5, 10, 3)) == 50 * 128
    assert st.row_words(PARAM_TOY, st.KS) == 25 and st.row_words(PARAM_EDGE, st.PF) == 12800 and st.row_words(PARAM_EDGE, st.PF, 4) == 2560
