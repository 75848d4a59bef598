"""XTS without a GPU: aes_clear.xts_encrypt / xts_decrypt against the IEEE 1619 vectors (xts.py), a stream continued inside a unit, the
rows of fheaes_xts_tweak_row against the multiplication by alpha^j in Python integers, fheaes_aes_xts_plan against the segment rule
restated here, the argument refusals of the host-only calls and of the Python layer, the exports and null contexts."""
import ctypes

import pytest

import xts
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import xts_args

NEW_EXPORTS = ("fheaes_aes_xts_decrypt_bits", "fheaes_aes_xts_decrypt_packed", "fheaes_xts_tweaks", "fheaes_xts_tweak_row", "fheaes_aes_xts_plan",
               "fheaes_inv_mix_columns_batch")
INVALID = -1


# ---- 1. the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


def test_new_entry_points_reject_a_null_context():
    lib = _native.load_library()
    buf = (ctypes.c_uint64 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        for bits in (128, 192, 256):
            assert lib.fheaes_aes_xts_decrypt_bits(None, buf, buf, bits, buf, 1, 32, 0, buf, 1, buf, ms) == INVALID
            assert lib.fheaes_aes_xts_decrypt_packed(None, buf, buf, bits, buf, 1, 32, 0, buf, 1, buf, ms) == INVALID
        assert lib.fheaes_xts_tweaks(None, buf, 1, 0, 1, buf, ms) == INVALID
        assert lib.fheaes_inv_mix_columns_batch(None, buf, 1, buf, ms) == INVALID


# ---- 2. the clear mode -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("number", sorted(xts.VECTORS))
def test_ieee_1619_vectors(number):
    key1, key2, sector, pt, expected = xts.VECTORS[number]
    ct = aes_clear.xts_encrypt(key1, key2, sector, pt)
    assert xts.matches(ct, expected)
    assert aes_clear.xts_decrypt(key1, key2, sector, ct) == pt


def test_a_stream_continues_with_first_block():
    key1, key2, sector, pt, _ = xts.VECTORS[10]
    ct = aes_clear.xts_encrypt(key1, key2, sector, pt)
    for cut in (1, 7, 31):
        assert aes_clear.xts_decrypt(key1, key2, sector, ct[16 * cut:], first_block=cut) == pt[16 * cut:]
        assert aes_clear.xts_encrypt(key1, key2, sector, pt[16 * cut:], first_block=cut) == ct[16 * cut:]
    assert aes_clear.xts_decrypt(key1, key2, sector, b"") == b""


def test_clear_mode_refusals():
    for bad in (lambda: aes_clear.xts_decrypt(bytes(16), bytes(32), 0, bytes(16)), lambda: aes_clear.xts_decrypt(bytes(24), bytes(24), 0, bytes(16)),
                lambda: aes_clear.xts_decrypt(bytes(16), bytes(16), 0, bytes(17)), lambda: aes_clear.xts_tweak_block(1 << 128)):
        with pytest.raises(ValueError):
            bad()
    assert aes_clear.xts_tweak_block(0x0102) == 0x0201 << 112           # little-endian number: its low byte is byte 0, the u128's top byte


# ---- 3. the rows -------------------------------------------------------------------------------------------------------------------------
def test_tweak_rows_are_the_multiplication_by_alpha_j():
    heaviest = 0
    for j in range(xts.MAX_OFFSET + 1):
        want = xts.rows(j)
        for i in range(128):
            got = _native.xts_tweak_row(j, i)
            assert len(set(got)) == len(got) and sorted(got) == want[i], (j, i, got, want[i])
            heaviest = max(heaviest, len(got))
    assert heaviest == 4
    assert max(len(r) for r in xts.rows(122)) == 5                         # why 121 is the last offset of one gather


def test_tweak_row_refusals():
    lib = _native.load_library()
    src, n = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
    assert lib.fheaes_xts_tweak_row(121, 127, src, ctypes.byref(n)) == 0
    assert lib.fheaes_xts_tweak_row(122, 0, src, ctypes.byref(n)) == INVALID
    assert lib.fheaes_xts_tweak_row(0, 128, src, ctypes.byref(n)) == INVALID
    assert lib.fheaes_xts_tweak_row(0, 0, None, ctypes.byref(n)) == INVALID
    assert lib.fheaes_xts_tweak_row(0, 0, src, None) == INVALID
    with pytest.raises(_native.FheAesError):
        _native.xts_tweak_row(122, 0)


# ---- 4. the plan -------------------------------------------------------------------------------------------------------------------------
def plan_restated(bpu, first_block, n_blocks):
    """(serial refreshes, gathered tweaks, touched units): per unit, one tweak per block of the call and one chained anchor per segment
    boundary below its last block"""
    blocks = range(first_block, first_block + n_blocks)
    units = sorted({g // bpu for g in blocks})
    last = {u: max(g % bpu for g in blocks if g // bpu == u) for u in units}
    return max(v // xts.SEGMENT + 1 for v in last.values()), n_blocks + sum(v // xts.SEGMENT for v in last.values()), len(units)


@pytest.mark.parametrize("bits,nr", [(128, 10), (256, 14)])
@pytest.mark.parametrize("bpu,first_block,n_blocks,segments", [
    (32, 0, 128, 1),         # four 512-byte units
    (256, 0, 256, 3),        # one 4,096-byte unit: segments 0..119, 120..239, 240..255
    (256, 0, 512, 3),
    (256, 119, 4, 2),        # a shard starting at block 119: across the first seam
    (256, 119, 256, 3),      # ... into the next unit
    (256, 250, 3, 3),        # two segments yield their anchor only
    (123, 119, 4, 2),
    (120, 0, 120, 1), (121, 0, 121, 2), (1, 5, 9, 1)])
def test_plan(bits, nr, bpu, first_block, n_blocks, segments):
    n_units = (first_block + n_blocks + bpu - 1) // bpu
    pl = _native.aes_xts_plan(n_units, bpu, first_block, n_blocks, bits)
    seg, gathered, units = plan_restated(bpu, first_block, n_blocks)
    assert seg == segments and pl["segments"] == segments
    assert pl["tweak_refresh_bytes"] == 16 * (gathered + units)
    assert pl["cipher_bytes"] == 16 * nr * n_blocks
    assert pl["max_terms"] <= 5
    # 16 byte-WoPBS of refresh per block, beyond that only the anchors: one per unit and one per segment boundary crossed
    assert 16 * n_blocks < pl["tweak_refresh_bytes"] <= 16 * (n_blocks + units * (1 + (bpu - 1) // xts.SEGMENT))


def test_plan_refusals():
    ok = lambda *a: _native.aes_xts_plan(*a)
    assert ok(1, 32, 0, 0) == {"segments": 0, "tweak_refresh_bytes": 0, "cipher_bytes": 0, "max_terms": 0}
    assert ok(1, 1 << 20, 0, 1)["segments"] == 1
    for bad in ((1, 32, 0, 33), (1, 32, 31, 2), (0, 32, 0, 1), (1, 0, 0, 1), (1, (1 << 20) + 1, 0, 1), (1, 32, 0, 1, 192), (1, 32, 0, 1, 100),
                (1 << 40, 32, (1 << 64) - 1, 2)):
        with pytest.raises(_native.FheAesError):
            ok(*bad)
    lib = _native.load_library()
    a, t = ctypes.c_uint64(), ctypes.c_uint32()
    assert lib.fheaes_aes_xts_plan(1, 32, 0, 1, 128, None, ctypes.byref(a), ctypes.byref(a), ctypes.byref(t)) == INVALID
    assert lib.fheaes_aes_xts_plan(1, 32, 0, 1, 128, ctypes.byref(a), ctypes.byref(a), ctypes.byref(a), None) == INVALID


# ---- 5. the Python layer's arguments --------------------------------------------------------------------------------------------------------
def test_xts_args():
    assert xts_args(7, bytes(16 * 70), 512, 0) == ([7, 8, 9], 32, [bytes(16)] * 70)
    assert xts_args(7, bytes(32), 512, 31)[0] == [7, 8]                      # a call that starts at the last block of unit 0
    assert xts_args([5, 9], [1, 2], 16, 0) == ([5, 9], 1, [1, 2])
    assert xts_args(0, b"", 512, 0) == ([], 32, [])
    for bad in (lambda: xts_args(0, bytes(17), 512, 0), lambda: xts_args(0, bytes(16), 520, 0), lambda: xts_args(0, bytes(16), 0, 0),
                lambda: xts_args(0, bytes(16), 16 * ((1 << 20) + 1), 0), lambda: xts_args([1], bytes(48), 32, 0), lambda: xts_args(0, bytes(16), 512, -1)):
        with pytest.raises(ValueError):
            bad()
