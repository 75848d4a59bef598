"""CMAC without a GPU: aes_clear.cmac / cmac_verify against the SP 800-38B / RFC 4493 known answers (cmac.py) for the three key sizes,
rejected tags, messages and lengths, cmac_blocks on the lengths around a block, the rows of fheaes_cmac_subkey_row against a
Python-integer doubling and against fheaes_xts_tweak_row under the byte map, fheaes_aes_cmac_plan on ragged lengths, the Python layer's
arguments, the exports and null contexts."""
import ctypes

import pytest

import cmac
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import cmac_args

NEW_EXPORTS = ("fheaes_cmac_subkey_row", "fheaes_cmac_double", "fheaes_aes_cmac_subkeys_keyed", "fheaes_aes_cmac_subkeys_keyed_packed",
               "fheaes_aes_cmac_keyed", "fheaes_aes_cmac_keyed_packed", "fheaes_aes_cmac_plan")
INVALID = -1
u128 = lambda b: int.from_bytes(b, "big")


# ---- 1. the clear model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", list(cmac.VECTORS))
def test_known_answers(bits):
    key, k1, k2, tags = cmac.VECTORS[bits]
    assert aes_clear.cmac_subkeys(key) == (u128(k1), u128(k2))
    for length, tag in zip(cmac.LENGTHS, tags):
        msg = cmac.MESSAGE[:length]
        assert aes_clear.cmac(key, msg) == tag, length
        assert aes_clear.cmac(key, msg, 8) == tag[:8]
        assert aes_clear.cmac_verify(key, msg, tag) and aes_clear.cmac_verify(key, msg, tag[:4]) and aes_clear.cmac_verify(key, msg, tag[:13])
    assert aes_clear.aes_encrypt_block(cmac.VECTORS[128][0], 0) == u128(cmac.L_128)


@pytest.mark.parametrize("bits", list(cmac.VECTORS))
def test_flipped_bits_are_rejected(bits):
    key, _, _, tags = cmac.VECTORS[bits]
    flip = lambda data, i: data[:i] + bytes([data[i] ^ 0x10]) + data[i + 1:]
    for length, tag in zip(cmac.LENGTHS, tags):
        msg = cmac.MESSAGE[:length]
        assert not aes_clear.cmac_verify(key, msg, flip(tag, 0)) and not aes_clear.cmac_verify(key, msg, flip(tag, 15))
        assert not aes_clear.cmac_verify(key, msg, flip(tag, 7)[:8])
        assert aes_clear.cmac_verify(key, msg, flip(tag, 8)[:8])                              # a bit beyond the truncated length
        if length:
            assert not aes_clear.cmac_verify(key, flip(msg, 0), tag) and not aes_clear.cmac_verify(key, flip(msg, length - 1), tag)
            assert not aes_clear.cmac_verify(key, msg[:-1], tag)                              # one byte shorter: across a block boundary at 16 and 64
        assert not aes_clear.cmac_verify(key, msg + b"\x00", tag) and not aes_clear.cmac_verify(key, msg + b"\x80", tag)
    assert not aes_clear.cmac_verify(key, b"", b"") and not aes_clear.cmac_verify(key, b"", bytes(17))
    with pytest.raises(ValueError):
        aes_clear.cmac(key, b"", 0)
    with pytest.raises(ValueError):
        aes_clear.cmac(key, b"", 17)


def test_blocks_around_a_block_boundary():
    pad = lambda data: u128(data + b"\x80" + bytes(15 - len(data) % 16))
    m = bytes(range(1, 33))
    assert aes_clear.cmac_blocks(b"") == ([1 << 127], 1)
    assert aes_clear.cmac_blocks(m[:1]) == ([pad(m[:1])], 1) and pad(m[:1]) == 0x0180 << 112
    assert aes_clear.cmac_blocks(m[:15]) == ([u128(m[:15] + b"\x80")], 1)
    assert aes_clear.cmac_blocks(m[:16]) == ([u128(m[:16])], 0)
    assert aes_clear.cmac_blocks(m[:17]) == ([u128(m[:16]), 0x1180 << 112], 1)
    assert aes_clear.cmac_blocks(m) == ([u128(m[:16]), u128(m[16:])], 0)


# ---- 2. the rows -------------------------------------------------------------------------------------------------------------------------
def test_subkey_rows_are_the_doubling():
    ones = []
    for which, heaviest in ((0, 2), (1, 3)):
        want = cmac.rows(which)
        got = [_native.cmac_subkey_row(which, i) for i in range(128)]
        for i in range(128):
            assert len(set(got[i])) == len(got[i]) and sorted(got[i]) == want[i], (which, i, got[i], want[i])
        assert max(len(r) for r in got) == heaviest
        ones.append(sum(len(r) for r in got))
    assert ones == [131, 134]
    # the doubling itself, on the AES-128 vector: L -> K1 -> K2
    _, k1, k2, _ = cmac.VECTORS[128]
    assert cmac.double(u128(cmac.L_128)) == u128(k1) and cmac.double(u128(cmac.L_128), 2) == u128(k2)


def test_subkey_rows_are_the_xts_rows_in_the_other_byte_order():
    assert all(cmac.degree(cmac.degree(i)) == i for i in range(128)) and cmac.degree(0) == 120 and cmac.degree(127) == 7
    for which in range(2):
        for i in range(128):
            want = sorted(cmac.degree(s) for s in _native.xts_tweak_row(which + 1, cmac.degree(i)))
            assert sorted(_native.cmac_subkey_row(which, i)) == want, (which, i)


def test_subkey_row_refusals():
    lib = _native.load_library()
    src, n = (ctypes.c_uint32 * 3)(), ctypes.c_uint32()
    assert lib.fheaes_cmac_subkey_row(1, 127, src, ctypes.byref(n)) == 0
    assert lib.fheaes_cmac_subkey_row(2, 0, src, ctypes.byref(n)) == INVALID
    assert lib.fheaes_cmac_subkey_row(0, 128, src, ctypes.byref(n)) == INVALID
    assert lib.fheaes_cmac_subkey_row(0, 0, None, ctypes.byref(n)) == INVALID
    assert lib.fheaes_cmac_subkey_row(0, 0, src, None) == INVALID
    with pytest.raises(_native.FheAesError):
        _native.cmac_subkey_row(2, 0)


# ---- 3. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_on_ragged_lengths():
    assert _native.aes_cmac_plan([0, 1, 15, 16, 17, 32, 40]) == {"steps": 3, "chained_blocks": 1 + 1 + 1 + 1 + 2 + 2 + 3, "padded_streams": 5}
    assert _native.aes_cmac_plan([]) == {"steps": 0, "chained_blocks": 0, "padded_streams": 0}
    assert _native.aes_cmac_plan([0]) == {"steps": 1, "chained_blocks": 1, "padded_streams": 1}
    assert _native.aes_cmac_plan([48] * 64) == {"steps": 3, "chained_blocks": 192, "padded_streams": 0}
    assert _native.aes_cmac_plan([16 << 16]) == {"steps": 1 << 16, "chained_blocks": 1 << 16, "padded_streams": 0}
    lens = [(37 * i) % 90 for i in range(40)]
    blocks = [max(1, (v + 15) // 16) for v in lens]
    pl = _native.aes_cmac_plan(lens)
    assert pl == {"steps": max(blocks), "chained_blocks": sum(blocks), "padded_streams": sum(1 for v in lens if v == 0 or v % 16)}
    assert blocks == [len(aes_clear.cmac_blocks(bytes(v))[0]) for v in lens]


def test_plan_refusals():
    lib = _native.load_library()
    one = (ctypes.c_uint64 * 1)(16)
    a = ctypes.c_uint64()
    r = ctypes.byref(a)
    assert lib.fheaes_aes_cmac_plan(one, 1, r, r, r) == 0
    assert lib.fheaes_aes_cmac_plan(None, 0, r, r, r) == 0
    assert lib.fheaes_aes_cmac_plan(None, 1, r, r, r) == INVALID
    assert lib.fheaes_aes_cmac_plan(one, 1, None, r, r) == INVALID
    assert lib.fheaes_aes_cmac_plan(one, 1, r, None, r) == INVALID
    assert lib.fheaes_aes_cmac_plan(one, 1, r, r, None) == INVALID
    assert lib.fheaes_aes_cmac_plan(one, (1 << 20) + 1, r, r, r) == INVALID
    assert lib.fheaes_aes_cmac_plan((ctypes.c_uint64 * 1)((16 << 16) + 1), 1, r, r, r) == INVALID      # one byte more than 2^16 blocks
    with pytest.raises(_native.FheAesError):
        _native.aes_cmac_plan([1 << 21])


# ---- 4. the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


def test_new_entry_points_reject_a_null_context():
    lib = _native.load_library()
    w, u32, u64, u8 = (ctypes.c_uint64 * 16)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint8 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_cmac_double(None, w, 1, w, ms) == INVALID
        assert lib.fheaes_aes_cmac_subkeys_keyed(None, w, 128, 1, w, ms) == INVALID
        assert lib.fheaes_aes_cmac_subkeys_keyed_packed(None, w, 128, 1, w, ms) == INVALID
        assert lib.fheaes_aes_cmac_keyed(None, w, 128, 1, None, 1, u32, u64, u8, None, None, w, None, ms) == INVALID
        assert lib.fheaes_aes_cmac_keyed_packed(None, w, 128, 1, None, 1, u32, u64, u8, u8, u32, None, w, ms) == INVALID


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------------------
def test_cmac_args_builds_the_per_stream_arrays():
    a = cmac_args([(0, b""), (2, bytes(16)), (1, bytearray(b"abc")), (0, bytes(33))])
    assert a["key_of_stream"] == [0, 2, 1, 0] and a["message_bytes"] == [0, 16, 3, 33] and a["chain_blocks"] == [1, 1, 1, 3]
    assert a["data"] == bytes(16) + b"abc" + bytes(33) and a["tags"] is None and a["tag_bytes"] is None
    a = cmac_args([(1, b"xy", bytes(range(4))), (0, b"", bytes(range(13)))])
    assert a["tag_bytes"] == [4, 13] and a["tags"] == [[0, 1, 2, 3] + [0] * 12, list(range(13)) + [0] * 3] and a["data"] == b"xy"
    assert cmac_args([]) == {"key_of_stream": [], "message_bytes": [], "data": b"", "chain_blocks": [], "tags": None, "tag_bytes": None}
    for bad in ([(0, b"", bytes(3))], [(0, b"", bytes(17))], [(0, b""), (0, b"", bytes(8))], [(0,)], [(0, b"", bytes(8), 1)]):
        with pytest.raises(ValueError):
            cmac_args(bad)
