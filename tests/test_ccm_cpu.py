"""CCM without a GPU: aes_clear.ccm_encrypt / ccm_decrypt against SP 800-38C examples 1-3 and RFC 3610 vector 1 (ccm.py), rejected
tags and ciphertexts, ccm_blocks against hand-written B0 and AAD blocks, fheaes_aes_mac_plan on ragged stream lengths, the Python
layer's arguments and shards, the exports and null contexts."""
import ctypes

import pytest

import ccm
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import _shards_by_cost, ccm_args

NEW_EXPORTS = ("fheaes_aes_cbc_mac_keyed", "fheaes_aes_cbc_mac_keyed_packed", "fheaes_aes_ccm_open_keyed", "fheaes_aes_ccm_open_keyed_packed",
               "fheaes_mac_link", "fheaes_aes_mac_plan")
INVALID = -1


# ---- 1. the clear model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ccm.VECTORS))
def test_known_answers(name):
    key, nonce, aad, payload, t, out = ccm.VECTORS[name]
    assert aes_clear.ccm_encrypt(key, nonce, aad, payload, t) == out
    assert aes_clear.ccm_decrypt(key, nonce, aad, out, t) == payload


@pytest.mark.parametrize("name", list(ccm.VECTORS))
def test_flipped_bits_are_rejected(name):
    key, nonce, aad, payload, t, out = ccm.VECTORS[name]
    flip = lambda data, i: data[:i] + bytes([data[i] ^ 0x10]) + data[i + 1:]
    assert aes_clear.ccm_decrypt(key, nonce, aad, flip(out, len(out) - 1), t) is None         # the last byte of the tag
    assert aes_clear.ccm_decrypt(key, nonce, aad, flip(out, len(out) - t), t) is None         # its first byte
    assert aes_clear.ccm_decrypt(key, nonce, aad, flip(out, 0), t) is None                    # a ciphertext bit
    assert aes_clear.ccm_decrypt(key, nonce, flip(aad, 0), out, t) is None
    assert aes_clear.ccm_decrypt(key, flip(nonce, 0), aad, out, t) is None


def test_cbc_mac_is_the_chain():
    key = ccm.run(0x40, 16)
    assert aes_clear.cbc_mac(key, []) == 0 and aes_clear.cbc_mac(key, [], init=5) == 5
    assert aes_clear.cbc_mac(key, [7]) == aes_clear.aes_encrypt_block(key, 7)
    assert aes_clear.cbc_mac(key, [7, 9], init=3) == aes_clear.aes_encrypt_block(key, aes_clear.aes_encrypt_block(key, 7 ^ 3) ^ 9)


def test_blocks_of_example_1_and_of_a_long_aad():
    _, nonce, aad, payload, t, _ = ccm.VECTORS["ex1"]
    b0, aad_blocks, ctr = aes_clear.ccm_blocks(nonce, aad, len(payload), t)
    assert b0 == int("4f101112131415160000000000000004", 16)                                  # flags 64 + 8 * 1 + 7
    assert aad_blocks == [int("00080001020304050607000000000000", 16)]
    assert ctr == [int("07101112131415160000000000000000", 16), int("07101112131415160000000000000001", 16)]
    aad = bytes(i & 0xFF for i in range(0xFF00))
    b0, aad_blocks, ctr = aes_clear.ccm_blocks(ccm.run(0x10, 13), aad, 0, 16)
    assert b0 == int("79" + ccm.run(0x10, 13).hex() + "0000", 16)                             # 64 + 8 * 7 + (q - 1 = 1) = 0x79
    assert len(aad_blocks) == (6 + 0xFF00 + 15) // 16 == 4081
    assert aad_blocks[0] == int("fffe0000ff00" + bytes(range(10)).hex(), 16)
    assert aad_blocks[-1] == int(aad[-6:].hex() + "00" * 10, 16)
    assert ctr == [int("01" + ccm.run(0x10, 13).hex() + "0000", 16)]
    assert aes_clear.ccm_blocks(ccm.run(0, 7), b"", 17, 4)[0] >> 120 == 8 * 1 + 7               # no AAD: bit 6 clear
    assert aes_clear.ccm_blocks(ccm.run(0, 7), bytes(0xFEFF), 0, 4)[1][0] >> 112 == 0xFEFF    # the last 2-byte length


def test_formatting_refusals():
    ok = ccm.run(0, 12)
    for bad in (lambda: aes_clear.ccm_blocks(bytes(6), b"", 0, 8), lambda: aes_clear.ccm_blocks(bytes(14), b"", 0, 8),
                lambda: aes_clear.ccm_blocks(ok, b"", 0, 2), lambda: aes_clear.ccm_blocks(ok, b"", 0, 7), lambda: aes_clear.ccm_blocks(ok, b"", 0, 18),
                lambda: aes_clear.ccm_blocks(bytes(13), b"", 1 << 16, 8), lambda: aes_clear.ccm_decrypt(bytes(16), ok, b"", bytes(3), 4)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_on_ragged_lengths():
    assert _native.aes_mac_plan([3, 1, 2]) == {"steps": 3, "n_active": [3, 2, 1], "chained_blocks": 6, "public_blocks": 0}
    assert _native.aes_mac_plan([2, 0, 5, 2, 0]) == {"steps": 5, "n_active": [3, 3, 1, 1, 1], "chained_blocks": 9, "public_blocks": 0}
    assert _native.aes_mac_plan([0, 0]) == {"steps": 0, "n_active": [], "chained_blocks": 0, "public_blocks": 0}
    assert _native.aes_mac_plan([]) == {"steps": 0, "n_active": [], "chained_blocks": 0, "public_blocks": 0}
    # a CCM call: 64 messages of one AAD block and two payload blocks
    assert _native.aes_mac_plan([3] * 64, [2] * 64) == {"steps": 3, "n_active": [64] * 3, "chained_blocks": 192, "public_blocks": 256}
    assert _native.aes_mac_plan([0, 1, 2], [0, 0, 2])["public_blocks"] == 8
    lens = [(7 * i) % 5 for i in range(40)]
    pl = _native.aes_mac_plan(lens)
    assert pl["n_active"] == [sum(1 for v in lens if v > i) for i in range(max(lens))] and pl["chained_blocks"] == sum(lens)


def test_plan_refusals():
    lib = _native.load_library()
    one = (ctypes.c_uint32 * 1)(1)
    a, act = ctypes.c_uint64(), (ctypes.c_uint64 * 1)()
    call = lambda sb, pb, n, steps, cap: lib.fheaes_aes_mac_plan(sb, pb, n, steps, act, cap, ctypes.byref(a), ctypes.byref(a))
    assert call(one, None, 1, ctypes.byref(a), 1) == 0
    assert call(None, None, 1, ctypes.byref(a), 1) == INVALID
    assert call(one, None, 1, None, 1) == INVALID
    assert call(one, None, 1, ctypes.byref(a), 0) == INVALID                                  # one step does not fit
    assert call(one, None, (1 << 20) + 1, ctypes.byref(a), 1) == INVALID
    assert call((ctypes.c_uint32 * 1)((1 << 16) + 1), None, 1, ctypes.byref(a), 1) == INVALID
    assert call(one, (ctypes.c_uint32 * 1)(2), 1, ctypes.byref(a), 1) == INVALID              # more payload blocks than the chain has
    with pytest.raises(_native.FheAesError):
        _native.aes_mac_plan([1 << 17])


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()


def test_new_entry_points_reject_a_null_context():
    lib = _native.load_library()
    w, u32, u8 = (ctypes.c_uint64 * 16)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 16)()
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_aes_cbc_mac_keyed(None, w, 128, 1, 1, u32, u32, u8, None, None, None, w, ms) == INVALID
        assert lib.fheaes_aes_cbc_mac_keyed_packed(None, w, 128, 1, 1, u32, u32, u8, None, None, None, w, ms) == INVALID
        assert lib.fheaes_aes_ccm_open_keyed(None, w, 128, 1, 1, u32, u32, w, w, w, u8, u8, u32, w, w, ms) == INVALID
        assert lib.fheaes_aes_ccm_open_keyed_packed(None, w, 128, 1, 1, u32, u32, w, w, w, u8, u8, u32, w, w, ms) == INVALID
        assert lib.fheaes_mac_link(None, w, 1, 1, None, None, 0, None, None, u8, ms) == INVALID


# ---- 4. the Python layer -------------------------------------------------------------------------------------------------------------------
def test_ccm_args_formats_in_python():
    a = ccm_args([ccm.message(0, "ex1"), ccm.message(1, "rfc1"), (0, ccm.run(0, 13), b"", b"", bytes(4))])
    assert a["key_of_stream"] == [0, 1, 0] and a["head_blocks"] == [2, 2, 1] and a["payload_bytes"] == [4, 23, 0] and a["tag_bytes"] == [4, 8, 4]
    assert a["block_of_message"] == [0, 1, 3, 3]
    assert a["head"][0] == int("4f101112131415160000000000000004", 16) and len(a["head"]) == 5
    assert a["ctr0"][0] == int("07101112131415160000000000000000", 16)
    assert a["ciphertext"] == ccm.VECTORS["ex1"][5][:4] + ccm.VECTORS["rfc1"][5][:23]
    assert a["tags"][0] == list(ccm.VECTORS["ex1"][5][4:]) + [0] * 12
    with pytest.raises(ValueError):
        ccm_args([(0, bytes(6), b"", b"", bytes(4))])
    with pytest.raises(ValueError):
        ccm_args([(0, bytes(12), b"", b"", bytes(5))])


def test_shards_are_whole_contiguous_and_balanced():
    for costs, g in (([3, 1, 2], 2), ([1] * 6, 2), ([5], 2), ([], 2), ([1, 1, 1, 9], 3), ([4] * 4, 4), ([1, 2], 3), ([0, 0], 2)):
        shards = _shards_by_cost(costs, g)
        assert len(shards) == g and shards[0][0] == 0 and shards[-1][1] == len(costs)
        assert all(lo <= hi for lo, hi in shards) and all(shards[i][1] == shards[i + 1][0] for i in range(g - 1))
    assert _shards_by_cost([1, 1, 1, 9], 3) == [(0, 3), (3, 4), (4, 4)]
    assert _shards_by_cost([1] * 6, 2) == [(0, 3), (3, 6)]
