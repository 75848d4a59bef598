"""AES key unwrap (RFC 3394) without a GPU: the clear wrap and unwrap on the six vectors of RFC 3394 section 4, random round trips and
every single-bit flip of a wrapped key; the index form of the unwrap (step s: register n - s mod n, counter 6n - s) against the RFC's
double loop; the numpy model of the link step by step against the byte-level unwrap, which pins the row addressing of load, shuffle and
unload; fheaes_aes_kw_plan, the new exports, and server.kw_args."""
import ctypes

import numpy as np
import pytest

import keywrap
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import kw_args

INVALID = -1
NEW_EXPORTS = ("fheaes_aes_kw_unwrap_keyed", "fheaes_aes_kw_unwrap_keyed_packed", "fheaes_kw_link", "fheaes_aes_kw_plan")


# ---- 1. the clear model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(keywrap.VECTORS))
def test_rfc3394_vectors_both_ways(name):
    kek, payload, wrapped = keywrap.vector(name)
    assert len(wrapped) == len(payload) + 8
    assert aes_clear.key_wrap(kek, payload) == wrapped
    assert aes_clear.key_unwrap(kek, wrapped) == (True, payload)


def test_random_round_trips():
    rng = np.random.default_rng(0x3394)
    for bits in (128, 192, 256):
        for n in range(2, 9):
            kek, data = rng.bytes(bits // 8), rng.bytes(8 * n)
            wrapped = aes_clear.key_wrap(kek, data)
            assert len(wrapped) == 8 * (n + 1)
            assert aes_clear.key_unwrap(kek, wrapped) == (True, data)
            other = bytes([kek[0] ^ 1]) + kek[1:]
            assert aes_clear.key_unwrap(other, wrapped)[0] is False


def test_every_single_bit_flip_is_rejected():
    kek, _, wrapped = keywrap.vector("4.1")
    for bit in range(192):
        bad = bytearray(wrapped)
        bad[bit // 8] ^= 1 << (bit % 8)
        assert aes_clear.key_unwrap(kek, bytes(bad))[0] is False, bit


def test_lengths_outside_two_to_eight_semiblocks_are_refused():
    kek = bytes(16)
    for size in (0, 8, 15, 17, 72):
        with pytest.raises(ValueError):
            aes_clear.key_wrap(kek, bytes(size))
    for size in (16, 23, 80):
        with pytest.raises(ValueError):
            aes_clear.key_unwrap(kek, bytes(size))


# ---- 2. the index form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(2, 9))
def test_steps_are_the_rfc_double_loop(n):
    steps = [(keywrap.counter(n, s), keywrap.register(n, s)) for s in range(6 * n)]
    assert steps == keywrap.rfc_steps(n)
    assert all(keywrap.register(n, s) != keywrap.register(n, s - 1) for s in range(1, 6 * n))      # what lets a shuffle run in place
    assert keywrap.register(n, 6 * n - 1) == 1                                                     # the unload's register
    assert max(t for t, _ in steps) == 6 * n <= 48 < 256                                           # the counter fits block byte 7


# ---- 3. the link, on trivial encodings -----------------------------------------------------------------------------------------------------
def _body_bytes(rows):
    """[8 m][kN+1] trivial encodings -> m bytes, decoded by the MSB of the body word; the mask words must be zero"""
    assert not rows[:, :-1].any()
    bits = (rows[:, -1] >> np.uint64(63)).astype(np.uint64).reshape(-1, 8)
    assert np.array_equal(rows[:, -1], (bits << np.uint64(63)).reshape(-1))
    return bytes((bits << np.arange(8, dtype=np.uint64)).sum(axis=1).astype(np.uint8).tolist())


def _trivial_block(value, lw):
    rows = np.zeros((128, lw), dtype=np.uint64)
    keywrap.add_trivial(rows, value.to_bytes(16, "big"))
    return rows.reshape(16, 8, lw)


@pytest.mark.parametrize("n,bits", [(2, 128), (3, 192), (8, 256)])
def test_np_link_step_by_step_is_the_byte_level_unwrap(n, bits):
    """two keys under one KEK, the second with a flipped bit; clear AES between the links"""
    lw = 5
    rng = np.random.default_rng(n)
    kek, data = rng.bytes(bits // 8), rng.bytes(8 * n)
    good = aes_clear.key_wrap(kek, data)
    bad = good[:9] + bytes([good[9] ^ 0x10]) + good[10:]
    wrapped = [good, bad]
    a = [int.from_bytes(w[:8], "big") for w in wrapped]
    r = [[int.from_bytes(w[8 * i:8 * i + 8], "big") for i in range(n + 1)] for w in wrapped]          # r[key][i], i = 1 .. n
    state = np.full((2, 16, 8, lw), 0xA5, dtype=np.uint64)
    regs = np.full((2, 8 * n, 8, lw), 0xA5, dtype=np.uint64)
    for s in range(6 * n):
        state, regs = keywrap.np_link(state, regs, n, s, wrapped)
        t, i = keywrap.counter(n, s), keywrap.register(n, s)
        for key in range(2):
            block = ((a[key] ^ t) << 64) | r[key][i]
            assert _body_bytes(state[key].reshape(128, lw)) == block.to_bytes(16, "big"), (s, key)
            held = _body_bytes(regs[key].reshape(64 * n, lw))
            for j in range(1, n + 1):                      # register i_s went into the state as a copy: the file holds every R[j]
                assert held[8 * (j - 1):8 * j] == r[key][j].to_bytes(8, "big"), (s, key, j)
            b = aes_clear.aes_decrypt_block(kek, block)
            a[key], r[key][i] = b >> 64, b & ((1 << 64) - 1)
            state[key] = _trivial_block(b, lw)
    state, regs = keywrap.np_link(state, regs, n, 6 * n, wrapped)
    for key, w in enumerate(wrapped):
        ok, payload = aes_clear.key_unwrap(kek, w)
        assert _body_bytes(regs[key].reshape(64 * n, lw)) == payload
        diff = _body_bytes(state[key].reshape(128, lw))
        assert diff[8:] == bytes(8) and (diff[:8] == bytes(8)) == ok
        assert diff[:8] == (a[key] ^ keywrap.ICV).to_bytes(8, "big")
    assert aes_clear.key_unwrap(kek, good) == (True, data) and aes_clear.key_unwrap(kek, bad)[0] is False


def test_np_link_moves_whole_words():
    """a shuffle on arbitrary words: the two half blocks move word for word, A gets 1 << 63 on the body words of the counter's bits"""
    n, s, lw = 3, 4, 4
    rng = np.random.default_rng(7)
    state = rng.integers(0, 1 << 64, (1, 16, 8, lw), dtype=np.uint64)
    regs = rng.integers(0, 1 << 64, (1, 8 * n, 8, lw), dtype=np.uint64)
    st, rg = keywrap.np_link(state, regs, n, s, None)
    i_in, i_out = keywrap.register(n, s) - 1, keywrap.register(n, s - 1) - 1
    assert np.array_equal(st[0, 8:], regs[0, 8 * i_in:8 * i_in + 8]) and np.array_equal(rg[0, 8 * i_out:8 * i_out + 8], state[0, 8:])
    other = 3 - i_in - i_out
    assert np.array_equal(rg[0, 8 * other:8 * other + 8], regs[0, 8 * other:8 * other + 8])
    delta = st[0, :8] - state[0, :8]
    assert not delta[:7].any() and not delta[7, :, :-1].any()
    t = keywrap.counter(n, s)
    assert delta[7, :, -1].tolist() == [(t >> b & 1) << 63 for b in range(8)]


# ---- 4. the plan ---------------------------------------------------------------------------------------------------------------------------
def test_plan_values():
    for bits, nr in ((128, 10), (192, 12), (256, 14)):
        for n in range(2, 9):
            for n_keys in (0, 1, 64, 4096):
                assert _native.aes_kw_plan(bits, n, n_keys) == {"steps": 6 * n, "cipher_blocks": 6 * n * n_keys,
                                                                "byte_wopbs": 16 * nr * 6 * n * n_keys + 8 * n * n_keys + 16 * n_keys}
    assert _native.aes_kw_plan(128, 2, 64) == {"steps": 12, "cipher_blocks": 768, "byte_wopbs": 122880 + 1024 + 1024}


def test_plan_refusals():
    lib = _native.load_library()
    a = ctypes.c_uint64()
    r = ctypes.byref(a)
    assert lib.fheaes_aes_kw_plan(128, 2, 1, r, r, r) == 0
    for bits in (0, 64, 129):
        assert lib.fheaes_aes_kw_plan(bits, 2, 1, r, r, r) == INVALID
    for n in (0, 1, 9):
        assert lib.fheaes_aes_kw_plan(128, n, 1, r, r, r) == INVALID
    assert lib.fheaes_aes_kw_plan(128, 2, 4097, r, r, r) == INVALID
    assert lib.fheaes_aes_kw_plan(128, 2, 1, None, r, r) == INVALID
    assert lib.fheaes_aes_kw_plan(128, 2, 1, r, None, r) == INVALID
    assert lib.fheaes_aes_kw_plan(128, 2, 1, r, r, None) == INVALID
    with pytest.raises(_native.FheAesError):
        _native.aes_kw_plan(128, 9, 1)


# ---- 5. the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    lib = _native.load_library()
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_symbols()
    header = (_native._build.ROOT / "include" / "fheaes.h").read_text()
    for name, value in (("FHEAES_KW_MIN_SEMIBLOCKS", _native.KW_MIN_SEMIBLOCKS), ("FHEAES_KW_MAX_SEMIBLOCKS", _native.KW_MAX_SEMIBLOCKS),
                        ("FHEAES_KW_MAX_KEYS", _native.KW_MAX_KEYS)):
        assert "#define %s %d\n" % (name, value) in header
    assert (_native.KW_MIN_SEMIBLOCKS, _native.KW_MAX_SEMIBLOCKS, _native.KW_MAX_KEYS) == (2, 8, 4096)
    assert b" 0.4 " in lib.fheaes_version()


def test_new_entry_points_reject_a_null_context():
    lib = _native.load_library()
    w, u32, u8 = (ctypes.c_uint64 * 16)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 24)()
    for ms in (_native.HOST, _native.DEVICE):
        assert lib.fheaes_aes_kw_unwrap_keyed(None, w, 128, 1, 1, u32, 2, u8, w, w, ms) == INVALID
        assert lib.fheaes_aes_kw_unwrap_keyed_packed(None, w, 128, 1, 1, None, 2, u8, w, w, ms) == INVALID
        assert lib.fheaes_kw_link(None, w, w, 1, 2, 0, u8, ms) == INVALID


# ---- 6. the Python layer -------------------------------------------------------------------------------------------------------------------
def test_kw_args_builds_the_arrays():
    w1, w2 = bytes(range(24)), bytes(range(100, 124))
    a = kw_args([w1, bytearray(w2)])
    assert a["semiblocks"] == 2 and a["kek_of_key"] is None
    assert a["wrapped"].dtype == np.uint8 and a["wrapped"].shape == (2, 24) and a["wrapped"].tobytes() == w1 + w2
    a = kw_args([w1, w2, w1], kek_of_key=[2, 0, 1], n_keks=3)
    assert a["kek_of_key"] == [2, 0, 1] and a["wrapped"].shape == (3, 24)
    assert kw_args([bytes(72)])["semiblocks"] == 8 and kw_args([bytes(40)], [0])["kek_of_key"] == [0]
    empty = kw_args([])
    assert empty["semiblocks"] == 2 and empty["wrapped"].shape == (0, 24) and empty["kek_of_key"] is None
    for bad in (lambda: kw_args([w1, bytes(32)]), lambda: kw_args([bytes(16)]), lambda: kw_args([bytes(80)]), lambda: kw_args([bytes(25)]),
                lambda: kw_args([w1], n_keks=2), lambda: kw_args([w1, w2], [0], 2), lambda: kw_args([w1], [2], 2), lambda: kw_args([w1], [-1], 2)):
        with pytest.raises(ValueError):
            bad()


def test_wrapped_bytes_takes_byte_strings_and_arrays():
    w1, w2 = bytes(range(24)), bytes(range(100, 124))
    a = _native.wrapped_bytes([w1, bytearray(w2)], 2)
    assert a.dtype == np.uint8 and a.shape == (2, 24) and a.flags["C_CONTIGUOUS"] and a.tobytes() == w1 + w2
    assert np.array_equal(_native.wrapped_bytes(kw_args([w1, w2])["wrapped"][1:], 2), a[1:])
    assert _native.wrapped_bytes([], 3).shape == (0, 32)
    with pytest.raises(ValueError):
        _native.wrapped_bytes([w1], 3)


def test_server_methods_exist():
    from tfhe_aes_amd.server import Server, ServerGroup

    for cls in (Server, ServerGroup):
        assert callable(cls.aes_key_unwrap) and callable(cls.aes_key_unwrap_packed)
