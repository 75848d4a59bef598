"""XTS-AES decryption on the MI355X.  The tweak layer alone (fheaes_xts_tweaks) against numpy sums over the rows that Python-integer
doubling gives; fheaes_aes_xts_decrypt_bits word for word against xts.compose -- aes_encrypt_public, the identity
many_wopbs_without_padding, those rows, aes_decrypt_equivalent, all of them older than the call -- so every comparison is array_equal;
plaintexts from the IEEE 1619 vectors and from aes_clear.  The noise of an output word is held to tests/noise_model.py."""
import numpy as np
import pytest

import noise_model as nm
import xts
from aes_model import DEC_MULS, INV_MC, AesModel
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, oc, opt_server, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server, ServerGroup

pytestmark = pytest.mark.gpu

EDGE = (0, (1 << 64) - 1, 1 << 63, (1 << 63) - 1)
KEY1, KEY2 = bytes.fromhex("a1b2c3d4e5f60718293a4b5c6d7e8f90"), bytes.fromhex("0f1e2d3c4b5a69788796a5b4c3d2e1f0")


def _anchor(p, n_units, seed):
    """random anchors whose rows 0..3, 124..127 (and what the reduction folds onto them) are constant edge words, so that sums wrap"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, (n_units, 128, p.big1), dtype=np.uint64)
    for i, v in enumerate(EDGE):
        a[:, i] = v
        a[:, 127 - i] = EDGE[3 - i]
        a[:, 60 + i, ::2] = v
    return a


def _pt_rows(data: bytes):
    return np.frombuffer(data, dtype=np.uint8).reshape(-1, 16)


# ---- the tweak layer alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_units,off0,n_off", [(1, 0, 122), (2, 119, 3)])
def test_tweak_layer_is_the_rows_summed(toy, n_units, off0, n_off):
    p = toy.params
    eng = _native.Engine(p, device=0)                                        # no keys: the gather needs none
    try:
        a = _anchor(p, n_units, 0x7E5 + n_units)
        want = np.stack([xts.np_tweaks(a[u], range(off0, off0 + n_off)) for u in range(n_units)])
        d_a = dev(a)
        buf, rows = guarded(n_units * n_off * 128, p.big1)
        eng.xts_tweaks(d_a, n_units, off0, n_off, rows)
        eng.synchronize()
        got = host(rows).reshape(want.shape)
        assert guards_intact(buf)
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        assert eng.noise_level_seen() == (4, 5)                              # the layer's largest row, declared to the guard
        if n_units == 2:                                                     # host arrays take the same path through staging
            out = np.empty_like(want)
            eng.xts_tweaks(a, n_units, off0, n_off, out)
            assert np.array_equal(out, want)
    finally:
        eng.close()


def test_tweak_layer_refusals(toy):
    p = toy.params
    eng = _native.Engine(p, device=0)
    try:
        lib, h, D = eng._lib, eng._h, _native.DEVICE
        d_a = dev(_anchor(p, 1, 1))
        buf, rows = guarded(2 * 128, p.big1)
        for off0, n_off in ((122, 1), (121, 2), (0, 123), (0, 0)):
            assert lib.fheaes_xts_tweaks(h, d_a.data_ptr(), 1, off0, n_off, rows.data_ptr(), D) == -1 and b"121" in lib.fheaes_last_error(h)
        assert lib.fheaes_xts_tweaks(h, None, 1, 0, 1, rows.data_ptr(), D) == -1
        assert lib.fheaes_xts_tweaks(h, d_a.data_ptr(), 1, 0, 1, None, D) == -1
        assert lib.fheaes_xts_tweaks(h, d_a.data_ptr(), 1, 0, 2, d_a.data_ptr(), D) == -1 and b"overlap" in lib.fheaes_last_error(h)
        assert lib.fheaes_xts_tweaks(h, d_a.data_ptr(), 0, 0, 1, rows.data_ptr(), D) == 0
        eng.synchronize()
        assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
        assert eng.noise_level_seen() == (0, 5)
    finally:
        eng.close()


def test_inv_mix_columns_alone_is_the_four_term_gather(toy, toy_server, tc):
    """fheaes_inv_mix_columns_batch, the yardstick tools/xts.py times the tweak kernel against: gather_add_kernel with the four-term
    table and no round key, against the model's numpy sums, on host arrays and inside guard rows"""
    p = toy.params
    values = np.random.default_rng(0x1AC).integers(0, 256, 48)
    y = toy_server.many_sbox(tc.encrypt_bytes(values), inv=True).reshape(3, 16, 4, 8, p.big1)
    want = AesModel._mix(y, INV_MC, DEC_MULS, 0)
    got = np.empty_like(want)
    toy.engine().inv_mix_columns_batch(y, 3, got)
    assert np.array_equal(got, want)
    assert np.array_equal(tc.decrypt_bytes(got).reshape(-1).tolist(), sum((aes_clear._mix([int(v) for v in values[16 * b:16 * b + 16]], (14, 11, 13, 9)) for b in range(3)), []))
    buf, rows = guarded(3 * 128, p.big1)
    toy.engine().inv_mix_columns_batch(dev(y), 3, rows)
    toy.engine().synchronize()
    assert guards_intact(buf) and np.array_equal(host(rows).reshape(want.shape), want)
    lib, h = toy.engine()._lib, toy.engine()._h
    assert lib.fheaes_inv_mix_columns_batch(h, None, 3, rows.data_ptr(), _native.DEVICE) == -1
    assert lib.fheaes_inv_mix_columns_batch(h, rows.data_ptr(), 1, rows.data_ptr(), _native.DEVICE) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert lib.fheaes_inv_mix_columns_batch(h, rows.data_ptr(), 65536, rows.data_ptr(), _native.DEVICE) == -1
    assert lib.fheaes_inv_mix_columns_batch(h, None, 0, None, _native.DEVICE) == 0


# ---- the call against the composition ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(toy_server, tc):
    """(decryption round keys of key 1, round keys of key 2) of IEEE vectors 2 and 10 and of this file's own pair, made on the GPU"""
    def pair(key1, key2):
        rk1, rk2 = (toy_server.aes_key_expansion(tc.encrypt_aes_key(k)) for k in (key1, key2))
        return toy_server.aes_decryption_round_keys(rk1), rk2
    return {2: pair(*xts.VECTORS[2][:2]), 10: pair(*xts.VECTORS[10][:2]), "own": pair(KEY1, KEY2)}


def _own_data(sectors, bpu, n_units, seed):
    """random plaintext of n_units whole units under KEY1 / KEY2 and its ciphertext"""
    pt = np.random.default_rng(seed).bytes(16 * bpu * n_units)
    ct = b"".join(aes_clear.xts_encrypt(KEY1, KEY2, sectors[u], pt[16 * bpu * u:16 * bpu * (u + 1)]) for u in range(n_units))
    return pt, ct


SHAPES = {
    "vector 2": (2, None, 2, 0, 2),                      # keys, sectors, blocks per unit, first block, blocks
    "vector 10": (10, None, 32, 0, 3),
    "two units": ("own", [5, 9], 3, 1, 4),               # blocks 1, 2 of unit 0 and 0, 1 of unit 1
    "seam": ("own", [77], 123, 119, 4),                  # offset 119, then 0, 1, 2 of segment 1 through the chained anchor
}
_results = {}


def shape_case(name, toy_server, tc, keys):
    """(what the call gives, the composition, its refreshed tweaks, the plaintext of the call's blocks, the call's arguments), computed once"""
    if name not in _results:
        which, sectors, bpu, first, n = SHAPES[name]
        if sectors is None:
            _, _, sector, pt, _ = xts.VECTORS[which]
            sectors, ct = [sector], aes_clear.xts_encrypt(*xts.VECTORS[which][:4])
            assert xts.matches(ct, xts.VECTORS[which][4])
        else:
            pt, ct = _own_data(sectors, bpu, len(sectors), 0x515)
        pt, ct = pt[16 * first:16 * (first + n)], ct[16 * first:16 * (first + n)]
        dw1, rk2 = keys[which]
        got = toy_server.aes_xts_decrypt(dw1, rk2, sectors, ct, unit_bytes=16 * bpu, first_block=first)
        want, T = xts.compose(toy_server, tc, dw1, rk2, sectors, ct, bpu, first)
        _results[name] = (got, want, T, pt, (dw1, rk2, sectors, ct, 16 * bpu, first))
    return _results[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_toy_call_is_the_composition(toy, toy_server, tc, keys, name):
    got, want, _, pt, _ = shape_case(name, toy_server, tc, keys)
    assert got.shape == (len(pt) // 16, 16, 8, toy.params.big1) and got.dtype == np.uint64
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    assert np.array_equal(tc.decrypt_bytes(got), _pt_rows(pt))


def test_toy_seam_plaintext_is_aes_clear(toy_server, tc, keys):
    got, _, _, pt, (_, _, sectors, ct, unit_bytes, first) = shape_case("seam", toy_server, tc, keys)
    assert aes_clear.xts_decrypt(KEY1, KEY2, sectors[0], ct, first_block=first) == pt
    assert _native.aes_xts_plan(1, unit_bytes // 16, first, 4)["segments"] == 2


def test_toy_host_arrays_and_resident_tensors_agree(toy, toy_server, tc, keys):
    p = toy.params
    want, _, _, _, (dw1, rk2, sectors, ct, unit_bytes, first) = shape_case("two units", toy_server, tc, keys)
    buf, rows = guarded(4 * 128, p.big1)
    got = toy_server.aes_xts_decrypt(dev(dw1), dev(rk2), sectors, ct, unit_bytes=unit_bytes, first_block=first, out=rows.view(4, 16, 8, p.big1))
    toy_server.synchronize()
    assert got.is_cuda and guards_intact(buf)
    assert np.array_equal(host(got), want)


def test_toy_packed_stores_and_lwe_form_keys_agree(toy_server, tc, keys):
    want, _, _, _, (dw1, rk2, sectors, ct, unit_bytes, first) = shape_case("two units", toy_server, tc, keys)
    p1, p2 = toy_server.pack_round_keys(dw1), toy_server.pack_round_keys(rk2)
    got = toy_server.aes_xts_decrypt(p1, p2, sectors, ct, unit_bytes=unit_bytes, first_block=first)
    unpacked = toy_server.aes_xts_decrypt(toy_server.unpack_round_keys(p1)[0], toy_server.unpack_round_keys(p2)[0], sectors, ct, unit_bytes=unit_bytes,
                                          first_block=first)
    assert np.array_equal(got, unpacked)
    assert np.array_equal(tc.decrypt_bytes(got), tc.decrypt_bytes(want))
    assert np.array_equal(toy_server.aes_xts_decrypt(p1, rk2, sectors, ct, unit_bytes=unit_bytes, first_block=first), got)      # one form per call: rk2 is packed first


def test_toy_server_group_shards_inside_a_unit(toy, toy_server, tc, keys):
    dw1, rk2 = keys["own"]
    pt, ct = _own_data([3, 4], 4, 2, 0x6B0)
    pt, ct = pt[:96], ct[:96]                                                  # 6 blocks of 4-block units on 2 contexts: the cut is inside unit 0
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        got = group.aes_xts_decrypt(dw1, rk2, 3, ct, unit_bytes=64)
    finally:
        for s in group.servers:
            s.engine.close()
    assert np.array_equal(got, toy_server.aes_xts_decrypt(dw1, rk2, 3, ct, unit_bytes=64))
    assert np.array_equal(tc.decrypt_bytes(got), _pt_rows(pt))


def test_toy_noise_level_and_equal_sectors(toy, tc):
    srv = Server(toy.keys, device=0)
    try:
        assert srv.engine.noise_level_seen() == (0, 5)
        rk1, rk2 = (srv.aes_key_expansion(tc.encrypt_aes_key(k)) for k in (KEY1, KEY2))
        dw1 = srv.aes_decryption_round_keys(rk1)
        ct = aes_clear.xts_encrypt(KEY1, KEY2, 7, bytes(range(32)))
        twice = srv.aes_xts_decrypt(dw1, rk2, [7, 7], ct + ct, unit_bytes=32)
        seen, limit = srv.engine.noise_level_seen()
        assert seen <= 5 and limit == 5
        once = srv.aes_xts_decrypt(dw1, rk2, [7], ct, unit_bytes=32)
    finally:
        srv.engine.close()
    assert np.array_equal(twice[:2], twice[2:]) and np.array_equal(twice[:2], once)       # sharing the tweaks' S-Boxes is invisible in the result
    assert np.array_equal(tc.decrypt_bytes(once), _pt_rows(bytes(range(32))))


def test_toy_output_noise(toy, toy_server, tc, keys):
    """An output word is InvS (a fresh WoPBS output whose input byte, at the output's position p, is SBOX[x_p ^ key1_p], x = P ^ T the
    cipher's result) + dw[0] = w[0], the client's own encryption of key 1 + the refreshed T (a fresh identity WoPBS output on T's byte).
    Four blocks: 64 bytes of each kind, independent word by word at PARAM_TOY (noise_model.wopbs_independent)."""
    M = nm.NoiseModel.of_client(toy.client)
    got, _, _, pt, (_, _, sectors, ct, unit_bytes, first) = shape_case("two units", toy_server, tc, keys)
    bpu = unit_bytes // 16
    T = np.array([xts.tweak_bytes(KEY2, sectors[(first + b) // bpu], (first + b) % bpu) for b in range(4)], dtype=np.int64)
    x = _pt_rows(pt).astype(np.int64) ^ T
    last = np.array(aes_clear.SBOX, dtype=np.int64)[x ^ np.frombuffer(KEY1, dtype=np.uint8).astype(np.int64)[None]]
    fresh_key = (toy.params.glwe_noise_std * 2.0 ** 64) ** 2
    var = (M.wopbs(8, last) + fresh_key + M.wopbs(8, T))[:, :, None]
    err, vals = nm.wopbs_error(tc, got)
    assert np.array_equal(vals, _pt_rows(pt))
    n = M.wopbs_independent(64, 8)
    assert nm.rejects_doubling(n)
    nm.assert_noise(err, var, n, "XTS output toy", left_out=2 * M.wopbs_left_out())


def test_toy_errors_leave_the_output_untouched(toy, toy_server, tc, keys):
    p = toy.params
    eng = toy.engine()
    lib, h, D = eng._lib, eng._h, _native.DEVICE
    dw1, rk2 = keys["own"]
    d_dw1, d_rk2 = dev(dw1), dev(rk2)
    buf, rows = guarded(2 * 128, p.big1)
    out = rows.view(2, 16, 8, p.big1)
    bp = _native.u128_pairs([1, 2]).ctypes.data_as(_native._u64p)
    call = lambda k1, k2, bits, tw, n_units, bpu, first, c, n, o: lib.fheaes_aes_xts_decrypt_bits(h, k1, k2, bits, tw, n_units, bpu, first, c, n, o, D)
    k1, k2, o = d_dw1.data_ptr(), d_rk2.data_ptr(), out.data_ptr()
    assert call(k1, k2, 192, bp, 1, 2, 0, bp, 2, o) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert call(k1, k2, 100, bp, 1, 2, 0, bp, 2, o) == -1
    assert call(k1, k2, 128, bp, 1, 0, 0, bp, 2, o) == -1 and b"blocks_per_unit" in lib.fheaes_last_error(h)
    assert call(k1, k2, 128, bp, 1, (1 << 20) + 1, 0, bp, 2, o) == -1
    assert call(k1, k2, 128, bp, 1, 2, 1, bp, 2, o) == -1 and b"n_units" in lib.fheaes_last_error(h)      # block 2 lies in unit 1
    assert call(k1, k2, 128, bp, 0, 2, 0, bp, 2, o) == -1
    for nulls in ((None, k2, bp, bp, o), (k1, None, bp, bp, o), (k1, k2, None, bp, o), (k1, k2, bp, None, o), (k1, k2, bp, bp, None)):
        assert call(nulls[0], nulls[1], 128, nulls[2], 1, 2, 0, nulls[3], 2, nulls[4]) == -1
    assert call(k1, k2, 128, bp, 1, 2, 0, bp, 2, k1) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(k1, k2, 128, bp, 1, 2, 0, bp, 2, k2) == -1
    assert call(k1, k2, 128, bp, 1, 2, 0, bp, 0, o) == 0
    for bad in (lambda: toy_server.aes_xts_decrypt(d_dw1, d_rk2, 0, bytes(17), out=out),
                lambda: toy_server.aes_xts_decrypt(d_dw1, d_rk2, 0, bytes(32), unit_bytes=24, out=out),
                lambda: toy_server.aes_xts_decrypt(d_dw1, d_rk2, [0], bytes(32), unit_bytes=16, out=out),
                lambda: toy_server.aes_xts_decrypt(d_dw1, dev(keys[10][1]), 0, bytes(32), out=out),
                lambda: toy_server.aes_xts_decrypt(d_dw1, d_rk2, 0, bytes(48), out=out)):
        with pytest.raises(ValueError):
            bad()
    toy_server.synchronize()
    assert bool((rows == SENTINEL).all().item()) and guards_intact(buf)
    assert toy_server.aes_xts_decrypt(dw1, rk2, 0, b"").shape == (0, 16, 8, p.big1)
    fresh = _native.Engine(p, device=0)                                       # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_xts_decrypt_bits(dw1, rk2, 128, [0], 2, 0, [1], np.empty((1, 16, 8, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


# ---- PARAM_OPT ----------------------------------------------------------------------------------------------------------------------------------
def test_param_opt_vector_2(opt, opt_server, oc):
    key1, key2, sector, pt, expected = xts.VECTORS[2]
    ct = aes_clear.xts_encrypt(key1, key2, sector, pt)
    assert ct == expected
    rk1, rk2 = (opt_server.aes_key_expansion(oc.encrypt_aes_key(k)) for k in (key1, key2))
    dw1 = opt_server.aes_decryption_round_keys(rk1)
    got = opt_server.aes_xts_decrypt(dw1, rk2, sector, ct, unit_bytes=32)
    want, _ = xts.compose(opt_server, oc, dw1, rk2, [sector], ct, 2)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    assert np.array_equal(oc.decrypt_bytes(got), _pt_rows(pt))
