"""Every chunked entry point across its chunk seam, at PARAM_TOY (tests/chunk_seams.py has the shapes and why each is the smallest that
crosses).  The host code cuts batches above MAX_CHUNK_BITS = 32,768 bits (64 GLWEs, 23 AES-128 keys, 2 GiB of CMUX tree) into chunks and
caps grids with stride loops; the second chunk's pointer arithmetic ran under no test.  Every comparison is array_equal on uint64 words
against numpy / Python-integer references, the oracle, or the same entry point on a batch that fits one chunk; the data differs on both
sides of every seam, so a second chunk that reads or writes at the first chunk's offset gives other words.  Every test takes a context of
its own -- a chunk size can depend on what a context ran before -- and asserts from its profile counters that the seam was crossed;
resident outputs sit between sentinel guard rows."""
import numpy as np
import pytest

import chunk_seams as cs
import wire_formats as wf
from aes_model import ref_pack, ref_unpack
from gpu_support import dev, guarded, guards_intact, host, settled, tc  # noqa: F401
from oracle import oracle as orc
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.client import SeededCiphertexts, packed_mod_words, test_key as det_key
from tfhe_aes_amd.server import Server, gen_lut

pytestmark = pytest.mark.gpu

OFF = _native.AES_WINDOW_OFF


def _guarded_copy(a, rows):
    """a host array as the middle rows of a sentinel-guarded device tensor: an in-place call's state between guard rows"""
    a = np.ascontiguousarray(a)
    buf, mid = guarded(rows, a.size // rows)
    mid.copy_(dev(a.reshape(rows, -1)))
    return settled(buf), mid


def _stage(prof, name, launches, units):
    assert (prof[name]["launches"], prof[name]["units"]) == (launches, units), "%s: %r" % (name, prof[name])


def _differ(got, want):
    return "%d words differ" % int((got != want).sum())


# ---- A. data movement ------------------------------------------------------------------------------------------------------------------------
def test_unpack_bits_second_launch_starts_at_glwe_64(toy):
    p = toy.params
    glwe = cs.random_words(0xA1, (cs.M_GLWES, (p.k + 1) * p.N))
    eng = _native.Engine(p, device=0)                                         # unpacking needs no keys
    try:
        d_in = dev(glwe)
        buf, rows = guarded(cs.M_BITS, p.big1)
        eng.profile_reset()
        eng.unpack_bits(d_in, cs.M_BITS, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "linear", cs.M_LAUNCHES, cs.M_BITS)
        got, want = host(rows), ref_unpack(glwe, cs.M_BITS, p)
        assert np.array_equal(got, want), _differ(got, want)
        assert guards_intact(buf)
    finally:
        eng.close()


@pytest.mark.parametrize("w", [13, 16])
def test_unpack_bits_mod_second_launch_reads_its_fields(toy, w):
    """width 13: fields that straddle words, and a GLWE stride of 208 words, no power of two"""
    p = toy.params
    fields = (p.k + 1) * p.N
    packed = cs.random_words(0xA2 + w, (cs.M_GLWES, packed_mod_words(p, w)))
    eng = _native.Engine(p, device=0)
    try:
        d_in = dev(packed)
        buf, rows = guarded(cs.M_BITS, p.big1)
        eng.profile_reset()
        eng.unpack_bits_mod(d_in, cs.M_BITS, w, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "linear", cs.M_LAUNCHES, cs.M_BITS)
        got, want = host(rows), ref_unpack(wf.read_back_glwes(packed, fields, w), cs.M_BITS, p)
        assert np.array_equal(got, want), _differ(got, want)
        assert guards_intact(buf)
    finally:
        eng.close()


@pytest.mark.parametrize("w", [13, 16])
def test_packed_mod_switch_of_66_glwes_with_the_edge_words_at_the_seam(toy, w):
    p = toy.params
    glwe = cs.edge_glwes_at_the_seam(w, (p.k + 1) * p.N)
    want = wf.switch_glwes(glwe, w)
    eng = _native.Engine(p, device=0)
    try:
        d_in = dev(glwe)
        buf, rows = guarded(cs.M_GLWES, want.shape[1])
        eng.profile_reset()
        eng.packed_mod_switch(d_in, cs.M_GLWES, w, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "linear", cs.chunks(cs.M_GLWES, cs.CHUNK_GLWES), cs.M_GLWES * p.N)
        got = host(rows)
        assert np.array_equal(got, want), _differ(got, want)
        assert guards_intact(buf)
    finally:
        eng.close()


@pytest.mark.parametrize("case", sorted(cs.FIRST_INDICES))
def test_expand_lwe_seeded_second_launch_continues_the_index(toy, case):
    p, first = toy.params, cs.FIRST_INDICES[case]
    assert (first + cs.MAX_CHUNK_BITS) % (1 << 64) in ((1 << 32) - 2, (1 << 64) - 1)
    sc = SeededCiphertexts(p, det_key(0xE8, 4, 0x5EA), first, cs.random_words(0xA4, cs.M_BITS))
    want = sc.expand()
    eng = _native.Engine(p, device=0)
    try:
        d_bodies = dev(sc.bodies)
        buf, rows = guarded(cs.M_BITS, p.big1)
        eng.profile_reset()
        eng.expand_lwe_seeded(sc.mask_key, first, d_bodies, cs.M_BITS, rows)
        eng.synchronize()
        _stage(eng.profile_read(), "linear", cs.M_LAUNCHES, cs.M_BITS)
        got = host(rows)
        assert np.array_equal(got, want), _differ(got, want)
        assert guards_intact(buf)
    finally:
        eng.close()


def test_pack_bits_at_the_chunk_cap(toy):
    """a workspace sized for 32,768 bits has room for 65,536 here, so MAX_CHUNK_BITS is what cuts: two chunks.  A full oracle key switch of
    33k bits is too slow on the CPU and GLWE g depends on bits g N .. g N + N - 1 alone: the call in two parts gives the same words, and
    GLWEs 63, 64 and 65 are the reference packing of their 1,025 bits.  Then the same at width 16 against the switch of the 64-bit result"""
    p = toy.params
    gw, m = (p.k + 1) * p.N, cs.M_BITS
    lwe = cs.random_words(0xA5, (m, p.big1))                                  # any words: the key switch is pure integer arithmetic
    eng = _native.Engine(p, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        eng.reserve(cs.MAX_CHUNK_BITS)
        d_lwe = dev(lwe)
        buf, rows = guarded(cs.M_GLWES, gw)
        eng.profile_reset()
        eng.pack_bits(d_lwe, m, rows)
        eng.synchronize()
        prof = eng.profile_read()
        _stage(prof, "pfpks", 2, m)
        _stage(prof, "linear", 2, m)
        got = host(rows)
        assert guards_intact(buf)
        pbuf, parts = guarded(cs.M_GLWES, gw)
        eng.profile_reset()
        eng.pack_bits(d_lwe[:cs.MAX_CHUNK_BITS], cs.MAX_CHUNK_BITS, parts[:cs.CHUNK_GLWES])
        eng.pack_bits(d_lwe[cs.MAX_CHUNK_BITS:], m - cs.MAX_CHUNK_BITS, parts[cs.CHUNK_GLWES:])
        eng.synchronize()
        _stage(eng.profile_read(), "pfpks", 2, m)
        assert np.array_equal(got, host(parts)), _differ(got, host(parts))
        assert guards_intact(pbuf)
        lo = (cs.CHUNK_GLWES - 1) * p.N
        want = ref_pack(toy, lwe[lo:])
        assert want.shape == (3, gw) and np.array_equal(got[cs.CHUNK_GLWES - 1:], want), _differ(got[cs.CHUNK_GLWES - 1:], want)
        # width 16: every chunk folded into the workspace and switched from there
        mbuf, mrows = guarded(cs.M_GLWES, packed_mod_words(p, 16))
        eng.profile_reset()
        eng.pack_bits_mod(d_lwe, m, 16, mrows)
        eng.synchronize()
        prof = eng.profile_read()
        _stage(prof, "pfpks", 2, m)
        _stage(prof, "linear", 2, m)
        want16 = wf.switch_glwes(got, 16)
        assert np.array_equal(host(mrows), want16), _differ(host(mrows), want16)
        assert guards_intact(mbuf)
    finally:
        eng.close()


# ---- B. many AES keys ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys29(tc):
    """(clear bytes [29][11][16], their encryptions [29][11][16][8][kN+1]): round keys need not come from a key expansion"""
    clear = np.random.default_rng(0xB29).integers(0, 256, (cs.N_KEYS_PACK, 11, 16)).astype(np.uint8)
    return clear, tc.encrypt_bytes(clear.reshape(-1)).reshape(cs.N_KEYS_PACK, 11, 16, 8, -1)


def test_pack_round_keys_of_29_keys_in_2_and_in_15_chunks(toy, keys29):
    p = toy.params
    _, rk = keys29
    n, G, m, gw = cs.N_KEYS_PACK, 3, cs.KEY_BITS_PACKED, (p.k + 1) * p.N
    srv, small = Server(toy.keys, device=0), Server(toy.keys, device=0)
    try:
        d_rk = dev(rk)
        buf, rows = guarded(n * G, gw)
        srv.engine.profile_reset()
        srv.engine.pack_round_keys(d_rk, 128, n, rows)                        # a fresh context: chunks of 23 keys
        srv.synchronize()
        prof = srv.engine.profile_read()
        _stage(prof, "pfpks", cs.chunks(n, cs.KEYS_PER_CHUNK), n * m)
        _stage(prof, "linear", 2, n * m)
        store = host(rows).reshape(n, G, gw)
        assert guards_intact(buf)
        small.engine.reserve(2048)                                            # a workspace of 2,048 x 2,048 words: 4,096 / 1,408 = 2 keys a chunk
        sbuf, srows = guarded(n * G, gw)
        small.engine.profile_reset()
        small.engine.pack_round_keys(d_rk, 128, n, srows)
        small.synchronize()
        _stage(small.engine.profile_read(), "pfpks", 15, n * m)
        assert np.array_equal(host(srows).reshape(n, G, gw), store) and guards_intact(sbuf)
        for i in range(n):
            want = srv.pack(rk[i])
            assert np.array_equal(store[i], want), "key %d: %s" % (i, _differ(store[i], want))
        for i in (cs.KEYS_PER_CHUNK - 1, cs.KEYS_PER_CHUNK, n - 1):
            assert np.array_equal(store[i], ref_pack(toy, rk[i])), "key %d against the reference packing" % i
        first, count = cs.KEYS_PER_CHUNK - 1, n - cs.KEYS_PER_CHUNK + 1       # 22, 7
        ubuf, urows = guarded(count * m, p.big1)
        srv.engine.profile_reset()
        srv.engine.unpack_round_keys(rows, 128, first, count, urows)
        srv.synchronize()
        _stage(srv.engine.profile_read(), "linear", count, count * m)
        want = np.concatenate([ref_unpack(store[first + j], m, p) for j in range(count)])
        assert np.array_equal(host(urows), want) and guards_intact(ubuf)
    finally:
        srv.engine.close()
        small.engine.close()


def test_decryption_round_keys_of_29_keys_with_the_seam_inside_key_28(toy, keys29, tc):
    """144 middle bytes per key, 4,176 bytes, 33,408 bits: both WoPBS take two chunks, and chunk 2 starts at middle byte 64 of key 28"""
    p = toy.params
    clear, rk = keys29
    n = cs.N_KEYS_PACK
    bits = n * cs.MID_BYTES * 8
    assert cs.MAX_CHUNK_BITS // 8 - (n - 1) * cs.MID_BYTES == 64
    srv = Server(toy.keys, device=0)
    try:
        d_rk = dev(rk)
        buf, rows = guarded(n * 11 * 16 * 8, p.big1)
        srv.engine.profile_reset()
        srv.engine.aes_decryption_round_keys_batch(d_rk, 128, n, rows)
        srv.synchronize()
        prof = srv.engine.profile_read()
        _stage(prof, "keyswitch", 4, 2 * bits)
        _stage(prof, "blind_rotate", 4, 2 * bits)
        dw = host(rows).reshape(rk.shape)
        assert guards_intact(buf)
        for i in range(n):
            want = srv.aes_decryption_round_keys(rk[i])
            assert np.array_equal(dw[i], want), "key %d: %s" % (i, _differ(dw[i], want))
        want = np.array([aes_clear.inv_mix_columns_round_keys(clear[i].tolist()) for i in range(n)], dtype=np.uint8)
        assert np.array_equal(tc.decrypt_bytes(dw), want)
    finally:
        srv.engine.close()


def test_key_expansion_of_1025_keys_resident(toy, tc):
    """4 bytes per key and step: 4,100 bytes, 32,800 bits, key 1,024 alone in chunk 2 of each of the 50 WoPBS; 5.9 GB of round keys that
    stay on the GPU but for slices 0, 1, 1,023 and 1,024"""
    import torch

    p, n = toy.params, cs.N_KEYS_EXPAND
    keys = np.random.default_rng(0xB8).integers(0, 256, (n, 16)).astype(np.uint8)
    keys[n - 1] = keys[0] ^ np.random.default_rng(0xB9).integers(1, 256, 16).astype(np.uint8)      # differs from key 0 in every byte position
    assert len({k.tobytes() for k in keys}) == n and (keys[n - 1] != keys[0]).all()
    ek = tc.encrypt_bytes(keys.reshape(-1)).reshape(n, 16, 8, p.big1)
    idx = [0, 1, n - 2, n - 1]
    srv = Server(toy.keys, device=0)
    buf = rows = d_ek = None
    try:
        d_ek = dev(ek)
        buf, rows = guarded(n * 11 * 16 * 8, p.big1)
        srv.engine.profile_reset()
        srv.engine.aes_key_expansion_batch(d_ek, 128, n, rows)
        srv.synchronize()
        prof = srv.engine.profile_read()
        _stage(prof, "keyswitch", 2 * cs.EXPAND_WOPBS, cs.EXPAND_WOPBS * 4 * n * 8)
        assert guards_intact(buf)
        got = host(settled(rows.view(n, 11 * 16 * 8 * p.big1)[idx])).reshape(4, 11, 16, 8, p.big1)
        for j, i in enumerate(idx):
            want = srv.aes_key_expansion(ek[i])
            assert np.array_equal(got[j], want), "key %d: %s" % (i, _differ(got[j], want))
            assert np.array_equal(tc.decrypt_bytes(got[j]), np.array(aes_clear.expand_key(keys[i].tobytes()), dtype=np.uint8)), "key %d" % i
    finally:
        srv.engine.close()
        del buf, rows, d_ek
        torch.cuda.empty_cache()


# ---- C. WoPBS --------------------------------------------------------------------------------------------------------------------------------
def test_wopbs_with_per_input_luts_across_the_seam(toy, tc):
    """3,641 inputs of 9 bits, input i under v -> (v + a_i) mod 512 with a_i = i mod 509: the second chunk's LUTs start at input 3,640"""
    p, n, nb = toy.params, cs.PER_INPUT_N, cs.PER_INPUT_BITS
    adds = cs.per_input_adds()
    vals = np.random.default_rng(0xC9).integers(0, 1 << nb, n)
    x = tc.encrypt_bits(cs.bits_of(vals, nb))
    base = np.stack([gen_lut(2, 1, 512, nb, lambda v, a=a: (v + a) % 512) for a in range(cs.PER_INPUT_LUTS)])
    luts = np.ascontiguousarray(base[adds][:, None])                          # [n][1][9][512]
    eng = _native.Engine(p, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        d_x, d_luts = dev(x), dev(luts)
        buf, rows = guarded(n * nb, p.big1)
        eng.profile_reset()
        eng.wopbs_batch(d_x, n, nb, d_luts, 1, True, rows)
        eng.synchronize()
        prof = eng.profile_read()
        _stage(prof, "keyswitch", 2, n * nb)
        _stage(prof, "vertical_packing", 2, n * nb)
        got = host(rows).reshape(n, 1, nb, p.big1)
        assert guards_intact(buf)
        dec = tc.decrypt_bits(got)[:, 0].astype(np.int64)
        assert np.array_equal((dec << np.arange(nb)).sum(axis=1), (vals + adds) % 512)
        sl = slice(cs.PER_INPUT_CHUNK - 2, cs.PER_INPUT_CHUNK + 1)            # the last two inputs of chunk 1, the first of chunk 2
        want = toy.oracle.wopbs_batch(x[sl], luts[sl], lut_per_input=True)
        assert np.array_equal(got[sl], want), _differ(got[sl], want)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def wide_luts():
    """width -> LUTs [n][width][2^width]: four functions at 16 bits, one at 13, 14 and 15"""
    out = {cs.TREE_BITS: np.stack([gen_lut(2, 1, 512, cs.TREE_BITS, f) for f in cs.TREE_FUNCTIONS])}
    for nb in (13, 14, 15):
        out[nb] = np.stack([gen_lut(2, 1, 512, nb, lambda v, nb=nb: cs.TREE_FUNCTIONS[0](v) % (1 << nb))])
    return out


def test_wopbs_of_16_bits_reaches_the_chunk_bound_of_the_cmux_tree(toy, tc, wide_luts):
    """4 LUTs x 16 output bits x 2^7 GLWEs x 8 KB = 2^26 bytes of tree per input: 32 inputs fill the 2 GiB bound, input 32 is chunk 2"""
    p, n, nb, nl = toy.params, cs.TREE_N, cs.TREE_BITS, cs.TREE_LUTS
    vals = cs.tree_values()
    x = tc.encrypt_bits(cs.bits_of(vals, nb))
    luts = wide_luts[nb]
    eng = _native.Engine(p, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        d_x, d_luts = dev(x), dev(luts)
        buf, rows = guarded(n * nl * nb, p.big1)
        eng.profile_reset()
        eng.wopbs_batch(d_x, n, nb, d_luts, nl, False, rows)
        eng.synchronize()
        prof = eng.profile_read()
        _stage(prof, "keyswitch", cs.chunks(n, cs.TREE_CHUNK), n * nb)
        _stage(prof, "vertical_packing", 2, n * nl * nb)
        got = host(rows).reshape(n, nl, nb, p.big1)
        assert guards_intact(buf)
        dec = tc.decrypt_bits(got)
        for i, v in enumerate(vals):
            for li, f in enumerate(cs.TREE_FUNCTIONS):
                assert cs.value_of(dec[i, li]) == f(v), (i, v, li)
        idx = [0, cs.TREE_CHUNK - 1, cs.TREE_CHUNK]
        want = toy.oracle.wopbs_batch(x[idx], luts)
        assert np.array_equal(got[idx], want), _differ(got[idx], want)
    finally:
        eng.close()


@pytest.mark.parametrize("nb", [13, 14, 15, 16])
def test_wopbs_widths_13_to_16_against_the_oracle(toy, tc, wide_luts, nb):
    """4 to 7 tree levels, both parities of the ping-pong root"""
    p = toy.params
    luts = wide_luts[nb][:1]
    f = (lambda v: cs.TREE_FUNCTIONS[0](v) % (1 << nb))
    vals = [(1 << nb) - 1, 0x1A5C % (1 << nb), (1 << (nb - 1)) | 0x203]
    x = tc.encrypt_bits(cs.bits_of(vals, nb))
    eng = _native.Engine(p, device=0)
    try:
        eng.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        d_x, d_luts = dev(x), dev(luts)
        buf, rows = guarded(3 * nb, p.big1)
        eng.wopbs_batch(d_x, 3, nb, d_luts, 1, False, rows)
        eng.synchronize()
        got = host(rows).reshape(3, 1, nb, p.big1)
        assert guards_intact(buf)
        want = toy.oracle.wopbs_batch(x, luts)
        assert np.array_equal(got, want), _differ(got, want)
        dec = tc.decrypt_bits(got)
        assert [cs.value_of(dec[i, 0]) for i in range(3)] == [f(v) for v in vals]
    finally:
        eng.close()


# ---- D. K4's second pass ---------------------------------------------------------------------------------------------------------------------
def test_forward_fourier_second_pass_of_a_workgroup(toy):
    """131,072 + 17 polynomials: 8,192 workgroups x 16, then workgroups 0 and 1 come round again and reuse their LDS tiles"""
    distinct, which = cs.fourier_inputs()
    polys = len(which)
    assert polys == cs.FOURIER_FIRST_PASS + cs.FOURIER_TAIL
    four = orc.polys_to_fourier(distinct).view(np.uint64).reshape(len(distinct), 512)
    eng = _native.Engine(toy.params, device=0)
    try:
        d_in = dev(distinct[which])
        buf, rows = guarded(polys, 512)
        eng.profile_reset()
        eng.forward_fourier_batch(d_in, rows, polys)
        eng.synchronize()
        _stage(eng.profile_read(), "ggsw_fft", 1, polys)
        got = host(rows)
        assert guards_intact(buf)
        same = (got == four[which]).all(axis=1)
        assert same.all(), "%d rows differ, the first at %d" % (int((~same).sum()), int(np.argmin(same)))
    finally:
        eng.close()


# ---- E. linear layers and schedules above 256 blocks -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks257(tc):
    """3 clear AES-128 keys and their round keys encrypted byte by byte, 257 random blocks and their encryptions, a key per block"""
    rng = np.random.default_rng(0xE12)
    keys = [rng.bytes(16) for _ in range(3)]
    rk = np.stack([tc.encrypt_bytes(np.array(aes_clear.expand_key(k), dtype=np.uint8).reshape(-1)).reshape(11, 16, 8, -1) for k in keys])
    pts = [int.from_bytes(rng.bytes(16), "big") for _ in range(cs.BLOCKS)]
    kob = [b % 3 for b in range(cs.BLOCKS)]
    assert kob[256] != kob[0] and kob[256] != kob[255]
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    return dict(keys=keys, rk=rk, pts=pts, kob=kob, st=st)


@pytest.mark.parametrize("window", [OFF, cs.WINDOW], ids=["round by round", "window 200"])
@pytest.mark.parametrize("source", ["lwe", "packed"])
def test_257_blocks_under_3_keys(toy, tc, blocks257, source, window):
    """a step of 257 blocks is 32,896 bits: two WoPBS chunks, block 256 behind the seam and in add_bcast_kernel's second pass, under another
    key than blocks 0 and 255.  Blocks 0, 1, 255 and 256 are the words of the same call on the sub-batches [0:2] and [255:257] (a WoPBS is
    a function of its input words).  Windows of 200 blocks straddle steps and read key_of_block from block 200 on"""
    p, t, n = toy.params, blocks257, cs.BLOCKS
    kob, sw = t["kob"], 16 * 8 * p.big1
    srv = Server(toy.keys, device=0)
    eng = srv.engine
    try:
        eng.aes_set_window(window)
        d_keys = dev(t["rk"])
        if source == "packed":
            pbuf, prows = guarded(3 * 3, (p.k + 1) * p.N)
            eng.pack_round_keys(d_keys, 128, 3, prows)
            srv.synchronize()
            assert guards_intact(pbuf)
            d_keys = prows
        enc_call = eng.aes_encrypt_keyed_packed if source == "packed" else eng.aes_encrypt_keyed
        dec_call = eng.aes_decrypt_keyed_packed if source == "packed" else eng.aes_decrypt_keyed

        def run(call, state, lo, hi, steps=None):
            buf, rows = _guarded_copy(state[lo:hi], (hi - lo) * 128)
            eng.profile_reset()
            call(d_keys, 128, 3, kob[lo:hi], rows, hi - lo)
            srv.synchronize()
            if steps:
                prof = eng.profile_read()
                if window == OFF:
                    _stage(prof, "keyswitch", 2 * steps, steps * n * 128)
                    _stage(prof, "blind_rotate", 2 * steps, steps * n * 128)
                else:
                    k2, k1 = cs.window_launches(n, steps, window)
                    _stage(prof, "keyswitch", k1, steps * n * 128)
                    _stage(prof, "blind_rotate", k2, steps * n * 128)
                _stage(prof, "linear", 1 + (steps if window == OFF else k1), (1 + steps) * n)
            assert guards_intact(buf)
            return host(rows).reshape(hi - lo, 16, 8, p.big1)

        enc = run(enc_call, t["st"], 0, n, steps=10)
        for lo, hi in ((0, 2), (n - 2, n)):
            want = run(enc_call, t["st"], lo, hi)
            assert np.array_equal(enc[lo:hi], want), "encrypt, blocks %d..%d: %s" % (lo, hi, _differ(enc[lo:hi], want))
        assert [tc.decrypt_u128(enc[b]) for b in range(n)] == [aes_clear.aes_encrypt_block(t["keys"][k], v) for k, v in zip(kob, t["pts"])]
        dec = run(dec_call, enc, 0, n, steps=19)
        for lo, hi in ((0, 2), (n - 2, n)):
            want = run(dec_call, enc, lo, hi)
            assert np.array_equal(dec[lo:hi], want), "decrypt, blocks %d..%d: %s" % (lo, hi, _differ(dec[lo:hi], want))
        assert [tc.decrypt_u128(dec[b]) for b in range(n)] == t["pts"]
    finally:
        eng.close()


def test_public_blocks_with_pools_above_one_chunk(toy, tc, blocks257):
    """300 random blocks share nothing from round 2 on: pools of 4,800 bytes, 38,400 bits, two chunks per WoPBS and an indexed gather over
    more than 4,096 pool entries.  The pool of round 1 holds the distinct (position, byte) pairs, at most 4,096 for any batch: one chunk"""
    p, n = toy.params, cs.PUBLIC_BLOCKS
    rng = np.random.default_rng(0xE13)
    blocks = [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]
    key, rk = blocks257["keys"][0], blocks257["rk"][0]
    plan = _native.aes_public_plan(blocks)
    first = cs.public_pool_round_1(blocks)
    assert plan == [first] + [16 * n] * 9 and first <= 4096
    srv = Server(toy.keys, device=0)
    try:
        d_rk = dev(rk)
        buf, rows = guarded(n * 128, p.big1)
        srv.engine.profile_reset()
        srv.aes_encrypt_public(d_rk, blocks, out=rows.view(n, 16, 8, p.big1))
        srv.synchronize()
        prof = srv.engine.profile_read()
        _stage(prof, "keyswitch", 1 + 2 * 9, 8 * sum(plan))
        _stage(prof, "blind_rotate", 1 + 2 * 9, 8 * sum(plan))
        assert prof["linear"]["launches"] == 11
        got = host(rows).reshape(n, 16, 8, p.big1)
        assert guards_intact(buf)
        for b in (0, 255, 256, n - 1):
            want = srv.aes_encrypt_public(rk, [blocks[b]])[0]
            assert np.array_equal(got[b], want), "block %d: %s" % (b, _differ(got[b], want))
        assert [tc.decrypt_u128(got[b]) for b in range(n)] == [aes_clear.aes_encrypt_block(key, v) for v in blocks]
    finally:
        srv.engine.close()
