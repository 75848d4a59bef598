"""Every call array across byte 2^31 and byte 2^32, at PARAM_TOY (limits.py has the shapes, the counts and the reasoning).

A dropped high half in one `row * words + w`, in the pointer arithmetic of a chunked entry point or in a host cast gives perfectly
formed wrong ciphertexts for every unit past the line and nothing else.  Each test here puts one array of a call beyond byte 2^32
(the smallest count that leaves two whole units there -- where the entry point cuts its batch into chunks, two units into the first
chunk that starts beyond the line, so that the host's pointer to a chunk passes it as well as the kernels' offsets), as a view that begins 2^31 bytes and two guard units into an allocation of
its own, sentinel in front and behind: a sign-extended 32-bit offset lands in the margin and changes a sentinel, a zero-extended one
lands inside the array, on a unit of another residue.

Data.  Unit i of a crossing array is unit i mod P of a base of P honest units (P prime, limits.py).  The expected output is the output
of the same call on the first P units, tiled the same way; that base call is pinned first -- against the CPU oracle word for word for
the crypto stages, against the numpy models the suite already has for the data movers.  All units are compared on the device in
slices of 256 MB; a mismatch reports the first differing unit and word.  Every test asserts, before it compares anything, that its
array's last byte lies beyond 2^32 and, from the profile counters, that the launches that hold the line ran.

Every test has a context of its own and at most three allocations of crossing size; they are freed when the test ends, whatever its
outcome, and the allocator's cache is emptied.  Wall time and peak device memory: DESIGN.md section 5, "Limits under test".
"""
import numpy as np
import pytest

import ccm
import keywrap
import limits as lm
import wire_formats as wf
from aes_model import DEC_MULS, INV_MC, AesModel, ref_pack, ref_unpack
from aes_vectors import F1_KEY, own_client
from gpu_support import GUARD, SENTINEL, dev, filled, guarded, guards_intact, host, settled
from oracle import oracle as orc
from tfhe_aes_amd import PARAM_TOY, _native, aes_clear
from tfhe_aes_amd.client import MASK_TAG_LWE, mask_words

pytestmark = pytest.mark.gpu

P = PARAM_TOY
LW = P.big1                      # 513 words a row
BYTE_W, BLOCK_W = 8 * LW, 128 * LW
SLICE_BYTES = 256 << 20
CHUNK = 32768                    # MAX_CHUNK_BITS of engine_launch.h
K2_CALL = 65536                  # K2_CALL_MAX_BITS


# ---- device arrays -------------------------------------------------------------------------------------------------------------------
def _step(words):
    return max(1, SLICE_BYTES // (8 * words))


def _residues(lo, hi, period, index):
    import torch

    i = torch.arange(lo, hi, device="cuda")
    return index(i) if index else i % period


def tile_into(t, base, index=None):
    """t[i] = base[index(i)] (default i mod len(base)), slice by slice"""
    for lo in range(0, t.shape[0], _step(t.shape[1])):
        hi = min(t.shape[0], lo + _step(t.shape[1]))
        t[lo:hi] = base[_residues(lo, hi, base.shape[0], index)]
    return settled(t)


def tiled(base, n, index=None):
    import torch

    return tile_into(torch.empty((n, base.shape[1]), dtype=torch.int64, device="cuda"), base, index)


def first_difference(t, base, index=None):
    """None if t[i] == base[index(i)] for all i, else (unit, word, got, want) of the first word that differs; on the device, in slices"""
    import torch

    for lo in range(0, t.shape[0], _step(t.shape[1])):
        hi = min(t.shape[0], lo + _step(t.shape[1]))
        want = base[_residues(lo, hi, base.shape[0], index)]
        if not torch.equal(t[lo:hi], want):
            bad = t[lo:hi] != want
            r = int(torch.nonzero(bad.any(dim=1))[0])
            w = int(torch.nonzero(bad[r])[0])
            return lo + r, w, int(t[lo + r, w]) & lm.LINE32 ** 2 - 1, int(want[r, w]) & lm.LINE32 ** 2 - 1
        del want
    return None


def all_sentinel(t):
    for lo in range(0, t.shape[0], _step(t.shape[1])):
        if not bool((t[lo:lo + _step(t.shape[1])] == SENTINEL).all().item()):
            return False
    return True


class Crossing:
    """`units` units of `words` 64-bit words as a view that begins limits.margin_bytes() into an allocation of its own:
    [2^31 bytes and GUARD units | the array | GUARD units], all sentinel"""

    def __init__(self, units, words):
        import torch

        self.units, self.words, self.size = units, words, 8 * words
        self.front = lm.margin_bytes(GUARD, self.size) // self.size
        self.buf = torch.full((self.front + units + GUARD, words), SENTINEL, dtype=torch.int64, device="cuda")
        self.view = self.buf[self.front:self.front + units]
        self.last_byte = lm.last_byte(units, self.size)
        assert self.view.is_contiguous() and self.view.data_ptr() - self.buf.data_ptr() == self.front * self.size >= lm.LINE31 + GUARD * self.size
        assert self.last_byte > lm.LINE32 and lm.units_beyond(units, self.size) >= 2, "the array does not cross byte 2^32"
        settled(self.buf)

    def margins_intact(self):
        return all_sentinel(self.buf[:self.front]) and all_sentinel(self.buf[self.front + self.units:])

    def check(self, base, what, index=None):
        """the margins untouched and every unit the base's"""
        assert self.margins_intact(), "%s: a store outside the array, inside its allocation" % what
        bad = first_difference(self.view, base, index)
        assert bad is None, "%s: unit %d of %d (unit %d holds byte 2^32), word %d: got %#x, want %#x" % (
            (what, bad[0], self.units, lm.unit_holding(lm.LINE32, self.size)) + bad[1:])


@pytest.fixture
def crossing():
    """make(units, words) -> Crossing; at most three a test, all freed when it ends"""
    import torch

    made = []

    def make(units, words):
        assert len(made) < 3
        made.append(Crossing(units, words))
        return made[-1]

    try:
        yield make
    finally:
        used = torch.cuda.mem_get_info()
        print("device memory in use at the end of the test: %.2f GB" % ((used[1] - used[0]) / 1e9))
        for c in made:
            c.buf = c.view = None
        made.clear()
        torch.cuda.empty_cache()


@pytest.fixture
def eng(toy):
    """a context of the test's own under the session's toy keys"""
    import torch

    E = _native.Engine(P, device=0)
    try:
        E.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        yield E
    finally:
        E.close()
        torch.cuda.empty_cache()


def _stage(E, stage, launches, units):
    got = E.profile_read()[stage]
    assert (got["launches"], got["units"]) == (launches, units), (stage, got, launches, units)


def _u(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want, what):
    got, want = _u(got), _u(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: the base call differs from its reference in %d words, first at %s" % (
        what, int((got != want).sum()), np.argwhere(got != want)[0])


# ---- the bases: P honest units and their references, computed once -------------------------------------------------------------------
@pytest.fixture(scope="module")
def tc(toy):
    return own_client(toy)


@pytest.fixture(scope="module")
def row_base(toy, tc):
    """P_ROWS honest rows and what the oracle makes of them: K1, K2, K3 and K4 of the first P_ROWS polynomials"""
    rng = np.random.default_rng(0x11317)
    x = tc.encrypt_bits(rng.integers(0, 2, lm.P_ROWS))
    small = toy.oracle.keyswitch(x)
    pbs = toy.oracle.cbs_pbs(small)
    ggsw = toy.oracle.pfpks(pbs).reshape(lm.P_ROWS, -1)
    polys = np.ascontiguousarray(ggsw.reshape(-1, P.N)[:lm.P_ROWS])
    return {"x": x, "small": small, "pbs": pbs, "ggsw": ggsw, "polys": polys, "fourier": _u(orc.polys_to_fourier(polys)).reshape(lm.P_ROWS, P.N)}


@pytest.fixture(scope="module")
def byte_base(toy, tc):
    """P_BYTES honest bytes and the oracle's S-Box, the three LUTs of a cipher round and the four multiples of the inverse cipher"""
    values = np.random.default_rng(0x127).integers(0, 256, lm.P_BYTES)
    ct = tc.encrypt_bytes(values)
    out = {"values": values, "ct": ct}
    for name, which in (("sbox", orc.LUTSET_SBOX), ("round", orc.LUTSET_ENC_ROUND), ("dec_mul", orc.LUTSET_DEC_MUL)):
        out[name] = toy.oracle.wopbs_batch(ct, orc.build_lutset(which))
    return out


@pytest.fixture(scope="module")
def block_base(toy, tc):
    """P_BLOCKS honest blocks, the oracle's round keys of the SP 800-38A key and its AES-128 of every block"""
    pts = [int.from_bytes(np.random.default_rng(0x5B + i).bytes(16), "big") for i in range(lm.P_BLOCKS)]
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    rk = toy.oracle.aes_key_expansion(tc.encrypt_aes_key(F1_KEY))
    return {"pts": pts, "st": st, "rk": rk, "enc": np.stack([toy.oracle.aes_encrypt(rk, s) for s in st])}


def _random_blocks(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (n, 16, 8, LW), dtype=np.uint64)


# ---- 1. the stage calls ------------------------------------------------------------------------------------------------------------------
def test_keyswitch_input_beyond_the_line(eng, crossing, row_base):
    m = lm.crossing_count(lm.ROW)
    x = crossing(m, LW)
    base = dev(row_base["x"])
    buf_b, out_b = guarded(lm.P_ROWS, P.n + 1)
    eng.keyswitch_batch(base, out_b, lm.P_ROWS)
    eng.synchronize()
    _same(host(out_b), row_base["small"], "K1")
    tile_into(x.view, base)
    buf, out = guarded(m, P.n + 1)
    eng.profile_reset()
    eng.keyswitch_batch(x.view, out, m)
    eng.synchronize()
    _stage(eng, "keyswitch", 1, m)
    assert guards_intact(buf) and guards_intact(buf_b)
    x.check(base, "K1's input")                                             # read only
    bad = first_difference(out, out_b)
    assert bad is None, "K1: row %d (row %d holds byte 2^32 of the input), word %d: got %#x, want %#x" % ((bad[0], lm.unit_holding(lm.LINE32, lm.ROW)) + bad[1:])


def test_cbs_pbs_output_beyond_the_line(eng, crossing, row_base):
    m = lm.chunked_count(lm.ROW, K2_CALL)
    out = crossing(m, LW)
    small = dev(row_base["small"])
    buf_b, out_b = guarded(lm.P_ROWS, LW)
    eng.cbs_pbs_batch(small, out_b, lm.P_ROWS)
    eng.synchronize()
    _same(host(out_b), row_base["pbs"], "K2")
    assert guards_intact(buf_b)
    x = tiled(small, m)
    eng.profile_reset()
    eng.cbs_pbs_batch(x, out.view, m)
    eng.synchronize()
    _stage(eng, "blind_rotate", 17, m)                                     # launch 15 holds byte 2^32, launch 16 starts beyond it
    assert lm.unit_holding(lm.LINE32, lm.ROW) // K2_CALL == 15 and m // K2_CALL == 16 and 16 * K2_CALL * lm.ROW > lm.LINE32
    out.check(out_b, "K2's output")


def test_pfpks_output_beyond_the_line(eng, crossing, row_base):
    m, words = lm.crossing_count(lm.K3_ROW), (P.k + 1) ** 2 * P.N
    assert m == 262146
    out = crossing(m, words)
    pbs = dev(row_base["pbs"])
    buf_b, out_b = guarded(lm.P_ROWS, words)
    eng.pfpks_batch(pbs, out_b, lm.P_ROWS)
    eng.synchronize()
    _same(host(out_b), row_base["ggsw"], "K3")
    assert guards_intact(buf_b)
    x = tiled(pbs, m)
    eng.profile_reset()
    eng.pfpks_batch(x, out.view, m)
    eng.synchronize()
    _stage(eng, "pfpks", 1, m)
    out.check(out_b, "K3's output")


def test_forward_fourier_both_sides_beyond_the_line(eng, crossing, row_base):
    n = lm.crossing_count(lm.POLY)
    assert n == 1048578
    x, out = crossing(n, P.N), crossing(n, P.N)
    base = dev(row_base["polys"])
    buf_b, out_b = guarded(lm.P_ROWS, P.N)
    eng.forward_fourier_batch(base, out_b, lm.P_ROWS)
    eng.synchronize()
    _same(host(out_b), row_base["fourier"], "K4")
    assert guards_intact(buf_b)
    tile_into(x.view, base)
    eng.profile_reset()
    eng.forward_fourier_batch(x.view, out.view, n)
    eng.synchronize()
    _stage(eng, "ggsw_fft", 1, n)
    x.check(base, "K4's input")
    out.check(out_b, "K4's output")


def test_vertical_packing_ggsw_input_beyond_the_line(eng, crossing, toy, byte_base):
    """the Fourier GGSWs of 32,770 8-bit inputs; the base's are the oracle's circuit bootstrap of P_INPUTS honest bytes, transformed"""
    n, words = lm.crossing_count(lm.GGSW8), 8 * P.ggsw_words
    assert n == 32770 and 8 * words == lm.GGSW8
    q = lm.P_INPUTS
    small = toy.oracle.keyswitch(byte_base["ct"][:q])
    ggsw_f = orc.polys_to_fourier(toy.oracle.circuit_bootstrap(small.reshape(-1, P.n + 1)).reshape(-1, P.N)).reshape(q, 8, 1, 2, 2, 256, 2)
    luts = orc.build_lutset(orc.LUTSET_SBOX)
    want = np.stack([orc.vertical_packing(P, ggsw_f[i], 8, luts) for i in range(q)]).reshape(q, BYTE_W)
    _same(want, byte_base["sbox"][:q].reshape(q, BYTE_W), "the oracle's K5 on its own GGSWs")
    g = crossing(n, words)
    base, luts_d = dev(_u(ggsw_f).reshape(q, words)), dev(luts)
    buf_b, out_b = guarded(q, BYTE_W)
    eng.vertical_packing_batch(base, q, 8, luts_d, 1, False, out_b)
    eng.synchronize()
    _same(host(out_b), want, "K5")
    assert guards_intact(buf_b)
    tile_into(g.view, base)
    buf, out = guarded(n, BYTE_W)
    eng.profile_reset()
    eng.vertical_packing_batch(g.view, n, 8, luts_d, 1, False, out)
    eng.synchronize()
    _stage(eng, "vertical_packing", 1, n * 8)
    assert guards_intact(buf)
    g.check(base, "K5's GGSWs")
    bad = first_difference(out, out_b)
    assert bad is None, "K5: input %d (input %d starts at byte 2^32), word %d: got %#x, want %#x" % ((bad[0], lm.unit_holding(lm.LINE32, lm.GGSW8)) + bad[1:])


def test_wopbs_8_bits_both_sides_beyond_the_line(eng, crossing, byte_base):
    n = lm.chunked_count(lm.BYTE, CHUNK // 8)
    assert n == 131074
    x, out = crossing(n, BYTE_W), crossing(n, BYTE_W)
    base, luts = dev(byte_base["ct"].reshape(lm.P_BYTES, BYTE_W)), dev(orc.build_lutset(orc.LUTSET_SBOX))
    buf_b, out_b = guarded(lm.P_BYTES, BYTE_W)
    eng.wopbs_batch(base, lm.P_BYTES, 8, luts, 1, False, out_b)
    eng.synchronize()
    _same(host(out_b), byte_base["sbox"].reshape(lm.P_BYTES, BYTE_W), "the WoPBS")
    assert guards_intact(buf_b)
    tile_into(x.view, base)
    eng.profile_reset()
    eng.wopbs_batch(x.view, n, 8, luts, 1, False, out.view)
    eng.synchronize()
    chunks = -(-n // (CHUNK // 8))
    assert chunks == 33 and lm.unit_holding(lm.LINE32, lm.BYTE) // (CHUNK // 8) == 31          # chunk 31 holds the line, chunk 32 starts beyond it
    for stage, units in (("keyswitch", 8 * n), ("blind_rotate", 8 * n), ("pfpks", 8 * n), ("ggsw_fft", 8 * n * 4), ("vertical_packing", 8 * n)):
        _stage(eng, stage, chunks, units)
    x.check(base, "the WoPBS's input")
    out.check(out_b, "the WoPBS's output")


# ---- 2. the S-Boxes ----------------------------------------------------------------------------------------------------------------------
def test_sbox_in_place_beyond_the_line(eng, crossing, tc, byte_base):
    n = lm.chunked_count(lm.BYTE, CHUNK // 8)
    st = crossing(n, BYTE_W)
    base = dev(byte_base["ct"].reshape(lm.P_BYTES, BYTE_W))
    buf_b, out_b = guarded(lm.P_BYTES, BYTE_W)
    settled(out_b.copy_(base))
    eng.sbox(out_b, lm.P_BYTES, False)
    eng.synchronize()
    _same(host(out_b), byte_base["sbox"].reshape(lm.P_BYTES, BYTE_W), "sbox")
    assert guards_intact(buf_b)
    assert tc.decrypt_bytes(byte_base["sbox"][:, 0]).tolist() == [aes_clear.SBOX[v] for v in byte_base["values"]]
    tile_into(st.view, base)
    eng.profile_reset()
    eng.sbox(st.view, n, False)
    eng.synchronize()
    _stage(eng, "blind_rotate", 33, 8 * n)
    st.check(out_b, "sbox in place")


def test_many_sbox_output_three_times_its_input(eng, crossing, byte_base):
    """the output [n][3][8][kN+1] crosses the line at a third of the bytes the input needs to: input 1.4 GB, output 4.3 GB"""
    n = lm.chunked_count(3 * lm.BYTE, CHUNK // 8)
    out = crossing(n, 3 * BYTE_W)
    assert n * lm.BYTE < lm.LINE31
    base = dev(byte_base["ct"].reshape(lm.P_BYTES, BYTE_W))
    buf_b, out_b = guarded(lm.P_BYTES, 3 * BYTE_W)
    eng.many_sbox(base, lm.P_BYTES, False, out_b)
    eng.synchronize()
    _same(host(out_b), byte_base["round"].reshape(lm.P_BYTES, 3 * BYTE_W), "many_sbox")
    assert guards_intact(buf_b)
    x = tiled(base, n)
    eng.profile_reset()
    eng.many_sbox(x, n, False, out.view)
    eng.synchronize()
    chunks = -(-n // (CHUNK // 8))
    _stage(eng, "vertical_packing", chunks, 3 * 8 * n)
    assert lm.unit_holding(lm.LINE32, 3 * lm.BYTE) // (CHUNK // 8) == chunks - 2 == 10      # the last chunk starts beyond the line
    out.check(out_b, "many_sbox's output")


# ---- 3. the linear layer alone -------------------------------------------------------------------------------------------------------------
def test_inv_mix_columns_input_beyond_the_line(crossing, byte_base):
    n, q = lm.crossing_count(lm.IMC_BLOCK), lm.P_IMC
    assert n == 2047
    y = byte_base["dec_mul"][:16 * q].reshape(q, 16, 4, 8, LW)
    want = AesModel._mix(y, INV_MC, DEC_MULS, 0).reshape(q, BLOCK_W)
    x = crossing(n, 4 * BLOCK_W)
    E = _native.Engine(P, device=0)                                         # no keys: the gather needs none
    try:
        base = dev(y.reshape(q, 4 * BLOCK_W))
        buf_b, out_b = guarded(q, BLOCK_W)
        E.inv_mix_columns_batch(base, q, out_b)
        E.synchronize()
        _same(host(out_b), want, "InvMixColumns")
        tile_into(x.view, base)
        buf, out = guarded(n, BLOCK_W)
        E.profile_reset()
        E.inv_mix_columns_batch(x.view, n, out)
        E.synchronize()
        _stage(E, "linear", 1, n)
        assert guards_intact(buf) and guards_intact(buf_b)
        x.check(base, "InvMixColumns' input")
        bad = first_difference(out, out_b)
        assert bad is None, "InvMixColumns: block %d (block %d holds byte 2^32 of the input), word %d: got %#x, want %#x" % (
            (bad[0], lm.unit_holding(lm.LINE32, lm.IMC_BLOCK)) + bad[1:])
    finally:
        E.close()


ADDENDS = [1, 0xFF, (1 << 64) - 1, (1 << 128) - 1, 0x0123456789ABCDEF << 60]          # a carry through one byte, eight, all sixteen, none


def test_add_scalar_state_beyond_the_line(eng, crossing, toy, tc, block_base):
    n, q = lm.crossing_count(lm.BLOCK), lm.P_BLOCKS
    assert n == 8179 and len(ADDENDS) == q
    st = crossing(n, BLOCK_W)
    want = np.stack([toy.oracle.add_scalar(block_base["st"][j], ADDENDS[j]) for j in range(q)])
    assert [tc.decrypt_u128(want[j]) for j in range(q)] == [(block_base["pts"][j] + ADDENDS[j]) % (1 << 128) for j in range(q)]
    base = dev(block_base["st"].reshape(q, BLOCK_W))
    buf_b, out_b = guarded(q, BLOCK_W)
    settled(out_b.copy_(base))
    eng.add_scalar(out_b, q, ADDENDS)
    eng.synchronize()
    _same(host(out_b), want.reshape(q, BLOCK_W), "add_scalar")
    assert guards_intact(buf_b)
    tile_into(st.view, base)
    eng.profile_reset()
    eng.add_scalar(st.view, n, [ADDENDS[i % q] for i in range(n)])
    eng.synchronize()
    per_step = [-(-n // (CHUNK // bits)) for bits in [8] + [9] * 15]
    _stage(eng, "blind_rotate", sum(per_step), n * (8 + 9 * 15))
    st.check(out_b, "add_scalar's state")


# ---- 4. one whole cipher call --------------------------------------------------------------------------------------------------------------
def test_aes_encrypt_state_beyond_the_line(eng, crossing, tc, block_base):
    """fheaes_aes_encrypt_bits on 8,180 blocks, AES-128, the window automatic: the one long case.  Every block of the state is compared
    with the oracle's five (the tiling check); the five decrypt to aes_clear's, and so do the blocks on either side of both lines,
    downloaded from the state itself"""
    n, q = lm.AES_BLOCKS, lm.P_BLOCKS
    st = crossing(n, BLOCK_W)
    base, rk = dev(block_base["st"].reshape(q, BLOCK_W)), dev(block_base["rk"])
    buf_b, out_b = guarded(q, BLOCK_W)
    settled(out_b.copy_(base))
    eng.aes_encrypt_bits(rk, 128, out_b, q)
    eng.synchronize()
    _same(host(out_b), block_base["enc"].reshape(q, BLOCK_W), "aes_encrypt")
    assert guards_intact(buf_b)
    clear = [aes_clear.aes_encrypt_block(F1_KEY, v) for v in block_base["pts"]]
    assert [tc.decrypt_u128(b) for b in block_base["enc"]] == clear
    tile_into(st.view, base)
    w = eng.aes_window(n, 10)
    eng.profile_reset()
    eng.aes_encrypt_bits(rk, 128, st.view, n)
    eng.synchronize()
    launches = -(-10 * n // w) if w else 10 * -(-n // (CHUNK // 128))
    _stage(eng, "blind_rotate", launches, 10 * n * 128)
    assert eng.profile_read()["linear"]["units"] == 11 * n                  # the first AddRoundKey and ten layers over every block
    st.check(out_b, "the cipher's state")
    at = sorted({0, lm.unit_holding(lm.LINE31, lm.BLOCK), lm.unit_holding(lm.LINE31, lm.BLOCK) + 1, lm.unit_holding(lm.LINE32, lm.BLOCK),
                 lm.unit_holding(lm.LINE32, lm.BLOCK) + 1, n - 1})
    for i in at:
        assert tc.decrypt_u128(host(st.view[i]).reshape(16, 8, LW)) == clear[i % q], "block %d" % i


# ---- 5. the data movers ----------------------------------------------------------------------------------------------------------------------
Q_GLWE = 7                       # the period of an array tiled by GLWEs of 512 bits (2,049 of them a crossing array; 2^32 is no multiple)


def _by_glwe(q):
    """row t of an array tiled by GLWEs: row t mod 512 of GLWE (t // 512) mod q of the base"""
    return lambda t: (t // P.N) % q * P.N + t % P.N


def _glwe_base(seed, width=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 64, (Q_GLWE, (P.k + 1) * (P.N if width is None else 8 * width)), dtype=np.uint64)


@pytest.mark.parametrize("width", [64, 16])
def test_unpack_output_beyond_the_line(crossing, width):
    """fheaes_unpack_bits (64) and fheaes_unpack_bits_mod at w = 16: a permutation with signs of random words, against ref_unpack"""
    m = lm.chunked_count(lm.ROW, CHUNK)
    glwes = -(-m // P.N)
    out = crossing(m, LW)
    packed = _glwe_base(0x0D + width, None if width == 64 else width)
    full = packed if width == 64 else wf.read_back_glwes(packed, (P.k + 1) * P.N, width)
    want = ref_unpack(full, Q_GLWE * P.N, P)
    E = _native.Engine(P, device=0)                                         # no keys: unpacking needs none
    try:
        call = (lambda a, n, o: E.unpack_bits(a, n, o)) if width == 64 else (lambda a, n, o: E.unpack_bits_mod(a, n, width, o))
        base = dev(packed)
        buf_b, out_b = guarded(Q_GLWE * P.N, LW)
        call(base, Q_GLWE * P.N, out_b)
        E.synchronize()
        _same(host(out_b), want, "unpack")
        assert guards_intact(buf_b)
        x = tiled(base, glwes)
        E.profile_reset()
        call(x, m, out.view)
        E.synchronize()
        _stage(E, "linear", -(-m // CHUNK), m)
        assert lm.unit_holding(lm.LINE32, lm.ROW) // CHUNK == 31 and m // CHUNK == 32        # the last launch starts beyond the line
        out.check(out_b, "unpack's output", _by_glwe(Q_GLWE))
    finally:
        E.close()


Q_PACK = 3                       # pack_bits' base: 3 GLWEs of honest rows through the reference's key switch and fold


@pytest.mark.parametrize("width", [64, 16])
def test_pack_input_beyond_the_line(eng, crossing, toy, tc, width):
    """fheaes_pack_bits (64) and fheaes_pack_bits_mod at w = 16 against ref_pack (and switch_glwes); the last GLWE holds 2 bits"""
    m = lm.chunked_count(lm.ROW, CHUNK)
    glwes, last = -(-m // P.N), m % P.N
    at = (glwes - 1) % Q_PACK                                                # the base GLWE whose first rows the last GLWE packs
    assert glwes == 2049 and last == 2 and at == 2
    x = crossing(m, LW)
    rows = tc.encrypt_bits(np.random.default_rng(0x9AC).integers(0, 2, Q_PACK * P.N))
    want = ref_pack(toy, rows)
    want_last = ref_pack(toy, rows[at * P.N:at * P.N + last])
    words = (P.k + 1) * P.N
    if width != 64:
        want, want_last, words = wf.switch_glwes(want, width), wf.switch_glwes(want_last, width), (P.k + 1) * 8 * width
    call = (lambda a, n, o: eng.pack_bits(a, n, o)) if width == 64 else (lambda a, n, o: eng.pack_bits_mod(a, n, width, o))
    eng.reserve(CHUNK)          # packing works inside the workspace it finds: sized by the base call it would cut the batch at 1,536 bits
    base = dev(rows)
    buf_b, out_b = guarded(Q_PACK, words)
    call(base, Q_PACK * P.N, out_b)
    eng.synchronize()
    _same(host(out_b), want, "pack")
    assert guards_intact(buf_b)
    tile_into(x.view, base, _by_glwe(Q_PACK))
    buf, out = guarded(glwes, words)
    eng.profile_reset()
    call(x.view, m, out)
    eng.synchronize()
    _stage(eng, "pfpks", -(-m // CHUNK), m)
    assert guards_intact(buf)
    x.check(base, "pack's input", _by_glwe(Q_PACK))
    bad = first_difference(out[:-1], out_b)
    assert bad is None, "pack: GLWE %d of %d, word %d: got %#x, want %#x" % ((bad[0], glwes) + bad[1:])
    _same(host(out[-1:]), want_last, "the last GLWE, %d bits" % last)


def test_expand_lwe_seeded_output_beyond_the_line(crossing):
    """no tiling: every row has masks of its own.  first_index puts ciphertext 2^32 -- the first with a high nonce word -- on the row that
    holds byte 2^31.  Rows at both lines and at both ends against client.mask_words; all rows against the same call made in pieces of
    32,768 rows that cross nothing"""
    import torch

    m = lm.chunked_count(lm.ROW, CHUNK)
    out = crossing(m, LW)
    at31, at32 = lm.unit_holding(lm.LINE31, lm.ROW), lm.unit_holding(lm.LINE32, lm.ROW)
    first = (1 << 32) - at31
    key = np.random.default_rng(0xE8).integers(0, 1 << 32, 8, dtype=np.uint32)
    bodies = np.random.default_rng(0xB0D).integers(0, 1 << 64, m, dtype=np.uint64)
    E = _native.Engine(P, device=0)                                         # no keys
    try:
        d_bodies = dev(bodies)
        E.profile_reset()
        E.expand_lwe_seeded(key, first, d_bodies, m, out.view)
        E.synchronize()
        _stage(E, "linear", -(-m // CHUNK), m)
        assert out.margins_intact()
        for r in (0, 1, at31 - 1, at31, at31 + 1, at32 - 1, at32, at32 + 1, at32 + 2, m - 1):
            got = host(out.view[r])
            assert np.array_equal(got[:P.big], mask_words(key, MASK_TAG_LWE, 1, P.big, first_ct=first + r)[0]) and got[P.big] == bodies[r], "row %d" % r
        piece = torch.empty((CHUNK, LW), dtype=torch.int64, device="cuda")
        for t0 in range(0, m, CHUNK):
            mc = min(CHUNK, m - t0)
            E.expand_lwe_seeded(key, first + t0, settled(d_bodies[t0:t0 + mc]), mc, piece)
            E.synchronize()
            bad = first_difference(out.view[t0:t0 + mc], piece[:mc], lambda i: i)
            assert bad is None, "row %d (row %d holds byte 2^32), word %d: got %#x, the call on this piece alone %#x" % ((t0 + bad[0], at32) + bad[1:])
    finally:
        E.close()


def test_xts_whiten_state_beyond_the_line(crossing, tc):
    """in place, over 5 tweak rows through a table that is not monotone, clear bytes on; against numpy sums"""
    n, q = lm.crossing_count(lm.BLOCK), lm.P_BLOCKS
    st = crossing(n, BLOCK_W)
    state, tweaks = _random_blocks(q, 0xF30), _random_blocks(q, 0xF31)
    clear = np.random.default_rng(0xF32).integers(0, 256, (q, 16), dtype=np.uint8)
    tab = [(2 * j + 1) % q for j in range(q)]
    with np.errstate(over="ignore"):
        want = (state + tweaks[tab] + tc.trivial_bytes(clear)).reshape(q, BLOCK_W)
    E = _native.Engine(P, device=0)                                         # no keys
    try:
        base, d_tweaks = dev(state.reshape(q, BLOCK_W)), dev(tweaks)
        buf_b, out_b = guarded(q, BLOCK_W)
        settled(out_b.copy_(base))
        d = out_b.view(q, 16, 8, LW)
        E.xts_whiten(d, d, d_tweaks, tab, clear)
        E.synchronize()
        _same(host(out_b), want, "xts_whiten")
        assert guards_intact(buf_b)
        tile_into(st.view, base)
        d = st.view.view(n, 16, 8, LW)
        E.profile_reset()
        E.xts_whiten(d, d, d_tweaks, [tab[i % q] for i in range(n)], np.concatenate([clear] * (n // q + 1))[:n])
        E.synchronize()
        _stage(E, "linear", 1, n)
        st.check(out_b, "xts_whiten's state")
    finally:
        E.close()


def test_mac_link_state_beyond_the_line(crossing, tc):
    """a payload step: state += the first enc_bytes bytes of an addend block + clear bytes; against ccm.np_link"""
    n, q = lm.crossing_count(lm.BLOCK), lm.P_BLOCKS
    st = crossing(n, BLOCK_W)
    state, enc = _random_blocks(q, 0xF40), _random_blocks(q, 0xF41)
    clear = np.random.default_rng(0xF42).integers(0, 256, (q, 16), dtype=np.uint8)
    src, eb = [(j + 2) % q for j in range(q)], [0, 1, 15, 16, 5]
    with np.errstate(over="ignore"):
        want = ccm.np_link(tc, state, False, None, enc, src, eb, clear).reshape(q, BLOCK_W)
    E = _native.Engine(P, device=0)                                         # no keys
    try:
        base, d_enc = dev(state.reshape(q, BLOCK_W)), dev(enc)
        buf_b, out_b = guarded(q, BLOCK_W)
        settled(out_b.copy_(base))
        E.mac_link(out_b.view(q, 16, 8, LW), False, None, d_enc, src, eb, clear)
        E.synchronize()
        _same(host(out_b), want, "mac_link")
        assert guards_intact(buf_b)
        tile_into(st.view, base)
        E.profile_reset()
        E.mac_link(st.view.view(n, 16, 8, LW), False, None, d_enc, [src[i % q] for i in range(n)], [eb[i % q] for i in range(n)],
                   np.concatenate([clear] * (n // q + 1))[:n])
        E.synchronize()
        _stage(E, "linear", 1, n)
        st.check(out_b, "mac_link's state")
    finally:
        E.close()


def test_kw_link_registers_beyond_the_line(crossing):
    """8 semiblocks: the registers of one key are 2,101,248 bytes, those of 2,047 keys cross the line (a state is a quarter of that and
    a call takes 4,096 keys, so the state array cannot).  The load, which writes every word, then the first shuffle, which moves
    register 8 into the state and the state's half into register 1; against keywrap.np_link"""
    n_keys, n, q = lm.crossing_count(lm.IMC_BLOCK), 8, lm.P_IMC
    assert n_keys == 2047 and 64 * BYTE_W * 8 == lm.IMC_BLOCK
    regs = crossing(n_keys, 64 * BYTE_W)
    rng = np.random.default_rng(0x3394)
    wrapped = [rng.bytes(8 * (n + 1)) for _ in range(q)]
    zero_s, zero_r = np.zeros((q, 16, 8, LW), dtype=np.uint64), np.zeros((q, 8 * n, 8, LW), dtype=np.uint64)
    s0, r0 = keywrap.np_link(zero_s, zero_r, n, 0, wrapped)
    s0 = s0 + _random_blocks(q, 0xF50)                                      # not only trivial words: the shuffle moves whole rows
    r0 = r0 + np.random.default_rng(0xF51).integers(0, 1 << 64, r0.shape, dtype=np.uint64)
    s1, r1 = keywrap.np_link(s0, r0, n, 1, wrapped)
    E = _native.Engine(P, device=0)                                         # no keys
    try:
        buf_s, state = guarded(n_keys, BLOCK_W)
        shape_s, shape_r = (n_keys, 16, 8, LW), (n_keys, 8 * n, 8, LW)
        E.profile_reset()
        E.kw_link(state.view(shape_s), regs.view.view(shape_r), n, 0, [wrapped[i % q] for i in range(n_keys)])
        E.synchronize()
        _stage(E, "linear", 1, n_keys)
        want_s, want_r = keywrap.np_link(zero_s, zero_r, n, 0, wrapped)
        assert guards_intact(buf_s)
        regs.check(dev(want_r.reshape(q, -1)), "the load's registers")
        assert first_difference(state, dev(want_s.reshape(q, -1))) is None
        tile_into(state, dev(s0.reshape(q, -1)))
        tile_into(regs.view, dev(r0.reshape(q, -1)))
        E.kw_link(state.view(shape_s), regs.view.view(shape_r), n, 1, None)
        E.synchronize()
        assert guards_intact(buf_s)
        regs.check(dev(r1.reshape(q, -1)), "the shuffle's registers")
        bad = first_difference(state, dev(s1.reshape(q, -1)))
        assert bad is None, "the shuffle's state: key %d, word %d: got %#x, want %#x" % bad
    finally:
        E.close()


def test_gate_bits_in_place_beyond_the_line(eng, crossing, toy, tc, row_base):
    """one gate a row, so that the gates are a crossing array too and row i depends on i mod P alone; the base against the oracle's
    circuit bootstrap and external product (gate_model.gate_reference)"""
    import gate_model as gm

    m, q = lm.chunked_count(lm.ROW, CHUNK), lm.P_ROWS
    gates, st = crossing(m, LW), crossing(m, LW)
    valid = tc.encrypt_bits(np.random.default_rng(0x6A7E).integers(0, 2, q))
    ggsw = toy.oracle.circuit_bootstrap(toy.oracle.keyswitch(valid))
    want = np.concatenate([gm.gate_reference(P, ggsw[i], row_base["x"][i:i + 1], 0) for i in range(q)])
    base, g_base = dev(row_base["x"]), dev(valid)
    buf_b, out_b = guarded(q, LW)
    settled(out_b.copy_(base))
    eng.gate_bits(g_base, [1] * q, out_b, q, out_b)
    eng.synchronize()
    _same(host(out_b), want, "gate_bits")
    assert guards_intact(buf_b)
    tile_into(gates.view, g_base)
    tile_into(st.view, base)
    eng.profile_reset()
    eng.gate_bits(gates.view, np.ones(m, dtype=np.uint64), st.view, m, st.view)
    eng.synchronize()
    _stage(eng, "blind_rotate", -(-m // CHUNK), m)
    gates.check(g_base, "the gates")
    st.check(out_b, "the gated rows")


# ---- 6. the key side -----------------------------------------------------------------------------------------------------------------------
def test_keyed_cipher_round_keys_beyond_the_line(eng, crossing, toy, tc):
    """746 AES-128 keys in LWE form, 5,778,432 bytes each: key 743 holds byte 2^32, keys 744 and 745 lie beyond it (745 keys are the
    first to cross; one more leaves two whole keys there, as every other case does), key 371 holds byte 2^31.  Two blocks under the keys
    on either side of the line -- 742, 743 and 744, 745 -- and one under key 372, against the single-key call under the same round keys
    (an older call, held to the oracle by its own tests) and, decrypted, against aes_clear.  Then the same 746 keys packed --
    fheaes_pack_round_keys reads the crossing array -- and the same blocks from the packed store"""
    n_keys, q, key_w = lm.KEYS128, 3, 11 * BLOCK_W
    assert lm.unit_holding(lm.LINE32, lm.KEY128) == 743 and lm.unit_holding(lm.LINE31, lm.KEY128) == 371
    rks = crossing(n_keys, key_w)
    keys = [bytes(np.random.default_rng(0x6E7 + j).bytes(16)) for j in range(q)]
    d_keys = dev(np.stack([tc.encrypt_aes_key(k) for k in keys]))
    base = filled((q, key_w), 0)
    eng.aes_key_expansion_batch(d_keys, 128, q, base)
    eng.synchronize()
    assert tc.decrypt_bytes(host(base).reshape(q, 11, 16, 8, LW)).reshape(q, 176).tolist() == [sum(aes_clear.expand_key(k), []) for k in keys]
    kob = [742, 743, 744, 745, 372]
    nb = len(kob)
    pts = [0x00112233445566778899AABBCCDDEEFF + i for i in range(nb)]
    st = np.stack([tc.encrypt_u128(v) for v in pts])
    want = []
    for b in range(nb):
        d = dev(st[b])
        eng.aes_encrypt_bits(settled(base[kob[b] % q].contiguous()), 128, d, 1)
        eng.synchronize()
        want.append(host(d))
    assert [tc.decrypt_u128(w) for w in want] == [aes_clear.aes_encrypt_block(keys[kob[b] % q], pts[b]) for b in range(nb)]
    tile_into(rks.view, base)
    buf, d_st = guarded(nb, BLOCK_W)
    settled(d_st.copy_(dev(st.reshape(nb, BLOCK_W))))
    eng.profile_reset()
    eng.aes_encrypt_keyed(rks.view, 128, n_keys, kob, d_st, nb)
    eng.synchronize()
    _stage(eng, "linear", 11, nb * 11)
    assert guards_intact(buf)
    rks.check(base, "the round keys")
    _same(host(d_st), np.stack(want).reshape(nb, BLOCK_W), "aes_encrypt_keyed under keys %s" % kob)
    # the packed store of the same keys
    g = _native.round_keys_packed_glwes(128)
    store_w = g * (P.k + 1) * P.N
    buf_p, store = guarded(n_keys, store_w)
    buf_pb, store_b = guarded(q, store_w)
    eng.pack_round_keys(base, 128, q, store_b)
    eng.pack_round_keys(rks.view, 128, n_keys, store)
    eng.synchronize()
    assert guards_intact(buf_p) and guards_intact(buf_pb)
    _same(host(store_b[0]).reshape(g, -1), ref_pack(toy, host(base[0]).reshape(-1, LW)), "pack_round_keys, key 0")
    bad = first_difference(store, store_b)
    assert bad is None, "pack_round_keys: key %d, word %d: got %#x, want %#x" % bad
    settled(d_st.copy_(dev(st.reshape(nb, BLOCK_W))))
    eng.aes_encrypt_keyed_packed(store, 128, n_keys, kob, d_st, nb)
    eng.synchronize()
    assert guards_intact(buf)
    got = host(d_st).reshape(nb, 16, 8, LW)
    assert [tc.decrypt_u128(got[b]) for b in range(nb)] == [aes_clear.aes_encrypt_block(keys[kob[b] % q], pts[b]) for b in range(nb)]
    for b in range(nb):                                                      # word for word the single-key call from a store of that key alone
        d = dev(st[b])
        eng.aes_encrypt_keyed_packed(settled(store_b[kob[b] % q:kob[b] % q + 1].contiguous()), 128, 1, [0], d, 1)
        eng.synchronize()
        _same(got[b], host(d), "aes_encrypt_keyed_packed, block %d under key %d" % (b, kob[b]))
