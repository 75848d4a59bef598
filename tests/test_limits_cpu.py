"""limits.py pinned on the CPU: the line table of every array shape, the smallest-count rule, the residues that make a truncated
offset visible, the binding's argument types against the header's, and the parameter sets fheaes_create refuses before it looks for
a device."""
import ctypes
import dataclasses

import pytest

import limits as lm
from test_shim_sources import header_decls
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _native

PERIODS = {"LWE row": lm.P_ROWS, "byte": lm.P_BYTES, "block": lm.P_BLOCKS, "inv_mix_columns input block": lm.P_IMC,
           "K3 output row": lm.P_ROWS, "polynomial": lm.P_ROWS, "Fourier GGSWs of one 8-bit input": lm.P_INPUTS}


def test_unit_sizes_are_the_toy_shapes():
    p = PARAM_TOY
    assert lm.TOY_ROW_WORDS == p.big1 and lm.ROW == 4104 and lm.BYTE == 32832 and lm.BLOCK == 525312 and lm.IMC_BLOCK == 2101248
    assert lm.K3_ROW == (p.k + 1) ** 2 * p.N * 8 == 16384 and lm.POLY == p.N * 8 == 4096 and lm.GGSW8 == 8 * p.ggsw_words * 8 == 131072
    assert lm.KEY128 == 5778432
    assert PARAM_OPT.big1 * 8 == 16392 and 2048 * 128 * 16392 > lm.LINE32          # 2,048 blocks at PARAM_OPT are 4.3 GB


@pytest.mark.parametrize("shape", sorted(lm.TABLE))
def test_line_table(shape):
    size, at31, at32 = lm.TABLE[shape]
    assert lm.unit_holding(lm.LINE31, size) == at31 and lm.unit_holding(lm.LINE32, size) == at32
    assert at31 * size <= lm.LINE31 < (at31 + 1) * size and at32 * size <= lm.LINE32 < (at32 + 1) * size
    aligned = lm.LINE32 % size == 0
    assert aligned == (shape in ("K3 output row", "polynomial", "Fourier GGSWs of one 8-bit input"))
    assert lm.first_beyond(lm.LINE32, size) == at32 + (0 if aligned else 1)


def test_the_row_that_holds_the_line_starts_4072_bytes_before_it():
    assert 1046531 * lm.ROW == 4294963224 == lm.LINE32 - 4072


@pytest.mark.parametrize("shape", sorted(lm.TABLE))
def test_smallest_count_rule(shape):
    size = lm.TABLE[shape][0]
    n = lm.crossing_count(size)
    assert lm.units_beyond(n, size) == 2 and lm.units_beyond(n - 1, size) == 1
    assert (n - 2) * size >= lm.LINE32 and lm.last_byte(n, size) > lm.LINE32
    assert lm.units_beyond(n, size, lm.LINE31) > 2                                # and byte 2^31 long before


def test_counts_the_issue_names():
    assert lm.crossing_count(lm.ROW) == 1046534 and lm.crossing_count(lm.BYTE) == 130819 and lm.crossing_count(lm.BLOCK) == 8179
    assert lm.crossing_count(lm.IMC_BLOCK) == 2047 and lm.crossing_count(lm.K3_ROW) == 262146
    assert lm.crossing_count(lm.POLY) == 1048578 and lm.crossing_count(lm.GGSW8) == 32770
    assert lm.AES_BLOCKS >= lm.crossing_count(lm.BLOCK) and lm.units_beyond(lm.AES_BLOCKS, lm.BLOCK) == 3
    # AES-128 keys in LWE form: key 743 holds the line; 745 keys are the first to cross it (key 744 lies wholly beyond, 744 keys leave
    # none there); the case runs one more, so that two keys lie beyond the line as two units do in every other case
    assert lm.unit_holding(lm.LINE32, lm.KEY128) == 743 and lm.units_beyond(745, lm.KEY128) == 1 and lm.units_beyond(744, lm.KEY128) == 0
    assert lm.KEYS128 == lm.crossing_count(lm.KEY128) == 746 and 745 * lm.KEY128 > lm.LINE32


def test_chunked_counts():
    """the first chunk that starts at or beyond the line, and two units into it; one chunk fewer starts below the line"""
    for size, per, want in ((lm.ROW, 32768, 1048578), (lm.ROW, 65536, 1048578), (lm.BYTE, 4096, 131074), (3 * lm.BYTE, 4096, 45058)):
        n = lm.chunked_count(size, per)
        assert n == want and (n - 2) % per == 0 and (n - 2) * size >= lm.LINE32 > (n - 2 - per) * size
        assert n >= lm.crossing_count(size) and lm.units_beyond(n, size) >= 2
    assert 45058 * lm.BYTE < lm.LINE31                                          # many_sbox's input stays small


def test_periods_are_prime_and_coprime_to_sizes_and_lines():
    for period in (lm.P_ROWS, lm.P_BYTES, lm.P_BLOCKS, lm.P_IMC, lm.P_INPUTS):
        assert lm.is_prime(period)
        assert lm.LINE32 % period and lm.LINE31 % period
    assert [n for n in range(20) if lm.is_prime(n)] == [2, 3, 5, 7, 11, 13, 17, 19]
    for shape, (size, _, _) in lm.TABLE.items():
        assert size % PERIODS[shape]


@pytest.mark.parametrize("shape", sorted(lm.TABLE))
def test_a_truncated_offset_lands_on_another_residue(shape):
    """every unit beyond byte 2^32: with its offset cut to 32 bits it is a unit of another residue, and mid-unit wherever the unit
    size does not divide 2^32; sign-extended, it lands inside the margin or the array, never in front of the allocation"""
    size, period = lm.TABLE[shape][0], PERIODS[shape]
    n = lm.crossing_count(size)
    for i in range(lm.first_beyond(lm.LINE32, size), n):
        j, inside = lm.truncated_unit(i, size)
        assert j != i and j % period != i % period
        assert (inside != 0) == (lm.LINE32 % size != 0)
    margin = lm.margin_bytes(2, size)
    assert margin >= lm.LINE31 + 2 * size and margin % size == 0
    for i in range(lm.first_beyond(lm.LINE31, size), n):
        assert -margin <= lm.sign_extended_offset(i, size) < n * size
    # a unit between the two lines read through a signed 32-bit offset: in front of the array, inside the margin
    i = lm.first_beyond(lm.LINE31, size)
    assert -margin <= lm.sign_extended_offset(i, size) < 0


# ---- _native.SIGNATURES against include/fheaes.h -----------------------------------------------------------------------------------
def test_signatures_have_the_headers_types():
    """argument count, pointer or scalar for every argument and the return value, and every scalar's width and signedness: a c_uint32
    where the header says uint64_t would truncate exactly the counts the limits tests send"""
    header = header_decls()
    assert set(header) == set(_native.SIGNATURES)
    for name, (res, args) in sorted(_native.SIGNATURES.items()):
        hret, hkinds = header[name]
        assert len(args) == len(hkinds), "%s: %d arguments bound, %d declared" % (name, len(args), len(hkinds))
        assert lm.ctypes_kind(res) == lm.header_kind(hret), "%s returns %s, bound as %r" % (name, hret, res)
        for i, (a, h) in enumerate(zip(args, hkinds)):
            assert lm.ctypes_kind(a) == lm.header_kind(h), "%s argument %d: header %s, bound as %r" % (name, i, h, a)


def test_the_kinds_tell_widths_apart():
    assert lm.ctypes_kind(ctypes.c_uint32) != lm.ctypes_kind(ctypes.c_uint64) != lm.ctypes_kind(ctypes.c_int)
    assert lm.ctypes_kind(ctypes.c_uint32) != lm.ctypes_kind(ctypes.c_int)
    assert lm.ctypes_kind(ctypes.c_void_p) == lm.ctypes_kind(ctypes.POINTER(ctypes.c_uint64)) == lm.header_kind("*u64") == ("pointer",)
    assert lm.header_kind("u64") == ("scalar", 64, False) and lm.header_kind("i32") == ("scalar", 32, True)
    assert lm.ctypes_kind(None) == lm.header_kind("void")


# ---- parameter sets fheaes_create refuses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [("lwe_dimension", 0), ("lwe_dimension", 4097), ("glwe_dimension", 2), ("glwe_dimension", 3)])
def test_create_refuses_what_supported_does_not_admit(field, value):
    """refused before any device is looked for, with FHEAES_ERR_INVALID and a message naming the field"""
    with pytest.raises(_native.FheAesError) as e:
        _native.Engine(dataclasses.replace(PARAM_TOY, **{field: value}), device=0)
    assert e.value.code == -1 and field in str(e.value), str(e.value)
