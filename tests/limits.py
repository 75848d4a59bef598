"""Shapes and line arithmetic of the limits tests: where byte 2^31 and byte 2^32 fall in every array shape a call reads or writes at
PARAM_TOY, the smallest counts that cross byte 2^32, the tiling that makes a lost high half of an offset visible, and what the binding's
ctypes say about widths.  Pure Python and numpy, no GPU: test_limits_cpu.py pins this file, test_gpu_limits.py and
test_gpu_lwe_dimension.py run what it describes.

The lines.  A byte offset formed in 32 bits goes wrong at 2^31 (a signed product turns negative) or at 2^32 (an unsigned one drops
its high half).  An array of `count` units of `size` bytes crosses a line when some unit starts at or beyond it.

The counts.  crossing_count(size) is the smallest count that leaves two whole units beyond byte 2^32: the first unit that starts at or
beyond the line is number ceil(2^32 / size), and two of them make the count ceil(2^32 / size) + 2.  One unit fewer leaves one.
Where an entry point cuts its batch into chunks, the kernels see offsets inside a chunk and the host adds the chunk's start: there the
count is chunked_count(size, units per chunk), two units into the first chunk that starts at or beyond the line.

The tiling.  No host array has 4 GiB: unit i of a crossing array is unit i mod P of a base of P honest units, P prime.  Every unit
size here and 2^32 are coprime to P (the sizes are below P^2 and no multiple of P; 2^32 is a power of 2), so 2^32 is no multiple of
P units: an offset that lost its high half reads or writes the unit of another residue -- and, where the unit size does not divide
2^32, in the middle of it.  The expected output of a call on a tiled input is the output of the same call on the first P units,
tiled the same way: P units of any size are a whole number of periods of the rows they are made of.
"""
import ctypes

LINE31, LINE32 = 1 << 31, 1 << 32

# PARAM_TOY: k = 1, N = 512, one LWE ciphertext = kN + 1 = 513 words
TOY_ROW_WORDS = 513
ROW = TOY_ROW_WORDS * 8                  # 4,104 bytes
BYTE = 8 * ROW                           # an encrypted byte: 8 rows
BLOCK = 16 * BYTE                        # an AES block: 128 rows
IMC_BLOCK = 16 * 4 * BYTE                # one block of inv_mix_columns' input, [16][4][8][513]
K3_ROW = 2 * 2 * 512 * 8                 # one GGSW level out of K3: (k+1)^2 N words
POLY = 512 * 8                           # one polynomial, K4's input and its output (256 complex doubles)
GGSW8 = 8 * K3_ROW                       # the Fourier GGSWs of one 8-bit input
KEY128 = 11 * BLOCK                      # the LWE round keys of one AES-128 key, [11][16][8][513]

# array shape -> (bytes per unit, unit holding byte 2^31, unit holding byte 2^32)
TABLE = {
    "LWE row": (ROW, 523265, 1046531),
    "byte": (BYTE, 65408, 130816),
    "block": (BLOCK, 4088, 8176),
    "inv_mix_columns input block": (IMC_BLOCK, 1022, 2044),
    "K3 output row": (K3_ROW, 131072, 262144),
    "polynomial": (POLY, 524288, 1048576),
    "Fourier GGSWs of one 8-bit input": (GGSW8, 16384, 32768),
}

P_ROWS = 1031            # the period of an array tiled by rows
P_BYTES = 127            # ... by bytes: the base goes through the CPU oracle's WoPBS, 8 bits a unit
P_BLOCKS = 5             # ... by blocks: the base goes through the CPU oracle's whole cipher
P_IMC = 7                # ... by inv_mix_columns input blocks (block 2,045 cut to 32 bits is block 0: 5 would divide the distance)
P_INPUTS = 13            # ... by the GGSWs of 8-bit inputs, 1 MiB of doubles a unit on the host

AES_BLOCKS = 8180        # the whole-cipher case
KEYS128 = 746            # AES-128 toy keys in LWE form: key 743 holds byte 2^32, keys 744 and 745 start beyond it (745 keys are the first to cross)


def is_prime(n: int) -> bool:
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def unit_holding(line: int, size: int) -> int:
    """the unit of an array of `size`-byte units that holds byte number `line`"""
    return line // size


def first_beyond(line: int, size: int) -> int:
    """the first unit that starts at or beyond byte `line`"""
    return -(-line // size)


def units_beyond(count: int, size: int, line: int = LINE32) -> int:
    """whole units of an array of `count` units that start at or beyond `line`"""
    return max(0, count - first_beyond(line, size))


def crossing_count(size: int, line: int = LINE32) -> int:
    """the smallest count that leaves two whole units beyond `line`"""
    return first_beyond(line, size) + 2


def chunked_count(size: int, per_chunk: int, line: int = LINE32) -> int:
    """for an entry point that cuts its batch into chunks of `per_chunk` units and hands the kernels a pointer to each chunk: the smallest
    count that leaves two whole units beyond `line` in a chunk that STARTS at or beyond it.  crossing_count() alone puts the line inside
    the last chunk, whose start the host still forms below the line; here the host's own offset passes it"""
    return -(-first_beyond(line, size) // per_chunk) * per_chunk + 2


def last_byte(count: int, size: int) -> int:
    return count * size - 1


def truncated_unit(i: int, size: int, bits: int = 32):
    """(unit, byte inside it) where unit i's offset lands once only its low `bits` bits are kept"""
    off = (i * size) & ((1 << bits) - 1)
    return off // size, off % size


def sign_extended_offset(i: int, size: int) -> int:
    """unit i's byte offset as a signed 32-bit product sees it"""
    off = (i * size) & 0xFFFFFFFF
    return off - (1 << 32) if off >> 31 else off


def margin_bytes(guard_units: int, size: int) -> int:
    """what lies in front of a crossing array inside its own allocation: 2^31 bytes and the guard units, rounded up to whole units, so
    that a sign-extended 32-bit offset (at least -2^31) still lands in memory the test owns"""
    return (first_beyond(LINE31, size) + guard_units) * size


# ---- the binding's types against the header's ------------------------------------------------------------------------------------
# a header kind as tests/test_shim_sources.py spells it -> ("pointer",) or ("scalar", bits, signed) or ("void",)
HEADER_SCALARS = {"i32": (32, True), "u32": (32, False), "u64": (64, False), "usize": (ctypes.sizeof(ctypes.c_size_t) * 8, False),
                  "f64": (64, True), "uint8_t": (8, False)}


def header_kind(kind: str):
    if kind == "void":
        return ("void",)
    if kind.startswith("*"):
        return ("pointer",)
    bits, signed = HEADER_SCALARS[kind]
    return ("scalar", bits, signed)


_CTYPES_SCALARS = {ctypes.c_int: True, ctypes.c_uint32: False, ctypes.c_uint64: False, ctypes.c_size_t: False, ctypes.c_int64: True,
                   ctypes.c_int32: True, ctypes.c_uint8: False, ctypes.c_uint16: False, ctypes.c_int16: True, ctypes.c_int8: True,
                   ctypes.c_double: True}


def ctypes_kind(t):
    """a restype or argtype of _native.SIGNATURES in the same terms; c_void_p stands for any data pointer"""
    if t is None:
        return ("void",)
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents") or issubclass(t, ctypes._Pointer):
        return ("pointer",)
    for base, signed in _CTYPES_SCALARS.items():
        if t is base:
            return ("scalar", ctypes.sizeof(t) * 8, signed)
    raise TypeError("no kind for %r" % (t,))
