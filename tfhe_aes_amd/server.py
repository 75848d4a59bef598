"""``Server`` and the S-Box front end: the reference's operator API for the hot path.

Same names, argument meaning and error behaviour as
  /root/reference/src/server/server.rs        Server::{new, aes_encrypt, aes_decrypt, aes_key_expansion, add_scalar}
  (plus aes_decryption_round_keys / aes_decrypt_equivalent: the FIPS-197 section 5.3.5 equivalent inverse cipher; plus AES-192
  and AES-256, which the reference does not have: the same methods read the key size from the leading axis of the key / round keys;
  plus aes_encrypt_public / aes_ctr: public blocks and SP 800-38A CTR with a PUBLIC nonce, every distinct S-Box input evaluated once;
  plus aes_decrypt_public / aes_cbc_decrypt / aes_cfb_decrypt / aes_gcm_ctr: the decryption direction of the public calls and the
  modes whose decryption works on public blocks -- CBC, CFB-128 and the 32-bit counter of GCM;
  plus aes_xts_decrypt: XTS-AES (IEEE 1619) decryption of a public ciphertext, the per-block tweaks derived under encryption;
  plus aes_cbc_mac_streams / aes_ccm_decrypt: CBC-MAC chains over many streams and AES-CCM decryption with an encrypted `valid` bit;
  plus the *_many / *_keyed / aes_ctr_streams methods: many AES keys under one FHE key, round keys [n_keys][Nr+1][16][8][kN+1] and a key
  index per block, word for word the single-key methods key by key; plus packed round keys: pack_round_keys / unpack_round_keys /
  aes_key_expansion_packed, and a PackedRoundKeys -- 3 / 4 / 4 GLWEs per key -- wherever a method takes round keys, the key words read
  from it inside the linear layers, word for word the same method on the unpacked store)
  /root/reference/src/server/sbox/sbox.rs     sbox, many_sbox, mul2 .. mul14
  /root/reference/src/server/sbox/many_wopbs.rs  many_wopbs_without_padding
  /root/reference/src/server/sbox/gen_lut.rs  gen_lut
but batched (a leading block axis) and over flat uint64 arrays:
  byte = [8][kN+1], state = [16][8][kN+1], AES key = [16 | 24 | 32][8][kN+1], round keys = [Nr+1][16][8][kN+1] with
  Nr = 10 | 12 | 14 rounds (FIPS-197 Fig. 4).
Arrays may be numpy (host; staged through HBM by the engine) or torch CUDA tensors (resident,
asynchronous on the engine's stream).  All compute happens in libfheaes.so (HIP); this module
only allocates outputs and forwards.  README.md:57-59 of the reference spells the methods
``aes_encryption`` / ``aes_decryption``; both spellings are provided.
"""
from __future__ import annotations

import dataclasses
import os
from typing import NamedTuple

import numpy as np

from . import _native
from .aes_clear import INV_SBOX, SBOX, mul2, mul3, mul9, mul11, mul13, mul14  # noqa: F401  (re-exported like sbox.rs)
from .client import PackedRoundKeys, SeededCiphertexts, ServerKeys, packed_key_glwes, packed_mod_words
from .dist import shard_blocks
from .params import WopbsParameters


def gen_lut(message_mod: int, carry_mod: int, poly_size: int, nb_block: int, f) -> np.ndarray:
    """gen_lut.rs:9-42.  Returns [nb_block][max(2^nb_block, poly_size)] uint64 (gen_lut.rs:19-23), entry = output bit << 63."""
    if message_mod != 2 or carry_mod != 1:
        raise ValueError("the path uses message_modulus 2, carry_modulus 1 (client.rs:53-54)")
    if poly_size != 512 or not 1 <= nb_block <= 16:
        raise ValueError("polynomial_size must be 512 and nb_block in 1..16")
    table = np.array([int(f(x)) for x in range(1 << nb_block)], dtype=np.uint64)
    return _native.gen_lut(nb_block, table)


def _empty_like(ref, shape):
    if isinstance(ref, np.ndarray):
        return np.empty(shape, dtype=np.uint64)
    import torch

    return torch.empty(shape, dtype=torch.int64, device=ref.device)


def _to_space(arr: np.ndarray, ref):
    if isinstance(ref, np.ndarray):
        return np.ascontiguousarray(arr, dtype=np.uint64)
    import torch

    dev = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint64).view(np.int64)).to(ref.device)
    # the copy ran on torch's current stream; the engine reads `dev` on ITS stream: finish the copy first
    torch.cuda.current_stream(ref.device).synchronize()
    return dev


KEY_BYTES_TO_BITS = {16: 128, 24: 192, 32: 256}       # leading axis of an encrypted AES key
ROUND_KEYS_TO_BITS = {11: 128, 13: 192, 15: 256}      # leading axis of its round keys, Nr + 1


def _key_bits(arr, table, what, ndim=4) -> int:
    """the AES key size an encrypted key / round-key array stands for; any other leading size is refused before the library is called"""
    lead = int(arr.shape[0])
    if arr.ndim != ndim or lead not in table:
        raise ValueError("%s must be [%s]%s[8][kN+1], got shape %s" % (what, " | ".join(map(str, table)), "[16]" * (ndim - 3), tuple(arr.shape)))
    return table[lead]


def many_keys_shape(p, keys, least: int = 1):
    """keys [n_keys][16 | 24 | 32][8][kN+1] of one size -> (the AES key size, the shape of their round keys [n_keys][Nr+1][16][8][kN+1]).
    least = 1: a Server's batch holds at least one key; least = 0: a ServerGroup's may be empty -- no context works then -- so the key
    size is read from the shape, there being no keys[0] to ask"""
    if keys.ndim != 4 or int(keys.shape[0]) < least or (not least and int(keys.shape[1]) not in KEY_BYTES_TO_BITS):
        raise ValueError("keys must be [n_keys][16 | 24 | 32][8][kN+1]%s, got shape %s" % (" with n_keys >= 1" * least, tuple(keys.shape)))
    bits = _key_bits(keys[0], KEY_BYTES_TO_BITS, "key", ndim=3) if least else KEY_BYTES_TO_BITS[int(keys.shape[1])]
    return bits, (int(keys.shape[0]), bits // 32 + 7, 16, 8, p.big1)


def _n_rows(shape) -> int:
    m = 1
    for d in shape:
        m *= int(d)
    return m


def pack_shape(p, ct, width: int):
    """Server.pack's argument [..., kN+1] -> (its number of bits m, the packed shape [ceil(m / N)][words of a GLWE at `width`])"""
    if int(ct.shape[-1]) != p.big1:
        raise ValueError("pack takes [..., kN+1] = [..., %d] words, got shape %s" % (p.big1, tuple(ct.shape)))
    m = _n_rows(ct.shape[:-1])
    return m, ((m + p.N - 1) // p.N, packed_mod_words(p, width))


def unpack_shape(p, packed, shape, width: int):
    """Server.unpack's arguments -> (`shape` as a tuple, its number of bits m); `packed` must be those bits' packed shape"""
    shape = (int(shape),) if isinstance(shape, int) else tuple(int(d) for d in shape)
    m = _n_rows(shape)
    gw = packed_mod_words(p, width)
    if tuple(packed.shape) != ((m + p.N - 1) // p.N, gw):
        raise ValueError("%d bits are packed as [%d][%d] words, got shape %s" % (m, (m + p.N - 1) // p.N, gw, tuple(packed.shape)))
    return shape, m


def _cut(a, lo: int, hi: int):
    """items lo .. hi of an optional per-item list or array: None stays None"""
    return None if a is None else a[lo:hi]


def _data_blocks(data, n_blocks: int):
    """CTR's clear data as a list of n_blocks blocks (ints or 16 bytes each); one `bytes` of 16 n_blocks is cut into blocks"""
    if data is None:
        return None
    if isinstance(data, (bytes, bytearray)):
        if len(data) != 16 * n_blocks:
            raise ValueError("data must hold 16 bytes per block (a partial last block: pad it, then slice the result)")
        return [bytes(data[16 * i:16 * i + 16]) for i in range(n_blocks)]
    data = list(data)
    if len(data) != n_blocks:
        raise ValueError("one data block per counter block expected")
    return data


class RoundKeys(NamedTuple):
    """a round-key argument as the library takes it: the array (which also says which memory space the call works in), the AES key size,
    the number of keys, and whether the array is a packed store"""
    words: object
    key_bits: int
    n_keys: int
    packed: bool


def resolve_round_keys(params, arg, what="round keys", many=False, lwe_only=False) -> RoundKeys:
    """The one reading of a round-key argument, for Server and ServerGroup alike.  `arg` is [Nr+1][16][8][kN+1], [n_keys][Nr+1][16][8][kN+1]
    or a PackedRoundKeys made for `params`.  many False: a single-key method -- one key's array, or a store that holds one key; True: a
    keyed method -- the [n_keys] array or any store; None: either array, one key's read as [1][Nr+1][16][8][kN+1] (the calls on streams,
    pack_round_keys).  lwe_only: the method converts LWE-form keys and a store is refused."""
    if isinstance(arg, PackedRoundKeys):
        if lwe_only:
            raise ValueError("%s in the LWE form [Nr+1][16][8][kN+1] are expected, got a PackedRoundKeys" % what)
        if arg.params != params:
            raise ValueError("these round keys were packed for %s, the server runs %s" % (arg.params.name, params.name))
        if many is False and arg.n_keys != 1:
            raise ValueError("a single-key method takes a store of one key (prk[i]); this one holds %d" % arg.n_keys)
        return RoundKeys(arg.data, arg.key_bits, arg.n_keys, True)
    if many is False:
        return RoundKeys(arg, _key_bits(arg, ROUND_KEYS_TO_BITS, what), 1, False)
    if many is None and arg.ndim == 4:
        arg = arg[None]
    if arg.ndim != 5 or int(arg.shape[0]) < 1:
        raise ValueError("%s of many keys must be [n_keys][11 | 13 | 15][16][8][kN+1] with n_keys >= 1, got shape %s" % (what, tuple(arg.shape)))
    return RoundKeys(arg, _key_bits(arg[0], ROUND_KEYS_TO_BITS, what), int(arg.shape[0]), False)


def _u128(v, what: str) -> int:
    v = int.from_bytes(v, "big") if isinstance(v, (bytes, bytearray)) else int(v)
    if not 0 <= v < 1 << 128:
        raise ValueError("%s is a 128-bit value" % what)
    return v


def _cipher_blocks(ciphertext):
    """a ciphertext as a list of blocks (ints or 16 bytes each); one `bytes` of whole blocks is cut into blocks"""
    if isinstance(ciphertext, (bytes, bytearray)):
        if len(ciphertext) % 16:
            raise ValueError("a ciphertext of whole 16-byte blocks is expected, got %d bytes" % len(ciphertext))
        return [bytes(ciphertext[i:i + 16]) for i in range(0, len(ciphertext), 16)]
    return list(ciphertext)


def _check_counter_bits(counter_bits):
    if counter_bits not in (32, 128):
        raise ValueError("counter_bits must be 32 (the counter field of GCM) or 128 (SP 800-38A), got %r" % (counter_bits,))


def gcm_ctr_args(iv, data, n_blocks, first_block: int = 0):
    """aes_gcm_ctr's arguments -> (J0 = iv || 00000001, n_blocks, data blocks or None)"""
    if not isinstance(iv, (bytes, bytearray)) or len(iv) != 12:
        raise ValueError("aes_gcm_ctr takes a 12-byte IV: any other length derives J0 with GHASH, which is not offered")
    if int(first_block) < 0:
        raise ValueError("first_block must be >= 0")
    if n_blocks is None:
        if data is None:
            raise ValueError("n_blocks or data is needed")
        data = _cipher_blocks(data)
        n_blocks = len(data)
    return int.from_bytes(bytes(iv) + b"\x00\x00\x00\x01", "big"), int(n_blocks), _data_blocks(data, int(n_blocks))


def xts_args(sectors, ciphertext, unit_bytes: int, first_block: int):
    """aes_xts_decrypt's arguments -> (data-unit numbers of units 0 .., blocks per unit, ciphertext blocks).  `sectors`: an int (the number
    of unit 0, consecutive ones follow) or a list; the units are those the blocks first_block .. name"""
    unit_bytes, first_block = int(unit_bytes), int(first_block)
    if unit_bytes < 16 or unit_bytes % 16 or unit_bytes > 16 << 20:
        raise ValueError("a data unit has 1 to 2^20 whole 16-byte blocks (ciphertext stealing is not offered), got %d bytes" % unit_bytes)
    if first_block < 0:
        raise ValueError("first_block must be >= 0")
    ct = _cipher_blocks(ciphertext)
    bpu = unit_bytes // 16
    n_units = (first_block + len(ct) + bpu - 1) // bpu if ct else 0
    if isinstance(sectors, int):
        sectors = [sectors + u for u in range(n_units)]
    sectors = [int(v) for v in sectors]
    if len(sectors) < n_units:
        raise ValueError("blocks %d .. %d lie in %d data units, %d sectors given" % (first_block, first_block + len(ct), n_units, len(sectors)))
    return sectors, bpu, ct


def ccm_args(messages):
    """aes_ccm_decrypt's messages (key_index, nonce, aad, ciphertext, tag) -> the per-stream arrays of the C call, which sees blocks: the
    formatting (SP 800-38C A.2 / A.3: aes_clear.ccm_blocks) is done here.  A dict: key_of_stream, head_blocks (1 + AAD blocks), head (B0 and
    the AAD blocks, stream after stream), ctr0, payload_bytes, ciphertext (concatenated), tags [n][16] (zero-padded), tag_bytes, and
    block_of_message (where each message's plaintext blocks start in the output; its last entry is the total)"""
    from .aes_clear import ccm_blocks

    a = {"key_of_stream": [], "head_blocks": [], "head": [], "ctr0": [], "payload_bytes": [], "ciphertext": b"", "tags": [], "tag_bytes": [],
         "block_of_message": [0]}
    for key_index, nonce, aad, ciphertext, tag in messages:
        ciphertext, tag = bytes(ciphertext), bytes(tag)
        b0, aad_blocks, ctr = ccm_blocks(nonce, aad, len(ciphertext), len(tag))
        a["key_of_stream"].append(int(key_index))
        a["head_blocks"].append(1 + len(aad_blocks))
        a["head"] += [b0] + aad_blocks
        a["ctr0"].append(ctr[0])
        a["payload_bytes"].append(len(ciphertext))
        a["ciphertext"] += ciphertext
        a["tags"].append(list(tag) + [0] * (16 - len(tag)))
        a["tag_bytes"].append(len(tag))
        a["block_of_message"].append(a["block_of_message"][-1] + len(ctr) - 1)
    return a


def cmac_args(messages):
    """aes_cmac_streams' (key_index, message) or aes_cmac_verify's (key_index, message, tag) -> the per-stream arrays of the C call, which
    pads the blocks itself.  A dict: key_of_stream, message_bytes, data (the messages concatenated), chain_blocks (max(1, ceil(len / 16))
    per stream) and, where the entries carry tags, tags [n][16] (zero-padded) and tag_bytes -- else both None"""
    a = {"key_of_stream": [], "message_bytes": [], "data": b"", "chain_blocks": [], "tags": None, "tag_bytes": None}
    messages = [tuple(m) for m in messages]
    if len({len(m) for m in messages}) > 1 or any(len(m) not in (2, 3) for m in messages):
        raise ValueError("every entry is (key_index, message), or every entry is (key_index, message, tag)")
    if messages and len(messages[0]) == 3:
        a["tags"], a["tag_bytes"] = [], []
    for m in messages:
        msg = bytes(m[1])
        a["key_of_stream"].append(int(m[0]))
        a["message_bytes"].append(len(msg))
        a["data"] += msg
        a["chain_blocks"].append(max(1, (len(msg) + 15) // 16))
        if len(m) == 3:
            tag = bytes(m[2])
            if not 4 <= len(tag) <= 16:
                raise ValueError("a CMAC tag is compared on 4 to 16 bytes, got %d" % len(tag))
            a["tags"].append(list(tag) + [0] * (16 - len(tag)))
            a["tag_bytes"].append(len(tag))
    return a


def kw_args(wrapped, kek_of_key=None, n_keks: int = 1):
    """aes_key_unwrap's wrapped keys (byte strings of ONE length, 8 (n + 1) bytes for n = 2..8 semiblocks: RFC 3394) and the KEK index of
    every key -> the arrays of the C call.  A dict: semiblocks (n; 2 for an empty list), wrapped (uint8 [n_keys][8 (n + 1)]) and kek_of_key
    (a list of n_keys indices below n_keks, or None where there is one KEK and no list was given)"""
    wrapped = [bytes(w) for w in wrapped]
    sizes = {len(w) for w in wrapped}
    if len(sizes) > 1:
        raise ValueError("one call unwraps keys of one length, got lengths %s" % sorted(sizes))
    size = sizes.pop() if sizes else 8 * (_native.KW_MIN_SEMIBLOCKS + 1)
    n = size // 8 - 1
    if size % 8 or not _native.KW_MIN_SEMIBLOCKS <= n <= _native.KW_MAX_SEMIBLOCKS:
        raise ValueError("a wrapped key has 8 (n + 1) bytes for n = %d..%d semiblocks, got %d bytes" % (_native.KW_MIN_SEMIBLOCKS, _native.KW_MAX_SEMIBLOCKS, size))
    if kek_of_key is None:
        if n_keks != 1:
            raise ValueError("kek_of_key says which of the %d KEKs wraps every key" % n_keks)
    else:
        kek_of_key = [int(k) for k in kek_of_key]
        if len(kek_of_key) != len(wrapped) or any(not 0 <= k < n_keks for k in kek_of_key):
            raise ValueError("kek_of_key holds one index below %d per wrapped key" % n_keks)
    return {"semiblocks": n, "wrapped": np.frombuffer(b"".join(wrapped), dtype=np.uint8).reshape(len(wrapped), size), "kek_of_key": kek_of_key}


def _shards_by_cost(costs, g: int):
    """whole streams to g contexts, contiguous and balanced by cost: a stream goes to the context in whose g-th of the total cost its
    midpoint lies; shard i is [lo, hi), possibly empty"""
    total, run, hi = sum(costs), 0, [0] * g
    for s, c in enumerate(costs):
        hi[min(g - 1, (2 * run + c) * g // (2 * total)) if total else 0] = s + 1
        run += c
    for i in range(1, g):
        hi[i] = max(hi[i], hi[i - 1])
    return [(hi[i - 1] if i else 0, hi[i]) for i in range(g)]


def cbc_stream_blocks(streams):
    """CBC streams (key_index, iv, ciphertext) -> (key per block, ciphertext blocks, chaining blocks): block i of a stream is chained with
    block i - 1 of the same stream, the first with its iv"""
    key_of_block, blocks, chain = [], [], []
    for key_index, iv, ciphertext in streams:
        ct = _cipher_blocks(ciphertext)
        key_of_block += [int(key_index)] * len(ct)
        blocks += ct
        chain += ([_u128(iv, "iv")] + ct[:-1])[:len(ct)]
    return key_of_block, blocks, chain


def ctr_stream_blocks(streams, counter_bits: int = 128):
    """CTR streams (key_index, iv, first_block, n_blocks, data_or_None) -> (key per block, counter blocks, data blocks or None), the
    counters (iv + first_block + i) mod 2^128 as aes_ctr builds them (counter_bits = 32: only the low 32 bits of iv count); a stream
    without data contributes zero blocks of data"""
    _check_counter_bits(counter_bits)
    m = 1 << counter_bits
    key_of_block, blocks, data, any_data = [], [], [], False
    for key_index, iv, first_block, n_blocks, d in streams:
        n_blocks, first_block = int(n_blocks), int(first_block)
        if n_blocks < 0 or first_block < 0:
            raise ValueError("n_blocks and first_block must be >= 0")
        iv = int.from_bytes(iv, "big") if isinstance(iv, (bytes, bytearray)) else int(iv)
        if not 0 <= iv < 1 << 128:
            raise ValueError("iv is a 128-bit value")
        d = _data_blocks(d, n_blocks)
        any_data = any_data or d is not None
        key_of_block += [int(key_index)] * n_blocks
        blocks += [(iv & ~(m - 1)) | ((iv + first_block + i) & (m - 1)) for i in range(n_blocks)]
        data += [0] * n_blocks if d is None else d
    return key_of_block, blocks, data if any_data else None


class AuditRecord(NamedTuple):
    """one wrong row the audit found: audited launch number, row of that launch, first differing word, that word as the product launch
    wrote it (`got`) and as the latency form wrote it (`want`); `device`: the context's device (ServerGroup), None on a Server"""
    launch: int
    row: int
    word: int
    got: int
    want: int
    device: int | None = None


@dataclasses.dataclass
class AuditReport:
    """counters of the audit since Server.audit(): audited blind-rotation launches, rows compared, rows that differed, and the records
    of the first wrong rows (_native.AUDIT_RECORDS per context at most)"""
    launches: int = 0
    rows_checked: int = 0
    rows_wrong: int = 0
    records: list = dataclasses.field(default_factory=list)


class AuditMismatch(_native.FheAesError):
    """the audit found rows of a launch that the stage's second form computes differently (the latency form of the blind rotation, the plain
    form of a key switch): a defect of the engine or of the machine, and some result since Server.audit() is wrong.  `stage`: the first
    stage of _native.AUDIT_STAGES with a wrong row, `report`: that stage's AuditReport, `records`: its records, `reports`: every enabled
    stage's report by name"""

    def __init__(self, report: AuditReport, stage: str = "blind_rotate", reports: dict | None = None):
        first = report.records[0] if report.records else None
        super().__init__(-3, "the audit%s found %d wrong rows in %d checked over %d launches%s" % (
            "" if stage == "blind_rotate" else " of stage %s" % stage, report.rows_wrong, report.rows_checked, report.launches,
            "" if first is None else "; first: launch %d row %d word %d, %#018x for %#018x" % (first.launch, first.row, first.word, first.got, first.want)))
        self.stage = stage
        self.report = report
        self.records = report.records
        self.reports = {stage: report} if reports is None else reports


def _audit_stages(stages) -> tuple:
    """`stages` as a tuple in the order of _native.AUDIT_STAGES; a name outside it is a ValueError"""
    stages = (stages,) if isinstance(stages, str) else tuple(stages)
    unknown = [s for s in stages if s not in _native.AUDIT_STAGES]
    if unknown:
        raise ValueError("audit stages are a subset of %r (got %r)" % (_native.AUDIT_STAGES, unknown))
    return tuple(s for s in _native.AUDIT_STAGES if s in stages)


def _audit_check(reports: dict) -> AuditReport:
    """reports: the blind rotation's (all zero while its audit is off) and every enabled key switch's.  Raises AuditMismatch for the first
    stage with a wrong row; else the blind rotation's report"""
    for stage, report in reports.items():
        if report.rows_wrong:
            raise AuditMismatch(report, stage, reports)
    return reports["blind_rotate"]


class Server:
    """``Server::new`` (server.rs:32): takes the evaluation keys by value; the engine copies them to HBM."""

    def __init__(self, keys: ServerKeys | None, device: int = 0, engine: _native.Engine | None = None, clone_from: "Server | None" = None):
        """`clone_from`: take the converted key images from another Server's context, device to device (fheaes_clone_keys),
        instead of uploading `keys` again (which may then be None)."""
        self.params: WopbsParameters = clone_from.params if clone_from is not None else keys.params
        self.engine = engine or _native.Engine(self.params, device)
        # device temporaries this wrapper created for calls that are still in flight on the engine's stream; they must
        # outlive the kernels that read them (torch's caching allocator would hand the block out again): freed in synchronize()
        self._inflight = []
        self._audit_stages = ()          # the stages audit() enabled, in the order of _native.AUDIT_STAGES
        if clone_from is not None:
            self.engine.clone_keys_from(clone_from.engine)
        else:
            self.engine.upload_keys(np.ascontiguousarray(keys.ksk), np.ascontiguousarray(keys.bsk), np.ascontiguousarray(keys.pfpksk))

    # ---- S-Box front end --------------------------------------------------------
    def many_wopbs_without_padding(self, ct_in, luts):
        """many_wopbs.rs:31: ct_in [n][bits][kN+1]; luts: list of gen_lut tables [bits][W] (shared by all inputs) or an array
        [n][n_luts][bits][W] (one set per input), W = max(2^bits, 512).  Returns [n][n_luts][bits][kN+1].  The AES path uses
        bits = 8 and 9; wider inputs (up to 16 bits) go through the CMUX tree of vertical_packing first."""
        n, bits = int(ct_in.shape[0]), int(ct_in.shape[1])
        if isinstance(luts, (list, tuple)):
            lut_arr = np.stack([np.asarray(l, dtype=np.uint64) for l in luts])[None]
            per_input = False
        else:
            lut_arr = np.asarray(luts) if isinstance(luts, np.ndarray) else luts
            per_input = lut_arr.ndim == 4 and lut_arr.shape[0] == n and n > 1
            if lut_arr.ndim == 3:
                lut_arr = lut_arr[None]
        n_luts = int(lut_arr.shape[1])
        if int(lut_arr.shape[2]) != bits or int(lut_arr.shape[3]) != max(512, 1 << bits):
            raise ValueError("LUT shape does not match the input radix width")
        lut_dev = _to_space(lut_arr, ct_in) if isinstance(lut_arr, np.ndarray) else lut_arr
        out = _empty_like(ct_in, (n, n_luts, bits, self.params.big1))
        self.engine.wopbs_batch(ct_in, n, bits, lut_dev, n_luts, per_input, out)
        if not isinstance(ct_in, np.ndarray) and lut_dev is not luts:
            self._inflight.append(lut_dev)            # device call: only enqueued, the LUT copy is still being read
        return out

    def sbox(self, ct_in, inv: bool):
        """sbox.rs:46, in place over a batch of bytes [n][8][kN+1]."""
        self.engine.sbox(ct_in, int(ct_in.shape[0]), inv)
        return ct_in

    def many_sbox(self, ct_in, inv: bool):
        """sbox.rs:68: [n][8][kN+1] -> [n][L][8][kN+1]; L=3 (S, 2S, 3S) or 4 (9x, 11x, 13x, 14x)."""
        n = int(ct_in.shape[0])
        out = _empty_like(ct_in, (n, 4 if inv else 3, 8, self.params.big1))
        self.engine.many_sbox(ct_in, n, inv, out)
        return out

    # ---- Server API -------------------------------------------------------------
    def aes_key_expansion(self, key):
        """server.rs:107: key [16][8][kN+1] -> round keys [11][16][8][kN+1]; a key of 24 / 32 bytes (AES-192 / AES-256, FIPS-197
        section 5.2) -> [13 | 15][16][8][kN+1]."""
        bits = _key_bits(key, KEY_BYTES_TO_BITS, "key", ndim=3)
        rk = _empty_like(key, (bits // 32 + 7, 16, 8, self.params.big1))
        self.engine.aes_key_expansion_bits(key, bits, rk)
        return rk

    def aes_encrypt(self, encrypted_round_keys, state):
        """server.rs:39, in place.  state [16][8][kN+1] or a batch [B][16][8][kN+1]; 11 / 13 / 15 round keys: AES-128 / 192 / 256."""
        return self._one_key(self.engine.aes_encrypt_bits, self.engine.aes_encrypt_keyed_packed, self._round_keys(encrypted_round_keys), state)

    def aes_decrypt(self, encrypted_round_keys, state):
        """server.rs:67, in place; 11 / 13 / 15 round keys: AES-128 / 192 / 256."""
        return self._one_key(self.engine.aes_decrypt_bits, self.engine.aes_decrypt_keyed_packed, self._round_keys(encrypted_round_keys), state)

    def aes_decryption_round_keys(self, round_keys):
        """round keys [Nr+1][16][8][kN+1] -> the equivalent inverse cipher's (FIPS-197 section 5.3.5): w[0], InvMixColumns(w[1..Nr-1])
        refreshed to nominal noise, w[Nr].  Once per AES key (2 x 128 (Nr - 1) bit circuit bootstraps: 2 x 1,152 at AES-128); feeds
        aes_decrypt_equivalent."""
        k = self._round_keys(round_keys, lwe_only=True)
        dw = _empty_like(round_keys, tuple(round_keys.shape))
        self.engine.aes_decryption_round_keys_bits(k.words, k.key_bits, dw)
        return dw

    def aes_decrypt_equivalent(self, dec_round_keys, state):
        """the equivalent inverse cipher, in place: one WoPBS per round (Nr per block, as aes_encrypt) instead of aes_decrypt's two
        (server.rs:67-105, :86-89).  Same plaintext as aes_decrypt, other ciphertext words.  state [16][8][kN+1] or [B][16][8][kN+1]."""
        return self._one_key(self.engine.aes_decrypt_equivalent_bits, self.engine.aes_decrypt_equivalent_keyed_packed,
                             self._round_keys(dec_round_keys, "decryption round keys"), state)

    def _round_keys(self, arg, what="round keys", many=False, lwe_only=False) -> RoundKeys:
        return resolve_round_keys(self.params, arg, what, many, lwe_only)

    def _one_key(self, call, packed_call, k: RoundKeys, state):
        """a single-key cipher call, in place: the single-key entry point, or from a one-key store the keyed-packed one with every block
        under key 0"""
        n_blocks = 1 if state.ndim == 3 else int(state.shape[0])
        if k.packed:
            packed_call(k.words, k.key_bits, 1, [0] * n_blocks, state, n_blocks)
        else:
            call(k.words, k.key_bits, state, n_blocks)
        return state

    def add_scalar(self, state, i):
        """server.rs:172, in place.  ``i`` is one integer, or one per block of a batched state."""
        n_blocks = 1 if state.ndim == 3 else int(state.shape[0])
        counters = [i] * n_blocks if isinstance(i, int) else list(i)
        if len(counters) != n_blocks:
            raise ValueError("one counter per block expected")
        self.engine.add_scalar(state, n_blocks, counters)
        return state

    def aes_encrypt_public(self, encrypted_round_keys, blocks, out=None):
        """aes_encrypt of PUBLIC blocks (ints, or 16 `bytes` each) under encrypted round keys: a new [n][16][8][kN+1] (or `out`), in the memory
        space of the round keys, word for word aes_encrypt(round keys, Client.trivial_bytes(blocks)); every distinct S-Box input of
        the batch is evaluated once (include/fheaes.h: fheaes_aes_encrypt_public_bits)."""
        blocks, k = list(blocks), self._round_keys(encrypted_round_keys)
        if k.packed:
            return self._public_keyed(k, [0] * len(blocks), blocks, None, out)
        out = self._public_out(k.words, len(blocks), out)
        self.engine.aes_encrypt_public_bits(k.words, k.key_bits, blocks, out)
        return out

    def aes_ctr(self, encrypted_round_keys, iv, first_block: int, n_blocks: int, data=None, out=None, counter_bits: int = 128):
        """SP 800-38A CTR with a PUBLIC nonce: block i = E_K((iv + first_block + i) mod 2^128) ^ data[i] as a new [n_blocks][16][8][kN+1]
        (data None: the keystream).  `iv`: an int or 16 bytes; `data`: n_blocks ints / 16-byte blocks, or one `bytes` of 16 n_blocks.
        counter_bits = 32: only the low 32 bits of `iv` count, mod 2^32, and the upper 96 never change (the counter field of GCM)."""
        _check_counter_bits(counter_bits)
        k = self._round_keys(encrypted_round_keys)
        if k.packed:
            return self.aes_ctr_streams(encrypted_round_keys, [(0, iv, first_block, n_blocks, data)], out=out, counter_bits=counter_bits)
        n_blocks, first_block = int(n_blocks), int(first_block)
        if n_blocks < 0 or first_block < 0:
            raise ValueError("n_blocks and first_block must be >= 0")
        iv = int.from_bytes(iv, "big") if isinstance(iv, (bytes, bytearray)) else int(iv)
        if not 0 <= iv < 1 << 128:
            raise ValueError("iv is a 128-bit value")
        if counter_bits == 32:
            first_block &= 2 ** 32 - 1           # the counter is mod 2^32
        elif first_block >> 64:                  # the C ABI takes a 64-bit block index; the counter is mod 2^128 anyway
            iv, first_block = (iv + (first_block >> 64 << 64)) % (1 << 128), first_block & (2 ** 64 - 1)
        data = _data_blocks(data, n_blocks)
        out = self._public_out(k.words, n_blocks, out)
        self.engine.aes_ctr_bits(k.words, k.key_bits, iv, first_block, data, n_blocks, out, counter_bits=counter_bits)
        return out

    def aes_gcm_ctr(self, encrypted_round_keys, iv, data=None, n_blocks=None, first_block: int = 0, out=None):
        """The CTR part of AES-GCM (SP 800-38D GCTR) for a 12-byte IV: J0 = iv || 00000001 and data block first_block + i is
        E_K(inc32^(first_block + i + 1)(J0)) ^ data[i] (data None: n_blocks blocks of keystream).  GHASH and the tag are NOT computed: the
        caller authenticates the ciphertext before it gets here, or not at all."""
        j0, n_blocks, data = gcm_ctr_args(iv, data, n_blocks, first_block)
        return self.aes_ctr(encrypted_round_keys, j0, int(first_block) + 1, n_blocks, data=data, out=out, counter_bits=32)

    # ---- the decryption direction of the public calls: CBC and any mode that deciphers public blocks ----------
    def aes_decrypt_public(self, dec_round_keys, blocks, data=None, out=None):
        """aes_decrypt_equivalent of PUBLIC blocks (ints, or 16 `bytes` each) under encrypted decryption round keys
        (aes_decryption_round_keys): a new [n][16][8][kN+1] (or `out`), word for word aes_decrypt_equivalent(dec_round_keys,
        Client.trivial_bytes(blocks)) with the clear `data` blocks (as aes_ctr's) added in the last layer; every distinct S-Box input of the
        batch is evaluated once (include/fheaes.h: fheaes_aes_decrypt_public_bits)."""
        blocks, k = list(blocks), self._round_keys(dec_round_keys, "decryption round keys")
        if k.packed:
            return self._public_keyed(k, [0] * len(blocks), blocks, data, out, inverse=True)
        data = _data_blocks(data, len(blocks))
        out = self._public_out(k.words, len(blocks), out)
        self.engine.aes_decrypt_public_bits(k.words, k.key_bits, blocks, data, out)
        return out

    def aes_cbc_decrypt(self, dec_round_keys, iv, ciphertext, out=None):
        """SP 800-38A CBC decryption of a PUBLIC ciphertext: block i = D_K(C_i) ^ (i ? C_{i-1} : iv) as a new [n][16][8][kN+1].  `iv`: an
        int or 16 bytes; `ciphertext`: ints / 16-byte blocks, or one `bytes` of whole blocks.  To continue a stream pass the last ciphertext
        block of the part before as `iv`.  CBC encryption is serial (every block waits for the one before) and is not offered."""
        ct = _cipher_blocks(ciphertext)
        k = self._round_keys(dec_round_keys, "decryption round keys")
        if k.packed:
            return self.aes_cbc_streams(dec_round_keys, [(0, iv, ct)], out=out)
        out = self._public_out(k.words, len(ct), out)
        self.engine.aes_cbc_decrypt_bits(k.words, k.key_bits, _u128(iv, "iv"), ct, out)
        return out

    def aes_cfb_decrypt(self, encrypted_round_keys, iv, ciphertext, out=None):
        """SP 800-38A CFB-128 decryption of a PUBLIC ciphertext: block i = E_K(i ? C_{i-1} : iv) ^ C_i -- the FORWARD cipher on public
        blocks, so it takes the encryption round keys: aes_encrypt_public_keyed with blocks [iv, C_0, ..] and data C."""
        ct = _cipher_blocks(ciphertext)
        blocks = ([_u128(iv, "iv")] + ct[:-1])[:len(ct)]
        return self._public_keyed(self._round_keys(encrypted_round_keys), [0] * len(ct), blocks, ct, out)

    def aes_xts_decrypt(self, dec_round_keys1, round_keys2, sectors, ciphertext, unit_bytes: int = 512, first_block: int = 0, out=None):
        """XTS-AES decryption (IEEE 1619) of a PUBLIC ciphertext under two encrypted keys: block b of the call is block (first_block + b) %
        (unit_bytes / 16) of data unit (first_block + b) // (unit_bytes / 16), P = D_K1(C ^ T) ^ T with T = E_K2(sector) * alpha^block, as a
        new [n][16][8][kN+1].  dec_round_keys1: aes_decryption_round_keys of key 1; round_keys2: the expansion of key 2 (AES-128 or AES-256,
        both the same size; a PackedRoundKeys of one key for either).  `sectors`: the data-unit number of unit 0 (consecutive ones follow),
        or a list, one per unit; `ciphertext`: bytes of whole blocks, or u128 blocks.  Every tweak costs one more identity WoPBS per byte:
        16 (Nr + 1) byte-WoPBS per block (include/fheaes.h: fheaes_aes_xts_decrypt_bits).  Ciphertext stealing and XTS encryption are not offered."""
        from .aes_clear import xts_tweak_block

        sectors, bpu, ct = xts_args(sectors, ciphertext, unit_bytes, first_block)
        tweaks = [xts_tweak_block(v) for v in sectors]          # IEEE 1619 writes the number little-endian: its low byte is byte 0 of the block
        if isinstance(dec_round_keys1, PackedRoundKeys) != isinstance(round_keys2, PackedRoundKeys):
            # one call reads both key sets in one form: bring the LWE-form set to the other's
            dec_round_keys1, round_keys2 = (k if isinstance(k, PackedRoundKeys) else self.pack_round_keys(k) for k in (dec_round_keys1, round_keys2))
        k1, k2 = self._round_keys(dec_round_keys1, "decryption round keys"), self._round_keys(round_keys2)
        if k1.key_bits != k2.key_bits or k1.key_bits == 192:
            raise ValueError("XTS-AES takes two keys of 128 or of 256 bits, got %d and %d" % (k1.key_bits, k2.key_bits))
        out = self._public_out(k1.words, len(ct), out)
        if ct:
            self.engine.aes_xts_decrypt_bits(k1.words, k2.words, k1.key_bits, tweaks, bpu, int(first_block), ct, out, packed=k1.packed)
        return out

    # ---- many AES keys under one FHE key ----------------------------------------------
    def aes_key_expansion_many(self, keys, out=None):
        """keys [n_keys][16 | 24 | 32][8][kN+1] (one key size) -> round keys [n_keys][Nr+1][16][8][kN+1] (or `out`); slice i is
        aes_key_expansion(keys[i]) word for word, every step one WoPBS over all keys (include/fheaes.h: fheaes_aes_key_expansion_batch)."""
        bits, shape = many_keys_shape(self.params, keys)
        rk = self._many_out(keys, shape, out)
        self.engine.aes_key_expansion_batch(keys, bits, shape[0], rk)
        return rk

    @staticmethod
    def _many_out(ref, shape, out):
        if out is None:
            return _empty_like(ref, shape)
        if tuple(out.shape) != shape:
            raise ValueError("out must be %s, got %s" % (shape, tuple(out.shape)))
        return out

    def aes_decryption_round_keys_many(self, round_keys, out=None):
        """[n_keys][Nr+1][16][8][kN+1] -> the equivalent inverse cipher's round keys of every key (or `out`), the middle bytes of all keys in
        one batch; slice i is aes_decryption_round_keys(round_keys[i]) word for word."""
        k = self._round_keys(round_keys, many=True, lwe_only=True)
        dw = self._many_out(round_keys, tuple(round_keys.shape), out)
        self.engine.aes_decryption_round_keys_batch(k.words, k.key_bits, k.n_keys, dw)
        return dw

    def _keyed(self, call, round_keys, key_of_block, state, packed_call):
        k = self._round_keys(round_keys, many=True)
        if state.ndim != 4:
            raise ValueError("a keyed call works on a batch [n_blocks][16][8][kN+1]; wrap a single state as state[None]")
        (packed_call if k.packed else call)(k.words, k.key_bits, k.n_keys, list(key_of_block), state, int(state.shape[0]))
        return state

    def aes_encrypt_keyed(self, round_keys, key_of_block, state):
        """aes_encrypt with a key per block, in place: block b of state [n_blocks][16][8][kN+1] under round_keys[key_of_block[b]], the words
        aes_encrypt(round_keys[key_of_block[b]], ...) writes for it; every round is one WoPBS over all blocks."""
        return self._keyed(self.engine.aes_encrypt_keyed, round_keys, key_of_block, state, self.engine.aes_encrypt_keyed_packed)

    def aes_decrypt_keyed(self, round_keys, key_of_block, state):
        """aes_decrypt with a key per block, in place."""
        return self._keyed(self.engine.aes_decrypt_keyed, round_keys, key_of_block, state, self.engine.aes_decrypt_keyed_packed)

    def aes_decrypt_equivalent_keyed(self, dec_round_keys, key_of_block, state):
        """aes_decrypt_equivalent with a key per block, in place; dec_round_keys from aes_decryption_round_keys_many."""
        return self._keyed(self.engine.aes_decrypt_equivalent_keyed, dec_round_keys, key_of_block, state, self.engine.aes_decrypt_equivalent_keyed_packed)

    def aes_encrypt_public_keyed(self, round_keys, key_of_block, blocks, data=None, out=None):
        """aes_encrypt_public with a key per block (and, as aes_ctr, clear `data` blocks folded into the last layer): a new
        [n][16][8][kN+1] (or `out`).  Equal S-Box inputs under the same key are evaluated once, equal blocks under different keys are not shared."""
        return self._public_keyed(self._round_keys(round_keys, many=True), key_of_block, blocks, data, out)

    def _public_keyed(self, k: RoundKeys, key_of_block, blocks, data, out, inverse: bool = False):
        """the public blocks under k's keys, forward or (`inverse`, k being decryption round keys) through the equivalent inverse cipher"""
        blocks = list(blocks)
        data = _data_blocks(data, len(blocks))
        out = self._public_out(k.words, len(blocks), out)
        self.engine.aes_public_keyed(k.words, k.key_bits, k.n_keys, list(key_of_block), blocks, data, out, packed=k.packed, inverse=inverse)
        return out

    def aes_ctr_streams(self, round_keys, streams, out=None, counter_bits: int = 128):
        """several SP 800-38A CTR streams with PUBLIC nonces under several keys in one call: `streams` is a list of
        (key_index, iv, first_block, n_blocks, data_or_None), each as the arguments of aes_ctr; returns the streams' blocks concatenated in
        order, [sum n_blocks][16][8][kN+1], each stream's word for word aes_ctr(round_keys[key_index], iv, first_block, n_blocks, data).
        counter_bits as aes_ctr's, one value for all streams."""
        key_of_block, blocks, data = ctr_stream_blocks(streams, counter_bits)
        return self.aes_encrypt_public_keyed(round_keys, key_of_block, blocks, data=data, out=out)

    def aes_decrypt_public_keyed(self, dec_round_keys, key_of_block, blocks, data=None, out=None):
        """aes_decrypt_public with a key per block; dec_round_keys from aes_decryption_round_keys_many, or a PackedRoundKeys of them."""
        return self._public_keyed(self._round_keys(dec_round_keys, "decryption round keys", many=True), key_of_block, blocks, data, out, inverse=True)

    def aes_cbc_streams(self, dec_round_keys, streams, out=None):
        """several CBC ciphertexts under several keys in one call: `streams` is a list of (key_index, iv, ciphertext), each as the arguments
        of aes_cbc_decrypt; returns the streams' blocks concatenated in order, each stream's word for word
        aes_cbc_decrypt(dec_round_keys[key_index], iv, ciphertext)."""
        key_of_block, blocks, chain = cbc_stream_blocks(streams)
        return self.aes_decrypt_public_keyed(dec_round_keys, key_of_block, blocks, data=chain, out=out)

    # ---- CBC-MAC chains and CCM: the engine's integrity results --------------------------------
    def aes_cbc_mac_streams(self, round_keys, streams, init=None, out=None):
        """Raw CBC-MAC chains X_{i+1} = E_K(X_i ^ B_i) over many streams in one call: `streams` is a list of (key_index, blocks) or
        (key_index, blocks, enc, enc_bytes) -- `blocks` the stream's PUBLIC blocks (u128 or 16 bytes each), `enc` an optional encrypted
        addend [len(blocks)][16][8][kN+1] of which block i contributes its first enc_bytes[i] bytes (None: all 16).  `init`
        [n_streams][16][8][kN+1]: where the chains start (None: zero).  Returns the final X of every stream, [n_streams][16][8][kN+1] (or
        `out`), in the caller's order.  The streams are sorted by length; step i of all live streams is one cipher pass
        (include/fheaes.h: fheaes_aes_cbc_mac_keyed).  round_keys: [n_keys][Nr+1][16][8][kN+1], one key's [Nr+1][16][8][kN+1], or a
        PackedRoundKeys."""
        words, bits, n_keys, packed = self._round_keys(round_keys, many=None)
        streams = [tuple(st) + (None, None) * (len(st) == 2) for st in streams]
        keys, lens, clear, enc_bytes = [], [], [], []
        any_enc = any(st[2] is not None for st in streams)
        for key_index, blocks, enc, eb in streams:
            blocks = _cipher_blocks(blocks)
            keys.append(int(key_index)); lens.append(len(blocks))
            clear += [list(_u128(b, "a block").to_bytes(16, "big")) for b in blocks]
            if enc is None:
                enc_bytes += [0] * len(blocks)
            else:
                if tuple(enc.shape) != (len(blocks), 16, 8, self.params.big1):
                    raise ValueError("enc must be [%d][16][8][kN+1], got %s" % (len(blocks), tuple(enc.shape)))
                eb = [16] * len(blocks) if eb is None else [int(x) for x in eb]
                if len(eb) != len(blocks) or any(not 0 <= x <= 16 for x in eb):
                    raise ValueError("enc_bytes: one count in 0..16 per block expected")
                enc_bytes += eb
        n = len(streams)
        out = self._many_out(words, (n, 16, 8, self.params.big1), out)
        if n == 0:
            return out
        enc_all = None
        if any_enc:
            enc_all = _empty_like(words, (max(sum(lens), 1), 16, 8, self.params.big1))
            enc_all[...] = 0
            at = 0
            for (_, _, enc, _), k in zip(streams, lens):
                if enc is not None and k:
                    enc_all[at:at + k] = enc
                at += k
            if not isinstance(enc_all, np.ndarray):
                import torch

                torch.cuda.current_stream(enc_all.device).synchronize()       # torch filled it on its stream; the engine reads it on its own
        self.engine.aes_cbc_mac_keyed(words, bits, n_keys, keys, lens, clear, enc_all, enc_bytes if any_enc else None, init, out, packed=packed)
        if enc_all is not None and not isinstance(enc_all, np.ndarray):
            self._inflight.append(enc_all)            # device call: only enqueued, the gathered addends are still to be read
        return out

    def aes_ccm_decrypt(self, round_keys, messages, out=None, valid_out=None, gate: bool = False):
        """AES-CCM decryption (SP 800-38C, RFC 3610) of PUBLIC messages (key_index, nonce, aad, ciphertext, tag) under encrypted keys, the
        tag compared under encryption.  Returns (plaintext [total_blocks][16][8][kN+1], valid [n][kN+1], block_of_message): message i's
        plaintext is blocks block_of_message[i] .. block_of_message[i + 1], rows beyond its length zero words, and valid[i] decrypts
        (Client.decrypt_bits) to 1 iff its tag verifies.  gate=False: the plaintext is not gated on `valid`; gate=True: the rows of message i
        are multiplied by valid[i] (Server.gate, in place) before they are returned, so a forged message decrypts to zeros, as SP 800-38C
        asks; same shapes, `valid` as before.  One public call (B0, the counters), a
        CBC-MAC chain over all messages step by step, and two WoPBS for the comparison (include/fheaes.h: fheaes_aes_ccm_open_keyed).  The tag
        length is len(tag) (4, 6, .., 16), the nonce has 7..13 bytes.  round_keys as aes_cbc_mac_streams'."""
        words, bits, n_keys, packed = self._round_keys(round_keys, many=None)
        a = ccm_args(messages)
        n, total = len(a["tag_bytes"]), a["block_of_message"][-1]
        out = self._many_out(words, (total, 16, 8, self.params.big1), out)
        valid_out = self._many_out(words, (n, self.params.big1), valid_out)
        if n:
            self.engine.aes_ccm_open_keyed(words, bits, n_keys, a["key_of_stream"], a["head_blocks"], a["head"], a["ctr0"], a["payload_bytes"], a["ciphertext"],
                                           a["tags"], a["tag_bytes"], out if total else None, valid_out, packed=packed)
            if gate and total:
                at = a["block_of_message"]
                self.gate(out, valid_out, [128 * (at[i + 1] - at[i]) for i in range(n)], out=out)
        return out, valid_out, a["block_of_message"]

    # ---- CMAC: the MAC of public messages under encrypted keys, and its check -------------------
    def aes_cmac_subkeys(self, round_keys, out=None):
        """The CMAC subkeys (SP 800-38B 6.1) of every key: [n_keys][2][16][8][kN+1] (or `out`), [j][0] = K1 = L x and [j][1] = K2 = L x^2
        with L = E_K(0^128), both refreshed -- 48 byte-WoPBS per key on top of the public call on one zero block
        (include/fheaes.h: fheaes_aes_cmac_subkeys_keyed).  Derive them once per key set and pass them to aes_cmac_streams /
        aes_cmac_verify as `subkeys`.  round_keys as aes_cbc_mac_streams'."""
        words, bits, n_keys, packed = self._round_keys(round_keys, many=None)
        out = self._many_out(words, (n_keys, 2, 16, 8, self.params.big1), out)
        self.engine.aes_cmac_subkeys_keyed(words, bits, n_keys, out, packed=packed)
        return out

    def _cmac(self, round_keys, a, subkeys, mac_out, valid_out):
        words, bits, n_keys, packed = self._round_keys(round_keys, many=None)
        if subkeys is not None and tuple(subkeys.shape) != (n_keys, 2, 16, 8, self.params.big1):
            raise ValueError("subkeys must be [%d][2][16][8][kN+1] (aes_cmac_subkeys of these round keys), got %s" % (n_keys, tuple(subkeys.shape)))
        if a["key_of_stream"]:
            self.engine.aes_cmac_keyed(words, bits, n_keys, subkeys, a["key_of_stream"], a["message_bytes"], a["data"], a["tags"], a["tag_bytes"], mac_out, valid_out,
                                       packed=packed)

    def aes_cmac_streams(self, round_keys, streams, subkeys=None, out=None):
        """AES-CMAC (SP 800-38B, RFC 4493) of PUBLIC messages under encrypted keys: `streams` is a list of (key_index, message_bytes).
        Returns the encrypted tags, the full T of every stream, [n][16][8][kN+1] (or `out`) in the caller's order; a truncated tag is
        its leading bytes.  The CBC-MAC chain of aes_cbc_mac_streams over the padded blocks, each stream's last block with K1 (whole) or
        K2 (padded) as its encrypted addend (include/fheaes.h: fheaes_aes_cmac_keyed).  subkeys: aes_cmac_subkeys(round_keys), or None:
        derived in the call for the keys in use.  EAX's OMAC^t is this CMAC over [t]_128 || M and needs nothing more.  round_keys as
        aes_cbc_mac_streams'."""
        a = cmac_args(streams)
        if a["tags"] is not None:
            raise ValueError("aes_cmac_streams takes (key_index, message); a tag is checked by aes_cmac_verify")
        words = self._round_keys(round_keys, many=None).words
        out = self._many_out(words, (len(a["key_of_stream"]), 16, 8, self.params.big1), out)
        self._cmac(round_keys, a, subkeys, out, None)
        return out

    def aes_cmac_verify(self, round_keys, messages, subkeys=None, valid_out=None):
        """The CMAC tag check under encryption: `messages` is a list of (key_index, message, tag) with a tag of 4..16 bytes, compared with
        the leading bytes of the CMAC.  Returns valid [n][kN+1] (or `valid_out`): valid[i] decrypts (Client.decrypt_bits) to 1 iff
        message i's tag verifies.  All blocks are public, so no decryption precedes the check: the chain of aes_cmac_streams, then the
        two comparison WoPBS of aes_ccm_decrypt.  EAX's OMAC^t is this CMAC over [t]_128 || M and needs nothing more.  subkeys and
        round_keys as aes_cmac_streams'."""
        a = cmac_args(messages)
        if messages and a["tags"] is None:
            raise ValueError("aes_cmac_verify takes (key_index, message, tag)")
        words = self._round_keys(round_keys, many=None).words
        valid_out = self._many_out(words, (len(a["key_of_stream"]), self.params.big1), valid_out)
        self._cmac(round_keys, a, subkeys, None, valid_out)
        return valid_out

    # ---- AES key unwrap: wrapped AES keys in, encrypted keys out ---------------------------------
    def aes_key_unwrap(self, kek_dec_round_keys, wrapped, kek_of_key=None, out=None, valid_out=None, gate: bool = False):
        """The AES Key Unwrap of RFC 3394 / SP 800-38F under encrypted key-encryption keys: `wrapped` is a list of byte strings of one
        length, 8 (n + 1) bytes for a payload of n = 2..8 semiblocks -- public data, straight from a key store.  Returns (keys, valid):
        keys [n_keys][8 n][8][kN+1] (or `out`), the payloads as fresh ciphertexts -- for n = 2, 3, 4 an argument of aes_key_expansion_many
        -- NOT gated on valid unless gate=True, which multiplies key i's payload by valid[i] (Server.gate, in place): a tampered blob then
        yields the all-zero payload, as RFC 3394 asks; valid [n_keys][kN+1] (or `valid_out`), valid[i] decrypting (Client.decrypt_bits) to
        1 iff key i's integrity constant is right.  kek_dec_round_keys: aes_decryption_round_keys(_many) of one KEK or of many, or a PackedRoundKeys of
        them; kek_of_key: the KEK of every wrapped key, optional with one KEK.  6 n passes of the equivalent inverse cipher over all keys
        (include/fheaes.h: fheaes_aes_kw_unwrap_keyed), one C call per FHEAES_KW_MAX_KEYS keys."""
        k = self._round_keys(kek_dec_round_keys, "KEK decryption round keys", many=None)
        a = kw_args(wrapped, kek_of_key, k.n_keys)
        n, n_keys, cap = a["semiblocks"], len(a["wrapped"]), _native.KW_MAX_KEYS
        out = self._many_out(k.words, (n_keys, 8 * n, 8, self.params.big1), out)
        valid_out = self._many_out(k.words, (n_keys, self.params.big1), valid_out)
        for lo in range(0, n_keys, cap):
            kok = a["kek_of_key"][lo:lo + cap] if a["kek_of_key"] is not None else None
            self.engine.aes_kw_unwrap_keyed(k.words, k.key_bits, k.n_keys, kok, n, a["wrapped"][lo:lo + cap], out[lo:lo + cap], valid_out[lo:lo + cap],
                                            packed=k.packed)
        if gate and n_keys:
            self.gate(out, valid_out, out=out)
        return out, valid_out

    def aes_key_unwrap_packed(self, kek_dec_round_keys, wrapped, kek_of_key=None, chunk: int = 256, gate: bool = False):
        """aes_key_unwrap followed by aes_key_expansion_packed, `chunk` keys at a time, for payloads of 16, 24 and 32 bytes (AES keys):
        returns (a PackedRoundKeys of the unwrapped keys, valid [n_keys][kN+1]), both in the caller's order.  Neither the unwrapped keys
        nor their round keys in LWE form exist for more than `chunk` keys at once.  gate=True gates every key on its `valid` BEFORE the
        expansion: a tampered blob's store entry is then the round keys of the all-zero key."""
        k = self._round_keys(kek_dec_round_keys, "KEK decryption round keys", many=None)
        a = kw_args(wrapped, kek_of_key, k.n_keys)
        n_keys, bits, chunk = len(a["wrapped"]), 64 * a["semiblocks"], int(chunk)
        if bits not in ROUND_KEYS_TO_BITS.values() or n_keys < 1:
            raise ValueError("at least one wrapped AES key (a payload of 16, 24 or 32 bytes) expected")
        if chunk < 1:
            raise ValueError("chunk must be at least one key")
        p = self.params
        data = _empty_like(k.words, (n_keys, packed_key_glwes(p, bits), (p.k + 1) * p.N))
        valid = _empty_like(k.words, (n_keys, p.big1))
        for lo in range(0, n_keys, chunk):
            kok = a["kek_of_key"][lo:lo + chunk] if a["kek_of_key"] is not None else None
            keys, _ = self.aes_key_unwrap(kek_dec_round_keys, [bytes(w) for w in a["wrapped"][lo:lo + chunk]], kok, valid_out=valid[lo:lo + chunk], gate=gate)
            data[lo:lo + chunk] = self.aes_key_expansion_packed(keys, chunk).data
            if not isinstance(data, np.ndarray):
                import torch

                torch.cuda.current_stream(data.device).synchronize()     # the copy ran on torch's stream; the engine reads `data` on its own
            del keys
        return PackedRoundKeys(p, bits, data), valid

    def _public_out(self, round_keys, n_blocks: int, out):
        return self._many_out(round_keys, (n_blocks, 16, 8, self.params.big1), out)

    # ---- packed round keys -------------------------------------------------------
    def pack_round_keys(self, round_keys, out=None) -> PackedRoundKeys:
        """round keys [Nr+1][16][8][kN+1] or [n_keys][Nr+1][16][8][kN+1] (encryption or decryption round keys) -> a PackedRoundKeys in the
        same memory space: key i is pack(round_keys[i]) word for word, G = 3 / 4 / 4 GLWEs (fheaes_pack_round_keys).  `out`: where the
        [n_keys][G][(k+1)N] words go (e.g. a slice of a larger store)."""
        k, p = self._round_keys(round_keys, many=None, lwe_only=True), self.params
        data = self._many_out(k.words, (k.n_keys, packed_key_glwes(p, k.key_bits), (p.k + 1) * p.N), out)
        self.engine.pack_round_keys(k.words, k.key_bits, k.n_keys, data)
        return PackedRoundKeys(p, k.key_bits, data)

    def unpack_round_keys(self, prk: PackedRoundKeys, first: int = 0, count: int | None = None, out=None):
        """keys first .. first + count of a store back in the LWE form [count][Nr+1][16][8][kN+1] (count None: to the end), slice j word for
        word unpack(prk[first + j]): for migration and for tests; needs no keys (fheaes_unpack_round_keys)."""
        self._round_keys(prk, many=True)
        first = int(first)
        count = prk.n_keys - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > prk.n_keys:
            raise ValueError("keys %d .. %d of a store of %d" % (first, first + count, prk.n_keys))
        rk = self._many_out(prk.data, (count, prk.key_bits // 32 + 7, 16, 8, self.params.big1), out)
        self.engine.unpack_round_keys(prk.data, prk.key_bits, first, count, rk)
        return rk

    def aes_key_expansion_packed(self, keys, chunk: int = 256) -> PackedRoundKeys:
        """aes_key_expansion_many followed by pack_round_keys, `chunk` keys at a time: the LWE form of more than `chunk` keys never exists
        at once (23 MB a key at PARAM_OPT against 61 KB packed).  keys [n_keys][16 | 24 | 32][8][kN+1] -> a PackedRoundKeys of n_keys."""
        if keys.ndim != 4 or int(keys.shape[0]) < 1:
            raise ValueError("keys must be [n_keys][16 | 24 | 32][8][kN+1] with n_keys >= 1, got shape %s" % (tuple(keys.shape),))
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be at least one key")
        bits = _key_bits(keys[0], KEY_BYTES_TO_BITS, "key", ndim=3)
        p, n_keys = self.params, int(keys.shape[0])
        data = _empty_like(keys, (n_keys, packed_key_glwes(p, bits), (p.k + 1) * p.N))
        for lo in range(0, n_keys, chunk):
            rk = self.aes_key_expansion_many(keys[lo:lo + chunk])
            self.pack_round_keys(rk, out=data[lo:lo + chunk])
            if not isinstance(rk, np.ndarray):
                self.engine.synchronize()             # the chunk's LWE form is freed here: its readers must be done first
            del rk
        return PackedRoundKeys(p, bits, data)

    # ---- the gate: ciphertexts times an encrypted bit -------------------------------------------
    def _gate_runs(self, valid, m: int, runs, what: str):
        if valid.ndim != 2 or int(valid.shape[1]) != self.params.big1:
            raise ValueError("valid must be [n_gates][kN+1] = [n_gates][%d] words, got shape %s" % (self.params.big1, tuple(valid.shape)))
        n_gates = int(valid.shape[0])
        if runs is None:
            if n_gates == 0 or m % n_gates:
                raise ValueError("%d %s do not divide into equal runs under %d gates: pass the runs" % (m, what, n_gates))
            return [m // n_gates] * n_gates
        runs = [int(r) for r in runs]
        if len(runs) != n_gates or any(r < 0 for r in runs) or sum(runs) != m:
            raise ValueError("one run per gate, adding up to %d %s, expected" % (m, what))
        return runs

    def gate(self, ct, valid, bits_of_gate=None, out=None):
        """ct [..., kN+1] times the encrypted bits valid [n_gates][kN+1]: gate g multiplies the next bits_of_gate[g] ciphertexts of the
        flattened `ct` (None: equal runs of m / n_gates), so a gated bit decrypts to valid * bit -- what releases a plaintext or a key
        only if its check passed, without the server learning which.  One circuit bootstrap per gate and one external product per
        ciphertext (include/fheaes.h: fheaes_gate_bits); a gated ciphertext keeps the noise level of its input.  Returns a new array of
        ct's shape, or `out`, which may be `ct` itself (in place)."""
        p = self.params
        if int(ct.shape[-1]) != p.big1:
            raise ValueError("gate takes [..., kN+1] = [..., %d] words, got shape %s" % (p.big1, tuple(ct.shape)))
        m = 1
        for d in ct.shape[:-1]:
            m *= int(d)
        runs = self._gate_runs(valid, m, bits_of_gate, "ciphertexts")
        out = self._many_out(ct, tuple(ct.shape), out)
        if m:
            self.engine.gate_bits(valid, runs, ct, m, out)
        return out

    def gate_packed(self, packed, valid, glwes_of_gate=None, out=None):
        """Server.gate on packed GLWEs [G][(k+1)N] (Server.pack at width 64, a PackedRoundKeys' data): gate g multiplies the next
        glwes_of_gate[g] GLWEs, all N bits of each, by valid[g] -- one external product per 512 bits (fheaes_gate_packed).  Gate before
        a modulus switch, not after."""
        p = self.params
        gw = (p.k + 1) * p.N
        if int(packed.shape[-1]) != gw:
            raise ValueError("gate_packed takes [..., (k+1)N] = [..., %d] words, got shape %s" % (gw, tuple(packed.shape)))
        g = 1
        for d in packed.shape[:-1]:
            g *= int(d)
        runs = self._gate_runs(valid, g, glwes_of_gate, "GLWEs")
        out = self._many_out(packed, tuple(packed.shape), out)
        if g:
            self.engine.gate_packed(valid, runs, packed, g, out)
        return out

    # ---- packed ciphertexts ------------------------------------------------------
    def pack(self, ct, out=None, width: int = 64):
        """any [..., kN+1] array of one-bit LWE ciphertexts -> [G][(k+1)N], G = ceil(m / N) GLWE ciphertexts holding N = 512 bits each, in
        the memory space of `ct`: bit t of the flattened input sits in GLWE t // N, coefficient t % N (include/fheaes.h:
        fheaes_pack_bits).  409.8 times smaller at PARAM_OPT; no key beyond the ones the Server holds; Client.decrypt_packed reads it.
        `width` in 8..32: the words modulus-switched to `width` bits each, [G][(k+1) 8 width] (fheaes_pack_bits_mod; 16 is the width the
        header's noise arithmetic clears for PARAM_OPT: another 4 times smaller); Client.decrypt_packed(..., width=) reads that."""
        m, shape = pack_shape(self.params, ct, width)
        out = self._many_out(ct, shape, out)
        if m and width == 64:
            self.engine.pack_bits(ct, m, out)
        elif m:
            self.engine.pack_bits_mod(ct, m, width, out)
        return out

    def unpack(self, packed, shape, out=None, width: int = 64):
        """the inverse shape: [G][(k+1)N] -> [*shape, kN+1] (sample extraction of coefficient t % N of GLWE t // N for bit t), LWE
        ciphertexts under the big key that every entry point takes; `shape` may be an int (the number of bits).  `width` in 8..32:
        `packed` is the switched form [G][(k+1) 8 width] and the extraction reads its fields (fheaes_unpack_bits_mod)."""
        shape, m = unpack_shape(self.params, packed, shape, width)
        if out is None:
            out = _empty_like(packed, shape + (self.params.big1,))
        if m and width == 64:
            self.engine.unpack_bits(packed, m, out)
        elif m:
            self.engine.unpack_bits_mod(packed, m, width, out)
        return out

    # ---- seeded input ciphertexts ------------------------------------------------
    def expand(self, seeded: SeededCiphertexts, out=None):
        """SeededCiphertexts (public mask key, first index, bodies [...]) -> the full ciphertexts [..., kN+1], the masks regenerated on the
        GPU (fheaes_expand_lwe_seeded): word for word seeded.expand().  A host array, or -- when `out` is a resident tensor or the bodies
        are one -- a resident tensor, enqueued on the engine's stream; needs no keys."""
        p = self.params
        if seeded.params != p:
            raise ValueError("these ciphertexts were made for %s, the server runs %s" % (seeded.params.name, p.name))
        bodies = seeded.bodies
        shape = tuple(int(d) for d in bodies.shape) + (p.big1,)
        if out is None:
            out = _empty_like(bodies, shape)
        elif tuple(out.shape) != shape:
            raise ValueError("out must be %s, got %s" % (shape, tuple(out.shape)))
        if isinstance(bodies, np.ndarray):
            bodies = np.ascontiguousarray(bodies, dtype=np.uint64)
            if not isinstance(out, np.ndarray):
                bodies = _to_space(bodies, out)
                self._inflight.append(bodies)             # device call: only enqueued, the copy of the bodies is still being read
        m = 1
        for d in shape[:-1]:
            m *= d
        if m:
            self.engine.expand_lwe_seeded(seeded.mask_key, seeded.first_index, bodies, m, out)
        return out

    # README.md:57-59 spellings
    aes_encryption = aes_encrypt
    aes_decryption = aes_decrypt

    # ---- the audit: a check of the blind rotation that needs no secret key (fheaes_audit_set) -------------------------------------------
    def audit(self, rows: int = 64, min_bits: int = 0, seed: int | None = None, stages=("blind_rotate",)):
        """Re-run `rows` sampled rows (0: off; at most _native.AUDIT_MAX_ROWS) of every launch of at least min_bits bits of the `stages` (a
        subset of _native.AUDIT_STAGES) through the stage's second form -- the latency form of the blind rotation, the plain form of the
        key switches -- and compare on the GPU, bit for bit; `seed` None draws 64 bits from os.urandom.  Zeroes the counters; a stage
        that is not named is turned off, and rows = 0 turns every stage off.  Nothing waits for the comparison: ask audit_report() /
        audit_check() once the results matter."""
        stages = _audit_stages(stages) if rows else ()
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        others = [s for s in _native.AUDIT_STAGES if s != "blind_rotate" and (s in stages or s in self._audit_stages)]
        if "blind_rotate" in stages or "blind_rotate" in self._audit_stages or not rows:
            self.engine.audit_set(rows if "blind_rotate" in stages else 0, min_bits, seed)     # the default: exactly this call
        self._audit_stages = ()
        for s in others:
            self.engine.audit_stage_set(s, rows if s in stages else 0, min_bits, seed)
        self._audit_stages = stages

    def audit_report(self, stage: str = "blind_rotate") -> AuditReport:
        """synchronises, then the counters and records of `stage` since audit()"""
        r = self.engine.audit_read() if stage == "blind_rotate" else self.engine.audit_stage_read(stage)
        return AuditReport(r["launches"], r["rows_checked"], r["rows_wrong"], [AuditRecord(*(int(x) for x in rec)) for rec in r["records"]])

    def audit_reports(self) -> dict:
        """{stage: audit_report(stage)} over the stages audit() enabled, in the order of _native.AUDIT_STAGES"""
        return {s: self.audit_report(s) for s in self._audit_stages}

    def audit_check(self) -> AuditReport:
        """the report of the blind rotation's audit, raising AuditMismatch (with the stage and its records) if any row of an enabled stage
        since audit() differed"""
        return _audit_check({s: self.audit_report(s) for s in _native.AUDIT_STAGES if s == "blind_rotate" or s in self._audit_stages})

    def synchronize(self):
        self.engine.synchronize()
        self._inflight.clear()


class ServerGroup:
    """Several engine contexts behind one `Server`-shaped object: what the reference does with rayon over CTR blocks
    (main.rs:55-64, one `&Server` shared by the worker threads) done with one context per GPU -- or several on one GPU --
    and one host thread per context.  Keys are uploaded ONCE (context 0) and cloned device to device into the others
    (fheaes_clone_keys: xGMI between GPUs).  Blocks are sharded contiguously, block i -> context i * G / n (dist.shard_blocks);
    no data moves between contexts.  The Rust counterpart is `GpuServerGroup` in integration/rust_shim/src/lib.rs; the
    one-process-per-GPU path of bench.py (torch.distributed, RCCL broadcast of the seeded keys) is the other way to the same split."""

    def __init__(self, keys: ServerKeys, devices=(0,)):
        if not devices:
            raise ValueError("at least one device")
        self.params = keys.params
        self.devices = tuple(int(d) for d in devices)
        self.servers = [Server(keys, device=devices[0])]
        for d in devices[1:]:
            self.servers.append(Server(None, device=d, clone_from=self.servers[0]))

    def _run_shards(self, jobs):
        """one host thread per context; jobs[i] is None (an empty shard) or a callable for context i"""
        import threading

        errs = [None] * len(jobs)

        def work(i):
            try:
                if jobs[i] is not None:
                    jobs[i](self.servers[i])
                    self.servers[i].synchronize()
            except Exception as e:       # surfaced below, on the caller's thread
                errs[i] = e

        ts = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for e in errs:
            if e is not None:
                raise e

    # ---- the shared parts: two shard builders, one runner in front of _run_shards, the outputs a call allocates ---------------------------
    def _even(self, n: int):
        """n blocks, keys, GLWEs or ciphertexts in contiguous shares that differ by at most one: item i -> context i * G / n"""
        g = len(self.servers)
        return [shard_blocks(n, g, i) for i in range(g)]

    def _by_cost(self, costs):
        """whole streams, messages or gates per context, contiguous and balanced by cost; context 0 may idle"""
        return _shards_by_cost(costs, len(self.servers))

    def _each(self, shards, job, rows=None):
        """job(server i, lo, hi) for shard i = [lo, hi) of `shards`, all at once; the context of an empty shard receives no call.  rows:
        the row offset of every item where a shard is empty by its rows (items rows[lo] .. rows[hi]) and not by its items"""
        if rows is None:
            rows = range(shards[-1][1] + 1)           # item i is row i
        self._run_shards([None if rows[hi] <= rows[lo] else (lambda s, lo=lo, hi=hi: job(s, lo, hi)) for lo, hi in shards])

    def _fill(self, out, job):
        """even over the leading axis of `out`: job(server, lo, hi, out[lo:hi]); returns `out`"""
        self._each(self._even(int(out.shape[0])), lambda s, lo, hi: job(s, lo, hi, out[lo:hi]))
        return out

    def _first(self, result):
        """what context 0 alone computed, finished before it is returned: a resident result is then read from the other contexts' streams,
        which do not wait for context 0's"""
        self.servers[0].synchronize()
        return result

    _round_keys = Server._round_keys
    _many_out = staticmethod(Server._many_out)
    _public_out = Server._public_out

    def _new_blocks(self, round_keys, n: int, what="round keys", many=False):
        """what a call returns as a NEW [n][16][8][kN+1]: allocated next to the round keys, which are read -- and a malformed argument
        refused -- before that; every context fills its shard"""
        return self._public_out(self._round_keys(round_keys, what, many).words, n, None)

    # ---- in place, even over the blocks, the per-block lists sliced alongside ---------------------------------------------------------------
    def _in_place(self, state, call, *per_block):
        """call(server, its blocks of `state`, the same slice of every per-block list)"""
        if state.ndim != 4:
            # Server.aes_encrypt also takes ONE state [16][8][kN+1]; here the first axis is what gets sharded, so a single state would
            # be cut into 16 "blocks" of one byte each: refuse it instead of computing nonsense
            raise ValueError("ServerGroup works on a batch [n_blocks][16][8][kN+1]; wrap a single state as state[None]")
        return self._fill(state, lambda s, lo, hi, part: call(s, part, *(a[lo:hi] for a in per_block)))

    def aes_encrypt(self, round_keys, state):
        """[n_blocks][16][8][kN+1] in place (host arrays: every context stages its own shard)"""
        return self._in_place(state, lambda s, part: s.aes_encrypt(round_keys, part))

    def aes_decrypt(self, round_keys, state):
        return self._in_place(state, lambda s, part: s.aes_decrypt(round_keys, part))

    def aes_decrypt_equivalent(self, dec_round_keys, state):
        return self._in_place(state, lambda s, part: s.aes_decrypt_equivalent(dec_round_keys, part))

    def add_scalar(self, state, counters):
        return self._in_place(state, lambda s, part, cnt: s.add_scalar(part, cnt), list(counters))

    def aes_encrypt_keyed(self, round_keys, key_of_block, state):
        return self._in_place(state, lambda s, part, kob: s.aes_encrypt_keyed(round_keys, kob, part), list(key_of_block))

    def aes_decrypt_keyed(self, round_keys, key_of_block, state):
        return self._in_place(state, lambda s, part, kob: s.aes_decrypt_keyed(round_keys, kob, part), list(key_of_block))

    def aes_decrypt_equivalent_keyed(self, dec_round_keys, key_of_block, state):
        return self._in_place(state, lambda s, part, kob: s.aes_decrypt_equivalent_keyed(dec_round_keys, kob, part), list(key_of_block))

    # ---- a new output, even over the items; a shard at item lo > 0 is handed the public value that goes with lo ------------------------------
    def aes_encrypt_public(self, round_keys, blocks):
        """Server.aes_encrypt_public, the blocks sharded contiguously; each context plans the sharing inside its own shard"""
        blocks = list(blocks)
        return self._fill(self._new_blocks(round_keys, len(blocks)), lambda s, lo, hi, out: s.aes_encrypt_public(round_keys, blocks[lo:hi], out=out))

    def aes_ctr(self, round_keys, iv, first_block: int, n_blocks: int, data=None, counter_bits: int = 128):
        """Server.aes_ctr: context i takes the counter blocks of its shard (first_block + lo ..) and the matching data"""
        _check_counter_bits(counter_bits)
        data = _data_blocks(data, int(n_blocks))
        return self._fill(self._new_blocks(round_keys, int(n_blocks)), lambda s, lo, hi, out: s.aes_ctr(
            round_keys, iv, int(first_block) + lo, hi - lo, _cut(data, lo, hi), out=out, counter_bits=counter_bits))

    def aes_gcm_ctr(self, round_keys, iv, data=None, n_blocks=None, first_block: int = 0):
        """Server.aes_gcm_ctr: context i takes the data blocks first_block + lo .. of its shard"""
        _, n_blocks, data = gcm_ctr_args(iv, data, n_blocks, first_block)
        return self._fill(self._new_blocks(round_keys, n_blocks), lambda s, lo, hi, out: s.aes_gcm_ctr(
            round_keys, iv, _cut(data, lo, hi), hi - lo, int(first_block) + lo, out=out))

    def aes_decrypt_public(self, dec_round_keys, blocks, data=None):
        """Server.aes_decrypt_public, the blocks sharded contiguously; each context plans the sharing inside its own shard"""
        blocks = list(blocks)
        out = self._new_blocks(dec_round_keys, len(blocks), "decryption round keys")
        data = _data_blocks(data, len(blocks))
        return self._fill(out, lambda s, lo, hi, part: s.aes_decrypt_public(dec_round_keys, blocks[lo:hi], data=_cut(data, lo, hi), out=part))

    def _chained(self, method, round_keys, what, iv, ciphertext):
        """CBC and CFB: block i needs block i - 1, so a shard that starts at block lo > 0 is handed C_{lo-1} where shard 0 is handed the iv"""
        ct = _cipher_blocks(ciphertext)
        return self._fill(self._new_blocks(round_keys, len(ct), what), lambda s, lo, hi, out: getattr(s, method)(
            round_keys, ct[lo - 1] if lo else iv, ct[lo:hi], out=out))

    def aes_cbc_decrypt(self, dec_round_keys, iv, ciphertext):
        """Server.aes_cbc_decrypt: a shard that starts at block lo > 0 chains its first block with C_{lo-1}"""
        return self._chained("aes_cbc_decrypt", dec_round_keys, "decryption round keys", iv, ciphertext)

    def aes_cfb_decrypt(self, round_keys, iv, ciphertext):
        """Server.aes_cfb_decrypt: a shard that starts at block lo > 0 enciphers C_{lo-1} first"""
        return self._chained("aes_cfb_decrypt", round_keys, "round keys", iv, ciphertext)

    def aes_xts_decrypt(self, dec_round_keys1, round_keys2, sectors, ciphertext, unit_bytes: int = 512, first_block: int = 0):
        """Server.aes_xts_decrypt: a shard at block lo passes first_block + lo and needs nothing from its neighbour (it derives its own
        tweaks from the units' anchors)"""
        units, _, ct = xts_args(sectors, ciphertext, unit_bytes, first_block)
        return self._fill(self._new_blocks(dec_round_keys1, len(ct), "decryption round keys"), lambda s, lo, hi, out: s.aes_xts_decrypt(
            dec_round_keys1, round_keys2, units, ct[lo:hi], unit_bytes, int(first_block) + lo, out=out))

    # many AES keys: the keyed calls shard on blocks, every context reading the whole set of round keys; the per-key calls shard on keys
    def aes_key_expansion_many(self, keys):
        out = self._many_out(keys, many_keys_shape(self.params, keys, least=0)[1], None)
        return self._fill(out, lambda s, lo, hi, part: s.aes_key_expansion_many(keys[lo:hi], out=part))

    def aes_decryption_round_keys_many(self, round_keys):
        self._round_keys(round_keys, many=True, lwe_only=True)
        out = self._many_out(round_keys, tuple(round_keys.shape), None)
        return self._fill(out, lambda s, lo, hi, part: s.aes_decryption_round_keys_many(round_keys[lo:hi], out=part))

    def _keyed_public(self, method, round_keys, what, key_of_block, blocks, data):
        """Server.aes_encrypt_public_keyed / aes_decrypt_public_keyed, the blocks sharded contiguously; each context plans the sharing
        inside its own shard"""
        kob, blocks = list(key_of_block), list(blocks)
        data = _data_blocks(data, len(blocks))
        if len(kob) != len(blocks):
            raise ValueError("one key index per block expected")
        return self._fill(self._new_blocks(round_keys, len(blocks), what, many=True), lambda s, lo, hi, out: method(
            s, round_keys, kob[lo:hi], blocks[lo:hi], data=_cut(data, lo, hi), out=out))

    def aes_encrypt_public_keyed(self, round_keys, key_of_block, blocks, data=None):
        return self._keyed_public(Server.aes_encrypt_public_keyed, round_keys, "round keys", key_of_block, blocks, data)

    def aes_ctr_streams(self, round_keys, streams, counter_bits: int = 128):
        key_of_block, blocks, data = ctr_stream_blocks(streams, counter_bits)
        return self.aes_encrypt_public_keyed(round_keys, key_of_block, blocks, data=data)

    def aes_decrypt_public_keyed(self, dec_round_keys, key_of_block, blocks, data=None):
        return self._keyed_public(Server.aes_decrypt_public_keyed, dec_round_keys, "decryption round keys", key_of_block, blocks, data)

    def aes_cbc_streams(self, dec_round_keys, streams):
        """Server.aes_cbc_streams: the chaining blocks are built before the blocks are sharded, so a shard boundary inside a stream
        chains with the block before it"""
        key_of_block, blocks, chain = cbc_stream_blocks(streams)
        return self.aes_decrypt_public_keyed(dec_round_keys, key_of_block, blocks, data=chain)

    # ---- a new output, whole streams or messages by cost: a shard needs nothing from its neighbours ----------------------------------------
    def aes_cbc_mac_streams(self, round_keys, streams, init=None):
        """Server.aes_cbc_mac_streams: whole streams per context, contiguous and balanced by block count; a shard needs nothing from
        its neighbours"""
        streams = [tuple(st) for st in streams]
        out = self._new_blocks(round_keys, len(streams), many=None)
        self._each(self._by_cost([len(_cipher_blocks(st[1])) + 1 for st in streams]), lambda s, lo, hi: s.aes_cbc_mac_streams(
            round_keys, streams[lo:hi], init=_cut(init, lo, hi), out=out[lo:hi]))
        return out

    def aes_ccm_decrypt(self, round_keys, messages, gate: bool = False):
        """Server.aes_ccm_decrypt: whole messages per context, contiguous and balanced by chained plus public block count; with gate=True
        every context gates its own messages"""
        messages = [tuple(m) for m in messages]
        a = ccm_args(messages)
        at, n = a["block_of_message"], len(messages)
        words = self._round_keys(round_keys, many=None).words
        out, valid = self._public_out(words, at[-1], None), self._many_out(words, (n, self.params.big1), None)
        cost = [a["head_blocks"][i] - 1 + 2 * (at[i + 1] - at[i]) + 2 for i in range(n)]
        self._each(self._by_cost(cost), lambda s, lo, hi: s.aes_ccm_decrypt(
            round_keys, messages[lo:hi], out=out[at[lo]:at[hi]], valid_out=valid[lo:hi], gate=gate))
        return out, valid, at

    def aes_cmac_streams(self, round_keys, streams, subkeys=None):
        """Server.aes_cmac_streams: whole streams per context, contiguous and balanced by chain blocks; a context without `subkeys` derives
        those of its own shard's keys (the same words on every context).  EAX's OMAC^t is this CMAC over [t]_128 || M and needs nothing
        more."""
        streams = [tuple(st) for st in streams]
        out = self._new_blocks(round_keys, len(streams), many=None)
        self._each(self._by_cost(cmac_args(streams)["chain_blocks"]), lambda s, lo, hi: s.aes_cmac_streams(
            round_keys, streams[lo:hi], subkeys=subkeys, out=out[lo:hi]))
        return out

    def aes_cmac_verify(self, round_keys, messages, subkeys=None):
        """Server.aes_cmac_verify, sharded as aes_cmac_streams.  EAX's OMAC^t is this CMAC over [t]_128 || M and needs nothing more."""
        messages = [tuple(m) for m in messages]
        valid = self._many_out(self._round_keys(round_keys, many=None).words, (len(messages), self.params.big1), None)
        self._each(self._by_cost(cmac_args(messages)["chain_blocks"]), lambda s, lo, hi: s.aes_cmac_verify(
            round_keys, messages[lo:hi], subkeys=subkeys, valid_out=valid[lo:hi]))
        return valid

    # ---- key unwrap: even over the wrapped keys, the payloads and `valid` side by side ----------------------------------------------------------
    def _kw_args(self, kek_dec_round_keys, wrapped, kek_of_key):
        """both key unwraps' arguments -> (the KEKs as RoundKeys, semiblocks per key, the wrapped keys as a list of bytes, the KEK index of
        every key or None); whole wrapped keys go to a context, evenly: every chain has the same length"""
        k = self._round_keys(kek_dec_round_keys, "KEK decryption round keys", many=None)
        a = kw_args(wrapped, kek_of_key, k.n_keys)
        return k, a["semiblocks"], [bytes(w) for w in a["wrapped"]], a["kek_of_key"]

    def aes_key_unwrap(self, kek_dec_round_keys, wrapped, kek_of_key=None, gate: bool = False):
        """Server.aes_key_unwrap: whole keys per context, contiguous; every context reads all KEKs and, with gate=True, gates its own
        keys.  Returns (keys, valid)."""
        k, semiblocks, wrapped, kok = self._kw_args(kek_dec_round_keys, wrapped, kek_of_key)
        n, big1 = len(wrapped), self.params.big1
        keys, valid = self._many_out(k.words, (n, 8 * semiblocks, 8, big1), None), self._many_out(k.words, (n, big1), None)
        self._each(self._even(n), lambda s, lo, hi: s.aes_key_unwrap(
            kek_dec_round_keys, wrapped[lo:hi], _cut(kok, lo, hi), out=keys[lo:hi], valid_out=valid[lo:hi], gate=gate))
        return keys, valid

    def aes_key_unwrap_packed(self, kek_dec_round_keys, wrapped, kek_of_key=None, chunk: int = 256, gate: bool = False):
        """Server.aes_key_unwrap_packed with whole keys per context: every context unwraps, expands and packs its shard `chunk` keys at a
        time; the store and `valid` are put together in the caller's order.  Returns (PackedRoundKeys, valid)."""
        k, _, wrapped, kok = self._kw_args(kek_dec_round_keys, wrapped, kek_of_key)
        parts = {}                                   # by the shard's first key: (store, valid) of every context that worked

        def job(s, lo, hi):
            parts[lo] = s.aes_key_unwrap_packed(kek_dec_round_keys, wrapped[lo:hi], _cut(kok, lo, hi), chunk, gate=gate)

        shards = self._even(len(wrapped))
        if not wrapped:
            raise ValueError("at least one wrapped AES key (a payload of 16, 24 or 32 bytes) expected")
        self._each(shards, job)
        parts = [parts[lo] for lo in sorted(parts)]
        if isinstance(k.words, np.ndarray):
            data, valid = np.concatenate([x[0].data for x in parts]), np.concatenate([x[1] for x in parts])
        else:
            import torch

            data, valid = torch.cat([x[0].data for x in parts]), torch.cat([x[1] for x in parts])
            torch.cuda.current_stream(data.device).synchronize()
        return PackedRoundKeys(self.params, parts[0][0].key_bits, data), valid

    # ---- context 0 alone, then finished (_first): the calls on one key or one key set, whose result every context reads afterwards.  A packed
    # store is small, so every context reads the whole of it (as the keyed calls read all round keys); the cipher methods above take a
    # PackedRoundKeys wherever they take round keys, since every context's Server does
    def aes_key_expansion(self, key):
        """expanded on context 0"""
        return self._first(self.servers[0].aes_key_expansion(key))

    def aes_decryption_round_keys(self, round_keys):
        """converted on context 0"""
        return self._first(self.servers[0].aes_decryption_round_keys(round_keys))

    def aes_cmac_subkeys(self, round_keys):
        """derived on context 0"""
        return self._first(self.servers[0].aes_cmac_subkeys(round_keys))

    def pack_round_keys(self, round_keys) -> PackedRoundKeys:
        """packed on context 0"""
        return self._first(self.servers[0].pack_round_keys(round_keys))

    def unpack_round_keys(self, prk: PackedRoundKeys, first: int = 0, count: int | None = None):
        return self._first(self.servers[0].unpack_round_keys(prk, first, count))

    def aes_key_expansion_packed(self, keys, chunk: int = 256) -> PackedRoundKeys:
        return self._first(self.servers[0].aes_key_expansion_packed(keys, chunk))

    # ---- the gates: whole gates by cost, a context working iff its gates have rows -------------------------------------------------------------
    _gate_runs = Server._gate_runs

    def _gates(self, method, ct, valid, runs, unit_words: int):
        """whole gates per context, contiguous and balanced by run length: context i gates the rows of its gates, out of place"""
        flat = ct.reshape(-1, unit_words)
        runs = self._gate_runs(valid, int(flat.shape[0]), runs, "rows")
        out = _empty_like(ct, tuple(flat.shape))
        at = [0]
        for r in runs:
            at.append(at[-1] + r)
        self._each(self._by_cost([r + 1 for r in runs]), lambda s, lo, hi: getattr(s, method)(
            flat[at[lo]:at[hi]], valid[lo:hi], runs[lo:hi], out=out[at[lo]:at[hi]]), rows=at)
        return out.reshape(tuple(ct.shape))

    def gate(self, ct, valid, bits_of_gate=None):
        """Server.gate, sharded on whole gates; the words are those of one context whatever the number of contexts"""
        return self._gates("gate", ct, valid, bits_of_gate, self.params.big1)

    def gate_packed(self, packed, valid, glwes_of_gate=None):
        """Server.gate_packed, sharded on whole gates"""
        return self._gates("gate_packed", packed, valid, glwes_of_gate, (self.params.k + 1) * self.params.N)

    # ---- packing and seeded ciphertexts: even over GLWEs of N bits, the last one ragged, and over ciphertexts -------------------------------
    def pack(self, ct, width: int = 64):
        """Server.pack, sharded on whole GLWEs (N bits = 4 AES blocks): context i packs GLWEs i * G / n .. of the flattened input, so the
        words are those of one context whatever the number of contexts"""
        p = self.params
        m, shape = pack_shape(p, ct, width)
        flat = ct.reshape(-1, p.big1)
        return self._fill(_empty_like(ct, shape), lambda s, lo, hi, out: s.pack(flat[lo * p.N:min(hi * p.N, m)], out=out, width=width))

    def unpack(self, packed, shape, width: int = 64):
        """Server.unpack with the same split: context i extracts the bits of its GLWEs"""
        p = self.params
        shape, m = unpack_shape(p, packed, shape, width)
        out = _empty_like(packed, (m, p.big1))

        def job(s, lo, hi):
            b0, b1 = lo * p.N, min(hi * p.N, m)
            s.unpack(packed[lo:hi], b1 - b0, out=out[b0:b1], width=width)

        self._each(self._even(int(packed.shape[0])), job)
        return out.reshape(shape + (p.big1,))

    def expand(self, seeded: SeededCiphertexts):
        """Server.expand, sharded on ciphertexts: context i expands ciphertexts i * G / n .. of the flattened list and passes
        first_index + its offset, so the words are those of one context"""
        flat = seeded.bodies.reshape(-1)
        out = self._fill(_empty_like(flat, (int(flat.shape[0]), self.params.big1)), lambda s, lo, hi, part: s.expand(
            dataclasses.replace(seeded, first_index=(int(seeded.first_index) + lo) % (1 << 64), bodies=flat[lo:hi]), out=part))
        return out.reshape(tuple(int(d) for d in seeded.bodies.shape) + (self.params.big1,))

    def clone_info(self):
        """per cloned context: how its keys got there ({"path": "same_device" | "peer" | "staged", "bytes", "seconds"})"""
        return [s.engine.clone_info() for s in self.servers[1:]]

    def audit(self, rows: int = 64, min_bits: int = 0, seed: int | None = None, stages=("blind_rotate",)):
        """Server.audit on every context, each under a seed of its own: drawn from os.urandom, or -- a given `seed` -- seed + the context's index"""
        for i, s in enumerate(self.servers):
            s.audit(rows, min_bits, None if seed is None else (int(seed) + i) % (1 << 64), stages=stages)

    def audit_report(self, stage: str = "blind_rotate") -> AuditReport:
        """the contexts' counters of `stage` summed, their records tagged with the device"""
        total = AuditReport()
        for d, s in zip(self.devices, self.servers):
            r = s.audit_report(stage)
            total.launches += r.launches
            total.rows_checked += r.rows_checked
            total.rows_wrong += r.rows_wrong
            total.records += [rec._replace(device=d) for rec in r.records]
        return total

    def audit_check(self) -> AuditReport:
        """the summed report of the blind rotation's audit, raising AuditMismatch (with the stage, its summed report and, in `reports`, every
        checked stage's) if any row of an enabled stage differed on any context.  A group has no audit_reports(): audit_report(stage) per
        stage of servers[0]'s enabled stages gives the same"""
        return _audit_check({s: self.audit_report(s) for s in _native.AUDIT_STAGES if s == "blind_rotate" or s in self.servers[0]._audit_stages})
