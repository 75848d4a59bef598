"""ServerGroup decides, for every Server method it offers, which slice of the blocks, keys, streams, messages, gates, GLWEs or seeded
ciphertexts a context gets, which public value goes with it (first_block + lo, first_index + lo, the chaining block ct[lo - 1]) and where
its output lands.  The checks and result shapes are Server's own, the splits come from two builders (_even, _by_cost) and run through one
runner (_each); the slices and offsets are the group's alone.  This is the table of calls that test_group_splits_cpu.py runs on an echo model
of Server (g = 1..6, n = 0..7) and test_gpu_group_splits.py on groups of 1, 3 and 5 contexts at PARAM_TOY.  A helper module like
chunk_seams.py and workspace_state.py: no test, no fixture.

A case is (name, method, build, items, check_clear, sizes, least):

  method       the public method of ServerGroup (and of Server) the case calls
  build(env, n) -> h   the call on n items: h["a"] the positional arguments, h["kw"] the keyword arguments, h["state"] the position of
               the argument the call works on in place (None: it returns new arrays); the rest is what check_clear needs.  Every uint64
               array in h["a"] / h["kw"] (inside tuples, lists, a PackedRoundKeys or a SeededCiphertexts too) is an array of ciphertext
               words that may as well be resident
  items(h)     how the group splits the call, restated here and not read from the group: ("even", count) -- count blocks, keys, GLWEs or
               ciphertexts in contiguous shares that differ by at most one (dist.shard_blocks); ("cost", costs, rows) -- whole streams by
               cost (server._shards_by_cost), a context working iff its streams have rows (None: iff it has streams); ("first",) -- the
               call runs on context 0 alone
  check_clear(env, h, outs)   outs: the outputs as uint64 host arrays (flat()).  Decrypts them and compares with the clear model
               (tfhe_aes_amd.aes_clear): the reference is never the engine alone
  sizes        the n the GPU module runs: the smallest that split interestingly -- 4 blocks are 2 + 1 + 1 on 3 contexts and
               1 + 1 + 1 + 1 + 0 on 5; 2 keys are 1 + 1 + 0; n < g leaves empty shards; n = 0 leaves nothing but them
  least        the smallest n the method takes at all (a Server refuses fewer): the CPU module runs n = least .. 7

What the table leaves out, because one Server refuses it: n = 0 of aes_key_expansion_many, aes_decryption_round_keys_many,
aes_key_unwrap_packed, pack_round_keys, unpack_round_keys, aes_key_expansion_packed and aes_cmac_subkeys (a store or a batch holds at
least one key), and n = 0 of gate / gate_packed with bits_of_gate None (no gate, no equal runs).  A zero-length run is NOT refused: the
runs [0, 3, 1] stay.
"""
from collections import namedtuple

import numpy as np

import ccm
import cmac
import keywrap
import xts
from aes_vectors import A3_KEY, BASE, F1_KEY, F1_PT, F5, F5_CTR, FIPS_C, MASK128
from packed_key_model import key_glwes
from public_modes import GCM_IV, IV, cbc_encrypt, cfb128_encrypt
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.client import PackedRoundKeys, SeededCiphertexts, packed_key_glwes, packed_mod_words
from workspace_state import Env as _Env, dec_blocks, enc_blocks, key_sets, rand_blocks

Case = namedtuple("Case", "name method build items check_clear sizes least")

KEYS = (FIPS_C[128][0], F1_KEY)                      # key 0: FIPS-197 C.1, key 1: SP 800-38A F.1
KOB = [1, 0, 0, 1, 0, 1, 1]                          # the key of block i: 4 blocks under 2 keys are [1, 0, 0, 1]
EXCLUDED = ("clone_info", "audit", "audit_report", "audit_check")        # test_gpu_group_splits.py has the audit's own test
MAX_N = 7


# ---- the two environments ---------------------------------------------------------------------------------------------------------------
class Env(_Env):
    """workspace_state.Env, plus the one Server that makes the inputs only a Server can make: a packed store, packed GLWEs"""

    def __init__(self, kit, server):
        super().__init__(kit)
        self.server, self.cache = server, {}

    def store(self, sets, inverse=False):
        prk = self.server.pack_round_keys(sets)
        self.server.synchronize()
        return prk

    def packed(self, ct, width=64):
        out = self.server.pack(ct, width=width)
        self.server.synchronize()
        return out


class ShapeClient:
    """a client that encrypts nothing: distinct words in the shapes of a real one's, for the tests of the split arithmetic, which never
    decrypt"""

    def __init__(self, params):
        self.params, self.count = params, 0

    def _words(self, shape):
        size = int(np.prod(shape, dtype=np.int64))
        out = (np.arange(size, dtype=np.uint64) + np.uint64(self.count << 32)).reshape(shape)
        self.count += 1
        return out

    def encrypt_bits(self, bits):
        return self._words(np.asarray(bits).shape + (self.params.big1,))

    def encrypt_bytes(self, values):
        return self._words((np.asarray(values).size, 8, self.params.big1))

    def encrypt_aes_key(self, key):
        return self.encrypt_bytes(list(key))

    def encrypt_bits_seeded(self, bits, first_index=0):
        return SeededCiphertexts(self.params, np.arange(8, dtype=np.uint32) + np.uint32(self.count), int(first_index), self._words(np.asarray(bits).shape))


class ShapeEnv:
    """Env without keys, engine or oracle: build() gives arrays of the right shapes at any parameter set"""

    def __init__(self, params):
        self.p, self.client, self.cache = params, ShapeClient(params), {}

    def store(self, sets, inverse=False):
        p, bits = self.p, {11: 128, 13: 192, 15: 256}[int(sets.shape[-4])]
        n_keys = int(sets.shape[0]) if sets.ndim == 5 else 1
        return PackedRoundKeys(p, bits, self.client._words((n_keys, packed_key_glwes(p, bits), (p.k + 1) * p.N)))

    def packed(self, ct, width=64):
        m = int(np.prod(ct.shape[:-1], dtype=np.int64))
        return self.client._words(((m + self.p.N - 1) // self.p.N, packed_mod_words(self.p, width)))


# ---- helpers --------------------------------------------------------------------------------------------------------------------------------
def sets(env, keys=KEYS, inverse=False):
    """the keys' (decryption) round keys [n_keys][Nr+1][16][8][kN+1], encrypted once per environment: every call only reads them"""
    tag = ("sets", tuple(keys), inverse)
    if tag not in env.cache:
        env.cache[tag] = key_sets(env.client, keys, inverse)
    return env.cache[tag]


def call(target, case, h):
    """the case's call on a Server or a ServerGroup"""
    return getattr(target, case.method)(*h["a"], **h["kw"])


def flat(result):
    """what a call returned as a tuple of arrays: a PackedRoundKeys is its data, a list of integers (block_of_message) an array"""
    out = []
    for r in result if isinstance(result, tuple) else (result,):
        if isinstance(r, PackedRoundKeys):
            r = r.data
        out.append(np.array(r, dtype=np.int64) if isinstance(r, list) else r)
    return tuple(out)


def map_words(obj, f):
    """obj with f applied to every uint64 array in it: what makes a call's ciphertext arguments resident, or copies them"""
    if isinstance(obj, np.ndarray):
        return f(obj) if obj.dtype == np.uint64 else obj
    if isinstance(obj, PackedRoundKeys):
        return PackedRoundKeys(obj.params, obj.key_bits, f(obj.data))
    if isinstance(obj, SeededCiphertexts):
        return SeededCiphertexts(obj.params, obj.mask_key, obj.first_index, f(obj.bodies))
    if isinstance(obj, (list, tuple)):
        return type(obj)(map_words(x, f) for x in obj)
    if isinstance(obj, dict):
        return {k: map_words(v, f) for k, v in obj.items()}
    return obj


def fresh(h):
    """h with a copy of the state an in-place call overwrites; everything else is only read and stays shared"""
    if h["state"] is None:
        return h
    a = list(h["a"])
    a[h["state"]] = a[h["state"]].copy()
    return dict(h, a=a)


def working(split, g, shards_by_cost, shard_blocks):
    """the contexts of a group of g that must receive a call, from items(h)"""
    if split[0] == "first":
        return [0]
    if split[0] == "even":
        return [i for i in range(g) if shard_blocks(split[1], g, i)[1] > shard_blocks(split[1], g, i)[0]]
    _, costs, rows = split
    return [i for i, (lo, hi) in enumerate(shards_by_cost(costs, g)) if (hi > lo if rows is None else sum(rows[lo:hi]) > 0)]


def even(key):
    return lambda h: ("even", h[key])


def check_blocks(env, h, outs):
    assert dec_blocks(env.client, outs[0]) == h["expect"]


# ---- block-sharded, in place ----------------------------------------------------------------------------------------------------------------
DIRECTIONS = {"encrypt": (False, aes_clear.aes_encrypt_block), "decrypt": (False, aes_clear.aes_decrypt_block),
              "decrypt_equivalent": (True, aes_clear.aes_decrypt_block)}


def cipher_case(direction, keyed, store=False):
    inverse, clear = DIRECTIONS[direction]

    def build(env, n):
        kob = KOB[:n] if keyed else [0] * n
        given = rand_blocks(0xB10C + 3 * keyed + len(direction), n)
        if direction != "encrypt":
            given = [aes_clear.aes_encrypt_block(KEYS[k], b) for k, b in zip(kob, given)]
        rk = sets(env, KEYS, inverse)
        rk = (env.store(rk) if store else rk) if keyed else rk[0]
        state = enc_blocks(env.client, given).reshape((n, 16, 8, env.p.big1))
        return {"a": [rk, kob, state] if keyed else [rk, state], "kw": {}, "state": 2 if keyed else 1, "n": n,
                "expect": [clear(KEYS[k], b) for k, b in zip(kob, given)]}

    name = "aes_%s%s" % (direction, "_keyed" * keyed)
    return Case(name + "_store" * store, name, build, even("n"), check_blocks, (4, 1, 0), 0)


def build_add_scalar(env, n):
    states = ([BASE, (1 << 64) - 0x10, MASK128 - 5, 0x0123456789ABCDEF_FFFFFFFFFFFFFF00] + rand_blocks(0xADD, 3))[:n]
    counters = [0x1234, 0x1FF, (1 << 64) + 0x25, 7, 0, MASK128, 0x100][:n]             # four different ones, one of them 0x1FF
    return {"a": [enc_blocks(env.client, states).reshape((n, 16, 8, env.p.big1)), counters], "kw": {}, "state": 0, "n": n,
            "expect": [(s + c) & MASK128 for s, c in zip(states, counters)]}


# ---- public blocks ---------------------------------------------------------------------------------------------------------------------------
def public_case(method, inverse, keyed):
    f = aes_clear.aes_decrypt_block if inverse else aes_clear.aes_encrypt_block

    def build(env, n):
        kob = KOB[:n] if keyed else [1] * n
        blocks = ([BASE, BASE, BASE + 1] + rand_blocks(0x9B + inverse, 4))[:n]         # equal blocks on both sides of a shard edge
        data = None if method == "aes_encrypt_public" else (F1_PT + rand_blocks(0xDA7A, 3))[:n]
        rk = sets(env, KEYS, inverse)
        return {"a": [rk, kob, blocks] if keyed else [rk[1], blocks], "kw": {} if data is None else {"data": data}, "state": None, "n": n,
                "expect": [f(KEYS[k], b) ^ (data[i] if data else 0) for i, (k, b) in enumerate(zip(kob, blocks))]}

    return Case(method, method, build, even("n"), check_blocks, (4, 1, 0), 0)


GCM_FIRST = 3


def build_gcm(env, n):
    data = (F1_PT + rand_blocks(0x6C, 3))[:n]
    ks = aes_clear.gcm_keystream(F1_KEY, GCM_IV, GCM_FIRST, n)
    return {"a": [sets(env)[1], GCM_IV], "kw": {"data": data, "first_block": GCM_FIRST}, "state": None, "n": n, "expect": [k ^ d for k, d in zip(ks, data)]}


CTR_IV = (F5_CTR & ~0xFFFFFFFF) | 0xFFFFFFFD        # the low 32 bits wrap at block 3: at 128 bits the carry goes up, at 32 bits it is dropped


def ctr_case(counter_bits):
    def build(env, n):
        data = (F1_PT + rand_blocks(0xC7, 3))[:n]
        ks = aes_clear.ctr_keystream(F1_KEY, CTR_IV, 0, n, counter_bits)
        return {"a": [sets(env)[1], CTR_IV, 0, n], "kw": {"data": data, "counter_bits": counter_bits}, "state": None, "n": n,
                "expect": [k ^ d for k, d in zip(ks, data)]}

    return Case("aes_ctr_%d" % counter_bits, "aes_ctr", build, even("n"), check_blocks, (4, 1, 0), 0)


# ---- chained -----------------------------------------------------------------------------------------------------------------------------------
def build_cbc(env, n):
    ct = cbc_encrypt(F1_KEY, IV, (F1_PT + rand_blocks(0xCBC, 3))[:n])
    return {"a": [sets(env, KEYS, True)[1], IV, ct], "kw": {}, "state": None, "n": n, "expect": aes_clear.cbc_decrypt(F1_KEY, IV, ct)}


def build_cfb(env, n):
    ct = cfb128_encrypt(F1_KEY, IV, (F1_PT + rand_blocks(0xCFB, 3))[:n])
    return {"a": [sets(env)[1], IV, ct], "kw": {}, "state": None, "n": n, "expect": aes_clear.cfb128_decrypt(F1_KEY, IV, ct)}


CBC_STREAM_BLOCKS = [1, 2, 1, 3, 1, 2, 1]            # three streams: 4 blocks; on 3 contexts one shard starts inside a stream, one on a stream's iv
CTR_STREAM_BLOCKS = [1, 3, 2, 1, 1, 2, 1]


def build_cbc_streams(env, n):
    streams, expect = [], []
    for s, k in enumerate(CBC_STREAM_BLOCKS[:n]):
        key, iv = s % 2, (IV + 0x1111 * s) & MASK128
        ct = cbc_encrypt(KEYS[key], iv, rand_blocks(0x57 + s, k))
        streams.append((key, iv, ct))
        expect += aes_clear.cbc_decrypt(KEYS[key], iv, ct)
    return {"a": [sets(env, KEYS, True), streams], "kw": {}, "state": None, "n": len(expect), "expect": expect}


def build_ctr_streams(env, n):
    streams = [(1 - s % 2, (CTR_IV + (s << 64)) & MASK128, s, k, None if s == 1 and n > 2 else rand_blocks(0xC5 + s, k)) for s, k in enumerate(CTR_STREAM_BLOCKS[:n])]
    return {"a": [sets(env), streams], "kw": {}, "state": None, "n": sum(CTR_STREAM_BLOCKS[:n]), "expect": aes_clear.ctr_streams(KEYS, streams)}


# ---- XTS: data units of 2 blocks, the call starts at block 1 of unit 0 -----------------------------------------------------------------------
XTS_SECTORS = [0x3333333333, 0xFE, 7, (1 << 64) - 1]                      # unrelated numbers; 4 blocks touch the first three
XTS_FIRST, XTS_UNIT = 1, 32


def build_xts(env, n):
    key1, key2 = xts.VECTORS[2][0], xts.VECTORS[2][1]
    pts = [bytes(range(16 * i, 16 * i + 16)) for i in range(n)]
    data = b"".join(aes_clear.xts_encrypt(key1, key2, XTS_SECTORS[(XTS_FIRST + i) // 2], pt, first_block=(XTS_FIRST + i) % 2) for i, pt in enumerate(pts))
    units = (XTS_FIRST + n + 1) // 2 if n else 0
    return {"a": [sets(env, (key1,), True)[0], sets(env, (key2,))[0], XTS_SECTORS[:units], data], "kw": {"unit_bytes": XTS_UNIT, "first_block": XTS_FIRST},
            "state": None, "n": n, "expect": [int.from_bytes(pt, "big") for pt in pts]}


# ---- key-sharded --------------------------------------------------------------------------------------------------------------------------------
MANY_KEYS = {128: KEYS + (F5[128][0][::-1],) + tuple(bytes(range(s, s + 16)) for s in (0x80, 0x21, 0x32, 0x43, 0x54)),      # MAX_N + 1 distinct keys
             256: (A3_KEY,) + tuple(bytes(range(s, s + 32)) for s in (0x40, 0x51, 0x62, 0x73, 0x84, 0x95))}


def expansion_case(bits):
    def build(env, n):
        keys = MANY_KEYS[bits][:n]
        return {"a": [np.stack([env.client.encrypt_aes_key(k) for k in keys])], "kw": {}, "state": None, "n": n, "clear": keys}

    def check(env, h, outs):
        dec = env.client.decrypt_bytes(outs[0]).reshape(h["n"], -1, 16)
        for j, k in enumerate(h["clear"]):
            assert [[int(b) for b in row] for row in dec[j]] == [list(r) for r in aes_clear.expand_key(k)]

    return Case("aes_key_expansion_many_%d" % bits, "aes_key_expansion_many", build, even("n"), check, (2, 1) if bits == 128 else (2,), 1)


def build_dec_round_keys_many(env, n):
    keys = MANY_KEYS[128][:n]
    return {"a": [sets(env, keys)], "kw": {}, "state": None, "n": n, "clear": keys}


def check_dec_round_keys(env, h, outs):
    dec = env.client.decrypt_bytes(outs[0]).reshape(len(h["clear"]), 11, 16)
    for j, k in enumerate(h["clear"]):
        assert [[int(b) for b in row] for row in dec[j]] == [list(r) for r in aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(k))]


# ---- cost-sharded --------------------------------------------------------------------------------------------------------------------------------
MAC_BLOCKS = [1, 1, 5, 1, 2, 3, 1]                    # the chains' lengths; the third has an encrypted addend
MAC_ENC_BYTES = [16, 5, 0, 16, 3]


def build_cbc_mac(env, n, with_init=False):
    streams, expect, costs = [], [], []
    starts = rand_blocks(0x1417, n) if with_init else [0] * n
    for s, k in enumerate(MAC_BLOCKS[:n]):
        blocks = rand_blocks(0x3AC0 + s, k)
        if s == 2:
            addend = rand_blocks(0x3AD0, k)
            parts = [int.from_bytes(a.to_bytes(16, "big")[:eb] + bytes(16 - eb), "big") for a, eb in zip(addend, MAC_ENC_BYTES)]
            streams.append((s % 2, blocks, enc_blocks(env.client, addend), MAC_ENC_BYTES))
            expect.append(aes_clear.cbc_mac(KEYS[s % 2], [b ^ x for b, x in zip(blocks, parts)], starts[s]))
        else:
            streams.append((s % 2, blocks))
            expect.append(aes_clear.cbc_mac(KEYS[s % 2], blocks, starts[s]))
        costs.append(k + 1)
    kw = {"init": enc_blocks(env.client, starts).reshape((n, 16, 8, env.p.big1))} if with_init else {}
    return {"a": [sets(env), streams], "kw": kw, "state": None, "costs": costs, "expect": expect}


def cost_items(h):
    return ("cost", h["costs"], None)


CCM_KEYS = (ccm.VECTORS["ex1"][0], F1_KEY)
CCM_FORGED = 3


def ccm_messages(n):
    """message 0: SP 800-38C example 1 (4 payload bytes); 1: no payload at all; 2: two payload blocks, the last of 5 bytes; 3: one whole
    block and a forged tag; then more of the same kinds"""
    own = lambda k, nonce, aad, size, t: (ccm.own_message(k, CCM_KEYS[k], bytes(range(nonce, nonce + 12)), aad, bytes(range(0x50, 0x50 + size)), t), bytes(range(0x50, 0x50 + size)))
    made = [(ccm.message(0, "ex1"), ccm.VECTORS["ex1"][3]), own(1, 0x10, b"", 0, 8), own(0, 0x20, b"hdr", 21, 6), own(1, 0x30, b"", 16, 8),
            own(0, 0x40, b"", 0, 4), own(1, 0x50, b"twelve bytes", 17, 16), own(0, 0x60, b"", 1, 10)][:n]
    messages, payloads = [m for m, _ in made], [p for _, p in made]
    if n > CCM_FORGED:
        m = messages[CCM_FORGED]
        messages[CCM_FORGED] = m[:4] + (bytes([m[4][0] ^ 0x10]) + m[4][1:],)
    return messages, payloads


def ccm_case(gate):
    def build(env, n):
        messages, payloads = ccm_messages(n)
        valid = [int(i != CCM_FORGED) for i in range(n)]
        blocks = [(len(p) + 15) // 16 for p in payloads]
        for i, (k, nonce, aad, ct, tag) in enumerate(messages):
            clear = aes_clear.ccm_decrypt(CCM_KEYS[k], nonce, aad, ct + tag, len(tag))
            assert (clear == payloads[i]) if valid[i] else clear is None
        # chained plus public blocks, restated: the AAD blocks, two passes a payload block (counter and chain), B0 and the tag's S0
        costs = [(len(aes_clear.ccm_blocks(m[1], m[2], len(m[3]), len(m[4]))[1])) + 2 * b + 2 for m, b in zip(messages, blocks)]
        return {"a": [sets(env, CCM_KEYS), messages], "kw": {"gate": gate}, "state": None, "costs": costs, "payloads": payloads, "valid": valid, "blocks": blocks}

    def check(env, h, outs):
        pt, valid, at = outs
        assert [int(b) for b in env.client.decrypt_bits(valid)] == h["valid"]
        assert [int(x) for x in at] == [sum(h["blocks"][:i]) for i in range(len(h["blocks"]) + 1)]
        dec = bytes(int(b) for b in env.client.decrypt_bytes(pt).reshape(-1))
        for i, payload in enumerate(h["payloads"]):
            shown = bytes(len(payload)) if gate and not h["valid"][i] else payload
            assert dec[16 * int(at[i]):16 * int(at[i + 1])] == shown + bytes(-len(shown) % 16)

    return Case("aes_ccm_decrypt" + "_gate" * gate, "aes_ccm_decrypt", build, cost_items, check, (4, 1), 0)


CMAC_KEYS = (cmac.VECTORS[128][0], FIPS_C[128][0])
CMAC_BYTES = [0, 16, 17, 80, 40, 1, 32]
CMAC_FORGED = 2


def cmac_case(verify, subkeys, store=False, sizes_of=None, name=None):
    sizes_of = sizes_of or CMAC_BYTES

    def build(env, n):
        msgs = [(s % 2, bytes(range(s, s + k))) for s, k in enumerate(sizes_of[:n])]
        tags = [aes_clear.cmac(CMAC_KEYS[k], m) for k, m in msgs]
        rk = sets(env, CMAC_KEYS)
        h = {"a": [env.store(rk) if store else rk, msgs], "kw": {}, "state": None, "costs": [max(1, (len(m) + 15) // 16) for _, m in msgs]}
        if subkeys:
            h["kw"]["subkeys"] = np.stack([enc_blocks(env.client, list(aes_clear.cmac_subkeys(k))) for k in CMAC_KEYS])
        if verify:
            sent = [t[:8 + 4 * (s % 3)] for s, t in enumerate(tags)]
            if n > CMAC_FORGED:
                sent[CMAC_FORGED] = sent[CMAC_FORGED][:-1] + bytes([sent[CMAC_FORGED][-1] ^ 0x80])
            h["a"][1] = [m + (t,) for m, t in zip(msgs, sent)]
            h["valid"] = [int(s != CMAC_FORGED) for s in range(n)]
        else:
            h["expect"] = [int.from_bytes(t, "big") for t in tags]
        return h

    def check_valid(env, h, outs):
        assert [int(b) for b in env.client.decrypt_bits(outs[0])] == h["valid"]

    method = "aes_cmac_verify" if verify else "aes_cmac_streams"
    return Case(name or method + "_subkeys" * subkeys + "_store" * store, method, build, cost_items, check_valid if verify else check_blocks, (4, 1, 0) if not name else (2,), 0)


# ---- key unwrap: AES-128 keys under 2 KEKs, one blob tampered -----------------------------------------------------------------------------------
KEKS = (keywrap.vector("4.1")[0], F1_KEY)
KW_TAMPERED = 2


def unwrap_case(packed, gate):
    def build(env, n):
        payloads = ([keywrap.vector("4.1")[1], bytes(range(0xA0, 0xB0)), bytes(range(0x10, 0x20)), F5[128][0]] + [bytes(range(s, s + 16)) for s in (0x60, 0x70, 0x33)])[:n]
        kek_of_key = [0, 1, 1, 0, 1, 0, 0][:n]
        wrapped = [aes_clear.key_wrap(KEKS[k], p) for k, p in zip(kek_of_key, payloads)]
        if n:
            assert wrapped[0] == keywrap.vector("4.1")[2]                               # RFC 3394 4.1
        if n > KW_TAMPERED:
            w = wrapped[KW_TAMPERED]
            wrapped[KW_TAMPERED] = w[:9] + bytes([w[9] ^ 0x04]) + w[10:]
        clear = [aes_clear.key_unwrap(KEKS[k], w) for k, w in zip(kek_of_key, wrapped)]
        shown = [bytes(16) if gate and not ok else data for ok, data in clear]
        assert [ok for ok, _ in clear] == [i != KW_TAMPERED for i in range(n)]
        return {"a": [sets(env, KEKS, True), wrapped, kek_of_key], "kw": dict({"gate": gate}, **({"chunk": 1} if packed else {})), "state": None, "n": n,
                "valid": [int(ok) for ok, _ in clear], "payloads": shown}

    def check(env, h, outs):
        keys, valid = outs
        n = h["n"]
        assert [int(b) for b in env.client.decrypt_bits(valid)] == h["valid"]
        if packed:
            for j, payload in enumerate(h["payloads"]):
                got = env.client.decrypt_packed_bytes(keys.reshape(n, key_glwes(env.p, 128), -1)[j], 11 * 16)
                assert [int(b) for b in got] == [b for r in aes_clear.expand_key(payload) for b in r]
        else:
            assert [bytes(int(b) for b in row) for row in env.client.decrypt_bytes(keys.reshape(n, 16, 8, env.p.big1))] == h["payloads"]

    return Case("aes_key_unwrap" + "_packed" * packed + "_gate" * gate, "aes_key_unwrap" + "_packed" * packed, build, even("n"), check, (4, 1), 1 if packed else 0)


# ---- gates ---------------------------------------------------------------------------------------------------------------------------------------
GATE_RUNS = [0, 3, 1, 2, 0, 1, 2]
GATE_BITS = [1, 0, 1, 1, 0, 1, 0]


def gate_case(packed, runs_given):
    def build(env, n):
        runs = GATE_RUNS[:n] if runs_given else [2] * n
        gates = GATE_BITS[:n]
        p = env.p
        rows = sum(runs)
        if packed:
            m = max(0, rows * p.N - (p.N - 1))                                          # whole GLWEs, the last one holding one bit
            bits = np.random.default_rng(0x6A7E + n).integers(0, 2, m).astype(np.uint8)
            ct = env.packed(env.client.encrypt_bits(bits).reshape(m, p.big1))
            of_bit = [g for g, r in zip(gates, runs) for _ in range(r * p.N)][:m]
        else:
            bits = np.random.default_rng(0x6A7F + n).integers(0, 2, rows).astype(np.uint8)
            bits[:1] = 1
            ct = env.client.encrypt_bits(bits).reshape(rows, p.big1)
            of_bit = [g for g, r in zip(gates, runs) for _ in range(r)]
        valid = env.client.encrypt_bits(np.array(gates, dtype=np.uint8)).reshape(n, p.big1)
        return {"a": [ct, valid, runs if runs_given else None], "kw": {}, "state": None, "costs": [r + 1 for r in runs], "rows": runs,
                "expect": [int(b) * g for b, g in zip(bits, of_bit)]}

    def check(env, h, outs):
        got = env.client.decrypt_packed(outs[0], len(h["expect"])) if packed else env.client.decrypt_bits(outs[0])
        assert [int(b) for b in got] == h["expect"]

    name = "gate" + "_packed" * packed
    return Case(name + ("_runs" if runs_given else "_equal"), name, build, lambda h: ("cost", h["costs"], h["rows"]), check, (3,), 0 if runs_given else 1)


# ---- packing and wire formats ------------------------------------------------------------------------------------------------------------------
def pack_bits(env, n, seed):
    """n GLWEs: n - 1 full ones and one bit (n = 3: 2 N + 1 bits; n = 1: one bit)"""
    m = (n - 1) * env.p.N + 1 if n else 0
    bits = np.random.default_rng(seed + n).integers(0, 2, m).astype(np.uint8)
    bits[-1:] = 1
    return bits, env.client.encrypt_bits(bits).reshape(m, env.p.big1)


def pack_case(width, unpack):
    def build(env, n):
        bits, ct = pack_bits(env, n, 0x9AC0 + width)
        a = [env.packed(ct, width), len(bits)] if unpack else [ct]
        return {"a": a, "kw": {"width": width}, "state": None, "n": n, "expect": [int(b) for b in bits]}

    def check(env, h, outs):
        got = env.client.decrypt_bits(outs[0]) if unpack else env.client.decrypt_packed(outs[0], len(h["expect"]), width=width)
        assert [int(b) for b in got] == h["expect"]

    name = "unpack" if unpack else "pack"
    return Case("%s_%d" % (name, width), name, build, even("n"), check, (3, 1), 0)


EXPAND_FIRST = (1 << 32) - 2                             # the index carries into the high nonce word inside the call


def build_expand(env, n):
    bits = np.array([1, 0, 1, 1, 0, 0, 1][:n], dtype=np.uint8)
    s = env.client.encrypt_bits_seeded(bits, first_index=EXPAND_FIRST)
    return {"a": [s], "kw": {}, "state": None, "n": n, "expect": [int(b) for b in bits]}


def check_expand(env, h, outs):
    assert np.array_equal(outs[0], h["a"][0].expand())                                  # the numpy twin of the kernel
    assert [int(b) for b in env.client.decrypt_bits(outs[0])] == h["expect"]


# ---- the calls of context 0 ---------------------------------------------------------------------------------------------------------------------
def first(h):
    return ("first",)


def round_key_bytes(keys, inverse=False):
    out = []
    for k in keys:
        e = aes_clear.expand_key(k)
        out.append([b for r in (aes_clear.inv_mix_columns_round_keys(e) if inverse else e) for b in r])
    return out


def build_pack_round_keys(env, n):
    keys = MANY_KEYS[128][:n]
    return {"a": [sets(env, keys)], "kw": {}, "state": None, "n": n, "expect": round_key_bytes(keys)}


def check_packed_keys(env, h, outs):
    n = len(h["expect"])
    for j, want in enumerate(h["expect"]):
        assert [int(b) for b in env.client.decrypt_packed_bytes(outs[0].reshape(n, key_glwes(env.p, 128), -1)[j], 11 * 16)] == want


def build_unpack_round_keys(env, n):
    keys = MANY_KEYS[128][:n + 1]                        # n of the n + 1 keys of the store, from key 1
    return {"a": [env.store(sets(env, keys))], "kw": {"first": 1, "count": n}, "state": None, "n": n, "expect": round_key_bytes(keys[1:])}


def check_lwe_keys(env, h, outs):
    n = len(h["expect"])
    dec = env.client.decrypt_bytes(outs[0].reshape(n, -1, 8, env.p.big1))
    assert [[int(b) for b in row] for row in dec] == h["expect"]


def build_expansion_packed(env, n):
    keys = MANY_KEYS[128][:n]
    return {"a": [np.stack([env.client.encrypt_aes_key(k) for k in keys])], "kw": {"chunk": 1}, "state": None, "n": n, "expect": round_key_bytes(keys)}


def build_expansion(env, n):
    return {"a": [env.client.encrypt_aes_key(KEYS[1])], "kw": {}, "state": None, "n": 1, "expect": round_key_bytes(KEYS[1:])}


def build_dec_round_keys(env, n):
    return {"a": [sets(env)[1]], "kw": {}, "state": None, "n": 1, "expect": round_key_bytes(KEYS[1:], True)}


def build_cmac_subkeys(env, n):
    keys = (CMAC_KEYS * 4)[:n]
    return {"a": [sets(env, keys)], "kw": {}, "state": None, "n": n, "expect": [x for k in keys for x in aes_clear.cmac_subkeys(k)]}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
# split on 3 and on 5 contexts of the first size (DESIGN.md section 5 has the same column):
CASES = [
    # block-sharded, in place: 4 blocks = 2 + 1 + 1 | 1 + 1 + 1 + 1 + 0; 1 block = 1 + 0 + 0; 0 blocks: no context works
    cipher_case("encrypt", False), cipher_case("decrypt", False), cipher_case("decrypt_equivalent", False),
    Case("add_scalar", "add_scalar", build_add_scalar, even("n"), check_blocks, (4, 1, 0), 0),
    cipher_case("encrypt", True), cipher_case("decrypt", True), cipher_case("decrypt_equivalent", True),
    cipher_case("encrypt", True, store=True),                                           # a PackedRoundKeys in place of round keys, block-sharded
    # public blocks: the same splits
    public_case("aes_encrypt_public", False, False), public_case("aes_decrypt_public", True, False),
    public_case("aes_encrypt_public_keyed", False, True), public_case("aes_decrypt_public_keyed", True, True),
    Case("aes_gcm_ctr", "aes_gcm_ctr", build_gcm, even("n"), check_blocks, (4, 1, 0), 0),
    ctr_case(128), ctr_case(32),                                                        # the wrap at block 3: shard 2 of 3, shard 3 of 5
    # chained: 4 blocks; 3 streams of 1, 2, 1 blocks: shards [s0 s1a | s1b | s2] and [s0 | s1a | s1b | s2 | -]; 2 streams of 1 and 3 blocks
    Case("aes_cbc_decrypt", "aes_cbc_decrypt", build_cbc, even("n"), check_blocks, (4, 1, 0), 0),
    Case("aes_cfb_decrypt", "aes_cfb_decrypt", build_cfb, even("n"), check_blocks, (4, 1, 0), 0),
    Case("aes_cbc_streams", "aes_cbc_streams", build_cbc_streams, even("n"), check_blocks, (3, 0), 0),
    Case("aes_ctr_streams", "aes_ctr_streams", build_ctr_streams, even("n"), check_blocks, (2, 0), 0),
    # XTS: global blocks 1..4 = [u0.1 u1.0 | u1.1 | u2.0] and [u0.1 | u1.0 | u1.1 | u2.0 | -]
    Case("aes_xts_decrypt", "aes_xts_decrypt", build_xts, even("n"), check_blocks, (4, 1, 0), 0),
    # key-sharded: 2 keys = 1 + 1 + 0 | 1 + 1 + 0 + 0 + 0
    expansion_case(128), expansion_case(256),
    Case("aes_decryption_round_keys_many", "aes_decryption_round_keys_many", build_dec_round_keys_many, even("n"), check_dec_round_keys, (2, 1), 1),
    # cost-sharded.  chains of 1, 1, 5, 1 blocks (costs 2, 2, 6, 2): [c0 c1 | c2 | c3] and [c0 | c1 | c2 | - | c3]
    Case("aes_cbc_mac_streams", "aes_cbc_mac_streams", build_cbc_mac, cost_items, check_blocks, (4, 1, 0), 0),
    Case("aes_cbc_mac_streams_init", "aes_cbc_mac_streams", lambda env, n: build_cbc_mac(env, n, True), cost_items, check_blocks, (2,), 0),
    # CCM, costs 5, 2, 7, 4: [m0 | m1 m2 | m3] and [m0 | m1 | m2 | - | m3]: on 5 contexts the message without payload is alone, its output slice empty
    ccm_case(False), ccm_case(True),
    # CMAC of 0, 16, 17, 80 bytes (costs 1, 1, 2, 5): [m0 m1 | m2 | m3] and [m0 m1 | m2 | - | m3 | -]
    cmac_case(False, False), cmac_case(False, True), cmac_case(True, False), cmac_case(True, True),
    cmac_case(False, False, store=True),                                                # a PackedRoundKeys, cost-sharded
    # costs [3, 1]: [- | m0 | m1] -- context 0 idles; [- | m0 | - | - | m1]
    cmac_case(False, False, sizes_of=[48, 16], name="aes_cmac_streams_first_context_idle"),
    # key unwrap: 4 keys = 2 + 1 + 1 | 1 + 1 + 1 + 1 + 0; a single key = 1 + 0 + 0
    unwrap_case(False, False), unwrap_case(False, True), unwrap_case(True, False), unwrap_case(True, True),
    # gates with runs 0, 3, 1 (costs 1, 4, 2): [g0 | g1 | g2] and [g0 | - | g1 | - | g2], the context of g0 having no row to gate; 3 equal runs of 2
    gate_case(False, True), gate_case(False, False), gate_case(True, True), gate_case(True, False),
    # packing: 3 GLWEs (2 N + 1 bits) = 1 + 1 + 1 | 1 + 1 + 1 + 0 + 0, the last GLWE ragged and alone; 1 bit; 5 seeded ciphertexts = 2 + 2 + 1 | 1 each
    pack_case(64, False), pack_case(16, False), pack_case(64, True), pack_case(16, True),
    Case("expand", "expand", build_expand, even("n"), check_expand, (5, 0), 0),
    # context 0 alone; finished when the call returns
    Case("pack_round_keys", "pack_round_keys", build_pack_round_keys, first, check_packed_keys, (2,), 1),
    Case("unpack_round_keys", "unpack_round_keys", build_unpack_round_keys, first, check_lwe_keys, (2,), 1),
    Case("aes_key_expansion_packed", "aes_key_expansion_packed", build_expansion_packed, first, check_packed_keys, (2,), 1),
    Case("aes_key_expansion", "aes_key_expansion", build_expansion, first, check_lwe_keys, (1,), 1),
    Case("aes_decryption_round_keys", "aes_decryption_round_keys", build_dec_round_keys, first, check_lwe_keys, (1,), 1),
    Case("aes_cmac_subkeys", "aes_cmac_subkeys", build_cmac_subkeys, first, check_blocks, (2,), 1),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
IN_PLACE_BLOCKS = ("aes_encrypt", "aes_decrypt", "aes_decrypt_equivalent", "add_scalar", "aes_encrypt_keyed", "aes_decrypt_keyed", "aes_decrypt_equivalent_keyed")
RUNS = [(c, n) for c in CASES for n in c.sizes]          # what the GPU module runs


def run_id(run):
    return "%s-%d" % (run[0].name, run[1])
