"""ServerGroup's split arithmetic without a GPU: the two shard functions by their properties, every case of group_splits.CASES on an echo
model of Server for g = 1..6 contexts and n = 0..7 items, and what an exception in one shard leaves behind.

The echo model is a Server that never creates an engine: every computing method writes, per item of its output, one 64-bit tag hashed
from everything the real call's item depends on, in GLOBAL terms -- the counter block first_block + i, the chaining block, the data unit's
sector and the offset in it, the key's own words, the index first_index + i.  A ServerGroup around g such models must write what ONE
model writes on the whole input.  Both sides run the same model, so a mistake in the model cancels; a wrong slice, offset or chaining
block does not."""
import dataclasses
import hashlib
import inspect
import itertools
import json
import re
import threading
from pathlib import Path

import numpy as np
import pytest

import group_splits as gs
from tfhe_aes_amd import PARAM_TOY
from tfhe_aes_amd.client import PackedRoundKeys
from tfhe_aes_amd.dist import shard_blocks
from tfhe_aes_amd.server import Server, ServerGroup, _shards_by_cost, ccm_args, xts_args

# the shapes are all that matters here: polynomials of 8 coefficients make a block 128 x 9 words and a GLWE 8 bits
TINY = dataclasses.replace(PARAM_TOY, name="PARAM_ECHO", polynomial_size=8)
GROUPS = range(1, 7)


# ---- the shard functions ------------------------------------------------------------------------------------------------------------------
def tiles(shards, n):
    """contiguous, disjoint, in order, and covering [0, n)"""
    return shards[0][0] == 0 and shards[-1][1] == n and all(lo <= hi for lo, hi in shards) and all(a[1] == b[0] for a, b in zip(shards, shards[1:]))


@pytest.mark.parametrize("g", GROUPS)
def test_shard_blocks_tiles_the_range_in_shares_that_differ_by_at_most_one(g):
    for n in range(13):
        shards = [shard_blocks(n, g, i) for i in range(g)]
        assert tiles(shards, n), (n, g, shards)
        sizes = [hi - lo for lo, hi in shards]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True), (n, g, sizes)
    for bad in ((4, 0, 0), (4, g, g), (4, g, -1), (-1, g, 0)):
        with pytest.raises(ValueError):
            shard_blocks(*bad)


def cost_lists():
    for k in range(7):
        yield from itertools.product((0, 1, 2, 5, 40), repeat=k)
    rng = np.random.default_rng(0x5A4D)
    for _ in range(2000):
        yield tuple(int(c) for c in rng.integers(0, 41, int(rng.integers(7, 40))))


def test_shards_by_cost_tile_the_streams_and_no_shard_exceeds_its_share_by_more_than_one_stream():
    """a stream goes to the context in whose g-th of the total its midpoint lies: the midpoints of a shard's first and last stream are
    less than total / g apart, and the half streams beyond them add at most max(costs)"""
    for costs in cost_lists():
        costs = list(costs)
        total = sum(costs)
        for g in GROUPS:
            shards = _shards_by_cost(costs, g)
            assert len(shards) == g and tiles(shards, len(costs)), (costs, g, shards)
            if total == 0:
                assert shards[0] == (0, len(costs)) and all(lo == hi for lo, hi in shards[1:]), (costs, g, shards)
            else:
                assert all(sum(costs[lo:hi]) * g <= total + max(costs) * g for lo, hi in shards), (costs, g, shards)


def test_shards_by_cost_can_leave_the_first_context_idle():
    assert _shards_by_cost([3, 1], 3) == [(0, 0), (0, 1), (1, 2)]
    assert gs.working(("cost", [3, 1], None), 3, _shards_by_cost, shard_blocks) == [1, 2]


# ---- the echo model --------------------------------------------------------------------------------------------------------------------------
def tag(*parts):
    return np.uint64(int.from_bytes(hashlib.blake2b(repr(parts).encode(), digest_size=8).digest(), "little"))


def dig(a):
    """an array of words as a hashable value"""
    return None if a is None else hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).hexdigest()


def u128(v):
    return int.from_bytes(v, "big") if isinstance(v, (bytes, bytearray)) else int(v)


def blocks_of(data):
    if isinstance(data, (bytes, bytearray)):
        return [bytes(data[i:i + 16]) for i in range(0, len(data), 16)]
    return list(data)


class Echo(Server):
    """see the module's docstring.  calls: the methods the group called on this context; clean: synchronised since the last of them"""

    def __init__(self, params, fail=None):
        self.params, self._inflight, self.engine = params, [], None
        self.calls, self.clean, self.syncs, self.fail = [], True, 0, fail

    def synchronize(self):
        self.clean, self.syncs = True, self.syncs + 1

    def _called(self, name):
        self.calls.append(name)
        self.clean = False
        if self.fail is not None and name == self.fail[0]:
            raise self.fail[1]

    def _key(self, rk, index=None):
        """the words of one key of a round-key argument: what a cipher call on that key depends on"""
        words = rk.data if isinstance(rk, PackedRoundKeys) else rk
        return dig(words if index is None else words[index])

    def _one_of(self, rk):
        """a single-key call: the one key of a store, or the array itself"""
        return self._key(rk, 0) if isinstance(rk, PackedRoundKeys) else self._key(rk)

    def _stream_key(self, rk, index):
        """many=None: one key's [Nr+1][16][8][kN+1] read as a set of one"""
        if not isinstance(rk, PackedRoundKeys) and rk.ndim == 4:
            return self._key(rk)
        return self._key(rk, index)

    def _out(self, out, *shape):
        return np.zeros(shape + (self.params.big1,), dtype=np.uint64) if out is None else out

    # in place, per block
    def _cipher(self, name, rk, state):
        self._called(name)
        for i in range(len(state)):
            state[i] = tag(name, self._one_of(rk), dig(state[i]))
        return state

    def aes_encrypt(self, rk, state):
        return self._cipher("aes_encrypt", rk, state)

    def aes_decrypt(self, rk, state):
        return self._cipher("aes_decrypt", rk, state)

    def aes_decrypt_equivalent(self, rk, state):
        return self._cipher("aes_decrypt_equivalent", rk, state)

    def add_scalar(self, state, i):
        self._called("add_scalar")
        counters = [i] * len(state) if isinstance(i, int) else list(i)
        assert len(counters) == len(state)
        for b in range(len(state)):
            state[b] = tag("add_scalar", dig(state[b]), counters[b])
        return state

    def _cipher_keyed(self, name, rk, key_of_block, state):
        self._called(name)
        key_of_block = list(key_of_block)
        assert len(key_of_block) == len(state)
        for i in range(len(state)):
            state[i] = tag(name, self._key(rk, key_of_block[i]), dig(state[i]))
        return state

    def aes_encrypt_keyed(self, rk, key_of_block, state):
        return self._cipher_keyed("aes_encrypt_keyed", rk, key_of_block, state)

    def aes_decrypt_keyed(self, rk, key_of_block, state):
        return self._cipher_keyed("aes_decrypt_keyed", rk, key_of_block, state)

    def aes_decrypt_equivalent_keyed(self, rk, key_of_block, state):
        return self._cipher_keyed("aes_decrypt_equivalent_keyed", rk, key_of_block, state)

    # public blocks
    def _public(self, name, key_of, blocks, data, out):
        """block i: (the key's words, the public block, the clear data folded in)"""
        self._called(name)
        blocks = list(blocks)
        data = [None] * len(blocks) if data is None else blocks_of(data)
        assert len(data) == len(blocks)
        out = self._out(out, len(blocks), 16, 8)
        assert len(out) == len(blocks)
        for i, b in enumerate(blocks):
            out[i] = tag("public", name.startswith("aes_decrypt") or name == "aes_cbc", key_of(i), u128(b), None if data[i] is None else u128(data[i]))
        return out

    def aes_encrypt_public(self, rk, blocks, out=None):
        return self._public("aes_encrypt_public", lambda i: self._one_of(rk), blocks, None, out)

    def aes_decrypt_public(self, rk, blocks, data=None, out=None):
        return self._public("aes_decrypt_public", lambda i: self._one_of(rk), blocks, data, out)

    def _public_keyed(self, k, key_of_block, blocks, data, out, inverse=False):
        """where both keyed public calls end; the group reaches it through Server's own methods, which it calls unbound"""
        kob = list(key_of_block)
        assert len(kob) == len(list(blocks))
        return self._public("aes_decrypt_public_keyed" if inverse else "aes_encrypt_public_keyed", lambda i: dig(k.words[kob[i]]), blocks, data, out)

    def aes_encrypt_public_keyed(self, rk, key_of_block, blocks, data=None, out=None):
        return self._public_keyed(self._round_keys(rk, many=True), key_of_block, blocks, data, out)

    def aes_decrypt_public_keyed(self, rk, key_of_block, blocks, data=None, out=None):
        return self._public_keyed(self._round_keys(rk, "decryption round keys", many=True), key_of_block, blocks, data, out, inverse=True)

    def aes_ctr(self, rk, iv, first_block, n_blocks, data=None, out=None, counter_bits=128):
        self._called("aes_ctr")
        data = [None] * n_blocks if data is None else blocks_of(data)
        out = self._out(out, n_blocks, 16, 8)
        assert len(out) == n_blocks == len(data)
        for i in range(n_blocks):
            out[i] = tag("aes_ctr", self._one_of(rk), u128(iv), int(first_block) + i, None if data[i] is None else u128(data[i]), counter_bits)
        return out

    def aes_gcm_ctr(self, rk, iv, data=None, n_blocks=None, first_block=0, out=None):
        self._called("aes_gcm_ctr")
        data = None if data is None else blocks_of(data)
        n_blocks = len(data) if n_blocks is None else int(n_blocks)
        out = self._out(out, n_blocks, 16, 8)
        assert len(out) == n_blocks and (data is None or len(data) == n_blocks)
        for i in range(n_blocks):
            out[i] = tag("aes_gcm_ctr", self._one_of(rk), bytes(iv), int(first_block) + i, None if data is None else u128(data[i]))
        return out

    # chained: block i of a stream depends on its key, itself and the block before it (the stream's iv for its first)
    def _chained(self, name, rk, iv, ciphertext, out):
        self._called(name)
        ct = blocks_of(ciphertext)
        out = self._out(out, len(ct), 16, 8)
        assert len(out) == len(ct)
        for i, c in enumerate(ct):
            out[i] = tag(name, self._one_of(rk), u128(ct[i - 1] if i else iv), u128(c))
        return out

    def aes_cbc_decrypt(self, rk, iv, ciphertext, out=None):
        return self._chained("aes_cbc_decrypt", rk, iv, ciphertext, out)

    def aes_cfb_decrypt(self, rk, iv, ciphertext, out=None):
        return self._chained("aes_cfb_decrypt", rk, iv, ciphertext, out)

    def aes_cbc_streams(self, rk, streams, out=None):
        """the tags of aes_decrypt_public_keyed on (block, chaining block), the chain built here stream by stream"""
        kob, blocks, chain = [], [], []
        for key_index, iv, ciphertext in streams:
            ct = blocks_of(ciphertext)
            for j, c in enumerate(ct):
                kob.append(key_index); blocks.append(c); chain.append(ct[j - 1] if j else iv)
        return self._public("aes_decrypt_public_keyed", lambda i: self._key(rk, kob[i]), blocks, chain if blocks else None, out)

    def aes_ctr_streams(self, rk, streams, out=None, counter_bits=128):
        """the tags of aes_encrypt_public_keyed on (counter block, data), the counters built here stream by stream"""
        kob, blocks, data = [], [], []
        m = 1 << counter_bits
        any_data = any(st[4] is not None for st in streams)
        for key_index, iv, first_block, n_blocks, d in streams:
            iv, d = u128(iv), [0] * n_blocks if d is None else blocks_of(d)
            for i in range(n_blocks):
                kob.append(key_index); blocks.append((iv & ~(m - 1)) | ((iv + first_block + i) & (m - 1))); data.append(d[i])
        return self._public("aes_encrypt_public_keyed", lambda i: self._key(rk, kob[i]), blocks, data if any_data else None, out)

    def aes_xts_decrypt(self, rk1, rk2, sectors, ciphertext, unit_bytes=512, first_block=0, out=None):
        self._called("aes_xts_decrypt")
        sectors, bpu, ct = xts_args(sectors, ciphertext, unit_bytes, first_block)
        out = self._out(out, len(ct), 16, 8)
        assert len(out) == len(ct)
        for i, c in enumerate(ct):
            b = int(first_block) + i
            out[i] = tag("aes_xts_decrypt", self._one_of(rk1), self._one_of(rk2), sectors[b // bpu], b % bpu, u128(c))
        return out

    # per key
    def _per_key(self, name, arr, out, *shape):
        self._called(name)
        out = self._out(out, len(arr), *shape)
        assert len(out) == len(arr)
        for i in range(len(arr)):
            out[i] = tag(name, dig(arr[i]))
        return out

    def aes_key_expansion_many(self, keys, out=None):
        return self._per_key("aes_key_expansion_many", keys, out, int(keys.shape[1]) // 4 + 7, 16, 8)

    def aes_decryption_round_keys_many(self, rk, out=None):
        return self._per_key("aes_decryption_round_keys_many", rk, out, int(rk.shape[1]), 16, 8)

    def aes_key_expansion(self, key):
        self._called("aes_key_expansion")
        out = self._out(None, int(key.shape[0]) // 4 + 7, 16, 8)
        out[...] = tag("aes_key_expansion", dig(key))
        return out

    def aes_decryption_round_keys(self, rk):
        self._called("aes_decryption_round_keys")
        out = self._out(None, *rk.shape[:-1])
        out[...] = tag("aes_decryption_round_keys", dig(rk))
        return out

    # whole streams, messages and wrapped keys
    def aes_cbc_mac_streams(self, rk, streams, init=None, out=None):
        self._called("aes_cbc_mac_streams")
        out = self._out(out, len(streams), 16, 8)
        assert len(out) == len(streams) and (init is None or len(init) == len(streams))
        for i, st in enumerate(streams):
            st = tuple(st) + (None, None) * (len(st) == 2)
            out[i] = tag("aes_cbc_mac_streams", self._stream_key(rk, st[0]), [u128(b) for b in blocks_of(st[1])], dig(st[2]), st[3], None if init is None else dig(init[i]))
        return out

    def aes_ccm_decrypt(self, rk, messages, out=None, valid_out=None, gate=False):
        self._called("aes_ccm_decrypt")
        at = ccm_args(messages)["block_of_message"]
        out, valid_out = self._out(out, at[-1], 16, 8), self._out(valid_out, len(messages))
        assert len(out) == at[-1] and len(valid_out) == len(messages)
        for i, m in enumerate(messages):
            valid_out[i] = tag("ccm valid", self._stream_key(rk, m[0]), tuple(m))
            for row in range(at[i], at[i + 1]):
                out[row] = tag("aes_ccm_decrypt", self._stream_key(rk, m[0]), tuple(m), row - at[i], gate)
        return out, valid_out, at

    def aes_cmac_subkeys(self, rk, out=None):
        return self._per_key("aes_cmac_subkeys", rk if rk.ndim == 5 else rk[None], out, 2, 16, 8)

    def _cmac_tags(self, name, rk, entries, subkeys, out, *shape):
        self._called(name)
        out = self._out(out, len(entries), *shape)
        assert len(out) == len(entries)
        for i, e in enumerate(entries):
            out[i] = tag(name, self._stream_key(rk, e[0]), tuple(e), None if subkeys is None else dig(subkeys[e[0]]))
        return out

    def aes_cmac_streams(self, rk, streams, subkeys=None, out=None):
        return self._cmac_tags("aes_cmac_streams", rk, streams, subkeys, out, 16, 8)

    def aes_cmac_verify(self, rk, messages, subkeys=None, valid_out=None):
        return self._cmac_tags("aes_cmac_verify", rk, messages, subkeys, valid_out)

    def aes_key_unwrap(self, rk, wrapped, kek_of_key=None, out=None, valid_out=None, gate=False):
        self._called("aes_key_unwrap")
        wrapped = [bytes(w) for w in wrapped]
        semiblocks = len(wrapped[0]) // 8 - 1 if wrapped else 2
        out, valid_out = self._out(out, len(wrapped), 8 * semiblocks, 8), self._out(valid_out, len(wrapped))
        assert len(out) == len(valid_out) == len(wrapped) and (kek_of_key is None or len(kek_of_key) == len(wrapped))
        for i, w in enumerate(wrapped):
            kek = self._stream_key(rk, 0 if kek_of_key is None else kek_of_key[i])
            out[i], valid_out[i] = tag("aes_key_unwrap", kek, w, gate), tag("unwrap valid", kek, w)
        return out, valid_out

    def aes_key_unwrap_packed(self, rk, wrapped, kek_of_key=None, chunk=256, gate=False):
        p = self.params
        keys, valid = self.aes_key_unwrap(rk, wrapped, kek_of_key, gate=gate)
        data = np.zeros((len(keys), gs.packed_key_glwes(p, 128), (p.k + 1) * p.N), dtype=np.uint64)
        for i in range(len(keys)):
            data[i] = tag("expanded and packed", int(keys[i, 0, 0, 0]), chunk)
        return PackedRoundKeys(p, 128, data), valid

    # round-key stores
    def pack_round_keys(self, rk, out=None):
        self._called("pack_round_keys")
        p, rk = self.params, rk if rk.ndim == 5 else rk[None]
        data = np.zeros((len(rk), gs.packed_key_glwes(p, 128), (p.k + 1) * p.N), dtype=np.uint64) if out is None else out
        for i in range(len(rk)):
            data[i] = tag("pack_round_keys", dig(rk[i]))
        return PackedRoundKeys(p, 128, data)

    def unpack_round_keys(self, prk, first=0, count=None, out=None):
        self._called("unpack_round_keys")
        count = prk.n_keys - first if count is None else count
        out = self._out(out, count, 11, 16, 8)
        for j in range(count):
            out[j] = tag("unpack_round_keys", dig(prk.data[first + j]))
        return out

    def aes_key_expansion_packed(self, keys, chunk=256):
        self._called("aes_key_expansion_packed")
        p = self.params
        data = np.zeros((len(keys), gs.packed_key_glwes(p, 128), (p.k + 1) * p.N), dtype=np.uint64)
        for i in range(len(keys)):
            data[i] = tag("aes_key_expansion_packed", dig(keys[i]))
        return PackedRoundKeys(p, 128, data)

    # gates: a row depends on its own words and on the words of its gate
    def _gated(self, name, rows, valid, runs, out, what):
        self._called(name)
        flat_rows = rows.reshape(-1, rows.shape[-1])
        runs = self._gate_runs(valid, len(flat_rows), runs, what)
        out = np.zeros_like(rows) if out is None else out
        flat_out = out.reshape(-1, out.shape[-1])
        assert flat_out.shape == flat_rows.shape
        r = 0
        for g, run in enumerate(runs):
            for _ in range(run):
                flat_out[r] = tag(name, dig(valid[g]), dig(flat_rows[r]))
                r += 1
        return out

    def gate(self, ct, valid, bits_of_gate=None, out=None):
        return self._gated("gate", ct, valid, bits_of_gate, out, "ciphertexts")

    def gate_packed(self, packed, valid, glwes_of_gate=None, out=None):
        return self._gated("gate_packed", packed, valid, glwes_of_gate, out, "GLWEs")

    # packing: GLWE t // N holds bit t at coefficient t % N
    def pack(self, ct, out=None, width=64):
        self._called("pack")
        p = self.params
        flat_ct = ct.reshape(-1, p.big1)
        m = len(flat_ct)
        shape = ((m + p.N - 1) // p.N, gs.packed_mod_words(p, width))
        out = np.zeros(shape, dtype=np.uint64) if out is None else out
        assert tuple(out.shape) == shape
        for gl in range(shape[0]):
            out[gl] = tag("pack", width, [(t % p.N, dig(flat_ct[t])) for t in range(gl * p.N, min(m, (gl + 1) * p.N))])
        return out

    def unpack(self, packed, shape, out=None, width=64):
        self._called("unpack")
        p = self.params
        shape = (int(shape),) if isinstance(shape, int) else tuple(shape)
        m = int(np.prod(shape, dtype=np.int64))
        assert tuple(packed.shape) == ((m + p.N - 1) // p.N, gs.packed_mod_words(p, width))
        out = self._out(out, *shape)
        flat_out = out.reshape(-1, p.big1)
        assert len(flat_out) == m
        for t in range(m):
            flat_out[t] = tag("unpack", width, t % p.N, dig(packed[t // p.N]))
        return out

    def expand(self, seeded, out=None):
        self._called("expand")
        bodies = seeded.bodies.reshape(-1)
        out = self._out(out, *seeded.bodies.shape)
        flat_out = out.reshape(-1, self.params.big1)
        assert len(flat_out) == len(bodies)
        for t in range(len(bodies)):
            flat_out[t] = tag("expand", dig(seeded.mask_key), (int(seeded.first_index) + t) % (1 << 64), int(bodies[t]))
        return out


def echo_group(g, fail=None):
    """a ServerGroup around g echo models: no __init__, no device; fail = (context, (method, exception))"""
    grp = ServerGroup.__new__(ServerGroup)
    grp.params, grp.devices = TINY, (0,) * g
    grp.servers = [Echo(TINY, fail[1] if fail and fail[0] == i else None) for i in range(g)]
    return grp


# ---- the table on the echo model ---------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_public_method_of_server_group():
    public = {name for name, f in inspect.getmembers(ServerGroup, callable) if not name.startswith("_")}
    assert set(gs.EXCLUDED) <= public
    assert {c.method for c in gs.CASES} == public - set(gs.EXCLUDED)
    assert public - set(gs.EXCLUDED) <= {name for name in vars(Echo) if not name.startswith("_")}, "a group method the echo model would pass to an engine"
    assert {c.method for c in gs.CASES if c.method in gs.IN_PLACE_BLOCKS and 4 in c.sizes} == set(gs.IN_PLACE_BLOCKS)


def test_the_table_holds_the_shapes_its_comments_promise():
    env = gs.ShapeEnv(TINY)
    at = lambda name, n: gs.BY_NAME[name].build(env, n)
    w = lambda name, n, g: gs.working(gs.BY_NAME[name].items(at(name, n)), g, _shards_by_cost, shard_blocks)
    assert at("aes_encrypt_keyed", 4)["a"][1] == [1, 0, 0, 1] and 0x1FF in at("add_scalar", 4)["a"][1] and len(set(at("add_scalar", 4)["a"][1])) == 4
    assert at("aes_gcm_ctr", 4)["kw"]["first_block"] == 3
    assert at("aes_ctr_32", 4)["a"][1] & 0xFFFFFFFF == 0xFFFFFFFD and at("aes_ctr_32", 4)["a"][2] == 0
    assert [len(st[2]) for st in at("aes_cbc_streams", 3)["a"][1]] == [1, 2, 1] and [st[3] for st in at("aes_ctr_streams", 2)["a"][1]] == [1, 3]
    h = at("aes_xts_decrypt", 4)
    assert (h["kw"], len(h["a"][2]), len(h["a"][3])) == ({"unit_bytes": 32, "first_block": 1}, 3, 64)
    assert [len(st[1]) for st in at("aes_cbc_mac_streams", 4)["a"][1]] == [1, 1, 5, 1] and len(at("aes_cbc_mac_streams", 4)["a"][1][2]) == 4
    m = at("aes_ccm_decrypt", 4)["a"][1]
    assert [len(x[3]) for x in m] == [4, 0, 21, 16] and _shards_by_cost(at("aes_ccm_decrypt", 4)["costs"], 5)[1] == (1, 2)     # no payload, alone
    assert [len(x[1]) for x in at("aes_cmac_streams", 4)["a"][1]] == [0, 16, 17, 80]
    assert at("aes_cmac_streams_first_context_idle", 2)["costs"] == [3, 1] and w("aes_cmac_streams_first_context_idle", 2, 3) == [1, 2]
    assert at("aes_key_unwrap_packed", 4)["kw"] == {"gate": False, "chunk": 1} and at("aes_key_unwrap", 4)["a"][2] == [0, 1, 1, 0]
    assert at("gate_runs", 3)["a"][2] == [0, 3, 1] and at("gate_equal", 3)["a"][2] is None and w("gate_runs", 3, 3) == [1, 2]
    assert at("pack_64", 3)["a"][0].shape == (2 * TINY.N + 1, TINY.big1) and at("pack_16", 1)["a"][0].shape == (1, TINY.big1)
    assert at("expand", 5)["a"][0].first_index != 0 and at("expand", 5)["a"][0].bodies.shape == (5,)
    assert isinstance(at("aes_encrypt_keyed_store", 4)["a"][0], PackedRoundKeys) and isinstance(at("aes_cmac_streams_store", 4)["a"][0], PackedRoundKeys)
    assert w("aes_encrypt", 4, 3) == [0, 1, 2] and w("aes_encrypt", 4, 5) == [0, 1, 2, 3] and w("aes_key_expansion_many_128", 2, 3) == [0, 1]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", gs.CASES, ids=lambda c: c.name)
def test_a_group_of_echo_models_writes_what_one_model_writes(case):
    env = gs.ShapeEnv(TINY)
    for n in range(case.least, gs.MAX_N + 1):
        h = case.build(env, n)
        one = Echo(TINY)
        want = gs.flat(gs.call(one, case, gs.fresh(h)))
        assert one.calls, "the case reached no method of the model"
        split = case.items(h)
        for g in GROUPS:
            grp = echo_group(g)
            got = gs.flat(gs.call(grp, case, gs.fresh(h)))
            assert same(got, want), "%s on %d items over %d contexts" % (case.name, n, g)
            worked = [i for i, s in enumerate(grp.servers) if s.calls]
            assert worked == gs.working(split, g, _shards_by_cost, shard_blocks), (case.name, n, g)
            assert all(s.clean and s.syncs for s in grp.servers if s.calls), "a context that worked was not synchronised"
            assert all(s.syncs == 0 for s in grp.servers if not s.calls) or split[0] == "first"


# ---- the class itself ------------------------------------------------------------------------------------------------------------------------
def test_every_public_method_keeps_its_recorded_signature():
    """golden/server_group_signatures.json: str(inspect.signature) of every public method, recorded before the class was rewritten over
    shared helpers; a new method is added to the list, none changes its parameters by the way"""
    recorded = json.loads((Path(__file__).resolve().parent / "golden" / "server_group_signatures.json").read_text())
    now = {name: str(inspect.signature(f)) for name, f in inspect.getmembers(ServerGroup, callable) if not name.startswith("_")}
    assert now == recorded


def test_every_split_is_made_by_one_of_the_two_shard_builders():
    """ServerGroup._even and ServerGroup._by_cost each call their shard function once; no other line of the class calls either"""
    source = inspect.getsource(ServerGroup)
    a_call = re.compile(r"\b(shard_blocks|_shards_by_cost)\s*\(")
    for builder, function in ((ServerGroup._even, "shard_blocks"), (ServerGroup._by_cost, "_shards_by_cost")):
        own = inspect.getsource(builder)
        assert [m.group(1) for m in a_call.finditer(own)] == [function] and source.count(own) == 1
        source = source.replace(own, "")
    assert a_call.search(source) is None, a_call.search(source)


# ---- an exception in one shard ---------------------------------------------------------------------------------------------------------------
def test_an_exception_in_one_shard_surfaces_on_the_callers_thread_after_the_other_shards_finished():
    env = gs.ShapeEnv(TINY)
    case = gs.BY_NAME["aes_encrypt"]
    h = case.build(env, 4)                                                            # 2 + 1 + 1
    want = gs.flat(gs.call(Echo(TINY), case, gs.fresh(h)))[0]
    boom = RuntimeError("shard 2 of 3")
    grp = echo_group(3, fail=(1, ("aes_encrypt", boom)))
    mine = gs.fresh(h)
    before = mine["a"][1].copy()
    caller = threading.get_ident()
    with pytest.raises(RuntimeError) as e:
        gs.call(grp, case, mine)
    assert e.value is boom and threading.get_ident() == caller
    state = mine["a"][1]
    assert np.array_equal(state[:2], want[:2]) and np.array_equal(state[3:], want[3:]) and np.array_equal(state[2], before[2])
    assert [s.calls for s in grp.servers] == [["aes_encrypt"]] * 3
    assert [s.clean for s in grp.servers] == [True, False, True] and [s.syncs for s in grp.servers] == [1, 0, 1]
    grp.servers[1].fail = None                                                        # the next call on the same group works
    assert same(gs.flat(gs.call(grp, case, gs.fresh(h))), (want,))
    assert all(s.clean for s in grp.servers)
