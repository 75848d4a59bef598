"""The calls of a context share its scratch -- thirteen grow-only workspaces, four staging buffers, one pinned upload buffer, one stream
(csrc/engine_ctx.h) -- and this is the table of calls that test_gpu_workspace_state.py runs on a poisoned, regrown, released and
twice-used context, each at PARAM_TOY and at the smallest shape at which every table and every index of the call exists, with at
least 2 of every indexed thing.  A helper module like chunk_seams.py: no test, no fixture.  test_workspace_state_cpu.py pins the table
without a GPU.

A case is (name, entry, uses, pair, build, run, check_clear):

  entry        the C entry points whose code the case runs (a 128-bit alias and the _bits function it forwards to both count)
  uses         scratch buffers (fheaes_workspace_info names) the call is known to grow, by reading its schedule: after the anchor run
               they must not be empty, so that poisoning them is not vacuous; () is a call that uses no scratch at all, and the GPU test
               asserts exactly that
  pair         the GROWERS entry run between the anchor and step c: a different, larger call that leaves ws_misc and the f64 buffer
               ws_ggswf (and every WoPBS workspace) larger than the case itself needs
  build(env, variant) -> inputs: a dict of host values; the names in inputs["dev"] are arrays that travel to the GPU before a run.
               variant 0 / 1: two different inputs of one shape (step e issues both back to back); inputs["vector"], where a published
               vector fits the shape, is (the clear model's answer, the published value)
  run(srv, d)  d: the inputs with the "dev" arrays resident.  Makes the call(s), synchronises nothing, returns the resident output
               tensor or a tuple of them (in-place calls return their argument: the test uploads fresh inputs for every run)
  check_clear(env, inputs, outs)   outs: the outputs as uint64 host arrays.  Decrypts them and compares with the clear model
               (tfhe_aes_amd.aes_clear) or, for the stage calls whose outputs have no clear meaning of their own, with the CPU oracle's
               words: the reference is never the engine alone
"""
from collections import namedtuple

import numpy as np

import ccm
import cmac
import keywrap
import xts
from aes_vectors import A3_KEY, BASE, F1_KEY, F1_PT, F5, F5_CTR, FIPS_C, FIPS_C1_CT, FIPS_C_PT, MASK128, own_client
from packed_key_model import key_glwes
from public_modes import CBC, CFB128, IV, cbc_ct, cfb128_encrypt
from tfhe_aes_amd import aes_clear
from tfhe_aes_amd.client import SeededCiphertexts, bytes_to_u128, u128_to_bytes

Case = namedtuple("Case", "name entry uses pair build run check_clear")

WOPBS = ("ws_small", "ws_pbs", "ws_ggsw", "ws_ggswf", "ws_digits")      # K1's and K3's digit planes, the four stage outputs
KEYS = (FIPS_C[128][0], F1_KEY)                                          # key 0: FIPS-197 C.1, key 1: SP 800-38A F.1 / F.5
KOB = [1, 0, 1]                                                          # 3 blocks under 2 keys
KOBS = (KOB, [0, 1, 0])                                                  # ... and the table of variant 1: two calls in flight upload different ones
N = 512


class Env:
    """what build and check_clear need: the kit's parameter set and oracle, and a client with the kit's secret key and its own sequence
    of encryptions"""

    def __init__(self, kit):
        self.kit, self.p, self.oracle, self.client = kit, kit.params, kit.oracle, own_client(kit)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def enc_round_keys(c, expanded):
    """clear round keys [Nr+1][16] -> fresh encryptions [Nr+1][16][8][kN+1] (what a client that expands its own key would send)"""
    a = np.array(expanded, dtype=np.uint64)
    return c.encrypt_bytes(a.reshape(-1)).reshape(a.shape + (8, c.params.big1))


def enc_blocks(c, values):
    return c.encrypt_bytes(np.array([u128_to_bytes(v) for v in values], dtype=np.uint64).reshape(-1)).reshape(len(values), 16, 8, c.params.big1)


def dec_blocks(c, words):
    return [bytes_to_u128(row) for row in c.decrypt_bytes(words).reshape(-1, 16)]


def key_sets(c, keys, inverse=False):
    """[n_keys][11][16][8][kN+1]: the keys' (decryption) round keys, freshly encrypted"""
    exp = [aes_clear.expand_key(k) for k in keys]
    if inverse:
        exp = [aes_clear.inv_mix_columns_round_keys(e) for e in exp]
    return np.stack([enc_round_keys(c, e) for e in exp])


def rand_blocks(seed, n):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(16), "big") for _ in range(n)]


def hold(srv, *tensors):
    """device temporaries of a run stay alive until the Server's next synchronize (as the wrapper's own do)"""
    srv._inflight.extend(tensors)


def empty(ref, *shape, f64=False):
    import torch

    return torch.empty(shape, dtype=torch.float64 if f64 else torch.int64, device=ref.device)


PRODUCER_SIZE = 4096
PRODUCER_MS_PER_STEP = 1.0          # one 4,096^3 fp32 matmul on an MI355X: 17.0 ms for 16, 31.5 ms for 32; only sizes the chains


def producer_matrix():
    import torch

    a = torch.randn(PRODUCER_SIZE, PRODUCER_SIZE, device="cuda") / PRODUCER_SIZE ** 0.5
    torch.cuda.synchronize()
    return a


def producer(stream, a, steps):
    """a chain of `steps` matmuls on `stream`, each the input of the next: what keeps a stream busy for a known time, so that whatever is
    enqueued behind it is still waiting when the host moves on.  Returns (start event, end event, the last product: keep it alive)"""
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(stream)
        x = a
        for _ in range(steps):
            x = x @ a
        t1.record(stream)
    return t0, t1, x


# The calls that cannot return while the stream is still busy with what was enqueued before them, by design: one that uploads a second
# table waits, on the host, for its own first upload (upload_pinned waits for the last copy out of the one pinned buffer), and that copy
# waits for the stream.  Step e runs them like the others; only the assertion that the first call was wholly in flight is not made.
_SECOND_TABLE = "uploads more than one table: the second upload waits on the host for the first"
WAITS_INSIDE = {"aes_xts_decrypt": _SECOND_TABLE, "aes_cbc_mac_streams": _SECOND_TABLE, "aes_ccm_decrypt": _SECOND_TABLE, "aes_ccm_decrypt_gate": _SECOND_TABLE,
                "aes_cmac_verify": _SECOND_TABLE, "aes_cmac_subkeys": _SECOND_TABLE, "aes_key_unwrap": _SECOND_TABLE,
                "aes_key_unwrap_packed": "aes_key_expansion_packed synchronises before it frees each chunk's LWE form"}


def same_words(inputs, outs):
    """outs against the CPU oracle's words in inputs["want"]"""
    want = inputs["want"] if isinstance(inputs["want"], tuple) else (inputs["want"],)
    assert len(outs) == len(want)
    for got, w in zip(outs, want):
        assert np.array_equal(got.reshape(-1), np.ascontiguousarray(w).view(np.uint64).reshape(-1))


# ---- the fill patterns of fheaes_workspace_poison, restated from include/fheaes.h ---------------------------------------------------------
def pattern_bytes(cls, nbytes):
    """what FHEAES_WS_POISON_FILL leaves in a buffer of class `cls` ("f64", "words", "tables") and nbytes bytes"""
    if cls == "words":
        return b"\xa5" * nbytes
    word = (0x7FF87FF8 if cls == "f64" else 1).to_bytes(4, "little")
    return word * (nbytes // 4) + b"\xa5" * (nbytes % 4)


def pattern_words(cls, nbytes):
    """(first, last) as fheaes_workspace_info reports them for that buffer: its first 8 bytes and its last whole 8-byte word, a buffer of
    fewer than 8 bytes zero-extended"""
    b = pattern_bytes(cls, nbytes)
    take, last_off = min(8, nbytes), (nbytes // 8 - 1) * 8 if nbytes >= 8 else 0
    return int.from_bytes(b[:take], "little"), int.from_bytes(b[last_off:last_off + take], "little")


# ---- stages: K1 .. K5 and wopbs_batch on 3 inputs ------------------------------------------------------------------------------------
def _stage_bits(env, variant, m=3):
    bits = np.array([[1, 0, 1], [0, 1, 1]][variant][:m], dtype=np.uint8)
    return bits, env.client.encrypt_bits(bits)


def build_k1(env, v):
    _, x = _stage_bits(env, v)
    return {"dev": ["x"], "x": x, "want": env.oracle.keyswitch(x)}


def run_k1(srv, d):
    out = empty(d["x"], 3, srv.params.n + 1)
    srv.engine.keyswitch_batch(d["x"], out, 3)
    return out


def build_k2(env, v):
    _, x = _stage_bits(env, v)
    small = env.oracle.keyswitch(x)
    return {"dev": ["small"], "small": small, "want": env.oracle.cbs_pbs(small)}


def run_k2(srv, d):
    out = empty(d["small"], 3, srv.params.big1)
    srv.engine.cbs_pbs_batch(d["small"], out, 3)
    return out


def build_k3(env, v):
    x = np.random.default_rng(0x3300 + v).integers(0, 1 << 64, (3, env.p.big1), dtype=np.uint64)
    return {"dev": ["x"], "x": x, "want": env.oracle.pfpks(x)}


def run_k3(srv, d):
    p = srv.params
    out = empty(d["x"], 3, p.k + 1, (p.k + 1) * N)
    srv.engine.pfpks_batch(d["x"], out, 3)
    return out


def build_k4(env, v):
    from oracle import oracle as orc

    x = np.random.default_rng(0x4400 + v).integers(0, 1 << 64, (3, N), dtype=np.uint64)
    return {"dev": ["x"], "x": x, "want": orc.polys_to_fourier(x)}


def run_k4(srv, d):
    out = empty(d["x"], 3, 256, 2, f64=True)
    srv.engine.forward_fourier_batch(d["x"], out, 3)
    return out


STAGE_BYTES = ([0x53, 0xE1, 0x00], [0xFF, 0x53, 0x7A])


def build_k5(env, v):
    from oracle import oracle as orc

    x = env.client.encrypt_bytes(STAGE_BYTES[v])
    luts = orc.build_lutset(orc.LUTSET_DEC_MUL)
    want, dbg = env.oracle.wopbs_batch(x, luts, debug=True)
    ggsw_f = np.ascontiguousarray(orc.polys_to_fourier(dbg["ggsw"].reshape(3, 8, -1, N)))
    return {"dev": ["ggsw_f", "luts"], "ggsw_f": ggsw_f, "luts": np.ascontiguousarray(luts), "want": want, "values": STAGE_BYTES[v],
            "muls": (9, 11, 13, 14)}


def run_k5(srv, d):
    out = empty(d["luts"], 3, 4, 8, srv.params.big1)
    srv.engine.vertical_packing_batch(d["ggsw_f"], 3, 8, d["luts"], 4, False, out)
    return out


def check_k5(env, h, outs):
    same_words(h, outs)
    dec = env.client.decrypt_bytes(outs[0].reshape(3, 4, 8, env.p.big1))
    assert [[int(b) for b in row] for row in dec] == [[aes_clear.gf_mul(x, m) for m in h["muls"]] for x in h["values"]]


def build_wopbs8(env, v):
    from oracle import oracle as orc

    x = env.client.encrypt_bytes(STAGE_BYTES[v])
    luts = orc.build_lutset(orc.LUTSET_ENC_ROUND)[:3]
    return {"dev": ["x"], "x": x, "luts": [np.ascontiguousarray(l) for l in luts], "want": env.oracle.wopbs_batch(x, np.ascontiguousarray(luts)),
            "values": STAGE_BYTES[v]}


def run_wopbs(srv, d):
    return srv.many_wopbs_without_padding(d["x"], d["luts"])


def check_wopbs8(env, h, outs):
    same_words(h, outs)
    dec = env.client.decrypt_bytes(outs[0].reshape(3, 3, 8, env.p.big1))
    S = aes_clear.SBOX
    assert [[int(b) for b in row] for row in dec] == [[S[x], aes_clear.mul2(S[x]), aes_clear.mul3(S[x])] for x in h["values"]]


ADDS = ((0x7F, 0xF3, 0x01), (0x00, 0xFF, 0x80))


def build_wopbs9(env, v):
    """the add_scalar shape: 9 input bits (a byte and a carry), 2 LUTs that differ per input"""
    from tfhe_aes_amd.server import gen_lut

    bits = np.random.default_rng(0x9900 + v).integers(0, 2, (3, 9)).astype(np.uint8)
    x = env.client.encrypt_bits(bits)
    luts = np.stack([np.stack([gen_lut(2, 1, N, 9, lambda t, a=a: ((t & 0xFF) + (t >> 8) + a) % 256),
                               gen_lut(2, 1, N, 9, lambda t, a=a: 1 if (t & 0xFF) + (t >> 8) + a > 255 else 0)]) for a in ADDS[v]])
    return {"dev": ["x"], "x": x, "luts": luts, "want": env.oracle.wopbs_batch(x, luts, lut_per_input=True), "bits": bits, "adds": ADDS[v]}


def check_wopbs9(env, h, outs):
    same_words(h, outs)
    dec = env.client.decrypt_bits(outs[0].reshape(3, 2, 9, env.p.big1))
    for i, a in enumerate(h["adds"]):
        t = int(sum(int(h["bits"][i, j]) << j for j in range(9)))
        s = (t & 0xFF) + (t >> 8) + a
        assert int(sum(int(dec[i, 0, j]) << j for j in range(8))) == s % 256 and int(dec[i, 1, 0]) == (1 if s > 255 else 0)


def tree_function(t):
    return (t * 37 + 5) & 0x7FF


def build_wopbs11(env, v):
    """11 bits: the CMUX tree over bits 9 and 10 (ws_tree), then the rotation over bits 0..8"""
    from tfhe_aes_amd.server import gen_lut

    values = ([0x000, 0x7FF, 0x2A5], [0x400, 0x1FF, 0x6D3])[v]           # both values of both tree bits
    bits = np.array([[(t >> j) & 1 for j in range(11)] for t in values], dtype=np.uint8)
    x = env.client.encrypt_bits(bits)
    lut = gen_lut(2, 1, N, 11, tree_function)
    return {"dev": ["x"], "x": x, "luts": [lut], "want": env.oracle.wopbs_batch(x, lut[None]), "values": values}


def check_wopbs11(env, h, outs):
    same_words(h, outs)
    dec = env.client.decrypt_bits(outs[0].reshape(3, 1, 11, env.p.big1))
    assert [int(sum(int(dec[i, 0, j]) << j for j in range(11))) for i in range(3)] == [tree_function(t) for t in h["values"]]


# ---- S-Boxes on 3 bytes ---------------------------------------------------------------------------------------------------------------
def sbox_case(inv, many):
    S, mul = (aes_clear.INV_SBOX if inv else aes_clear.SBOX), aes_clear.gf_mul
    if many:
        clear = (lambda x: [mul(x, m) for m in (9, 11, 13, 14)]) if inv else (lambda x: [S[x], mul(S[x], 2), mul(S[x], 3)])
    else:
        clear = lambda x: S[x]

    def build(env, v):
        return {"dev": ["x"], "x": env.client.encrypt_bytes(STAGE_BYTES[v]), "expect": [clear(x) for x in STAGE_BYTES[v]]}

    def run(srv, d):
        return srv.many_sbox(d["x"], inv) if many else srv.sbox(d["x"], inv)

    def check(env, h, outs):
        dec = env.client.decrypt_bytes(outs[0])
        assert [([int(b) for b in row] if many else int(row)) for row in dec] == h["expect"]

    name = ("many_sbox" if many else "sbox") + ("_inv" if inv else "")
    return Case(name, ("fheaes_many_sbox" if many else "fheaes_sbox",), WOPBS + (() if many else ("ws_vp",)), "public_keyed_24", build, run, check)


# ---- key expansion and decryption round keys ------------------------------------------------------------------------------------------------
OTHER_KEYS = {16: bytes(range(0x80, 0x90)), 32: bytes(range(0x40, 0x60))}


def expansion_case(name, entry, keys_of_variant, call):
    """keys_of_variant[v]: the clear keys; call(srv, key tensor [n][len][8][kN+1]) -> the round keys"""
    def build(env, v):
        keys = keys_of_variant[v]
        h = {"dev": ["keys"], "keys": np.stack([env.client.encrypt_aes_key(k) for k in keys]), "clear": keys}
        last = bytes(aes_clear.expand_key(keys[0])[-1])
        if keys[0] == FIPS_C[128][0]:
            h["vector"] = (last, bytes.fromhex("13111d7fe3944a17f307a78b4d2b30c5"))              # FIPS-197 C.1, round[10].k_sch
        if keys[0] == A3_KEY:
            h["vector"] = (last[12:], bytes.fromhex("706c631e"))                                 # FIPS-197 A.3, w59
        return h

    def check(env, h, outs):
        n = len(h["clear"])
        dec = env.client.decrypt_bytes(outs[0]).reshape(n, -1, 16)
        for j, k in enumerate(h["clear"]):
            assert [[int(b) for b in row] for row in dec[j]] == [list(r) for r in aes_clear.expand_key(k)]

    return Case(name, entry, WOPBS + ("ws_tmp_a", "ws_tmp_b"), "public_keyed_24", build, lambda srv, d: call(srv, d["keys"]), check)


def _expand_128(srv, keys):
    rk = empty(keys, 11, 16, 8, srv.params.big1)
    srv.engine.aes_key_expansion(keys[0], rk)
    return rk


def dec_round_keys_case(name, entry, n_keys, call):
    def build(env, v):
        keys = (KEYS, (OTHER_KEYS[16], F5[128][0]))[v][:n_keys]
        return {"dev": ["rk"], "rk": key_sets(env.client, keys), "clear": keys}

    def check(env, h, outs):
        dec = env.client.decrypt_bytes(outs[0]).reshape(n_keys, 11, 16)
        for j, k in enumerate(h["clear"]):
            assert [[int(b) for b in row] for row in dec[j]] == [list(r) for r in aes_clear.inv_mix_columns_round_keys(aes_clear.expand_key(k))]

    return Case(name, entry, WOPBS + ("ws_vp", "ws_tmp_a"), "public_keyed_24", build, lambda srv, d: call(srv, d["rk"]), check)


def _dec_rk_128(srv, rk):
    dw = empty(rk, 11, 16, 8, srv.params.big1)
    srv.engine.aes_decryption_round_keys(rk[0], dw)
    return dw


# ---- the block ciphers ---------------------------------------------------------------------------------------------------------------------
# direction -> (round keys are decryption round keys, the clear function, the other direction's, the C name's middle)
DIRECTIONS = {"encrypt": (False, aes_clear.aes_encrypt_block, "encrypt"), "decrypt": (False, aes_clear.aes_decrypt_block, "decrypt"),
              "decrypt_equivalent": (True, aes_clear.aes_decrypt_block, "decrypt_equivalent")}
CIPHER_BLOCKS = ([FIPS_C_PT, BASE, MASK128], [0, F1_PT[0], BASE + 1])       # what the ENCRYPTION takes; a decryption takes its ciphertexts


def cipher_case(direction, form):
    """form: "plain" (2 blocks, key 0, the AES-128 entry point), "keyed" (3 blocks under 2 keys, KOB), "packed" (the same from a 2-key
    packed store, packed inside the run)"""
    inverse, clear, mid = DIRECTIONS[direction]
    n = 2 if form == "plain" else 3

    def build(env, v):
        key_of = [0] * n if form == "plain" else KOBS[v]
        pts = CIPHER_BLOCKS[v][:n]
        cts = [aes_clear.aes_encrypt_block(KEYS[k], b) for k, b in zip(key_of, pts)]
        given, expect = (pts, cts) if direction == "encrypt" else (cts, pts)
        assert [clear(KEYS[k], b) for k, b in zip(key_of, given)] == expect
        sets = key_sets(env.client, KEYS, inverse)
        h = {"dev": ["rk", "state"], "rk": sets[0] if form == "plain" else sets, "state": enc_blocks(env.client, given), "expect": expect, "kob": key_of}
        if v == 0 and form == "plain":
            h["vector"] = (expect[0], FIPS_C1_CT if direction == "encrypt" else FIPS_C_PT)       # FIPS-197 C.1: key 0, block 0
        return h

    def run(srv, d):
        if form == "plain":
            getattr(srv.engine, "aes_" + mid)(d["rk"], d["state"], n)
        elif form == "keyed":
            getattr(srv, "aes_%s_keyed" % mid)(d["rk"], d["kob"], d["state"])
        else:
            store = srv.pack_round_keys(d["rk"])
            hold(srv, store.data)
            getattr(srv, "aes_%s_keyed" % mid)(store, d["kob"], d["state"])
        return d["state"]

    def check(env, h, outs):
        assert dec_blocks(env.client, outs[0]) == h["expect"]

    entry = {"plain": ("fheaes_aes_%s" % mid, "fheaes_aes_%s_bits" % mid), "keyed": ("fheaes_aes_%s_keyed" % mid,),
             "packed": ("fheaes_pack_round_keys", "fheaes_aes_%s_keyed_packed" % mid)}[form]
    uses = WOPBS + ("ws_vp",) + (("ws_misc",) if form != "plain" else ())
    return Case("aes_%s%s" % (direction, {"plain": "", "keyed": "_keyed", "packed": "_keyed_packed"}[form]), entry, uses, "public_keyed_24", build, run, check)


def build_round_key_store(env, v):
    keys = (KEYS, (OTHER_KEYS[16], F5[128][0]))[v]
    return {"dev": ["rk"], "rk": key_sets(env.client, keys), "clear": keys}


def run_round_key_store(srv, d):
    store = srv.pack_round_keys(d["rk"])
    return store.data, srv.unpack_round_keys(store)


def check_round_key_store(env, h, outs):
    packed, unpacked = outs
    p = env.p
    for j, k in enumerate(h["clear"]):
        want = [b for r in aes_clear.expand_key(k) for b in r]
        assert [int(b) for b in env.client.decrypt_packed_bytes(packed.reshape(2, key_glwes(p, 128), -1)[j], 11 * 16)] == want
        assert [int(b) for b in env.client.decrypt_bytes(unpacked.reshape(2, 11 * 16, 8, p.big1)[j])] == want


# ---- add_scalar: 2 blocks, two different counters, one with a high word, both sums carrying across a word ------------------------------------
def build_add_scalar(env, v):
    states = ([BASE, (1 << 64) - 0x10], [MASK128 - 5, 0x0123456789ABCDEF_FFFFFFFFFFFFFF00])[v]
    counters = ([0x1234, (1 << 64) + 0x25], [7, (3 << 64) + 0x1FF])[v]
    return {"dev": ["state"], "state": enc_blocks(env.client, states), "counters": counters, "expect": [(s + c) & MASK128 for s, c in zip(states, counters)]}


def run_add_scalar(srv, d):
    return srv.add_scalar(d["state"], d["counters"])


def check_blocks(env, h, outs):
    assert dec_blocks(env.client, outs[0]) == h["expect"]


# ---- public modes on 3 blocks ---------------------------------------------------------------------------------------------------------------
def public_case(name, entry, build, run, inverse=False, keyed=False):
    def build_all(env, v):
        h = build(v)
        sets = key_sets(env.client, KEYS if keyed else [h.pop("key")], inverse)
        h.update({"dev": ["rk"], "rk": sets if keyed else sets[0]})
        return h

    # paired with the grower of the OTHER direction: a different call, other tables
    return Case(name, entry, WOPBS + ("ws_vp", "ws_misc"), "public_keyed_24" if inverse else "decrypt_public_keyed_24", build_all, run, check_blocks)


def _b_encrypt_public(v):
    blocks = ([BASE, BASE + 1, F1_PT[0]], [F1_PT[1], F1_PT[1] ^ 0xFF, 0])[v]         # two of them share 15 bytes
    h = {"key": F1_KEY, "blocks": blocks, "expect": [aes_clear.aes_encrypt_block(F1_KEY, b) for b in blocks]}
    if v == 0:
        h["vector"] = (h["expect"][2], 0x3AD77BB40D7A3660A89ECAF32466EF97)             # SP 800-38A F.1.1, block 1
    return h


def _b_ctr(v, counter_bits=128):
    # variant 1 at 128 bits carries out of the low 32; variant 0 at 32 bits wraps them at block 2, the upper 96 staying
    iv = (F5_CTR, (F5_CTR & ~0xFFFFFFFF) | 0xFFFFFFFE)[v] if counter_bits == 128 else ((BASE & ~0xFFFFFFFF) | 0xFFFFFFFE, F5_CTR)[v]
    data = (F1_PT[:3], F1_PT[1:4])[v]
    ks = aes_clear.ctr_keystream(F1_KEY, iv, 0, 3, counter_bits)
    h = {"key": F1_KEY, "iv": iv, "data": data, "counter_bits": counter_bits, "expect": [k ^ d for k, d in zip(ks, data)]}
    if v == 0 and counter_bits == 128:
        h["vector"] = (h["expect"][0], F5[128][1])                                      # SP 800-38A F.5.1, block 1
    return h


def _r_ctr(srv, d):
    return srv.aes_ctr(d["rk"], d["iv"], 0, 3, data=d["data"], counter_bits=d["counter_bits"])


def _b_decrypt_public(v):
    blocks, data = (cbc_ct(128)[:3], [IV] + cbc_ct(128)[:2]) if v == 0 else (rand_blocks(0xD0, 3), rand_blocks(0xD1, 3))
    h = {"key": F1_KEY, "blocks": blocks, "data": data, "expect": [aes_clear.aes_decrypt_block(F1_KEY, b) ^ x for b, x in zip(blocks, data)]}
    if v == 0:
        h["vector"] = (h["expect"], F1_PT[:3])                                          # SP 800-38A F.2.2 through its parts
    return h


def _b_cbc(v):
    ct = cbc_ct(128)[:3] if v == 0 else rand_blocks(0xCB, 3)
    iv = IV if v == 0 else BASE
    h = {"key": F1_KEY, "iv": iv, "ct": ct, "expect": aes_clear.cbc_decrypt(F1_KEY, iv, ct)}
    if v == 0:
        h["vector"] = ((ct[0], h["expect"]), (CBC[128][1], F1_PT[:3]))                  # SP 800-38A F.2.2
    return h


def _b_cfb(v):
    ct = cfb128_encrypt(CFB128[0], IV, F1_PT)[:3] if v == 0 else rand_blocks(0xCF, 3)
    iv = IV if v == 0 else BASE
    h = {"key": F1_KEY, "iv": iv, "ct": ct, "expect": aes_clear.cfb128_decrypt(F1_KEY, iv, ct)}
    if v == 0:
        h["vector"] = ((ct[0], h["expect"]), (CFB128[1], F1_PT[:3]))                    # SP 800-38A F.3.14
    return h


def _b_public_keyed(v, inverse=False):
    blocks, data = ([BASE, BASE, BASE + 1], F1_PT[:3]) if v == 0 else (rand_blocks(0xE0, 3), rand_blocks(0xE1, 3))    # equal blocks under two keys
    f = aes_clear.aes_decrypt_block if inverse else aes_clear.aes_encrypt_block
    return {"blocks": blocks, "data": data, "kob": KOBS[v], "expect": [f(KEYS[k], b) ^ x for k, b, x in zip(KOBS[v], blocks, data)]}


# ---- XTS: 2 units of 2 blocks --------------------------------------------------------------------------------------------------------------
def build_xts(env, v):
    key1, key2, sector, pt, ct = xts.VECTORS[2]
    if v == 1:
        sector, pt = 0xFE, bytes(range(32))
    pts = [pt, bytes(range(100, 132))]
    data = b"".join(aes_clear.xts_encrypt(key1, key2, sector + u, pts[u]) for u in range(2))
    h = {"dev": ["dw1", "rk2"], "dw1": key_sets(env.client, [key1], True)[0], "rk2": key_sets(env.client, [key2])[0], "sector": sector, "data": data,
         "expect": [int.from_bytes((pts[0] + pts[1])[i:i + 16], "big") for i in range(0, 64, 16)]}
    if v == 0:
        h["vector"] = (data[:32], ct)                                                   # IEEE 1619 annex B, vector 2
    return h


def run_xts(srv, d):
    return srv.aes_xts_decrypt(d["dw1"], d["rk2"], d["sector"], d["data"], unit_bytes=32)


# ---- MAC modes: 2 messages under 2 keys ----------------------------------------------------------------------------------------------------
def build_cbc_mac(env, v):
    """stream 0: two public blocks under key 1; stream 1: one block under key 0 whose first 5 bytes also get an encrypted addend"""
    b = rand_blocks(0x3AC0 + v, 3)
    addend = rand_blocks(0x3AD0 + v, 1)[0]
    part = int.from_bytes(u128_to_bytes(addend)[:5] + [0] * 11, "big")
    return {"dev": ["rk", "enc"], "rk": key_sets(env.client, KEYS), "enc": enc_blocks(env.client, [addend]), "blocks": b,
            "expect": [aes_clear.cbc_mac(KEYS[1], b[:2]), aes_clear.cbc_mac(KEYS[0], [b[2] ^ part])]}


def run_cbc_mac(srv, d):
    return srv.aes_cbc_mac_streams(d["rk"], [(1, d["blocks"][:2]), (0, d["blocks"][2:], d["enc"], [5])])


CCM_KEYS = (ccm.VECTORS["ex1"][0], F1_KEY)


def build_ccm(env, v):
    """message 0 under key 0 with a partial last block (variant 0: SP 800-38C example 1, 4 payload bytes; variant 1: 5 bytes of our own);
    message 1: 16 payload bytes under key 1.  One of the two carries a forged tag: message 1 in variant 0, message 0 in variant 1.  The
    plaintext of a forged message still decrypts (only the tag is wrong), which is what the ungated call must show and the gated one hide"""
    own_pt = bytes(range(0x50, 0x60))
    if v == 0:
        first, first_pt = ccm.message(0, "ex1"), ccm.VECTORS["ex1"][3]
    else:
        first_pt = bytes(range(5))
        first = ccm.own_message(0, CCM_KEYS[0], bytes(range(0x30, 0x3D)), b"hdr", first_pt, 6)
    msgs = [first, ccm.own_message(1, CCM_KEYS[1], bytes(range(12)), b"", own_pt, 8)]
    bad = 1 - v
    m = msgs[bad]
    msgs[bad] = m[:4] + (bytes([m[4][0] ^ 0x10]) + m[4][1:],)
    h = {"dev": ["rk"], "rk": key_sets(env.client, CCM_KEYS), "messages": msgs, "payloads": [first_pt, own_pt], "valid": [int(i != bad) for i in range(2)]}
    for i, (k, nonce, aad, ct, tag) in enumerate(msgs):
        clear = aes_clear.ccm_decrypt(CCM_KEYS[k], nonce, aad, ct + tag, len(tag))
        assert (clear == h["payloads"][i]) if h["valid"][i] else clear is None
    if v == 0:
        key, nonce, aad, payload, t, out = ccm.VECTORS["ex1"]
        h["vector"] = (aes_clear.ccm_encrypt(key, nonce, aad, payload, t), out)
    return h


def ccm_case(gate):
    def run(srv, d):
        pt, valid, _ = srv.aes_ccm_decrypt(d["rk"], d["messages"], gate=gate)
        return pt, valid

    def check(env, h, outs):
        pt, valid = outs
        assert [int(b) for b in env.client.decrypt_bits(valid)] == h["valid"]
        dec = env.client.decrypt_bytes(pt).reshape(2, 16)
        for i, payload in enumerate(h["payloads"]):
            shown = bytes(len(payload)) if gate and not h["valid"][i] else payload
            assert bytes(int(b) for b in dec[i]) == shown + bytes(16 - len(shown))

    return Case("aes_ccm_decrypt" + ("_gate" if gate else ""), ("fheaes_aes_ccm_open_keyed",) + (("fheaes_gate_bits",) if gate else ()),
                WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tmp_c", "ws_tree"), "public_keyed_24", build_ccm, run, check)


CMAC_KEYS = (cmac.VECTORS[128][0], FIPS_C[128][0])


def build_cmac_subkeys(env, v):
    keys = CMAC_KEYS if v == 0 else (OTHER_KEYS[16], F5[128][0][::-1])
    h = {"dev": ["rk"], "rk": key_sets(env.client, keys), "expect": [list(aes_clear.cmac_subkeys(k)) for k in keys]}
    if v == 0:
        h["vector"] = (h["expect"][0], [int.from_bytes(cmac.VECTORS[128][1], "big"), int.from_bytes(cmac.VECTORS[128][2], "big")])    # SP 800-38B D.1
    return h


def check_cmac_subkeys(env, h, outs):
    got = dec_blocks(env.client, outs[0])
    assert [got[0:2], got[2:4]] == h["expect"]


def build_cmac_verify(env, v):
    """message 0: one whole block under key 0 (K1); message 1: 40 bytes under key 1, padded (K2); variant 1: message 1's tag is forged"""
    m0, m1 = cmac.MESSAGE[:16], cmac.MESSAGE[:40]
    tags = [aes_clear.cmac(CMAC_KEYS[0], m0), aes_clear.cmac(CMAC_KEYS[1], m1, 8)]
    h = {"dev": ["rk"], "rk": key_sets(env.client, CMAC_KEYS), "valid": [1, 1 - v]}
    if v == 0:
        h["vector"] = (tags[0], cmac.VECTORS[128][3][1])                                # SP 800-38B D.1, example 2
    else:
        tags[1] = tags[1][:7] + bytes([tags[1][7] ^ 0x80])
    h["messages"] = [(0, m0, tags[0]), (1, m1, tags[1])]
    return h


def check_valid(env, h, outs):
    assert [int(b) for b in env.client.decrypt_bits(outs[-1])] == h["valid"]


# ---- key unwrap: 2 wrapped AES-128 keys under 2 KEKs, one of them tampered -------------------------------------------------------------------
def build_unwrap(env, v):
    kek0, payload0, wrapped0 = keywrap.vector("4.1")                                     # RFC 3394 4.1: KEK 000102..0F
    keks = (kek0, F1_KEY)
    payloads = [payload0, bytes(range(0xA0, 0xB0))] if v == 0 else [bytes(range(0x10, 0x20)), F5[128][0]]
    wrapped = [aes_clear.key_wrap(keks[1], payloads[0]) if v else wrapped0, aes_clear.key_wrap(keks[v == 0], payloads[1])]
    kek_of_key = [1, 0] if v else [0, 1]
    bad = 1 - v
    wrapped[bad] = wrapped[bad][:9] + bytes([wrapped[bad][9] ^ 0x04]) + wrapped[bad][10:]
    clear = [aes_clear.key_unwrap(keks[k], w) for k, w in zip(kek_of_key, wrapped)]
    h = {"dev": ["dw"], "dw": key_sets(env.client, keks, True), "wrapped": wrapped, "kek_of_key": kek_of_key, "valid": [int(ok) for ok, _ in clear],
         "payloads": [data for _, data in clear]}
    assert h["valid"] == [1 - (i == bad) for i in range(2)]
    if v == 0:
        h["vector"] = ((aes_clear.key_wrap(kek0, payload0), clear[0]), (wrapped0, (True, payload0)))
    return h


def run_unwrap(srv, d):
    return srv.aes_key_unwrap(d["dw"], d["wrapped"], d["kek_of_key"])


def check_unwrap(env, h, outs):
    keys, valid = outs
    check_valid(env, h, outs)
    dec = env.client.decrypt_bytes(keys.reshape(2, 16, 8, env.p.big1))
    assert [bytes(int(b) for b in row) for row in dec] == h["payloads"]


def run_unwrap_packed(srv, d):
    store, valid = srv.aes_key_unwrap_packed(d["dw"], d["wrapped"], d["kek_of_key"], chunk=1)
    return store.data, valid


def check_unwrap_packed(env, h, outs):
    packed, valid = outs
    check_valid(env, h, outs)
    for j, payload in enumerate(h["payloads"]):
        got = env.client.decrypt_packed_bytes(packed.reshape(2, key_glwes(env.p, 128), -1)[j], 11 * 16)
        assert [int(b) for b in got] == [b for r in aes_clear.expand_key(payload) for b in r]


# ---- the gate -----------------------------------------------------------------------------------------------------------------------------
def build_gate(env, v):
    gates, bits, runs = ([1, 0], [1, 1, 1], [2, 1]) if v == 0 else ([0, 1], [1, 0, 1], [1, 2])
    expect = [b * gates[0 if i < runs[0] else 1] for i, b in enumerate(bits)]
    return {"dev": ["valid", "ct"], "valid": env.client.encrypt_bits(np.array(gates, dtype=np.uint8)), "ct": env.client.encrypt_bits(np.array(bits, dtype=np.uint8)),
            "runs": runs, "expect": expect}


def run_gate(srv, d):
    return srv.gate(d["ct"], d["valid"], d["runs"])


def run_gate_ggsw(srv, d):
    """the four stage calls on the gate bits, then the kernel alone (fheaes_gate_bits' own composition, in the caller's buffers)"""
    from tfhe_aes_amd import _native

    p, E, g = srv.params, srv.engine, d["valid"]
    k1 = p.k + 1
    small, pbs, rows = empty(g, 2, p.n + 1), empty(g, 2, p.big1), empty(g, 2, k1, k1 * N)
    ggf, out = empty(g, 2 * k1 * k1, 256, 2, f64=True), empty(g, 3, p.big1)
    E.keyswitch_batch(g, small, 2)
    E.cbs_pbs_batch(small, pbs, 2)
    E.pfpks_batch(pbs, rows, 2)
    E.forward_fourier_batch(rows, ggf, 2 * k1 * k1)
    E.gate_ggsw(ggf, d["runs"], d["ct"], 3, _native.GATE_LWE, out)
    hold(srv, small, pbs, rows, ggf)
    return out


def check_bits(env, h, outs):
    assert [int(b) for b in env.client.decrypt_bits(outs[-1])] == h["expect"]


def build_gate_packed(env, v):
    """2 GLWEs under 2 gates: 513 bits packed, the first GLWE full, the second holding one bit"""
    gates = ([1, 0], [0, 1])[v]
    bits = np.random.default_rng(0x6A7E + v).integers(0, 2, 513).astype(np.uint8)
    bits[512] = 1
    return {"dev": ["valid", "ct"], "valid": env.client.encrypt_bits(np.array(gates, dtype=np.uint8)), "ct": env.client.encrypt_bits(bits),
            "expect": [int(b) * gates[i // N] for i, b in enumerate(bits)]}


def run_gate_packed(srv, d):
    packed = srv.pack(d["ct"])
    hold(srv, packed)
    return srv.gate_packed(packed, d["valid"], [1, 1])


def check_packed_bits(env, h, outs, width=64):
    assert [int(b) for b in env.client.decrypt_packed(outs[0], len(h["expect"]), width=width)] == h["expect"]


# ---- packing and wire formats ---------------------------------------------------------------------------------------------------------------
def pack_case(width):
    def build(env, v):
        bits = np.random.default_rng(0x9AC0 + v + width).integers(0, 2, 513).astype(np.uint8)
        return {"dev": ["ct"], "ct": env.client.encrypt_bits(bits), "expect": [int(b) for b in bits]}

    def run(srv, d):
        packed = srv.pack(d["ct"], width=width)
        return packed, srv.unpack(packed, 513, width=width)

    def check(env, h, outs):
        check_packed_bits(env, h, outs, width)
        check_bits(env, h, outs)

    wide = width == 64
    return Case("pack_unpack_513" + ("" if wide else "_width%d" % width),
                ("fheaes_pack_bits", "fheaes_unpack_bits") if wide else ("fheaes_pack_bits_mod", "fheaes_unpack_bits_mod"),
                ("ws_ggsw", "ws_digits") + (() if wide else ("ws_tmp_a",)), "public_keyed_24", build, run, check)


def build_expand(env, v):
    bits = np.array(([1, 0, 1], [0, 1, 1])[v], dtype=np.uint8)
    s = env.client.encrypt_bits_seeded(bits, first_index=(1 << 32) - 2 + v)              # the index carries into the high nonce word
    return {"dev": ["bodies"], "bodies": np.ascontiguousarray(s.bodies, dtype=np.uint64), "mask_key": np.array(s.mask_key, dtype=np.uint32),
            "first_index": int(s.first_index), "want": s.expand(), "expect": [int(b) for b in bits]}


def run_expand(srv, d):
    return srv.expand(SeededCiphertexts(srv.params, d["mask_key"], d["first_index"], d["bodies"]))


def check_expand(env, h, outs):
    same_words(h, outs)
    check_bits(env, h, outs)


# ---- the growers of step c ---------------------------------------------------------------------------------------------------------------------
def grower(inverse):
    """24 random blocks under 2 keys through the keyed public call: pools of up to 384 bytes = 3,072 bits a round where no case runs a
    WoPBS over more than 768, and index tables of 24 x 16 entries a round in ws_misc where no case uploads more than 8.3 KB"""
    f = aes_clear.aes_decrypt_block if inverse else aes_clear.aes_encrypt_block

    def build(env, v):
        blocks, data, kob = rand_blocks(0x6120 + inverse, 24), rand_blocks(0x6130 + inverse, 24), [i % 2 for i in range(24)]
        return {"dev": ["rk"], "rk": key_sets(env.client, KEYS, inverse), "blocks": blocks, "data": data, "kob": kob,
                "expect": [f(KEYS[k], b) ^ x for k, b, x in zip(kob, blocks, data)]}

    def run(srv, d):
        call = srv.aes_decrypt_public_keyed if inverse else srv.aes_encrypt_public_keyed
        return call(d["rk"], d["kob"], d["blocks"], data=d["data"])

    name = "decrypt_public_keyed_24" if inverse else "public_keyed_24"
    return Case(name, ("fheaes_aes_decrypt_public_keyed" if inverse else "fheaes_aes_public_keyed",), WOPBS + ("ws_vp", "ws_misc"), None, build, run, check_blocks)


GROWERS = {g.name: g for g in (grower(False), grower(True))}
GROWN = ("ws_misc", "ws_ggswf")          # what a grower must leave larger than the case's anchor did

# ---- the table -------------------------------------------------------------------------------------------------------------------------------
G = "public_keyed_24"
CASES = [
    Case("k1_keyswitch", ("fheaes_keyswitch_batch",), ("ws_digits",), G, build_k1, run_k1, lambda env, h, outs: same_words(h, outs)),
    Case("k2_cbs_pbs", ("fheaes_cbs_pbs_batch",), (), G, build_k2, run_k2, lambda env, h, outs: same_words(h, outs)),
    Case("k3_pfpks", ("fheaes_pfpks_batch",), ("ws_digits",), G, build_k3, run_k3, lambda env, h, outs: same_words(h, outs)),
    Case("k4_forward_fourier", ("fheaes_forward_fourier_batch",), (), G, build_k4, run_k4, lambda env, h, outs: same_words(h, outs)),
    Case("k5_vertical_packing", ("fheaes_vertical_packing_batch",), (), G, build_k5, run_k5, check_k5),
    Case("wopbs_8_bits_shared_luts", ("fheaes_wopbs_batch",), WOPBS, G, build_wopbs8, run_wopbs, check_wopbs8),
    Case("wopbs_9_bits_per_input_luts", ("fheaes_wopbs_batch",), WOPBS, G, build_wopbs9, run_wopbs, check_wopbs9),
    Case("wopbs_11_bits_tree", ("fheaes_wopbs_batch",), WOPBS + ("ws_tree",), G, build_wopbs11, run_wopbs, check_wopbs11),
    sbox_case(False, False), sbox_case(True, False), sbox_case(False, True), sbox_case(True, True),
    expansion_case("aes_key_expansion_128", ("fheaes_aes_key_expansion", "fheaes_aes_key_expansion_bits"), ([KEYS[0]], [OTHER_KEYS[16]]),
                   lambda srv, keys: _expand_128(srv, keys)),
    expansion_case("aes_key_expansion_256", ("fheaes_aes_key_expansion_bits",), ([A3_KEY], [OTHER_KEYS[32]]), lambda srv, keys: srv.aes_key_expansion(keys[0])),
    expansion_case("aes_key_expansion_batch", ("fheaes_aes_key_expansion_batch",), (KEYS, (OTHER_KEYS[16], F5[128][0][::-1])),
                   lambda srv, keys: srv.aes_key_expansion_many(keys)),
    dec_round_keys_case("aes_decryption_round_keys", ("fheaes_aes_decryption_round_keys", "fheaes_aes_decryption_round_keys_bits"), 1, _dec_rk_128),
    dec_round_keys_case("aes_decryption_round_keys_batch", ("fheaes_aes_decryption_round_keys_batch",), 2, lambda srv, rk: srv.aes_decryption_round_keys_many(rk)),
] + [cipher_case(direction, form) for form in ("plain", "keyed", "packed") for direction in DIRECTIONS] + [
    Case("pack_unpack_round_keys", ("fheaes_pack_round_keys", "fheaes_unpack_round_keys"), ("ws_ggsw", "ws_digits"), G, build_round_key_store,
         run_round_key_store, check_round_key_store),
    Case("add_scalar", ("fheaes_add_scalar",), WOPBS + ("ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_luts"), G, build_add_scalar, run_add_scalar, check_blocks),
    public_case("aes_encrypt_public", ("fheaes_aes_encrypt_public_bits",), _b_encrypt_public, lambda srv, d: srv.aes_encrypt_public(d["rk"], d["blocks"])),
    public_case("aes_ctr", ("fheaes_aes_ctr_bits",), _b_ctr, _r_ctr),
    public_case("aes_ctr32", ("fheaes_aes_ctr32_bits",), lambda v: _b_ctr(v, 32), _r_ctr),
    public_case("aes_decrypt_public", ("fheaes_aes_decrypt_public_bits",), _b_decrypt_public,
                lambda srv, d: srv.aes_decrypt_public(d["rk"], d["blocks"], data=d["data"]), inverse=True),
    public_case("aes_cbc_decrypt", ("fheaes_aes_cbc_decrypt_bits",), _b_cbc, lambda srv, d: srv.aes_cbc_decrypt(d["rk"], d["iv"], d["ct"]), inverse=True),
    public_case("aes_cfb_decrypt", ("fheaes_aes_public_keyed",), _b_cfb, lambda srv, d: srv.aes_cfb_decrypt(d["rk"], d["iv"], d["ct"])),
    public_case("aes_public_keyed", ("fheaes_aes_public_keyed",), _b_public_keyed,
                lambda srv, d: srv.aes_encrypt_public_keyed(d["rk"], d["kob"], d["blocks"], data=d["data"]), keyed=True),
    public_case("aes_decrypt_public_keyed", ("fheaes_aes_decrypt_public_keyed",), lambda v: _b_public_keyed(v, True),
                lambda srv, d: srv.aes_decrypt_public_keyed(d["rk"], d["kob"], d["blocks"], data=d["data"]), inverse=True, keyed=True),
    Case("aes_xts_decrypt", ("fheaes_aes_xts_decrypt_bits",), WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tmp_c"), G, build_xts, run_xts, check_blocks),
    Case("aes_cbc_mac_streams", ("fheaes_aes_cbc_mac_keyed",), WOPBS + ("ws_vp", "ws_misc", "ws_tmp_b"), G, build_cbc_mac, run_cbc_mac, check_blocks),
    ccm_case(False), ccm_case(True),
    Case("aes_cmac_subkeys", ("fheaes_aes_cmac_subkeys_keyed",), WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tmp_c"), G, build_cmac_subkeys,
         lambda srv, d: srv.aes_cmac_subkeys(d["rk"]), check_cmac_subkeys),
    Case("aes_cmac_verify", ("fheaes_aes_cmac_keyed",), WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tmp_c", "ws_tree"), G, build_cmac_verify,
         lambda srv, d: srv.aes_cmac_verify(d["rk"], d["messages"]), check_valid),
    Case("aes_key_unwrap", ("fheaes_aes_kw_unwrap_keyed",), WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tree"), G, build_unwrap, run_unwrap, check_unwrap),
    Case("aes_key_unwrap_packed", ("fheaes_aes_kw_unwrap_keyed", "fheaes_aes_key_expansion_batch", "fheaes_pack_round_keys"),
         WOPBS + ("ws_vp", "ws_misc", "ws_tmp_a", "ws_tmp_b", "ws_tree"), G, build_unwrap, run_unwrap_packed, check_unwrap_packed),
    Case("gate", ("fheaes_gate_bits",), WOPBS + ("ws_misc",), G, build_gate, run_gate, check_bits),
    Case("gate_packed", ("fheaes_pack_bits", "fheaes_gate_packed"), WOPBS + ("ws_misc",), G, build_gate_packed, run_gate_packed, check_packed_bits),
    Case("gate_ggsw", ("fheaes_keyswitch_batch", "fheaes_cbs_pbs_batch", "fheaes_pfpks_batch", "fheaes_forward_fourier_batch", "fheaes_gate_ggsw"),
         ("ws_digits", "ws_misc"), G, build_gate, run_gate_ggsw, check_bits),
    pack_case(64), pack_case(16),
    Case("expand_seeded", ("fheaes_expand_lwe_seeded",), (), G, build_expand, run_expand, check_expand),
]
BY_NAME = {c.name: c for c in CASES}

# The entry points that take a context and a memspace and that no case above reaches, each with its reason.
LEFTOVERS = {
    # key uploads: what creates every case's Server; they run before there is any scratch to depend on
    "fheaes_upload_keys": "key upload", "fheaes_upload_keys_seeded": "key upload",
    # K6 alone: one kernel launch (and one table upload) that the composed call of the table runs as part of its schedule
    "fheaes_inv_mix_columns_batch": "K6 alone: the gather aes_decrypt runs", "fheaes_xts_tweaks": "K6 alone: the gather aes_xts_decrypt runs",
    "fheaes_xts_whiten": "K6 alone: the whitening aes_xts_decrypt runs", "fheaes_mac_link": "K6 alone: the link aes_cbc_mac_streams runs",
    "fheaes_cmac_double": "K6 alone: the gather aes_cmac_subkeys runs", "fheaes_kw_link": "K6 alone: the link aes_key_unwrap runs",
    "fheaes_packed_mod_switch": "K6 alone: the switch pack at width 16 runs",
    # the packed round-key source of a schedule whose LWE form is in the table: one resolver (resolve_keys) in front of the same host code,
    # and the packed source itself is reached by the three _keyed_packed ciphers
    "fheaes_aes_xts_decrypt_packed": "packed source of aes_xts_decrypt", "fheaes_aes_public_keyed_packed": "packed source of aes_public_keyed",
    "fheaes_aes_decrypt_public_keyed_packed": "packed source of aes_decrypt_public_keyed", "fheaes_aes_cbc_mac_keyed_packed": "packed source of aes_cbc_mac_streams",
    "fheaes_aes_ccm_open_keyed_packed": "packed source of aes_ccm_decrypt", "fheaes_aes_cmac_subkeys_keyed_packed": "packed source of aes_cmac_subkeys",
    "fheaes_aes_cmac_keyed_packed": "packed source of aes_cmac_verify", "fheaes_aes_kw_unwrap_keyed_packed": "packed source of aes_key_unwrap",
}
