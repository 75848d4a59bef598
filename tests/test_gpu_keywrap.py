"""AES key unwrap (RFC 3394) on the MI355X.  The link alone (fheaes_kw_link) on edge words inside guard rows against keywrap.np_link;
fheaes_aes_kw_unwrap_keyed word for word against keywrap.compose_unwrap -- np_link plus entry points older than the call -- so every
comparison is array_equal; payloads and validity bits from aes_clear and the vectors of RFC 3394 section 4.

n = 8 semiblocks is left to the link test and to the CPU model (test_keywrap_cpu.py): its 48 serial cipher passes add nothing the
kernel can get wrong that the link at n = 8 and the calls at n = 2, 3, 4 do not show."""
import numpy as np
import pytest

import keywrap
import noise_model as nm
from aes_model import noise
from gpu_support import SENTINEL, dev, guarded, guards_intact, host, oc, opt_server, settled, tc, toy_server  # noqa: F401
from test_gpu_cmac import _edge_l
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import ServerGroup

pytestmark = pytest.mark.gpu

_results = {}


def _dec(tc, keys):
    """[n_keys][8 n][8][kN+1] -> the payloads as bytes"""
    return [bytes(k.tolist()) for k in tc.decrypt_bytes(keys)]


def _flip(data, i, bit=0x01):
    return data[:i] + bytes([data[i] ^ bit]) + data[i + 1:]


# ---- 1. the link alone ---------------------------------------------------------------------------------------------------------------------
def _edge_rows(p, n_keys, rows, seed):
    """random [n_keys][rows][kN+1] with the edge words 0, 2^64 - 1, 2^63 and 2^63 - 1 where test_gpu_cmac._edge_l places them, in every
    run of 128 rows"""
    runs = [_edge_l(p, n_keys, seed + i) for i in range((rows + 127) // 128)]
    return np.ascontiguousarray(np.concatenate(runs, axis=1)[:, :rows])


def _link_on_device(eng, p, n, state, regs, s, wrapped):
    sbuf, srows = guarded(len(state) * 128, p.big1)
    rbuf, rrows = guarded(len(state) * 64 * n, p.big1)
    if s > 0:                                                              # the load writes every word: it starts from the sentinels
        srows.copy_(dev(state.reshape(-1, p.big1)))
        rrows.copy_(dev(regs.reshape(-1, p.big1)))
        settled(rrows)
    eng.kw_link(srows.view(state.shape), rrows.view(regs.shape), n, s, wrapped)
    eng.synchronize()
    assert guards_intact(sbuf) and guards_intact(rbuf)
    return host(srows).reshape(state.shape), host(rrows).reshape(regs.shape)


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_link_is_the_numpy_model(toy, n, n_keys):
    """load, a shuffle inside a sweep, the shuffle where the register wraps from 1 to n, and the unload"""
    p = toy.params
    eng = _native.Engine(p, device=0)                                      # no keys: the link needs none
    try:
        rng = np.random.default_rng(0x3394 + 16 * n + n_keys)
        wrapped = [rng.bytes(8 * (n + 1)) for _ in range(n_keys)]
        state = _edge_rows(p, n_keys, 128, 0x5A + n).reshape(n_keys, 16, 8, p.big1)
        regs = _edge_rows(p, n_keys, 64 * n, 0xA5 + n).reshape(n_keys, 8 * n, 8, p.big1)
        assert keywrap.register(n, n - 1) == 1 and keywrap.register(n, n) == n
        assert eng.noise_level_seen() == (0, 5)
        for s, level in ((0, 1), (6 * n, 2), (1, 3), (n, 3)):
            want_state, want_regs = keywrap.np_link(state, regs, n, s, wrapped)
            got_state, got_regs = _link_on_device(eng, p, n, state, regs, s, wrapped if s == 0 else None)
            assert np.array_equal(got_state, want_state), "step %d: %d state words differ" % (s, int((got_state != want_state).sum()))
            assert np.array_equal(got_regs, want_regs), "step %d: %d register words differ" % (s, int((got_regs != want_regs).sum()))
            assert eng.noise_level_seen() == (level, 5), s
            h_state, h_regs = state.copy(), regs.copy()                    # host arrays take the staging path: the same words
            eng.kw_link(h_state, h_regs, n, s, wrapped if s == 0 else None)
            assert np.array_equal(h_state, want_state) and np.array_equal(h_regs, want_regs), s
    finally:
        eng.close()


def test_link_beyond_the_grid_cap(toy):
    """one key more than the 256 the launch gives the grid dimension that indexes keys at PARAM_TOY (mac_link's cap): the loop's second pass"""
    p, n, s, n_keys = toy.params, 2, 7, 257
    assert min((128 * p.big1 + 255) // 256, 64) == 64 and 16384 // 64 == n_keys - 1
    eng = _native.Engine(p, device=0)
    try:
        rng = np.random.default_rng(0x101)
        state = rng.integers(0, 1 << 64, (n_keys, 16, 8, p.big1), dtype=np.uint64)
        regs = rng.integers(0, 1 << 64, (n_keys, 8 * n, 8, p.big1), dtype=np.uint64)
        want_state, want_regs = keywrap.np_link(state, regs, n, s, None)
        got_state, got_regs = _link_on_device(eng, p, n, state, regs, s, None)
        assert np.array_equal(got_state, want_state) and np.array_equal(got_regs, want_regs)
        assert not np.array_equal(got_state[256], state[256])
    finally:
        eng.close()


# ---- KEKs and the cases --------------------------------------------------------------------------------------------------------------------
KEKS_128 = (keywrap.KEK[:16], bytes(range(0x40, 0x50)), bytes(range(0xC0, 0xD0)))
PAYLOADS_128 = [bytes(range(0x10 * i, 0x10 * i + 16)) for i in range(1, 6)]
KEK_OF_128 = [0, 2, 1, 2, 0]
V41, V46 = keywrap.vector("4.1"), keywrap.vector("4.6")
# (KEK bits, n) -> (KEKs, kek_of_key or None, payloads): 3 KEKs mixed over 5 keys, vector 4.1 first; one key of 24 bytes; vector 4.6
CASES = {
    (128, 2): (KEKS_128, KEK_OF_128, [V41[1]] + PAYLOADS_128[1:]),
    (192, 3): ((bytes(range(0x80, 0x98)),), None, [bytes(range(0x21, 0x39))]),
    (256, 4): ((V46[0],), None, [V46[1]]),
}


def wrapped_of(case):
    keks, kek_of, payloads = CASES[case]
    return [aes_clear.key_wrap(keks[kek_of[i] if kek_of else 0], d) for i, d in enumerate(payloads)]


@pytest.fixture(scope="module")
def keks(toy_server, tc):
    """the KEKs' decryption round keys, made on the GPU"""
    def many(ks):
        return toy_server.aes_decryption_round_keys_many(toy_server.aes_key_expansion_many(np.stack([tc.encrypt_aes_key(k) for k in ks])))
    return {case: many(CASES[case][0]) for case in CASES}


def unwrap_case(case, toy_server, tc, keks):
    if case not in _results:
        wrapped, kek_of = wrapped_of(case), CASES[case][1]
        _results[case] = (toy_server.aes_key_unwrap(keks[case], wrapped, kek_of), keywrap.compose_unwrap(toy_server, tc, keks[case], kek_of, wrapped))
    return _results[case]


# ---- 2. the call is the composition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "%d-%d" % c)
def test_toy_unwrap_is_the_composition(toy, toy_server, tc, keks, case):
    p, (bits, n) = toy.params, case
    payloads = CASES[case][2]
    wrapped = wrapped_of(case)
    if case == (128, 2):
        assert wrapped[0] == V41[2]
    if case == (256, 4):
        assert wrapped[0] == V46[2]
    (keys, valid), (want_keys, want_valid) = unwrap_case(case, toy_server, tc, keks)
    assert keys.shape == (len(payloads), 8 * n, 8, p.big1) and valid.shape == (len(payloads), p.big1) and keys.dtype == valid.dtype == np.uint64
    assert np.array_equal(keys, want_keys), "%d key words differ" % int((keys != want_keys).sum())
    assert np.array_equal(valid, want_valid), "%d valid words differ" % int((valid != want_valid).sum())
    assert _dec(tc, keys) == payloads
    assert tc.decrypt_bits(valid).tolist() == [1] * len(payloads)
    assert _native.aes_kw_plan(bits, n, len(payloads))["steps"] == 6 * n


# ---- 3. rejection, and a key put to work ---------------------------------------------------------------------------------------------------
def test_toy_rejection_and_onboarding(toy, toy_server, tc, keks):
    case = (128, 2)
    kek, payload, right = V41
    wrapped = [right, _flip(right, 3, 0x20), _flip(right, 16 + 5, 0x02), right]                # C[0] and C[2] with a flipped bit
    kek_of = [0, 0, 0, 1]                                                                      # the last one under the wrong KEK
    want_bits = [int(aes_clear.key_unwrap(KEKS_128[k], w)[0]) for k, w in zip(kek_of, wrapped)]
    assert want_bits == [1, 0, 0, 0]
    keys, valid = toy_server.aes_key_unwrap(keks[case], wrapped, kek_of)
    assert tc.decrypt_bits(valid).tolist() == want_bits
    assert _dec(tc, keys) == [aes_clear.key_unwrap(KEKS_128[k], w)[1] for k, w in zip(kek_of, wrapped)]      # NOT gated on valid
    assert np.array_equal(keys[0], unwrap_case(case, toy_server, tc, keks)[0][0][0])
    rk = toy_server.aes_key_expansion_many(np.ascontiguousarray(keys[:1]))
    iv = 0xF0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF
    stream = toy_server.aes_ctr(rk[0], iv, 0, 2)
    assert [int.from_bytes(bytes(b.tolist()), "big") for b in tc.decrypt_bytes(stream)] == aes_clear.ctr_keystream(payload, iv, 0, 2)


# ---- 4. equivalent paths -------------------------------------------------------------------------------------------------------------------
def test_toy_equivalent_paths(toy, toy_server, tc, keks):
    """a packed KEK store, resident tensors inside guard rows, one KEK without kek_of_key, a ServerGroup of two contexts, and the unwrap
    straight into a packed store: the same words"""
    p, case = toy.params, (128, 2)
    wrapped, kek_of, payloads = wrapped_of(case), CASES[case][1], CASES[case][2]
    (keys, valid), _ = unwrap_case(case, toy_server, tc, keks)
    packed = toy_server.pack_round_keys(keks[case])
    p_keys, p_valid = toy_server.aes_key_unwrap(packed, wrapped, kek_of)
    u_keys, u_valid = toy_server.aes_key_unwrap(toy_server.unpack_round_keys(packed), wrapped, kek_of)
    assert np.array_equal(p_keys, u_keys) and np.array_equal(p_valid, u_valid)
    assert _dec(tc, p_keys) == payloads and tc.decrypt_bits(p_valid).tolist() == [1] * 5
    kbuf, krows = guarded(5 * 128, p.big1)
    vbuf, vrows = guarded(5, p.big1)
    d_keys, d_valid = toy_server.aes_key_unwrap(dev(keks[case]), wrapped, kek_of, out=krows.view(5, 16, 8, p.big1), valid_out=vrows)
    toy_server.synchronize()
    assert d_keys.is_cuda and guards_intact(kbuf) and guards_intact(vbuf)
    assert np.array_equal(host(d_keys), keys) and np.array_equal(host(d_valid), valid)
    mine = [i for i, k in enumerate(kek_of) if k == 2]                                         # the keys of KEK 2, under that KEK alone
    one_keys, one_valid = toy_server.aes_key_unwrap(np.ascontiguousarray(keks[case][2]), [wrapped[i] for i in mine])
    assert np.array_equal(one_keys, keys[mine]) and np.array_equal(one_valid, valid[mine])
    group = ServerGroup(toy.keys, devices=(0, 0))
    try:
        g_keys, g_valid = group.aes_key_unwrap(keks[case], wrapped, kek_of)
        g_store, g_ok = group.aes_key_unwrap_packed(keks[case], wrapped, kek_of, chunk=2)
    finally:
        for s in group.servers:
            s.engine.close()
    assert np.array_equal(g_keys, keys) and np.array_equal(g_valid, valid)
    store, ok = toy_server.aes_key_unwrap_packed(keks[case], wrapped, kek_of, chunk=2)         # 5 keys in chunks of 2, 2 and 1
    want = toy_server.pack_round_keys(toy_server.aes_key_expansion_many(keys))
    assert store.key_bits == 128 and store.n_keys == 5
    assert np.array_equal(store.data, want.data) and np.array_equal(ok, valid)
    assert np.array_equal(g_store.data, want.data) and np.array_equal(g_ok, valid)


# ---- 5. keys_out is fresh ------------------------------------------------------------------------------------------------------------------
def test_toy_keys_out_is_fresh(toy, toy_server, tc, keks):
    """every word of keys_out is the output of an 8-bit identity WoPBS on its own byte: the band test_gpu_noise.py holds such outputs to"""
    case = (128, 2)
    (keys, _), _ = unwrap_case(case, toy_server, tc, keks)
    M = nm.NoiseModel.of_client(toy.client)
    values = np.array([list(d) for d in CASES[case][2]], dtype=np.int64)                       # [5][16]
    n = M.wopbs_independent(values.size, 8)
    assert nm.rejects_doubling(n)
    nm.assert_noise(noise(tc, keys), M.wopbs(8, values)[:, :, None], n, "unwrapped keys toy", left_out=M.wopbs_left_out())


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_toy_errors_leave_the_outputs_untouched(toy, toy_server, tc, keks):
    p = toy.params
    eng = toy.engine()
    lib, h, D = eng._lib, eng._h, _native.DEVICE
    d_dw = dev(keks[(128, 2)])
    kbuf, krows = guarded(2 * 128, p.big1)
    vbuf, vrows = guarded(2, p.big1)
    sbuf, srows = guarded(2 * 128, p.big1)
    dw, ko, vo, so = d_dw.data_ptr(), krows.data_ptr(), vrows.data_ptr(), srows.data_ptr()
    u32 = lambda *x: np.array(x, dtype=np.uint32).ctypes.data_as(_native._u32p)
    u8 = lambda x: np.array(x, dtype=np.uint8).ctypes.data_as(_native._u8p)
    base = dict(dw=dw, bits=128, n_keks=3, n=2, kok=u32(0, 2), sb=2, wr=u8([0] * 48), keys=ko, ok=vo)

    def call(fn=lib.fheaes_aes_kw_unwrap_keyed, **kw):
        x = dict(base, **kw)
        return fn(h, x["dw"], x["bits"], x["n_keks"], x["n"], x["kok"], x["sb"], x["wr"], x["keys"], x["ok"], D)

    for name in ("dw", "kok", "wr", "keys", "ok"):                                             # kek_of_key is optional with one KEK only
        assert call(**{name: None}) == -1, name
    for sb in (0, 1, 9):
        assert call(sb=sb) == -1 and b"semiblocks" in lib.fheaes_last_error(h)
    assert call(n=4097) == -1 and b"at most" in lib.fheaes_last_error(h)
    assert call(n_keks=0) == -1 and call(n_keks=65537) == -1 and b"n_keys" in lib.fheaes_last_error(h)
    assert call(kok=u32(0, 3)) == -1 and b"key_of_block" in lib.fheaes_last_error(h)
    for bits in (0, 100, 512):
        assert call(bits=bits) == -1 and b"key_bits" in lib.fheaes_last_error(h)
    assert call(keys=dw) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(ok=dw) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(ok=ko) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert call(fn=lib.fheaes_aes_kw_unwrap_keyed_packed, sb=9) == -1 and call(fn=lib.fheaes_aes_kw_unwrap_keyed_packed, keys=None) == -1
    assert call(n=0) == 0

    link = lambda state=so, regs=ko, n=2, sb=2, step=1, wr=None: lib.fheaes_kw_link(h, state, regs, n, sb, step, wr, D)
    assert link(state=None) == -1 and link(regs=None) == -1
    assert link(step=0) == -1                                                                  # the load reads `wrapped`
    assert link(step=13) == -1 and b"step" in lib.fheaes_last_error(h)
    assert link(sb=1) == -1 and link(sb=9) == -1 and link(n=4097) == -1
    assert link(regs=so) == -1 and b"overlap" in lib.fheaes_last_error(h)
    assert link(n=0) == 0
    for bad in (lambda: toy_server.aes_key_unwrap(d_dw, [bytes(24), bytes(32)], [0, 0]), lambda: toy_server.aes_key_unwrap(d_dw, [bytes(24)]),
                lambda: toy_server.aes_key_unwrap(d_dw, [bytes(24)], [3]), lambda: toy_server.aes_key_unwrap(d_dw, [bytes(16)], [0]),
                lambda: toy_server.aes_key_unwrap_packed(d_dw, [bytes(48)], [0]), lambda: toy_server.aes_key_unwrap_packed(d_dw, [], [])):
        with pytest.raises(ValueError):
            bad()
    toy_server.synchronize()
    assert bool((krows == SENTINEL).all().item()) and guards_intact(kbuf)
    assert bool((vrows == SENTINEL).all().item()) and guards_intact(vbuf)
    assert bool((srows == SENTINEL).all().item()) and guards_intact(sbuf)
    e_keys, e_valid = toy_server.aes_key_unwrap(keks[(128, 2)], [], [])
    assert e_keys.shape == (0, 16, 8, p.big1) and e_valid.shape == (0, p.big1)
    fresh = _native.Engine(p, device=0)                                                        # a context without keys
    try:
        with pytest.raises(_native.FheAesError) as e:
            fresh.aes_kw_unwrap_keyed(keks[(128, 2)], 128, 3, [0], 2, [bytes(24)], np.empty((1, 16, 8, p.big1), dtype=np.uint64),
                                      np.empty((1, p.big1), dtype=np.uint64))
        assert e.value.code == -2
    finally:
        fresh.close()


# ---- 7. one call at PARAM_OPT --------------------------------------------------------------------------------------------------------------
def test_opt_unwrap_of_the_rfc_vector(opt, opt_server, oc):
    """vector 4.1 and the same wrapped key with one bit flipped, two keys in one call"""
    kek, payload, wrapped = V41
    d_rk = opt_server.aes_key_expansion(dev(oc.encrypt_aes_key(kek)))
    d_dw = opt_server.aes_decryption_round_keys(d_rk)
    bad = _flip(wrapped, 23, 0x80)
    keys, valid = opt_server.aes_key_unwrap(d_dw, [wrapped, bad])
    opt_server.synchronize()
    assert keys.is_cuda and tuple(keys.shape) == (2, 16, 8, opt.params.big1)
    assert oc.decrypt_bits(host(valid)).tolist() == [1, 0]
    got = _dec(oc, host(keys))
    assert got[0] == payload and got[1] == aes_clear.key_unwrap(kek, bad)[1]
