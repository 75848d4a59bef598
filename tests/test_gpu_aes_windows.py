"""The block ciphers with their rounds rolled over windows of blocks (fheaes_aes_set_window, include/fheaes.h; the cut is modelled in
test_aes_windows_cpu.py).  Any window in 1..n is a correct schedule, so the toy parameters run every shape of segment with forced
windows: a launch inside one step, a launch across a step boundary with equal and with different LUT sets, a short last launch.  The
yardstick is the schedule without windows (FHEAES_AES_WINDOW_OFF), word for word, and that schedule is held to aes_model.AesModel and
to FIPS-197.  At PARAM_OPT the automatic window runs at the smallest batches that roll: 13 blocks (window 12, every launch crosses a step
boundary) and 32 blocks (window 24)."""
import numpy as np
import pytest

from aes_model import AesModel
from aes_vectors import BASE, FIPS_C, MASK128, NR, own_client
from gpu_support import dev, host, tc, toy_server  # noqa: F401
from tfhe_aes_amd import _native, aes_clear
from tfhe_aes_amd.server import Server

pytestmark = pytest.mark.gpu

OFF = _native.AES_WINDOW_OFF
PTS = [BASE, 0, MASK128, 0x3243F6A8885A308D313198A2E0370734, BASE + 1]
N = len(PTS)
CIPHERS = ("aes_encrypt", "aes_decrypt", "aes_decrypt_equivalent")
KOB = [0, 1, 1, 0, 1]


def steps_of(cipher, bits):
    return 2 * NR[bits] - 1 if cipher == "aes_decrypt" else NR[bits]


def run(srv, cipher, d_keys, state, *extra):
    """one in-place call on a fresh device copy of `state`; returns (words, the context's profile of the call)"""
    eng = srv.engine
    d = dev(state)
    eng.profile_enable(True)
    eng.profile_reset()
    getattr(srv, cipher)(d_keys, *extra, d)
    srv.synchronize()
    prof = eng.profile_read()
    eng.profile_enable(False)
    return host(d), prof


@pytest.fixture(scope="module")
def win_server(toy):
    """a context of its own: its window setting, profile counters and noise level are this module's"""
    srv = Server(toy.keys, device=0)
    yield srv
    srv.engine.close()


@pytest.fixture(scope="module")
def cases(toy, tc):
    """per key size, computed once on a context that only ever runs without windows: the round keys (both kinds, resident), five input
    blocks, and for every cipher its input, the words of the schedule without windows and that call's blind-rotation profile; the
    context's noise level after all of it"""
    srv = Server(toy.keys, device=0)
    srv.engine.aes_set_window(OFF)
    out = {}
    try:
        for bits in (128, 256):
            key = FIPS_C[bits][0]
            rk = srv.aes_key_expansion(tc.encrypt_aes_key(key))
            dw = srv.aes_decryption_round_keys(rk)
            d_rk, d_dw = dev(rk), dev(dw)
            st = np.stack([tc.encrypt_u128(v) for v in PTS])
            assert srv.engine.aes_window(N, NR[bits]) == 0
            enc, p_enc = run(srv, "aes_encrypt", d_rk, st)
            dec, p_dec = run(srv, "aes_decrypt", d_rk, enc)
            eq, p_eq = run(srv, "aes_decrypt_equivalent", d_dw, enc)
            out[bits] = {"key": key, "rk": rk, "dw": dw, "d_rk": d_rk, "d_dw": d_dw,
                         "aes_encrypt": (d_rk, st, enc, p_enc), "aes_decrypt": (d_rk, enc, dec, p_dec), "aes_decrypt_equivalent": (d_dw, enc, eq, p_eq)}
        out["noise"] = srv.engine.noise_level_seen()
    finally:
        srv.engine.close()
    return out


# ---- the yardstick itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [128, 256])
def test_toy_schedule_without_windows_is_the_model_on_every_block(toy, cases, tc, bits):
    c = cases[bits]
    model = AesModel(toy.oracle)
    _, st, enc, p_enc = c["aes_encrypt"]
    _, _, dec, p_dec = c["aes_decrypt"]
    _, _, eq, p_eq = c["aes_decrypt_equivalent"]
    assert np.array_equal(enc, model.encrypt(c["rk"], st))
    assert np.array_equal(dec, model.decrypt(c["rk"], enc))
    assert np.array_equal(eq, model.decrypt_equivalent(c["dw"], enc))
    assert [tc.decrypt_u128(enc[b]) for b in range(N)] == [aes_clear.aes_encrypt_block(c["key"], v) for v in PTS]
    assert [tc.decrypt_u128(dec[b]) for b in range(N)] == PTS and [tc.decrypt_u128(eq[b]) for b in range(N)] == PTS
    for cipher, prof in (("aes_encrypt", p_enc), ("aes_decrypt", p_dec), ("aes_decrypt_equivalent", p_eq)):
        t = steps_of(cipher, bits)
        assert prof["blind_rotate"]["launches"] == t and prof["blind_rotate"]["units"] == t * N * 128


# ---- forced windows, toy parameters ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 3, 4, 5])
@pytest.mark.parametrize("bits", [128, 256])
def test_toy_forced_window_gives_the_words_of_the_schedule_without_windows(cases, win_server, bits, w):
    eng = win_server.engine
    eng.aes_set_window(w)
    try:
        for cipher in CIPHERS:
            d_keys, st, want, p_off = cases[bits][cipher]
            t = steps_of(cipher, bits)
            assert eng.aes_window(N, t) == w
            got, prof = run(win_server, cipher, d_keys, st)
            assert np.array_equal(got, want), "%s, window %d: %d words differ" % (cipher, w, int((got != want).sum()))
            assert prof["blind_rotate"]["launches"] == -(-t * N // w)
            for stage in ("keyswitch", "blind_rotate", "pfpks", "ggsw_fft", "vertical_packing"):
                assert prof[stage]["units"] == p_off[stage]["units"], stage
            assert prof["linear"]["units"] == p_off["linear"]["units"]                  # every block-round through one linear layer
        assert eng.noise_level_seen() == cases["noise"]
    finally:
        eng.aes_set_window(0)


def test_toy_window_setting_is_clamped_and_per_context(cases, win_server, toy_server):
    eng = win_server.engine
    try:
        assert eng.aes_window(N, 10) == 0                      # automatic: the toy parameters have no paired form
        eng.aes_set_window(7)
        assert eng.aes_window(N, 10) == N and eng.aes_window(9, 10) == 7 and eng.aes_window(1000, 10) == 7
        eng.aes_set_window(1000)
        assert eng.aes_window(1000, 10) == 256                 # never more than 32,768 bits
        assert toy_server.engine.aes_window(N, 10) == 0        # another context is not affected
        eng.aes_set_window(OFF)
        assert eng.aes_window(N, 10) == 0
        d_keys, st, want, p_off = cases[128]["aes_encrypt"]
        got, prof = run(win_server, "aes_encrypt", d_keys, st)
        assert np.array_equal(got, want) and prof == {k: dict(v, ms=prof[k]["ms"]) for k, v in p_off.items()}
    finally:
        eng.aes_set_window(0)


@pytest.mark.parametrize("w", [3, 4])
def test_toy_keyed_calls_offset_the_key_table_by_the_segment(toy, cases, win_server, tc, w):
    """two keys, blocks [0, 1, 1, 0, 1]: a segment that starts at block b must read key_of_block from b on.  Key 0 is the single-key
    case's, so its blocks must carry that case's words (which are the model's); all blocks: the keyed call without windows, and AES"""
    eng = win_server.engine
    c = cases[128]
    key1 = bytes(range(16, 32))
    rk1 = win_server.aes_key_expansion(tc.encrypt_aes_key(key1))
    keys = [c["key"], key1]
    rk = np.stack([c["rk"], rk1])
    d_rk, d_dw = dev(rk), dev(win_server.aes_decryption_round_keys_many(rk))
    st = c["aes_encrypt"][1]
    want = {}
    try:
        for setting in (OFF, w):
            eng.aes_set_window(setting)
            enc, p = run(win_server, "aes_encrypt_keyed", d_rk, st, KOB)
            assert p["blind_rotate"]["launches"] == (10 if setting == OFF else -(-10 * N // w))
            dec, _ = run(win_server, "aes_decrypt_keyed", d_rk, enc, KOB)
            eq, _ = run(win_server, "aes_decrypt_equivalent_keyed", d_dw, enc, KOB)
            if setting == OFF:
                want = {"enc": enc, "dec": dec, "eq": eq}
                continue
            for name, got in (("enc", enc), ("dec", dec), ("eq", eq)):
                assert np.array_equal(got, want[name]), "%s, window %d: %d words differ" % (name, w, int((got != want[name]).sum()))
    finally:
        eng.aes_set_window(0)
    zero = [b for b, k in enumerate(KOB) if k == 0]
    assert np.array_equal(want["enc"][zero], c["aes_encrypt"][2][zero])
    assert [tc.decrypt_u128(want["enc"][b]) for b in range(N)] == [aes_clear.aes_encrypt_block(keys[k], v) for k, v in zip(KOB, PTS)]
    assert [tc.decrypt_u128(want["dec"][b]) for b in range(N)] == PTS and [tc.decrypt_u128(want["eq"][b]) for b in range(N)] == PTS


def test_toy_host_memory_call_with_a_window(cases, win_server):
    eng = win_server.engine
    _, st, want, _ = cases[256]["aes_decrypt"]
    eng.aes_set_window(3)
    try:
        got = win_server.aes_decrypt(cases[256]["rk"], st.copy())
    finally:
        eng.aes_set_window(0)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)


# ---- PARAM_OPT, the automatic window --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opt_keys(opt):
    oc = own_client(opt)
    srv = Server(opt.keys, device=0, engine=opt.engine())
    key = FIPS_C[128][0]
    d_ek = dev(oc.encrypt_aes_key(key))
    d_rk = srv.aes_key_expansion(d_ek)
    srv.synchronize()
    return srv, oc, key, d_rk


@pytest.mark.parametrize("cipher, n, window", [("aes_encrypt", 13, 12), ("aes_encrypt", 32, 24), ("aes_decrypt", 13, 12)])
def test_param_opt_automatic_window_matches_the_schedule_without_windows(opt_keys, cipher, n, window):
    import torch

    srv, oc, key, d_rk = opt_keys
    eng = srv.engine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    t = steps_of(cipher, 128)
    plan = _native.aes_window_plan(n, t, cus, 4)
    pts = [(BASE + 0x9E3779B97F4A7C15 * i) & MASK128 for i in range(n)]
    clear_in = pts if cipher == "aes_encrypt" else [aes_clear.aes_encrypt_block(key, v) for v in pts]
    clear_out = [aes_clear.aes_encrypt_block(key, v) for v in pts] if cipher == "aes_encrypt" else pts
    st = np.stack([oc.encrypt_u128(v) for v in clear_in])
    try:
        eng.aes_set_window(0)
        assert eng.k2_plan(n * 128)["form"] == 2
        assert eng.aes_window(n, t) == plan["window"]
        if cus == 256:
            assert plan["window"] == window
        got, prof = run(srv, cipher, d_rk, st)
        assert prof["blind_rotate"]["launches"] == plan["launches"] and prof["blind_rotate"]["units"] == t * n * 128
        eng.aes_set_window(OFF)
        assert eng.aes_window(n, t) == 0
        want, p_off = run(srv, cipher, d_rk, st)
        assert p_off["blind_rotate"]["launches"] == t and p_off["blind_rotate"]["units"] == t * n * 128
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        assert [oc.decrypt_u128(got[b]) for b in range(n)] == clear_out
    finally:
        eng.aes_set_window(0)


def test_param_opt_context_without_the_paired_kernel_does_not_roll(opt_keys):
    srv, oc, key, d_rk = opt_keys
    eng = srv.engine
    n = 13
    pts = [(BASE + i) & MASK128 for i in range(n)]
    st = np.stack([oc.encrypt_u128(v) for v in pts])
    try:
        eng.aes_set_window(OFF)
        want, _ = run(srv, "aes_encrypt", d_rk, st)
        eng.aes_set_window(0)
        eng.k2_set_forms(False, True)
        assert eng.aes_window(n, 10) == 0 and eng.k2_plan(n * 128)["form"] == 1
        got, prof = run(srv, "aes_encrypt", d_rk, st)
        assert prof["blind_rotate"]["launches"] == 10
        assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
        eng.k2_set_forms(True, True)
        assert eng.aes_window(n, 10) == _native.aes_window_plan(n, 10, eng_cus(), 4)["window"]
    finally:
        eng.k2_set_forms(True, True)
        eng.aes_set_window(0)
    assert [oc.decrypt_u128(got[b]) for b in range(n)] == [aes_clear.aes_encrypt_block(key, v) for v in pts]


def eng_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count
