"""tools/measure.py on the GPU, toy parameters: the timed loop resets a job before every run and leaves its last output in place, the
profiled call reports one call's counters, the device-event loop hands the engine's stream back.  What is inside the timed interval is
test_tools_measure_cpu.py's; here the loops meet a real engine, torch's stream and real events.  Loaded by path, as there."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from aes_vectors import FIPS_C, FIPS_C_PT
from gpu_support import dev, host, tc, toy_server  # noqa: F401
from tfhe_aes_amd import aes_clear

pytestmark = pytest.mark.gpu

spec = importlib.util.spec_from_file_location("tools_measure", Path(__file__).resolve().parent.parent / "tools" / "measure.py")
measure = importlib.util.module_from_spec(spec)
spec.loader.exec_module(measure)

BYTES = [0x00, 0x01, 0x53, 0x7F, 0x80, 0xA7, 0xFE, 0xFF, 0x10, 0x3C, 0x52, 0x63, 0x9A, 0xC4, 0xE1, 0x2B]


@pytest.fixture(scope="module")
def work(toy_server, tc):
    """name -> (run, reset) on resident tensors: an in-place one-block aes_encrypt of the FIPS-197 C.1 plaintext and an in-place S-Box on
    16 bytes, each with a reset that copies its input back; and the tensors they work on"""
    eng = toy_server.engine
    key = FIPS_C[128][0]
    d_rk = dev(toy_server.aes_key_expansion(tc.encrypt_aes_key(key)))
    block_in, bytes_in = tc.encrypt_u128(FIPS_C_PT), tc.encrypt_bytes(BYTES)
    d_block_in, d_bytes_in = dev(block_in), dev(bytes_in)
    d_block, d_bytes = dev(np.zeros_like(block_in)), dev(np.zeros_like(bytes_in))
    return {"aes_encrypt": (lambda: eng.aes_encrypt(d_rk, d_block, 1), lambda: d_block.copy_(d_block_in)),
            "sbox": (lambda: eng.sbox(d_bytes, len(BYTES), False), lambda: d_bytes.copy_(d_bytes_in))}, d_block, d_bytes


def sbox_verifies(eng, tc, jobs, d_bytes):
    import torch

    run, reset = jobs["sbox"]
    reset()
    torch.cuda.synchronize()
    run()
    eng.synchronize()
    return list(tc.decrypt_bytes(host(d_bytes))) == [aes_clear.SBOX[v] for v in BYTES]


def test_wall_loop_resets_before_every_run(toy_server, tc, work):
    jobs, d_block, d_bytes = work
    times = measure.wall(toy_server.engine, jobs, warmup=1, steps=2)
    assert list(times) == ["aes_encrypt", "sbox"]
    for name, ts in times.items():
        assert len(ts) == 2 and all(t > 0 for t in ts), (name, ts)
    # three runs in place: without the reset this would be the third iterate of the cipher
    assert tc.decrypt_u128(host(d_block)) == FIPS_C[128][1]
    assert list(tc.decrypt_bytes(host(d_bytes))) == [aes_clear.SBOX[v] for v in BYTES]


def test_profiled_call_counts_one_call(toy_server, work):
    """aes_encrypt_schedule: 9 + 1 steps of 128 bits, one chunk each, and the toy parameters do not roll rounds over windows: 10
    blind-rotation launches per call, and the same 10 for the second call because the counters are reset first"""
    jobs, _, _ = work
    eng = toy_server.engine
    first = measure.profiled(eng, *jobs["aes_encrypt"])
    second = measure.profiled(eng, *jobs["aes_encrypt"])
    print("blind_rotate launches:", first["blind_rotate"]["launches"], second["blind_rotate"]["launches"])
    assert first["blind_rotate"]["launches"] == second["blind_rotate"]["launches"]
    assert first["blind_rotate"]["launches"] == 10


def test_event_loop_hands_the_stream_back(toy_server, tc, work, monkeypatch):
    jobs, _, d_bytes = work
    eng = toy_server.engine
    handles = []
    set_stream = eng.set_stream
    monkeypatch.setattr(eng, "set_stream", lambda h: (handles.append(h), set_stream(h))[1])
    steps_seen = []
    times = measure.events(eng, {"sbox": jobs["sbox"][0]}, warmup=1, steps=2, reps=3, on_step=lambda i, of, last: steps_seen.append((i, of, list(last))))
    assert list(times) == ["sbox"] and len(times["sbox"]) == 2 and all(t > 0 for t in times["sbox"]), times
    assert steps_seen == [(1, 3, ["sbox"]), (2, 3, ["sbox"]), (3, 3, ["sbox"])]
    assert len(handles) == 2 and handles[0] and handles[1] is None      # a torch stream for the loop, then the engine's own again
    assert sbox_verifies(eng, tc, jobs, d_bytes)
