"""What the A/B tools under tools/ share: the PARAM_OPT session, the two timed loops, the profiled call, rows, checks and the JSON
record.  A tool is run as `python tools/<name>.py` and says `import measure`; what a number in profiles/*.json means is decided here.

The timing contract:

  wall      per step and per job: reset(), device synchronize, clock, run(), eng.synchronize(), clock.  The reset and the device
            synchronize are OUTSIDE the timed interval, the engine's synchronize is inside it (a device call only enqueues).  Every
            step runs every job of the call once, in the order of the dict, so jobs of one call alternate and a drift of the clocks
            meets them alike; jobs that must not alternate go into calls of their own.  The first `warmup` steps are dropped.
  events    the engine runs on a torch stream for the length of the call; per step and per job a pair of device events around `reps`
            back-to-back calls, milliseconds per call; every step times every job.  The engine is back on its own stream afterwards.
  profiled  one FURTHER call with the per-stage profile on (fheaes_profile_read: HIP events around every launch, which is why it is
            never one of the timed calls).  The counters are reset first, so they are this call's alone.

Seconds from `wall`, milliseconds from `events`, the raw profile_read dict from `profiled`: the tools round and filter.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from tfhe_aes_amd import PARAM_OPT, _build, _native  # noqa: E402
from tfhe_aes_amd.client import Client  # noqa: E402


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------
def progress(tool: str, msg: str) -> None:
    """to stderr: the JSON line on stdout stays alone, and a long run shows that it is alive"""
    print("[%s] %s" % (tool, msg), file=sys.stderr, flush=True)


def to_dev(a: np.ndarray):
    import torch

    d = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return d


def host(d) -> np.ndarray:
    return d.cpu().numpy().view(np.uint64)


def block_bytes(values) -> np.ndarray:
    return np.array([[(v >> (8 * (15 - b))) & 0xFF for b in range(16)] for v in values], dtype=np.uint8)


# ---- session ---------------------------------------------------------------------------------------------------------------------------
def session(seed: int, iv: int = 0, key: int = 0, library=None, allow_dev_build: bool = False):
    """(client, engine with the client's evaluation keys uploaded) at PARAM_OPT on device 0; library: the path of another build of
    libfheaes.so for the engine (_native.Engine), allow_dev_build: let it be a developer build"""
    client = Client(1, iv, key, params=PARAM_OPT, seed=seed)
    keys = client.server_keys()
    eng = _native.Engine(PARAM_OPT, device=0, allow_dev_build=allow_dev_build, library=library)
    eng.upload_keys(keys.ksk, keys.bsk, keys.pfpksk)
    return client, eng


# ---- the measurements ------------------------------------------------------------------------------------------------------------------
def wall(eng, jobs: dict, warmup: int, steps: int, sync=None, clock=time.perf_counter, on_step=None) -> dict:
    """jobs: name -> (run, reset).  {name: [seconds of each timed step]}; on_step(step, of, seconds the whole step took)"""
    if sync is None:
        import torch

        sync = torch.cuda.synchronize
    out = {k: [] for k in jobs}
    for i in range(warmup + steps):
        t_step = clock()
        for k, (run, reset) in jobs.items():
            reset()
            sync()
            t0 = clock()
            run()
            eng.synchronize()
            t1 = clock()
            if i >= warmup:
                out[k].append(t1 - t0)
        if on_step is not None:
            on_step(i + 1, warmup + steps, clock() - t_step)
    return out


def events(eng, jobs: dict, warmup: int, steps: int, reps: int, on_step=None) -> dict:
    """jobs: name -> run.  {name: [ms per call of each timed step]}; on_step(step, of, {name: ms per call in this step})"""
    import torch

    stream = torch.cuda.Stream()
    eng.set_stream(stream.cuda_stream)
    out = {k: [] for k in jobs}
    try:
        for i in range(warmup + steps):
            last = {}
            for k, run in jobs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                a.record(stream)
                for _ in range(reps):
                    run()
                b.record(stream)
                b.synchronize()
                last[k] = a.elapsed_time(b) / reps
                if i >= warmup:
                    out[k].append(last[k])
            if on_step is not None:
                on_step(i + 1, warmup + steps, last)
        stream.synchronize()
    finally:
        eng.set_stream(None)
    return out


def profiled(eng, run, reset=None, sync=None) -> dict:
    """profile_read of one call of `run`, after reset() and a device synchronize if a reset is given.  A `run` that raises leaves the
    profile on, as the tools always did: they end there"""
    if reset is not None:
        if sync is None:
            import torch

            sync = torch.cuda.synchronize
        reset()
        sync()
    eng.profile_enable(True)
    eng.profile_reset()
    run()
    prof = eng.profile_read()
    eng.profile_enable(False)
    return prof


def stage_ms(prof: dict, digits: int = 3) -> dict:
    return {k: round(v["ms"], digits) for k, v in prof.items()}


# ---- rows and checks -------------------------------------------------------------------------------------------------------------------
def row(seconds: list, blocks: int | None = None) -> dict:
    """the row of one job from its timed steps; blocks: how many blocks a call works on, for blocks_per_s"""
    med = statistics.median(seconds)
    rate = {} if blocks is None else {"blocks_per_s": round(blocks / med, 2)}
    return {**rate, "ms_median": round(1000 * med, 3), "ms_all": [round(1000 * t, 3) for t in seconds]}


def check(measured: float, predicted: float, bound: float | None) -> dict:
    """measured against a yardstick, both in ms; bound None: reported only"""
    return {"measured_ms": round(measured, 3), "predicted_ms": round(predicted, 3), "ratio": round(measured / predicted, 4), "bound": bound,
            "within_bound": None if bound is None else bool(measured <= bound * predicted)}


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def arg_parser(blocks: str | None = None, reps: int | None = None) -> argparse.ArgumentParser:
    """--steps, --warmup and --out, with --blocks / --reps in front where the tool gives their default"""
    ap = argparse.ArgumentParser()
    if blocks is not None:
        ap.add_argument("--blocks", default=blocks)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    if reps is not None:
        ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", default=None)
    return ap


def commit_id() -> str:
    try:
        return subprocess.run(["git", "-C", str(ROOT), "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip() + " + working tree"
    except Exception:
        return "unknown"


def header(tool: str, args) -> dict:
    """what every record starts with: which tool, which library and sources, which device, how many steps"""
    import torch

    return {"tool": tool, "params": PARAM_OPT.name, "version": _native.load_library().fheaes_version().decode(),
            "engine_src_sha256": _build.engine_source_hash(), "device": torch.cuda.get_device_name(0),
            "steps": args.steps, "warmup": args.warmup}


def emit(line: dict, out: str | None) -> None:
    """the record as one JSON line on stdout and, with --out, in that file"""
    text = json.dumps(line)
    print(text)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(text + "\n")


def exit_code(verified: bool, within_bounds: bool = True) -> int:
    """1: something did not verify; else 2: a bound was missed; else 0"""
    if not verified:
        return 1
    return 0 if within_bounds else 2
