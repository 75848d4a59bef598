"""tools/measure.py without a GPU: what the timed loop puts inside the timed interval and in which order the jobs run, the order of the
profiled call, rows, checks, exit codes and the record writer.  The module is loaded by path: tools/ is not on sys.path here
(tools/wire_formats.py and tests/wire_formats.py share a name).

The fakes: a clock that only the work advances (100 in a reset, 1 in a run, 2 in the engine's synchronize), so a timed sample is
exactly 3 if and only if the reset and the device synchronize are outside the interval and the engine's synchronize is inside it; and
one log that the jobs, the device synchronize and the engine all append to."""
import importlib.util
import json
from pathlib import Path

import pytest

spec = importlib.util.spec_from_file_location("tools_measure", Path(__file__).resolve().parent.parent / "tools" / "measure.py")
measure = importlib.util.module_from_spec(spec)
spec.loader.exec_module(measure)

PROFILE = {"blind_rotate": {"ms": 1.23456, "launches": 10, "units": 1280}, "linear": {"ms": 0.5, "launches": 0, "units": 0}}


class Fakes:
    def __init__(self):
        self.now = 0
        self.log = []

    def clock(self):
        return self.now

    def device_sync(self):
        self.log.append("device_sync")

    def job(self, name, fail=False):
        def run():
            self.log.append("run " + name)
            self.now += 1
            if fail:
                raise RuntimeError(name)

        def reset():
            self.log.append("reset " + name)
            self.now += 100

        return run, reset

    # the engine's side
    def synchronize(self):
        self.log.append("eng.synchronize")
        self.now += 2

    def profile_enable(self, on=True):
        self.log.append("enable(%s)" % on)

    def profile_reset(self):
        self.log.append("reset")

    def profile_read(self):
        self.log.append("read")
        return PROFILE


def test_wall_runs_every_job_once_per_step_in_order_and_times_run_plus_engine_synchronize():
    f = Fakes()
    steps_seen = []
    times = measure.wall(f, {"b": f.job("b"), "a": f.job("a")}, warmup=2, steps=3, sync=f.device_sync, clock=f.clock,
                         on_step=lambda i, of, s: steps_seen.append((i, of, s)))
    one = lambda k: ["reset " + k, "device_sync", "run " + k, "eng.synchronize"]  # noqa: E731
    assert f.log == (one("b") + one("a")) * 5
    assert times == {"b": [3, 3, 3], "a": [3, 3, 3]} and list(times) == ["b", "a"]
    assert steps_seen == [(i, 5, 206) for i in range(1, 6)]


def test_wall_with_one_job_gives_it_consecutive_runs():
    f = Fakes()
    times = measure.wall(f, {"only": f.job("only")}, warmup=1, steps=4, sync=f.device_sync, clock=f.clock)
    assert [e for e in f.log if e.startswith("run")] == ["run only"] * 5
    assert times == {"only": [3, 3, 3, 3]}


def test_profiled_call_order_and_raw_result():
    f = Fakes()
    run, reset = f.job("x")
    assert measure.profiled(f, run, reset, sync=f.device_sync) is PROFILE
    assert f.log == ["reset x", "device_sync", "enable(True)", "reset", "run x", "read", "enable(False)"]
    f.log.clear()
    assert measure.profiled(f, run) is PROFILE                       # no reset given: no reset, no device synchronize
    assert f.log == ["enable(True)", "reset", "run x", "read", "enable(False)"]


def test_profiled_call_that_raises_leaves_the_profile_on_as_the_tools_always_did():
    """none of the seven tools switched the profile off on the way out of a failing call (they end there); the shared call keeps that"""
    f = Fakes()
    run, reset = f.job("x", fail=True)
    with pytest.raises(RuntimeError):
        measure.profiled(f, run, reset, sync=f.device_sync)
    assert f.log == ["reset x", "device_sync", "enable(True)", "reset", "run x"]


def test_stage_ms_rounds_every_stage():
    assert measure.stage_ms(PROFILE) == {"blind_rotate": 1.235, "linear": 0.5}
    assert measure.stage_ms(PROFILE, 4) == {"blind_rotate": 1.2346, "linear": 0.5}


def test_row_rounds_to_microseconds_and_takes_the_median_of_odd_and_even_counts():
    odd = measure.row([0.0030004, 0.0010006, 0.0020004])
    assert odd == {"ms_median": 2.0, "ms_all": [3.0, 1.001, 2.0]} and list(odd) == ["ms_median", "ms_all"]
    assert measure.row([0.004, 0.001, 0.002, 0.0030009]) == {"ms_median": 2.5, "ms_all": [4.0, 1.0, 2.0, 3.001]}      # (2 + 3.0009) / 2 = 2.50045
    assert measure.row([0.5, 0.25], blocks=32) == {"blocks_per_s": 85.33, "ms_median": 375.0, "ms_all": [500.0, 250.0]}


def test_check_with_and_without_a_bound():
    assert measure.check(103.0004, 100.0, 1.03) == {"measured_ms": 103.0, "predicted_ms": 100.0, "ratio": 1.03, "bound": 1.03, "within_bound": False}
    assert measure.check(102.9, 100.0, 1.03)["within_bound"] is True
    free = measure.check(250.0, 100.0, None)
    assert free["within_bound"] is None and free["bound"] is None and free["ratio"] == 2.5


def test_exit_code_1_beats_2_beats_0():
    assert measure.exit_code(True) == 0 and measure.exit_code(True, True) == 0
    assert measure.exit_code(True, False) == 2
    assert measure.exit_code(False, True) == 1 and measure.exit_code(False, False) == 1


def test_emit_writes_the_same_single_line_to_stdout_and_to_out(tmp_path, capsys):
    line = {"tool": "t", "rows": {"a": [1, 2.5]}, "all_verified": True}
    out = tmp_path / "not" / "there" / "yet.json"
    measure.emit(line, str(out))
    printed = capsys.readouterr().out
    assert printed == out.read_text() and printed.endswith("\n") and printed.count("\n") == 1
    assert json.loads(printed) == line
    measure.emit(line, None)
    assert capsys.readouterr().out == printed


def test_arg_parser_defaults_are_the_tools_defaults():
    a = measure.arg_parser().parse_args([])
    assert (a.steps, a.warmup, a.out) == (5, 1, None) and not hasattr(a, "blocks") and not hasattr(a, "reps")
    b = measure.arg_parser(blocks="128,32", reps=10).parse_args(["--steps", "3", "--out", "x.json"])
    assert (b.blocks, b.steps, b.warmup, b.reps, b.out) == ("128,32", 3, 1, 10, "x.json")


def test_progress_goes_to_stderr_with_the_tool_name(capsys):
    measure.progress("some_tool", "step 1 of 2")
    cap = capsys.readouterr()
    assert cap.out == "" and cap.err == "[some_tool] step 1 of 2\n"


def test_block_bytes_is_big_endian():
    assert measure.block_bytes([0x000102030405060708090A0B0C0D0E0F, 1 << 127]).tolist() == [list(range(16)), [0x80] + [0] * 15]
