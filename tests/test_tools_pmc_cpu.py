"""tools/pmc_passes.sh without a profiler and without a GPU: ROCPROF points at a stub that logs its arguments and exits with the
status a file holds for call number n (or sleeps first).  What is pinned: the pass names and counters, as the counter summaries under
profiles/ were taken with them; the program after `--`; and that the script starts nothing more after a pass that fails or overruns."""
import json
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SCRIPT = ROOT / "tools" / "pmc_passes.sh"

COMMON = [
    ("fetch", ["FETCH_SIZE"]),
    ("write", ["WRITE_SIZE", "TCC_HIT_sum", "TCC_MISS_sum"]),
    ("sq", ["SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_INSTS_VALU", "SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT",
            "SQ_WAIT_INST_LDS"]),
    ("grbm", ["GRBM_GUI_ACTIVE", "TCP_TCC_READ_REQ_sum"]),
]
PASSES = {
    "k2": COMMON + [("act", ["SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_ACTIVE_INST_VMEM", "SQ_ACTIVE_INST_SCA", "SQ_THREAD_CYCLES_VALU",
                             "SQ_INSTS_LDS", "SQ_INSTS_VMEM"])],
    "k3": COMMON + [("mfma", ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_BUSY_CYCLES", "SQ_INSTS_VALU_MFMA_I8", "SQ_INSTS_MFMA"])],
}
PROGRAM = {"k2": ["run_k2.py", "16384", "1"], "k3": ["run_k3.py", "16384", "3"]}

# the stand-in for rocprofv3: one JSON line of its arguments per call into calls.log; exit status = line n of `statuses` for call n
# (0 where the file is shorter); `sleep` holds how long to sleep first
STUB = """#!/usr/bin/env python3
import json, sys, time
from pathlib import Path
here = Path(__file__).resolve().parent
with open(here / "calls.log", "a") as f:
    f.write(json.dumps(sys.argv[1:]) + "\\n")
n = len((here / "calls.log").read_text().splitlines())
time.sleep(float((here / "sleep").read_text()))
statuses = (here / "statuses").read_text().split()
print("call", n)
sys.exit(int(statuses[n - 1]) if n <= len(statuses) else 0)
"""


def run(tmp_path, args, statuses=(), sleep=0.0, env=()):
    stub = tmp_path / "rocprof_stub"
    stub.write_text(STUB)
    stub.chmod(0o755)
    (tmp_path / "statuses").write_text(" ".join(map(str, statuses)))
    (tmp_path / "sleep").write_text(str(sleep))
    res = subprocess.run(["bash", str(SCRIPT)] + [str(a) for a in args], env={**os.environ, "ROCPROF": str(stub), **dict(env)}, cwd=tmp_path,
                         capture_output=True, text=True)
    log = tmp_path / "calls.log"
    return res, [json.loads(line) for line in log.read_text().splitlines()] if log.exists() else []


def expected_call(kernel, name, counters, out, library=None):
    return (["--pmc"] + counters + ["--kernel-trace", "--output-format", "csv", "-d", str(out / name), "--", "python3", str(ROOT / "tools" / PROGRAM[kernel][0])]
            + PROGRAM[kernel][1:] + ([str(library)] if library else []))


@pytest.mark.parametrize("kernel", ["k2", "k3"])
@pytest.mark.parametrize("with_library", [False, True])
def test_every_pass_runs_once_with_its_counters(tmp_path, kernel, with_library):
    out = tmp_path / "out" / "pmc"
    library = tmp_path / "libfheaes_variant.so" if with_library else None
    res, calls = run(tmp_path, [kernel, out] + ([library] if library else []))
    assert res.returncode == 0, res.stderr
    assert len(calls) == 5
    assert calls == [expected_call(kernel, name, counters, out, library) for name, counters in PASSES[kernel]]
    for name, _ in PASSES[kernel]:
        assert (out / name).is_dir() and (out / (name + ".log")).read_text().startswith("call ")


def test_extra_passes_follow_the_list(tmp_path):
    out = tmp_path / "pmc"
    res, calls = run(tmp_path, ["k2", out, "lds=SQ_INSTS_LDS,SQ_LDS_BANK_CONFLICT", "one=SQ_WAVES"])
    assert res.returncode == 0, res.stderr
    assert calls == [expected_call("k2", name, counters, out) for name, counters in PASSES["k2"] + [("lds", ["SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT"]),
                                                                                                   ("one", ["SQ_WAVES"])]]


def test_a_failed_pass_ends_the_script_with_its_status(tmp_path):
    out = tmp_path / "pmc"
    res, calls = run(tmp_path, ["k2", out], statuses=[0, 139])
    assert res.returncode == 139
    assert len(calls) == 2 and calls[1] == expected_call("k2", "write", PASSES["k2"][1][1], out)
    assert sorted(p.name for p in out.iterdir() if p.is_dir()) == ["fetch", "write"]
    assert "done" not in res.stdout.split()


def test_a_pass_that_overruns_ends_the_script(tmp_path):
    out = tmp_path / "pmc"
    res, calls = run(tmp_path, ["k3", out], sleep=5, env={"PMC_TIMEOUT": "1"}.items())
    assert res.returncode == 124
    assert len(calls) == 1
    assert sorted(p.name for p in out.iterdir() if p.is_dir()) == ["fetch"]


def test_usage_errors_start_nothing(tmp_path):
    for args in ([], ["k5", tmp_path / "pmc"], ["k2"]):
        res, calls = run(tmp_path, args)
        assert res.returncode == 2 and calls == [], (args, res.stderr)
