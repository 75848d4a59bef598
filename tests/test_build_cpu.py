"""tfhe_aes_amd/_build.py's build helper and _native.load_library's libraries by path, without a compiler run of the engine and
without a GPU: the helper builds a target in tmp_path with a `make` written here, the loader meets the product library, a byte copy
of it and a three-line library made with gcc."""
import hashlib
import re
import shutil
import subprocess
import sys
import time
from pathlib import Path

import pytest

from tfhe_aes_amd import _build, _native

PAYLOAD_BYTES = 1 << 20

# one builder process of the concurrent test: argv = target, log.  `make` appends one line to the log, writes half of the payload,
# sleeps 0.3 s and writes the rest -- a reader of the target that could see the file being written would see half of it
CHILD = """
import sys, time
from pathlib import Path
sys.path.insert(0, %r)
from tfhe_aes_amd import _build
target, log = Path(sys.argv[1]), Path(sys.argv[2])
payload = bytes(i %% 251 for i in range(%d))
def make(tmp):
    with open(log, "a") as f:
        f.write("make\\n")
    with open(tmp / "payload", "wb") as f:
        f.write(payload[:len(payload) // 2])
        f.flush()
        time.sleep(0.3)
        f.write(payload[len(payload) // 2:])
    return tmp / "payload"
print(_build.fresh(target, [], make, False))
""" % (str(_build.ROOT), PAYLOAD_BYTES)


def litter(target: Path):
    """the temp directories of builds of `target` that are still there"""
    return [p for p in _build.BUILD_DIR.glob(target.name + ".*") if p.is_dir()]


def writer(text: bytes, log: list):
    def make(tmp: Path) -> Path:
        log.append(tmp)
        (tmp / "out").write_bytes(text)
        return tmp / "out"
    return make


def test_concurrent_builds_make_once_and_never_show_a_partial_file(tmp_path):
    target, log, script = tmp_path / "concurrent_payload.bin", tmp_path / "log", tmp_path / "child.py"
    script.write_text(CHILD)
    want = hashlib.sha256(bytes(i % 251 for i in range(PAYLOAD_BYTES))).hexdigest()
    children = [subprocess.Popen([sys.executable, str(script), str(target), str(log)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                for _ in range(8)]
    looks = 0
    while any(c.poll() is None for c in children):
        if target.exists():
            data = target.read_bytes()
            looks += 1
            assert len(data) == PAYLOAD_BYTES and hashlib.sha256(data).hexdigest() == want, "a partial target was visible (%d bytes)" % len(data)
    outs = [c.communicate() for c in children]
    assert [c.returncode for c in children] == [0] * 8, [e for _, e in outs]
    assert [o.strip() for o, _ in outs] == [str(target)] * 8
    assert log.read_text() == "make\n"
    assert hashlib.sha256(target.read_bytes()).hexdigest() == want
    assert litter(target) == []
    # whoever had to wait said so, once
    assert all(e.count("waiting for another process") <= 1 for _, e in outs)
    print("looked at the finished target %d times while the builders ran" % looks)


def test_failed_build_leaves_the_old_target_and_the_lock_free(tmp_path):
    target = tmp_path / "failing_payload.bin"
    target.write_bytes(b"the old build")

    def broken(tmp: Path) -> Path:
        (tmp / "out").write_bytes(b"half a bui")
        raise RuntimeError("compiler said no")

    with pytest.raises(RuntimeError, match="compiler said no"):
        _build.fresh(target, [], broken, True)
    assert target.read_bytes() == b"the old build"
    assert litter(target) == []
    log = []
    assert _build.fresh(target, [], writer(b"the new build", log), True) == target      # the lock was released: this does not block
    assert target.read_bytes() == b"the new build" and len(log) == 1
    assert litter(target) == []


def test_staleness_rule(tmp_path):
    import os

    target, dep, log = tmp_path / "stale_payload.bin", tmp_path / "dep", []
    dep.write_text("source")
    assert _build.fresh(target, [dep], writer(b"1", log), False) == target and len(log) == 1           # missing: built
    now = time.time()
    os.utime(dep, (now - 10, now - 10))
    os.utime(target, (now - 5, now - 5))
    _build.fresh(target, [dep, tmp_path / "not there"], writer(b"2", log), False)
    assert len(log) == 1 and target.read_bytes() == b"1"                                                # fresh: left alone
    os.utime(dep, (now, now))
    _build.fresh(target, [dep], writer(b"3", log), False)
    assert len(log) == 2 and target.read_bytes() == b"3"                                                # a newer dependency: rebuilt
    os.utime(target, (now + 5, now + 5))
    _build.fresh(target, [dep], writer(b"4", log), True)
    assert len(log) == 3 and target.read_bytes() == b"4"                                                # forced: rebuilt
    assert all(not tmp.exists() for tmp in log) and all(tmp.parent == _build.BUILD_DIR for tmp in log)


def test_libraries_are_loaded_by_path(tmp_path):
    product = _native.load_library()
    copy_path = tmp_path / "libfheaes_copy.so"
    shutil.copyfile(_build.ENGINE_SO, copy_path)
    by_path, copy = _native.load_library(path=_build.ENGINE_SO), _native.load_library(path=copy_path)
    assert by_path is not copy and by_path._handle != copy._handle
    for lib in (by_path, copy):
        assert isinstance(lib.fheaes_version(), bytes)
    assert copy.fheaes_version() == by_path.fheaes_version()
    assert _native.load_library(path=copy_path) is copy
    assert _native.load_library(path=str(tmp_path / "." / "libfheaes_copy.so")) is copy                # one object per RESOLVED path
    assert by_path is product and _native.load_library() is product and _native.load_library(build=False) is product


def test_partial_libraries(tmp_path):
    src, so = tmp_path / "only_version.c", tmp_path / "libonly_version.so"
    src.write_text('const char *fheaes_version(void) {\n    return "only the version";\n}\n')
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True, capture_output=True)
    with pytest.raises(AttributeError) as err:
        _native.load_library(path=so)
    assert re.search(r"\bfheaes_[a-z0-9_]+\b", str(err.value)) and "fheaes_version" not in str(err.value), err.value
    assert re.search(r"\bfheaes_[a-z0-9_]+\b", str(err.value)).group(0) in _native.SIGNATURES
    lib = _native.load_library(path=so, partial=True)
    assert lib.fheaes_version.restype is _native.SIGNATURES["fheaes_version"][0] and lib.fheaes_version() == b"only the version"
    assert not hasattr(lib, "fheaes_create")
    assert _native.load_library() is not lib


def test_no_tool_replaces_build_engine():
    """which library a tool talks to is an argument (Engine(library=), measure.session(library=)), never an assignment to
    _build.build_engine; and build_engine has no `extra` any more for a tool to pass"""
    for path in sorted((_build.ROOT / "tools").rglob("*")):
        if path.is_file():
            text = path.read_text(errors="ignore")
            assert not re.search(r"\bbuild_engine\s*=[^=]", text), path
            assert not re.search(r"build_engine\([^)]*extra", text), path
