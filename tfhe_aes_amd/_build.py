"""In-tree builds of the native libraries (no JIT cache: the .so files travel with the tree).

  tfhe_aes_amd/libfheaes.so         hipcc --offload-arch=gfx950   (HIP kernels + C ABI, the product)
  tfhe_aes_amd/libfheaes_client.so  gcc -fopenmp                   (host Client: keygen / encrypt / decrypt)
(The CPU checker under oracle/ has its own Makefile; the product never builds or loads it.)
"""
from __future__ import annotations

import fcntl
import os
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"

ENGINE_SO = PKG / "libfheaes.so"
CLIENT_SO = PKG / "libfheaes_client.so"

# Two translation units (csrc/ks_launch.h says why): engine.hip = everything but the key-switching kernels, compiled with LLVM's
# post-register-allocation scheduler OFF; keyswitch_tu.hip = K1 / K3 / the key-byte conversion, default schedulers.
ENGINE_SOURCES = [CSRC / "engine.hip", CSRC / "keyswitch_tu.hip"]
ENGINE_HEADERS = sorted(CSRC.glob("*.h")) + sorted(CSRC.glob("*.hpp")) + [ROOT / "include" / "fheaes.h"]
BUILD_DIR = PKG / "build"


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).exists() and Path(d).stat().st_mtime > t for d in deps)


def _run(cmd, **kw):
    res = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if res.returncode != 0:
        raise RuntimeError("build failed: %s\n%s\n%s" % (" ".join(map(str, cmd)), res.stdout, res.stderr))
    return res


def hipcc_path() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found")


def _common_flags():
    # -ffp-contract=off: the canonical arithmetic only fuses where the source says fma()
    # -disable-machine-licm: the transforms' ~50 lane-independent twiddle constants are 64-bit literals moved into SGPR pairs;
    #   hoisted out of the 669-iteration loop they would all be live at once (12 SGPRs spilled to a VGPR, 20 B/lane of scratch in
    #   the blind rotation); left where they are used they cost a scalar move each, on the otherwise idle scalar unit
    return [
        "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
        "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-disable-machine-licm", "-Wall",
        "-Wno-unused-function", "-I", str(ROOT / "include"), "-I", str(CSRC),
    ]


# round 6: the post-RA scheduler re-orders what the blind-rotation kernels place by hand; without it a 16,384-bit launch takes
# 197.3 instead of 200.5 ms (same box, same words; profiles/r06_k2_ablations.txt).  The key switch wants it ON (15.9 vs 16.6 ms).
NO_POST_RA_SCHED = ["-mllvm", "-enable-post-misched=false"]


def unit_flags(unit: str):
    """compile flags of one unit of the product library: "engine" (engine.hip) or "keyswitch" (keyswitch_tu.hip)"""
    if unit == "engine":
        return _common_flags() + ["-DFHEAES_SPLIT_KS"] + NO_POST_RA_SCHED
    if unit == "keyswitch":
        return _common_flags() + ["-DFHEAES_SPLIT_KS"]
    raise ValueError(unit)


def engine_flags():
    """flags of a SINGLE-UNIT developer build (`hipcc <these> -o lib.so csrc/engine.hip`, as build_variant does it): engine.hip alone
    is then a complete library, every kernel in it compiled under the scheduler setting of the "engine" unit"""
    return _common_flags() + ["-shared"] + NO_POST_RA_SCHED


def fresh(target: Path, deps, make, force: bool = False) -> Path:
    """`target`, rebuilt first if it is older than one of `deps` (or `force`): make(tmpdir) builds a new file in a directory of its own
    and returns it, and a rename puts it in place, so a reader only ever meets a complete file and a failed make leaves the old one.
    One process builds at a time (build/lock, next to the temp directories); one that waited takes what the other built."""
    target = Path(target)
    if not force and not _stale(target, deps):
        return target
    BUILD_DIR.mkdir(exist_ok=True)
    with open(BUILD_DIR / "lock", "w") as lock:
        try:
            fcntl.flock(lock, fcntl.LOCK_EX | fcntl.LOCK_NB)
        except BlockingIOError:
            print("[build] waiting for another process to finish building %s" % target.name, file=sys.stderr, flush=True)
            fcntl.flock(lock, fcntl.LOCK_EX)
        if force or _stale(target, deps):         # looked at again under the lock: the process this one waited for may have just built
            tmp = Path(tempfile.mkdtemp(prefix=target.name + ".", dir=BUILD_DIR))
            try:
                built = make(tmp)
                if os.stat(built).st_dev != os.stat(target.parent).st_dev:      # a target on another file system: a rename cannot cross
                    built = shutil.copy(built, target.with_name(target.name + ".new"))
                os.replace(built, target)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
    return target


def build_engine(force: bool = False) -> Path:
    def make(tmp: Path) -> Path:
        objs = []
        for src, unit in zip(ENGINE_SOURCES, ("engine", "keyswitch")):
            objs.append(str(tmp / (src.stem + ".o")))
            _run([hipcc_path()] + unit_flags(unit) + ["-c", "-o", objs[-1], str(src)])
        _run([hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(tmp / ENGINE_SO.name)] + objs)
        return tmp / ENGINE_SO.name

    # this file is a dependency too: it holds the compile flags (a library built before a flag changed must not be reused)
    return fresh(ENGINE_SO, ENGINE_SOURCES + ENGINE_HEADERS + [Path(__file__)], make, force)


def build_client(force: bool = False) -> Path:
    src = CSRC / "client.c"

    def make(tmp: Path) -> Path:
        _run(["gcc", "-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC",
              "-shared", "-std=gnu11", "-Wall", "-o", str(tmp / CLIENT_SO.name), str(src), "-lm"])
        return tmp / CLIENT_SO.name

    return fresh(CLIENT_SO, [src, ROOT / "include" / "fheaes.h"], make, force)


def build_variant(out_path, defines=()) -> Path:
    """the single-unit developer build (engine_flags()) of engine.hip with `defines` (knobs of csrc/knobs.h) as out_path: always built,
    through a temp file next to out_path, and marked -DFHEAES_DEV_BUILD, so that an Engine refuses it unless told allow_dev_build"""
    out_path = Path(out_path)
    tmp = out_path.with_name("%s.%d.tmp" % (out_path.name, os.getpid()))
    try:
        _run([hipcc_path()] + engine_flags() + ["-DFHEAES_DEV_BUILD"] + list(defines) + ["-o", str(tmp), str(ENGINE_SOURCES[0])])
        os.replace(tmp, out_path)
    finally:
        tmp.unlink(missing_ok=True)
    return out_path


def engine_source_hash() -> str:
    """sha256 over the engine's sources (csrc/*.hip, csrc/*.h, include/fheaes.h): stamps measurements (profiles/*.json)
    so that a counter summary is only ever attached to a run of the same kernels"""
    import hashlib

    h = hashlib.sha256()
    for f in sorted(ENGINE_SOURCES + ENGINE_HEADERS):
        h.update(Path(f).name.encode())
        h.update(Path(f).read_bytes())
    # ... and the compile flags (without the machine-specific include paths): the same sources under other flags are other kernels
    for unit in ("engine", "keyswitch"):
        h.update(" ".join(x for x in unit_flags(unit) if not x.startswith("/")).encode())
    return h.hexdigest()


def build_all(force: bool = False):
    return build_engine(force), build_client(force)
