#!/usr/bin/env python3
"""Machine code of every kernel of the product library, one line `sha256 size unit symbol` each: the check of a refactor that
must leave the device code as it is.  Needs hipcc, no GPU.

  python tools/kernel_bytes.py [TREE] > branch.txt      (TREE: root of a checkout, default this one; its own _build.py gives the flags)
  diff parent.txt branch.txt

Both product units are compiled device side only.  FUNC symbols are kernel code in .text; OBJECT symbols ending in .kd are the
64-byte kernel descriptors in .rodata, hashed WITHOUT bytes 16-23 (kernel_code_entry_byte_offset, the distance from descriptor to
code: it moves when another kernel of the unit comes or goes).  `.text` / `.rodata` rows hash the whole sections.  The one-byte
__hip_cuid_* symbol (a hash of the translation unit) is left out.  Two builds of one tree give identical output.
"""
import hashlib
import importlib.util
import subprocess
import sys
import tempfile
from pathlib import Path

def tool(build, name, *args):
    exe = Path(build.hipcc_path()).resolve().parent.parent / "llvm" / "bin" / name      # ROCm's own, else whatever PATH has
    return subprocess.run([str(exe) if exe.exists() else name, *args], check=True, capture_output=True, text=True).stdout


def unit_rows(build, unit, src, tmp):
    obj = str(Path(tmp) / (unit + ".o"))
    subprocess.run([build.hipcc_path()] + build.unit_flags(unit) +
                   ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", obj, str(src)], check=True)
    blob = Path(obj).read_bytes()
    sections = {}                                           # index -> (name, address, file offset, size)
    for line in tool(build, "llvm-readelf", "-SW", obj).splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 6 and f[0].isdigit() and f[2] in ("PROGBITS", "NOBITS"):
            sections[f[0]] = (f[1], int(f[3], 16), int(f[4], 16), int(f[5], 16))
    rows = [(name, blob[off:off + size]) for name, _, off, size in sections.values() if name in (".text", ".rodata")]
    for line in tool(build, "llvm-readelf", "-sW", "--demangle", obj).splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or f[6] not in sections or f[7].startswith("__hip_cuid_"):
            continue
        _, base, off, _ = sections[f[6]]
        start = off + int(f[1], 16) - base
        data = blob[start:start + int(f[2], 0)]
        if f[3] == "OBJECT" and f[7].rstrip(")").endswith(".kd"):
            data = data[:16] + data[24:]
        rows.append((f[7], data))
    return ["%s %7d %-9s %s" % (hashlib.sha256(d).hexdigest(), len(d), unit, name) for name, d in sorted(set(rows))]


def main():
    tree = Path(sys.argv[1] if len(sys.argv) > 1 else Path(__file__).resolve().parent.parent).resolve()
    spec = importlib.util.spec_from_file_location("_tree_build", tree / "tfhe_aes_amd" / "_build.py")
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    with tempfile.TemporaryDirectory() as tmp:
        for src, unit in zip(build.ENGINE_SOURCES, ("engine", "keyswitch")):
            print("\n".join(unit_rows(build, unit, src, tmp)), flush=True)


if __name__ == "__main__":
    main()
