"""Developer tool: time the blind-rotation kernel (K2) for builds with phases compiled out.
Builds variants of libfheaes.so into gpurun_out/abl/ and times fheaes_cbs_pbs_batch on M resident bits.
usage: python tools/ablate_k2.py [M] [name,name,... | so:<path of a prebuilt library>]"""
import ctypes
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401  (HIP runtime first, see _native.load_library)

sys.path.insert(0, "tools")
from gpu_power import Sampler, fmt  # noqa: E402

from tfhe_aes_amd import PARAM_OPT, _build, _native  # noqa: E402
from tfhe_aes_amd.client import Client  # noqa: E402

# Every flag is a knob of csrc/knobs.h: per-phase proxies of the paired blind rotation (WRONG results, timing only) and the phase stamps.
VARIANTS = {
    "base": [],
    "parkwg": [],     # the product build with fheaes_k2_set_parking(ctx, 0) (one private slot per workgroup), see RUNTIME
    "noxstore": ["-DBRP_ABL_NOXSTORE"], "nodstore": ["-DBRP_ABL_NODSTORE"], "nostores": ["-DBRP_ABL_NOXSTORE", "-DBRP_ABL_NODSTORE"],
    "noxread": ["-DBRP_ABL_NOXREAD"], "noxpose": ["-DBRP_ABL_NOXSTORE", "-DBRP_ABL_NOXREAD"], "nolds_fwd": ["-DBRP_ABL_NOXSTORE", "-DBRP_ABL_NOXREAD", "-DBRP_ABL_NODSTORE"],
    "nobar": ["-DBRP_ABL_NOBAR"], "nobar_skew0": ["-DBRP_ABL_NOBAR", "-DBRP_ABL_SKEW=0"], "nobar_skew40": ["-DBRP_ABL_NOBAR", "-DBRP_ABL_SKEW=40"],
    "nobar_skew80": ["-DBRP_ABL_NOBAR", "-DBRP_ABL_SKEW=80"], "nobar_skew160": ["-DBRP_ABL_NOBAR", "-DBRP_ABL_SKEW=160"],
    "nopeel": ["-DBRP_ABL_NOPEEL"], "noload": ["-DBR16_ABL_NOLOAD"], "nopark": ["-DBR16_ABL_NOPARK"],
    "nostores_noload": ["-DBRP_ABL_NOXSTORE", "-DBRP_ABL_NODSTORE", "-DBR16_ABL_NOLOAD"], "fewcmul": ["-DBRP_ABL_FEWCMUL"],
    "stamps": ["-DEP_STAMPS"],                       # per-phase s_memtime stamps, printed to stderr
}


RUNS = 4
# variants that are a runtime setting of the context, not a build
RUNTIME = {"parkwg": lambda lib, h: lib.fheaes_k2_set_parking(h, 0)}


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(VARIANTS)
    out = Path("gpurun_out/abl")
    out.mkdir(parents=True, exist_ok=True)
    p = PARAM_OPT
    c = Client(1, 1, 2, params=p, seed=0xAE50001)
    keys = c.server_keys()
    rng = np.random.default_rng(0)
    small = rng.integers(0, 1 << 64, (M, p.n + 1), dtype=np.uint64)
    for name in names:
        if name.startswith("so:"):                      # an already built library (A/B against an older build on the same box)
            so = Path(name[3:])
        else:
            so = out / ("libfheaes_%s.so" % name)
            cmd = [_build.hipcc_path()] + _build.engine_flags() + ["-DFHEAES_DEV_BUILD"] + VARIANTS[name] + ["-o", str(so), str(_build.ENGINE_SOURCES[0])]
            subprocess.run(cmd, check=True, capture_output=True)
        lib = ctypes.CDLL(str(so))
        for fn, (res, args) in _native.SIGNATURES.items():
            if not hasattr(lib, fn):                    # an older library (so:...) may lack entry points added since
                continue
            f = getattr(lib, fn)
            f.restype, f.argtypes = res, args
        h = ctypes.c_void_p()
        cp = p.c_struct()
        assert lib.fheaes_create(ctypes.byref(cp), 0, ctypes.byref(h)) == 0
        assert lib.fheaes_upload_keys(h, keys.ksk.ctypes.data, keys.bsk.ctypes.data, keys.pfpksk.ctypes.data, 0) == 0
        if name in RUNTIME:
            assert RUNTIME[name](lib, h) == 0
        d_in = torch.from_numpy(small.view(np.int64)).cuda()
        d_out = torch.empty((M, p.big1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ts = []
        assert lib.fheaes_cbs_pbs_batch(h, d_in.data_ptr(), M, 1, d_out.data_ptr(), 1) == 0      # warm-up (workspace, clocks)
        lib.fheaes_synchronize(h)
        with Sampler(period=0.01) as smp:                      # socket power / shader clock while the timed launches run
            for _ in range(RUNS):
                t = time.perf_counter()
                assert lib.fheaes_cbs_pbs_batch(h, d_in.data_ptr(), M, 1, d_out.data_ptr(), 1) == 0
                lib.fheaes_synchronize(h)
                ts.append(time.perf_counter() - t)
        import hashlib
        digest = hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()[:12]      # equal digests = bit-identical outputs (real variants must match base)
        print("%-16s M=%d  %.1f ms  (runs: %s)  out %s  %s" % (name, M, 1e3 * min(ts), " ".join("%.1f" % (1e3 * x) for x in ts), digest, fmt(smp.summary())), flush=True)
        lib.fheaes_destroy(h)


if __name__ == "__main__":
    main()
