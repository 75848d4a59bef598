"""Developer tool: time the blind-rotation kernel (K2) for builds with phases compiled out.
Builds variants of libfheaes.so (_build.build_variant) into its output directory (`out` in main()) and times Engine.cbs_pbs_batch on M resident bits; every
variant is an engine of its own in this one process, on the same keys.
usage: python tools/ablate_k2.py [M] [name,name,... | so:<path of a prebuilt library>]
HBM-side counters of the variants, once this has built them (the first failing pass ends the loop):
  for v in base nopark; do bash tools/pmc_passes.sh k2 <outdir>/$v <that directory>/libfheaes_$v.so || break; done
  (K2_PARKING=private in front for the runtime variant parkwg, on the product library)"""
import hashlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

import measure  # noqa: F401  (puts the repository root on sys.path)
from gpu_power import Sampler, fmt
from tfhe_aes_amd import PARAM_OPT, _build, _native
from tfhe_aes_amd.client import Client

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
RUNTIME = {"parkwg": lambda eng: eng.k2_set_parking(False)}


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
            so = _build.build_variant(out / ("libfheaes_%s.so" % name), VARIANTS[name])
        eng = _native.Engine(p, device=0, allow_dev_build=True, library=so)      # an older library (so:...) may lack entry points added since
        eng.upload_keys(keys.ksk, keys.bsk, keys.pfpksk)
        if name in RUNTIME:
            RUNTIME[name](eng)
        d_in = torch.from_numpy(small.view(np.int64)).cuda()
        d_out = torch.empty((M, p.big1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ts = []
        eng.cbs_pbs_batch(d_in, d_out, M)               # warm-up (workspace, clocks)
        eng.synchronize()
        with Sampler(period=0.01) as smp:                      # socket power / shader clock while the timed launches run
            for _ in range(RUNS):
                t = time.perf_counter()
                eng.cbs_pbs_batch(d_in, d_out, M)
                eng.synchronize()
                ts.append(time.perf_counter() - t)
        digest = hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()[:12]      # equal digests = bit-identical outputs (real variants must match base)
        print("%-16s M=%d  %.1f ms  (runs: %s)  out %s  %s" % (name, M, 1e3 * min(ts), " ".join("%.1f" % (1e3 * x) for x in ts), digest, fmt(smp.summary())), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
