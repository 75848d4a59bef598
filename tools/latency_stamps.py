"""Developer tool: per-phase cycle stamps of the small-batch blind-rotation kernel (a developer build with -DEP_STAMPS, which prints
them to stderr).  usage: python tools/latency_stamps.py [M] [further -D knobs of csrc/knobs.h]"""
import sys
from pathlib import Path

import numpy as np
import torch

import measure
from tfhe_aes_amd import PARAM_OPT as p, _build

M = int(sys.argv[1]) if len(sys.argv) > 1 else 128
out = Path("gpurun_out/abl"); out.mkdir(parents=True, exist_ok=True)
so = _build.build_variant(out / "libfheaes_lat_stamps.so", ["-DEP_STAMPS"] + sys.argv[2:])
_, eng = measure.session(0xAE50001, 1, 2, library=so, allow_dev_build=True)
rng = np.random.default_rng(0)
small = torch.from_numpy(rng.integers(0, 1 << 64, (M, p.n + 1), dtype=np.uint64).view(np.int64)).cuda()
o = torch.empty((M, p.big1), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
eng.cbs_pbs_batch(small, o, M)
eng.synchronize()
eng.close()
