#!/bin/bash
# The measurements behind profiles/rNN_*: run as ONE gpurun call from the repo root on the GPU box,
#   gpurun --timeout 1200 -- 'bash tools/final_measure.sh r03_v1'
# then copy in the container:
#   python tools/summarize_rocprof.py gpurun_out/<tag>/prof profiles/<tag>          (kernel stats + launch table)
#   cp gpurun_out/<tag>/<round>_pmc_blind_rotate.json profiles/ ; cp gpurun_out/<tag>/bench.json profiles/<tag>_bench.json
# Order: counter passes first (tools/pmc_passes.sh: separate rocprofv3 runs with --kernel-trace only; the program after `--` is
# python3 itself, no wrapper that would re-exec a GPU-initialised process), their summary is written next to the sources it was
# taken from (profiles/<round>_pmc_blind_rotate.json, stamped with the sha256 of the engine sources), THEN the un-profiled bench.py,
# whose roofline object picks traffic / valu_busy / ceiling_frac up from that file, then the kernel trace.  Every step that uses the
# GPU has a time limit of its own, and the script ends at the first step that fails: nothing more starts on a card after a fault.
set -e -o pipefail
TAG=${1:-final}
ROUND=${TAG%%_*}
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/gpurun_out/$TAG
mkdir -p $O
# the ISA-count x issue-cost model of the blind-rotation kernel (tools/k2_dyncount.py) for roofline.ceiling_frac
# (the product's engine unit: its flags come from tfhe_aes_amd/_build.py -- post-RA scheduler off, key-switching kernels in the other unit)
hipcc $(python3 -c 'from tfhe_aes_amd import _build; print(" ".join(_build.unit_flags("engine")))') -S --cuda-device-only \
      -o /tmp/engine_final.s $R/tfhe_aes_amd/csrc/engine.hip 2> /dev/null
python3 $R/tools/k2_dyncount.py /tmp/engine_final.s blind_rotate_pair_kernelILi5ELi5ELi8ELi3ELi2 1 0 | tee $O/k2_dyncount.txt
# build (if stale) BEFORE anything runs under the profiler: hipcc must not be spawned from a process tree rocprofv3 has GPU-initialised
python3 -c 'from tfhe_aes_amd import _build; _build.build_all()'
bash $R/tools/pmc_passes.sh k2 $O/pmc
cd $R
# 16,384 bits on 2,816 workgroups (2,560 of six ciphertexts, 256 of four): 5.8182 ciphertexts per workgroup on average
python3 tools/summarize_pmc.py $O/pmc "blind_rotate_pair_kernel<5, 5" profiles/${ROUND}_pmc_blind_rotate 16384 --cus 256 --dyncount $O/k2_dyncount.txt \
        --flops-per-ct-iteration 609280 --cts-per-wg 5.8182 --waves-per-wg 8 --algorithmic-bytes 698912768 > $O/pmc_summary.txt
cp profiles/${ROUND}_pmc_blind_rotate.json $O/
# the second kernel of a step (K3, packing key switch): its own counter passes and summary (bench.py attaches them to roofline_k3)
bash $R/tools/pmc_passes.sh k3 $O/pmc_k3
cd $R
python3 tools/summarize_pmc_k3.py $O/pmc_k3 profiles/${ROUND}_pmc_pfpks 16384 > $O/pmc_k3_summary.txt
cp profiles/${ROUND}_pmc_pfpks.json $O/
cd /tmp && export TMPDIR=/tmp
# time limits from the runs under profiles/ (r06_v*_bench*.json): a step takes 2.2 s, set-up (keys, key expansion) about 1 s, the CPU
# baseline 15 s, the other configurations of --full under a minute; three times that, so that only a hang meets the limit
timeout -k 10 300 python3 $R/bench.py --full > $O/bench.json 2> $O/bench.err
tail -1 $O/bench.json | cut -c1-300
# the driver's command with --full (every block of every step verified; exit code 1 on a wrong one): 25 steps of 2.2 s
timeout -k 10 480 python3 $R/bench.py --gpus 1 --steps 20 --warmup 5 --full > $O/bench_driver_style.json 2> $O/bench_driver_style.err
echo "driver-style bench: all verified"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python3 $R/bench.py --steps 1 --warmup 0 --full --no-cpu-baseline > $O/prof.log 2>&1
echo done
