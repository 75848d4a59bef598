#!/bin/bash
# Counter passes over one kernel at 16,384 bits, each a separate rocprofv3 run with --kernel-trace only (MI355X_MICROARCH.md, HBM section):
#   k2  one blind-rotation launch (tools/run_k2.py 16384 1)      k3  three packing key switch launches (tools/run_k3.py 16384 3)
# usage:  bash tools/pmc_passes.sh <k2|k3> <outdir> [library] [extra passes: name=CTR1,CTR2 ...]
#   python tools/summarize_pmc.py <outdir> "blind_rotate_pair_kernel<5, 5" profiles/<name> 16384       (k3: tools/summarize_pmc_k3.py)
# <outdir>/<pass>/ holds a pass's output, <outdir>/<pass>.log what it printed.  [library]: another build of libfheaes.so (a variant
# of tools/ablate_k2.py, say) instead of the product's.  Nothing is built here: build first, outside the profiler (_build.build_all()).
# The script ends at the first pass that does not exit 0, with that pass's status: after a fault or a timeout nothing more starts.
set -e -o pipefail
case "$1" in
  k2) RUN="run_k2.py 16384 1"
      LAST="act SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_THREAD_CYCLES_VALU SQ_INSTS_LDS SQ_INSTS_VMEM" ;;
  k3) RUN="run_k3.py 16384 3"
      LAST="mfma SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU_MFMA_I8 SQ_INSTS_MFMA" ;;
  *)  echo "usage: $0 <k2|k3> <outdir> [library] [name=CTR1,CTR2 ...]" >&2; exit 2 ;;
esac
[ -n "$2" ] || { echo "usage: $0 <k2|k3> <outdir> [library] [name=CTR1,CTR2 ...]" >&2; exit 2; }
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$2"
O=$(cd "$2" && pwd)
shift 2
LIB=
if [ $# -gt 0 ] && [ "${1#*=}" = "$1" ]; then LIB=$(realpath "$1"); shift; fi
PASSES=(
  "fetch FETCH_SIZE"
  "write WRITE_SIZE TCC_HIT_sum TCC_MISS_sum"
  "sq SQ_WAVE_CYCLES SQ_ACTIVE_INST_ANY SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS"
  "grbm GRBM_GUI_ACTIVE TCP_TCC_READ_REQ_sum"
  "$LAST"
)
for p in "$@"; do PASSES+=("${p%%=*} $(echo "${p#*=}" | tr , ' ')"); done
cd /tmp && export TMPDIR=/tmp
for pass in "${PASSES[@]}"; do
  set -- $pass; name=$1; shift
  mkdir -p "$O/$name"
  timeout -k 10 ${PMC_TIMEOUT:-150} ${ROCPROF:-rocprofv3} --pmc "$@" --kernel-trace --output-format csv -d "$O/$name" -- python3 $R/tools/$RUN $LIB > "$O/$name.log" 2>&1
  tail -1 "$O/$name.log"
done
echo done
