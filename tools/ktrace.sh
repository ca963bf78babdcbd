#!/bin/bash
# Per-kernel table (rocprofv3 --kernel-trace --stats) of a command, single stream.  Usage on the GPU box:
#   tools/ktrace.sh <out.txt> <steps incl. warm-up> <python script and arguments ...>
# e.g. tools/ktrace.sh gpurun_out/k.txt 4 bench.py --config bfv_matmul --steps 3 --warmup 1 --profile-mode
# or a module: tools/ktrace.sh out/k.txt 1 -m pytest tests/test_gpu_selection_boundaries.py -m gpu -q (paths from the repository root)
# KTRACE_DIR: where the trace goes (default: a fresh directory under /tmp), KTRACE_TIMEOUT: seconds (default 400), KTRACE_DUAL_STREAM: 1 keeps two streams
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT=$1; STEPS=$2; shift 2
D=${KTRACE_DIR:-/tmp/ktrace_$$}
export TMPDIR=/tmp
if [ "$1" = "-m" ]; then cd "$R"; CMD=(python3 "$@"); else cd /tmp; CMD=(python3 "$R/$1" "${@:2}"); fi
( [ "${KTRACE_DUAL_STREAM:-0}" = 1 ] || export HE355_DUAL_STREAM=0; timeout -k 10 ${KTRACE_TIMEOUT:-400} rocprofv3 --kernel-trace --stats --output-format csv -d $D -- "${CMD[@]}" > $D.log 2>&1 ) || { tail -5 $D.log; exit 1; }
cd "$R" && python3 tools/kstats.py $D $STEPS | tee "$OUT"
