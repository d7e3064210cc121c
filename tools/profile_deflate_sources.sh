#!/bin/bash
# SQ counters of deflate_chunks_kernel on the sources corpus: a kernel trace with statistics, then the counters in a pass of their own.
# usage: tools/profile_deflate_sources.sh <outdir-under-gpurun_out>
set -o pipefail
OUT="$GRAFT_REPO_ROOT/gpurun_out/$1"; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
P="$GRAFT_REPO_ROOT/tools/deflate_sources_probe.py"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -- python3 "$P" > "$OUT/trace.log" 2>&1 || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE --output-format csv -d "$OUT/pmc" -- python3 "$P" > "$OUT/pmc.log" 2>&1 || exit 2
find "$OUT" -name "*.csv" -size +8M -delete
exit 0
