#!/bin/bash
# A/B timing on ONE box: the product library against other builds, alternating runs so that the drift of the die is shared.
# An arm is  NAME             a variant build (make -C csrc variant NAME=.. VFLAGS=..): csrc/exp/libnwe_NAME.so
#            NAME=/path.so    any other library with this tree's entry points
#            NAME=/checkout   another checkout of the project with its library built, e.g. the parent commit's: its own bench.py
#            static           the product library with NWE_WORK_QUEUE=0: the hardware's static dealing of workgroups
#            nobackfill       the product library with NWE_WORK_QUEUE_BACKFILL=0: queued launches one after the other
#            notail           the product library with NWE_WORK_QUEUE_TAIL=0: the split items in a launch of their own, beside the packets
#            noskip           the product library with NWE_COLOUR_SKIP=0: every evaluation runs its colour layers
#            noblocks         the product library with NWE_PACKET_BLOCKS=0: packets of 32 consecutive pixels of a row
# Usage (on the GPU box): bash tools/ab_bench.sh arm1 [arm2 ...] -> one line per run on stdout, and in the file $AB_OUT if that is set
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${AB_OUT:-/dev/null}
: > $OUT
for rep in 1 2 3; do
  for v in product "$@"; do
    unset NWE_LIB NWE_WORK_QUEUE NWE_WORK_QUEUE_BACKFILL NWE_WORK_QUEUE_TAIL NWE_COLOUR_SKIP NWE_PACKET_BLOCKS
    TREE=$ROOT
    case "$v" in
      product) ;;
      static) export NWE_WORK_QUEUE=0 ;;
      nobackfill) export NWE_WORK_QUEUE_BACKFILL=0 ;;
      notail) export NWE_WORK_QUEUE_TAIL=0 ;;
      noskip) export NWE_COLOUR_SKIP=0 ;;
      noblocks) export NWE_PACKET_BLOCKS=0 ;;
      *=*) if [ -d "${v#*=}" ]; then TREE=${v#*=}; else export NWE_LIB=${v#*=}; fi ;;
      *) export NWE_LIB=$ROOT/nerf-workspaces-explorer_amd/csrc/exp/libnwe_$v.so ;;
    esac
    timeout -k 10 180 python3 $TREE/bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-configs 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); print('${v%%=*} rep $rep: kernel_ms %.2f ms_per_step %.2f' % (d['roofline']['kernel_ms'], d['ms_per_step']))" | tee -a $OUT
    [ ${PIPESTATUS[0]} -eq 0 ] || { echo "${v%%=*} rep $rep: bench.py failed, stopping" | tee -a $OUT; exit 1; }   # nothing more on a GPU that may have faulted
  done
done
