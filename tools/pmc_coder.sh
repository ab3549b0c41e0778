#!/bin/bash
# Counter profile of the lanes coder (ac_encode_lanes_k) with the chip to itself: one launch of tools/coder_alone.py at one
# block per lane, 28 lanes per workgroup, enough blocks for a workgroup on every CU -- in three rocprofv3 --pmc passes of
# their own (no trace domain in the same run, the program behind --).  SCALCE_AC_ROUND, where set, travels with the run.
#   bash tools/pmc_coder.sh r06_parent [blocks=7168]   -> profiles/r06_parent_coder_pmc.json (SCALCE_PROFILE_OUT, an
#   absolute path, names another directory; the raw counter files go there too and are removed at the end)
set -eu
TAG=${1:-r06_x}
BLOCKS=${2:-7168}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${SCALCE_PROFILE_OUT:-$R/profiles}
cd /tmp && export TMPDIR=/tmp
O=$OUT/prof_coder_$TAG; rm -rf $O; mkdir -p $O
export SCALCE_AC_BLOCKS_PER_WG=64 SCALCE_AC_LANES_USED=28
timeout -k 10 300 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY --output-format csv -d $O/pmc1 -o p -- python3 $R/tools/coder_alone.py $BLOCKS 64 > $O/pmc1.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_LDS --output-format csv -d $O/pmc2 -o p -- python3 $R/tools/coder_alone.py $BLOCKS 64 > $O/pmc2.log 2>&1
timeout -k 10 300 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES --output-format csv -d $O/pmc3 -o p -- python3 $R/tools/coder_alone.py $BLOCKS 64 > $O/pmc3.log 2>&1
cd $R
python3 tools/prof_summary.py coder $O $OUT/${TAG}_coder_pmc.json $BLOCKS
grep -h "ns per symbol" $O/pmc3.log | tail -1
rm -rf $O
