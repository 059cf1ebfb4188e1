#!/bin/bash
# Build L = 36-only (or, with ONLY=L128, L = 128-only) variants of the env-step kernels (acx_kernels.hip: the C-ABI,
# with the kernels and launchers in the headers it includes, + acx_curriculum.hip) for in-process A/B timing
# (tools/ab_rollout.py), in parallel.  -DFLAGs reach every header (ACX_ISA_*_ONLY is read by dispatch, acx_launch.h):
#   bash tools/ab_build.sh NAME "-DFLAG=.. -DFLAG2=.." [NAME2 "FLAGS2" ...]   -> abv/libacx_NAME.so (OUT=dir: another
# directory under the repo, e.g. one that travels with gpurun; abv/ does not)
# Another revision: SRC=/path/to/checkout/ac-solver-caltech_amd/csrc/acx_kernels.hip bash tools/ab_build.sh NAME ""
# (a checkout, e.g. `git worktree add`: the file's quoted includes take the headers and acx_curriculum.hip next to
# it).  Revisions before the kernels were split into headers are that single file (`git show` of it is enough).
# The round-3 occupancy / tile-order / stagger hooks this was used with are in commit history
# (profiles/r03/r03l_ab*.json, DESIGN.md "Rollout: what its time is made of").
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-abv}
mkdir -p $R/$OUT
C=$R/ac-solver-caltech_amd/csrc
SRC=${SRC:-$C/acx_kernels.hip}
CUR=$(dirname "$SRC")/acx_curriculum.hip
[ -f "$CUR" ] || CUR=$C/acx_curriculum.hip
pids=()
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I$R/include -Wno-pass-failed \
    -DACX_ISA_${ONLY:-L36}_ONLY $flags -I$C $SRC $CUR -o $R/$OUT/libacx_$name.so &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
ls -la $R/$OUT
