#!/bin/bash
# K-factored's planner of a revision against the tree's, without a GPU (tools/plan_bytes.cpp): the dumps of everything
# the two planners upload and fill must be the same file; then the host time of a plan, three shapes, alternating.
#   tools/plan_bytes.sh [REV]        (default: HEAD)
set -e -o pipefail
cd "$(dirname "$0")/.."
rev=${1:-HEAD}
work=$(mktemp -d)
mkdir -p $work/rev && git archive $rev covest_amd/csrc include | tar -x -C $work/rev
hipcc=/opt/rocm/bin/hipcc
for side in rev tree; do
  src=covest_amd/csrc; [ $side = rev ] && src=$work/rev/covest_amd/csrc
  $hipcc --offload-arch=gfx950 -O1 -std=c++17 -x hip -I$src -Wno-unused-result -c tools/plan_bytes.cpp -o $work/harness_$side.o
  $hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -c $src/plan_factored.cpp -o $work/plan_$side.o
  /opt/rocm/lib/llvm/bin/clang++ -o $work/plan_bytes_$side $work/harness_$side.o $work/plan_$side.o -lm -lpthread
  $work/plan_bytes_$side $work/dump_$side.bin
done
ls -l $work/dump_rev.bin $work/dump_tree.bin | awk '{print $5, "bytes"}'
grep -a -c "^== dense" $work/dump_tree.bin | sed 's/$/ dense builds/'; grep -a -c "^long " $work/dump_tree.bin | sed 's/$/ long parts/'
grep -a -c "shared=[1-9]" $work/dump_tree.bin | sed 's/$/ builds with shared tiles/'; grep -a -c "^== list" $work/dump_tree.bin | sed 's/$/ point lists/'
cmp $work/dump_rev.bin $work/dump_tree.bin && echo "the two dumps are identical"
for c in 1 12 14; do for r in 1 2 3; do for side in rev tree; do echo -n "$side "; $work/plan_bytes_$side /dev/null $c; done; done; done
rm -rf $work
