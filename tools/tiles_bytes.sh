#!/bin/bash
# The tile table and the grid handle's set-up of a revision against the tree's, without a GPU (tools/tiles_bytes.cpp): the
# dumps of everything tiles_host.cpp and abi_grid.cpp upload, bind and call must be the same file, in the shipped build and
# in the COVEST_DIAG build with COVEST_NO_SUM_ITEMS set; an input set that misses a listed feature fails; then the host
# time of four inputs, revision and tree alternating, three rounds.
#   tools/tiles_bytes.sh [REV] [OUT]       (default: HEAD, profiles/tiles_bytes.txt)
set -e -o pipefail
cd "$(dirname "$0")/.."
rev=${1:-HEAD}
report=${2:-profiles/tiles_bytes.txt}
work=$(mktemp -d)
mkdir -p $work/rev && git archive $rev covest_amd/csrc include | tar -x -C $work/rev
hipcc=/opt/rocm/bin/hipcc
for flavour in ship diag; do
  def=; [ $flavour = diag ] && def=-DCOVEST_DIAG
  for side in rev tree; do
    src=covest_amd/csrc; [ $side = rev ] && src=$work/rev/covest_amd/csrc
    $hipcc --offload-arch=gfx950 -O1 -std=c++17 -x hip -I$src -Wno-unused-result -Wno-unused-function $def -c tools/tiles_bytes.cpp -o $work/harness_${flavour}_$side.o
    for f in tiles_host abi_grid; do
      $hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -x hip $def -c $src/$f.cpp -o $work/${f}_${flavour}_$side.o
    done
    /opt/rocm/lib/llvm/bin/clang++ -o $work/tiles_bytes_${flavour}_$side $work/harness_${flavour}_$side.o $work/tiles_host_${flavour}_$side.o $work/abi_grid_${flavour}_$side.o -lm -lpthread
  done
done
{
  echo "# tools/tiles_bytes.sh $(git rev-parse --short $rev): tiles_host.cpp and abi_grid.cpp of that revision against the tree's"
  for flavour in ship diag; do
    [ $flavour = diag ] && export COVEST_NO_SUM_ITEMS=1
    echo "## $flavour build$([ $flavour = diag ] && echo ' (-DCOVEST_DIAG, COVEST_NO_SUM_ITEMS=1)')"
    for side in rev tree; do
      $work/tiles_bytes_${flavour}_$side $work/dump_${flavour}_$side.bin tests/golden > $work/features_${flavour}_$side.txt 2> /dev/null
    done
    cat $work/features_${flavour}_tree.txt
    echo "$(grep -a -c '^== tiles' $work/dump_${flavour}_tree.bin) build_tiles inputs, $(grep -a -c '^== grid' $work/dump_${flavour}_tree.bin) grid configurations"
    ls -l $work/dump_${flavour}_rev.bin $work/dump_${flavour}_tree.bin | awk '{print $5, "bytes"}'
    cmp $work/dump_${flavour}_rev.bin $work/dump_${flavour}_tree.bin && echo "the two dumps are identical"
  done
  unset COVEST_NO_SUM_ITEMS
  echo "## host time, revision and tree alternating, three rounds"
  for c in 0 1 2 3; do for r in 1 2 3; do for side in rev tree; do echo -n "$side  "; $work/tiles_bytes_ship_$side /dev/null tests/golden time $c; done; done; done
} | tee $report
rm -rf $work
