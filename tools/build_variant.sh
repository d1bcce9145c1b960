#!/bin/bash
# build an experimental variant of the library for A/B runs: tools/build_variant.sh <name> [-DMACRO=value ...]
# -> pbml_mantle_convection_amd/build/lib_<name>.so (select with MANTLE_LIB=...; see tools/ab.sh)
# sources and flags are those of build_ext.py
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/pbml_mantle_convection_amd/csrc
out=$root/pbml_mantle_convection_amd/build/var_$name
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p $out
pids=()
# one line per source: <file> <flags ...>
while read -r f flags; do
  $hipcc $flags "$@" -c $src/$f -o $out/${f%.hip}.o 2>/dev/null &
  pids+=($!)
done < <(cd $root && python -c '
from pbml_mantle_convection_amd.build_ext import SOURCES, FLAGS, EXTRA_FLAGS
for s in SOURCES: print(s, *FLAGS, *EXTRA_FLAGS.get(s, []))')
for p in "${pids[@]}"; do wait $p; done
$hipcc --offload-arch=gfx950 -shared -fPIC $out/*.o -o $root/pbml_mantle_convection_amd/build/lib_$name.so
echo $root/pbml_mantle_convection_amd/build/lib_$name.so
