#!/bin/bash
# Profiling aid: build an engine variant into build/alt/lib_<name>.so for an A/B run against the
# shipped library (FQ_ENGINE_LIB, tools/ab.sh).  The experiment lives in a copy of the fast kernel's
# source next to it, so the shipped file carries no switches:
#   cp fqtool_amd/csrc/pe_fast.hip fqtool_amd/csrc/pe_fast_try.hip   # edit the copy
#   PE_FAST_SRC=pe_fast_try.hip tools/ab_build.sh try [extra compiler flags, e.g. -DFQ_PHASE_STAMPS]
# Only the two fast-kernel objects are rebuilt (pe_fast_long.hip includes pe_fast.hip itself: give the
# copy's name in a copy of it too if the long build is part of the experiment); every other engine
# object is taken from what `make` built in build/obj (its host_*.o belong to the host tool).
set -eu
cd "$(dirname "$0")/.."
name=$1; shift
out=build/alt/$name; mkdir -p $out
HIPFLAGS="-std=c++17 -O3 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result"
/opt/rocm/bin/hipcc $HIPFLAGS "$@" -c fqtool_amd/csrc/${PE_FAST_SRC:-pe_fast.hip} -o $out/pe_fast.o & p1=$!
/opt/rocm/bin/hipcc $HIPFLAGS "$@" -c fqtool_amd/csrc/pe_fast_long.hip -o $out/pe_fast_long.o & p2=$!
wait $p1; wait $p2
objs=""
for o in build/obj/*.o; do
  case $o in
    build/obj/pe_fast.o|build/obj/pe_fast_long.o|build/obj/host_*.o) ;;
    *) objs="$objs $o" ;;
  esac
done
[ -n "$objs" ] || { echo "build/obj is empty: run make first" >&2; exit 1; }
/opt/rocm/bin/hipcc $HIPFLAGS -shared -o build/alt/lib_$name.so $objs $out/pe_fast.o $out/pe_fast_long.o
echo built build/alt/lib_$name.so
