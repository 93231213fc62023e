#!/bin/bash
# diagnostic: builds a variant of libyacht_hip.so with extra defines into /tmp/yk_NAME/
# (GPU box or here), through the product's Makefile: its list of sources and its flags.
# usage: tools/variant_lib.sh NAME "-DFOO=1 ..."; then
# YK_LIB_PATH=/tmp/yk_NAME/libyacht_hip.so python bench.py ...
# A NAME starting with "base" builds the sources staged under ab_base/csrc (an A/B baseline).
cd "$(dirname "$0")/.." || exit 2
set -e
name=$1; shift
src=$PWD/nypc-yacht-auction_amd/csrc
older=()
case $name in base*) src=$PWD/ab_base/csrc; older=(ALLOW_MISSING=1) ;; esac
out=/tmp/yk_$name
mkdir -p $out
# the diagnostic hooks (stamps, yk_diag_* readers) are not in the production sources: with a
# -DYK_* switch, build from a copy with them inserted (tools/diag_sources.py)
case " $* " in
  *" -DYK_"*)
    [ ${#older[@]} = 0 ] || { echo "hooks need the in-tree sources" >&2; exit 2; }
    python3 tools/diag_sources.py $out/stage > /dev/null
    src=$out/stage/csrc ;;
esac
rm -rf $out/obj $out/libyacht_hip.so  # (a failed compile must not link a stale object)
libs=""  # (baselines staged from before round 5 still call rocBLAS in the f32 trainer)
grep -q rocblas $src/yk_train.hip && libs="-L/opt/rocm/lib -lrocblas -Wl,-rpath,/opt/rocm/lib"
make -C nypc-yacht-auction_amd -j"${MAX_JOBS:-8}" SRCDIR=$src BUILD=$out/obj LIB=$out/libyacht_hip.so \
     EXTRA="$*" LDLIBS="$libs" "${older[@]}" > $out/build.log 2>&1 ||
  { tail -20 $out/build.log >&2; echo "variant $name: build failed" >&2; exit 1; }
echo "built $out/libyacht_hip.so"
