#!/bin/bash
# usage: build_variant.sh <source.hip> <out.so> [-D...]: the library with ONE source recompiled under extra flags (the other objects are cached
# in /tmp/bxi_obj): A/B builds in seconds instead of a minute.  Developer tool; the shipped library is built by boxinstseg_amd/build.py, whose
# FLAGS and SOURCES this script reads.
set -e
src=$1; out=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
C=$ROOT/boxinstseg_amd/csrc; O=/tmp/bxi_obj; mkdir -p $O
FLAGS=$(cd "$ROOT" && python -c "from boxinstseg_amd.build import FLAGS; print(' '.join(FLAGS))")
SOURCES=$(cd "$ROOT" && python -c "from boxinstseg_amd.build import SOURCES; print(' '.join(s[:-len('.hip')] for s in SOURCES))")
pids=()
for f in $SOURCES; do
  if [ "$f.hip" != "$src" ] && { [ ! -f $O/$f.o ] || [ $C/$f.hip -nt $O/$f.o ] || [ -n "$(find $C $ROOT/include -name '*.h*' -newer $O/$f.o | grep -v '\.hip$')" ]; }; then
    hipcc $FLAGS -c $C/$f.hip -o $O/$f.o & pids+=($!)
  fi
done
tag=$(echo "$src $@" | md5sum | cut -c1-8)
hipcc $FLAGS "$@" -c $C/$src -o $O/var_$tag.o
for p in "${pids[@]}"; do wait $p; done
objs=""
for f in $SOURCES; do
  if [ "$f.hip" == "$src" ]; then objs="$objs $O/var_$tag.o"; else objs="$objs $O/$f.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $out $objs
echo built $out
