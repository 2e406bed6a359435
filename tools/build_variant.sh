#!/bin/bash
# A/B aid: build tools/_ab/lib_<name>.so from the in-tree objects with ONE source recompiled (default gemm.hip), optionally
# from another copy of that source and with extra hipcc flags.   tools/build_variant.sh <name> [src.hip] [flags...]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$ROOT/multi-modal-retrieval-system-image-search-and-data-governance_amd/csrc
NAME=$1; SRC=${2:-$CS/gemm.hip}; shift; shift || true
BASE=$(basename "$SRC" .hip)
mkdir -p "$ROOT/tools/_ab" /tmp/mmr_variants
EXTRA=$(cd "$CS" && python3 -c 'import build, sys; print(" ".join(build.PER_SOURCE_FLAGS.get(sys.argv[1] + ".hip", [])))' "$BASE")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -Wno-unused-result -Wno-unused-value -I"$CS" $EXTRA "$@" \
    -c "$SRC" -o /tmp/mmr_variants/${NAME}_${BASE}.o
# every object the library links, in build.py's order (its SOURCES list)
SRCS=$(cd "$CS" && python3 -c 'import build; print(" ".join(s.rsplit(".", 1)[0] for s in build.SOURCES))')
OBJS=""
for o in $SRCS; do
  if [ "$o" = "$BASE" ]; then OBJS="$OBJS /tmp/mmr_variants/${NAME}_${BASE}.o"; else OBJS="$OBJS $CS/_obj/$o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/tools/_ab/lib_${NAME}.so" $OBJS -ldl
echo "$ROOT/tools/_ab/lib_${NAME}.so"
