#!/bin/bash
# Builds libbsvd_hip.so for gfx950 in-tree (bsvd_amd/libbsvd_hip.so).  hipcc cross-compiles without a GPU.
# Objects are rebuilt when a source / header is newer OR when the compile flags (EXTRA_HIPCC_FLAGS tuning defines
# included) differ from the ones the object was built with (recorded next to it in <obj>.flags).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$ROOT/include -I$HERE -Wall -Wno-unused-function ${EXTRA_HIPCC_FLAGS}"
OUT="${BSVD_OUT:-$ROOT/bsvd_amd/libbsvd_hip.so}"
# objects live outside the package: build/obj (product), build/obj_ab<i> (tools/build_ab.sh variants)
OBJ="$ROOT/build/obj${BSVD_OBJ_SUFFIX:-}"
mkdir -p "$OBJ"
. "$HERE/sources.sh"      # BSVD_SRCS, bsvd_src_flags
SRCS="$BSVD_SRCS"
pids=()
for src in $SRCS; do
  if [ ! -f "$OBJ/$src.o" ] || [ "$HERE/$src.hip" -nt "$OBJ/$src.o" ] || \
     [ "$HERE/bsvd_internal.h" -nt "$OBJ/$src.o" ] || [ "$HERE/wino_forms.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_surface_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_rgb_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_sigma_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_finish_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_nlf_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_vst_items.h" -nt "$OBJ/$src.o" ] || [ "$HERE/frame_grain_items.h" -nt "$OBJ/$src.o" ] || [ "$ROOT/include/bsvd_hip.h" -nt "$OBJ/$src.o" ] || \
     [ "$(cat "$OBJ/$src.flags" 2>/dev/null)" != "$FLAGS" ]; then
    XF="$(bsvd_src_flags $src)"
    ( $HIPCC $FLAGS $XF -c "$HERE/$src.hip" -o "$OBJ/$src.o" && echo "$FLAGS" > "$OBJ/$src.flags" ) &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
OBJS=""; for src in $SRCS; do OBJS="$OBJS $OBJ/$src.o"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC $OBJS -o "$OUT"
echo "built $OUT"
