#!/bin/bash
# Build libvvhip.so for gfx950 (MI355X).  The only list of sources and per-file flags:
#   build.sh                                          the product library, next to this file
#   build.sh --out FILE [--src DIR] [hipcc flags...]  another build of it for an A/B of two libraries (tools/build_variant.sh, tools/ab_libs.sh): written to FILE,
#                                                     sources taken from DIR (the videovanish_amd/csrc of a tree at another revision, `git archive REV videovanish_amd/csrc include`;
#                                                     default: this directory), extra flags on every compile; objects in their own directory, the product build is not touched
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
SRC=$HERE; OUT=$HERE/libvvhip.so; OBJ=$HERE/build
while [ $# -gt 0 ]; do
  case $1 in
    --src) SRC=$(cd "$2" && pwd); shift 2 ;;
    --out) mkdir -p "$(dirname "$2")"; OUT=$(cd "$(dirname "$2")" && pwd)/$(basename "$2"); OBJ=$HERE/build/$(basename "$2" .so); shift 2 ;;
    *) break ;;
  esac
done
EXTRA="$*"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function $EXTRA"
mkdir -p $OBJ
# objects of another source directory or other flags are stale
if [ "$(cat $OBJ/.stamp 2>/dev/null)" != "$SRC $EXTRA" ]; then rm -f $OBJ/*.o; echo "$SRC $EXTRA" > $OBJ/.stamp; fi
cd $SRC
pids=(); objs=()
compile() {   # compile <src> <obj> [extra flags]
  local src=$1 obj=$OBJ/$2.o stale=; shift 2
  objs+=($obj)
  for dep in $src.hip *.h ../../include/vvhip.h ../../include/vvspans.h ../../include/vvmask.h ../../include/vvtone.h ../../include/vvgrain.h ../../include/vvblend.h ../../include/vvplate.h ../../include/vvplategrain.h ../../include/vvalign.h ../../include/vvflicker.h ../../include/vvflickalign.h ../../include/vvshadow.h ../../include/platetone.h ../../include/detailmatch.h ../../include/grainshape.h ../../include/flicklocal.h ../../include/overlaymask.h ../../include/platewarp.h $HERE/build.sh; do
    if [ ! -f $obj ] || [ $dep -nt $obj ]; then stale=1; fi
  done
  if [ -n "$stale" ]; then
    hipcc $FLAGS "$@" -c $src.hip -o $obj &
    pids+=($!)
  fi
}
# the two GEMM sources hold every tile form x loader mode x operand type: one translation unit per operand type (BF16 / F16) halves the longest pole
for f in vv_gemm vv_gemm256; do
  compile $f ${f}_bf16 -DVV_DT_ONLY=0
  compile $f ${f}_f16 -DVV_DT_ONLY=1
done
for f in vv_api vv_motion vv_chain vv_norm vv_elem vv_image vv_roi vv_spans vv_mask vv_tone vv_grain vv_grainshape vv_blend vv_detail vv_plate vv_platetone vv_platewarp vv_shadow vv_overlay vv_align vv_flicker vv_flicklocal vv_flow vv_deform vv_sam2; do
  compile $f $f
done
# attention, small head dims: MFMA results feed VALU code (softmax) every tile -> keep accumulators in arch VGPRs
# (no v_accvgpr_read/write traffic); large head dims need the AGPR half of the register file
compile vv_attn vv_attn_small -DVV_ATTN_PART=0 -mllvm -amdgpu-mfma-vgpr-form
compile vv_attn32 vv_attn32 -mllvm -amdgpu-mfma-vgpr-form      # d = 40 / 80 on the 32x32x16 MFMA (the dominant kernels)
compile vv_attn vv_attn_large -DVV_ATTN_PART=1
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT "${objs[@]}"
echo "built $OUT"
# host-side frame I/O codec (FFV1, plain C, no GPU): libvvio.so
cd $HERE
if [ ! -f libvvio.so ] || [ vv_ffv1.c -nt libvvio.so ]; then
  gcc -O2 -std=c99 -fPIC -shared -Wall -o libvvio.so vv_ffv1.c
fi
