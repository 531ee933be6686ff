#!/bin/bash
# Builds libguidegen_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -fno-gpu-rdc"
# GG_CLEAN=1: drop every object first, so that the build is a real one (the driver's build() on a tree that carries old .o files)
if [ "${GG_CLEAN:-0}" = "1" ]; then rm -f ./*.o libguidegen_hip.so; fi
# an object is rebuilt when it is missing or older than its source or than ANY header: every *.h / *.inc here and the public header
stale() {
  [ -f $1.o ] || return 0
  for dep in $1.hip ./*.h ./*.inc ../../include/guidegen_hip.h; do
    if [ "$dep" -nt $1.o ]; then return 0; fi
  done
  return 1
}
OBJS=()
PIDS=()
for f in gg_conv gg_conv_halo gg_conv_halo3 gg_conv_box gg_conv_box_spec gg_conv_tiny gg_conv_tile gg_norm gg_attn gg_sampler gg_loss gg_patchgan gg_vq gg_metrics gg_components gg_surface gg_lpips gg_render gg_fold gg_f32 gg_resample gg_cond gg_ubench; do
  if stale $f; then
    echo "hipcc $f.hip"
    EXTRA=""
    # attention: MFMA results feed VALU softmax code directly; without this the compiler parks the score tiles in AGPRs and pays
    # ~250 v_accvgpr moves per 256-key tile
    if [ $f = gg_attn ]; then EXTRA="-mllvm -amdgpu-mfma-vgpr-form"; fi
    rm -f $f.o             # a failed compile must not leave the previous object to be linked
    $HIPCC $FLAGS $EXTRA -c $f.hip -o $f.o &
    PIDS+=($!)
  fi
  OBJS+=($f.o)
done
for pid in "${PIDS[@]:-}"; do
  if [ -n "$pid" ]; then wait "$pid" || { echo "build.sh: a compile failed" >&2; exit 1; }; fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o libguidegen_hip.so "${OBJS[@]}"
echo "built $(pwd)/libguidegen_hip.so"
