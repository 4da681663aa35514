#!/bin/bash
# Build libroomnet_hip.so and the test / A-B library libroomnet_hip_ab.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
#
# Every translation unit is named once, in the lists below; the compile loop and the link lines are derived from them.
# Environment (all optional; tools/build_inc.sh, build_variant.sh, build_variant2.sh and build_clock.sh are thin calls of this):
#   RN_FILES="FILE ..."       compile only these files; the other objects are reused from build/obj (run a full build first)
#   RN_VARIANT=NAME           experimental build: RN_FILES are compiled with RN_VARIANT_FLAGS added, into build/var_NAME, and linked
#                             with the other objects of build/obj into tools/ab/libroomnet_hip_NAME.so; the two libraries stay
#   RN_VARIANT_FLAGS="..."    extra hipcc flags of the variant's files (defines, -mllvm options)
#   RN_RW_FLAGS               replaces -mllvm -amdgpu-mfma-vgpr-form for the files of VGPR_FORM
#   RN_EXTRA_FLAGS            added to the link of libroomnet_hip.so
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"

PLAIN="rn_api rn_kernels_f32 rn_fused rn_generic rn_imageops rn_jpeg rn_jpeg_huff rn_jpeg_enc rn_jpeg_huffenc rn_cam_overlay rn_occlusion rn_faith rn_group rn_tail rn_conv16 rn_stage_f32m rn_backend rn_gradcam rn_bnstats rn_finetune rn_finetune7"
# MFMA results stay in VGPRs: the epilogue reads every accumulator with the VALU, and AGPR
# accumulators cost one v_accvgpr_read each (64 per row in the residual variant).
# (max-ilp scheduling was measured slower, see NOTES.md)
VGPR_FORM="rn_stage_rw rn_stage23x rn_stage5x rn_stage4x rn_stage6x"
# the test / A-B library: the same objects + the round-2 comparison kernels (RN_FLAG_PAIR_32X32), which the product library
# does not carry; the files that dispatch to them are compiled again with -DRN_ROUND2_ARMS (host code: rn_fused's only kernel is the
# constant-channel fill)
AB_ONLY="rn_stage23"            # (compiled like VGPR_FORM)
AB_REBUILT="rn_api rn_fused"
# register report: a spill in one of the hot kernels costs ~25 % of its time (seen on the fused stage pair) and hipcc
# does not warn about it
REPORTED="$AB_ONLY $VGPR_FORM rn_tail rn_conv16"

CFLAGS=(--offload-arch=gfx950 -O3 -std=c++20 -fno-slp-vectorize -fPIC -fvisibility=hidden
        -I"$ROOT/include" -I"$HERE" -Wall -Wno-unused-function -DRN_BUILDING)
LINK=("$HIPCC" --offload-arch=gfx950 -shared -fPIC)
OBJ="$ROOT/build/obj"
AB="$OBJ/ab"
VARIANT="${RN_VARIANT:-}"
FILES="${RN_FILES:-$PLAIN $VGPR_FORM $AB_ONLY}"
DEST="$OBJ"
[ -n "$VARIANT" ] && DEST="$ROOT/build/var_$VARIANT"
mkdir -p "$OBJ" "$AB" "$DEST" "$ROOT/roomnet_amd/lib"

has() { [[ " $1 " == *" $2 "* ]]; }
# objects are built separately so that per-file scheduler options can be applied
# (a failed background compile must fail the build: a bare `wait` returns 0 and the link would pick up a stale object)
PIDS=()
compile() {     # compile FILE OBJECT [flags]
    local f="$1" o="$2"
    shift 2
    local form=()
    if has "$VGPR_FORM $AB_ONLY" "$f"; then form=(${RN_RW_FLAGS:--mllvm -amdgpu-mfma-vgpr-form}); fi
    rm -f "$o"
    "$HIPCC" "${CFLAGS[@]}" "${form[@]}" "$@" -c "$HERE/$f.hip" -o "$o" &
    PIDS+=($!)
}
for f in $FILES; do
    has "$PLAIN $VGPR_FORM $AB_ONLY" "$f" || { echo "build.sh: unknown file $f" >&2; exit 2; }
    compile "$f" "$DEST/$f.o" ${VARIANT:+${RN_VARIANT_FLAGS:-}}
    if [ -z "$VARIANT" ] && has "$AB_REBUILT" "$f"; then compile "$f" "$AB/$f.o" -DRN_ROUND2_ARMS; fi
done
for p in "${PIDS[@]}"; do wait "$p"; done

objects() {     # objects LIST: the object of every file of LIST, the variant's own where it has one
    local f
    for f in $1; do
        if [ -n "$VARIANT" ] && has "$FILES" "$f"; then echo "$DEST/$f.o"; else echo "$OBJ/$f.o"; fi
    done
}
if [ -n "$VARIANT" ]; then
    mkdir -p "$ROOT/tools/ab"
    "${LINK[@]}" $(objects "$PLAIN $VGPR_FORM $AB_ONLY") -ldl -lpthread -o "$ROOT/tools/ab/libroomnet_hip_$VARIANT.so"
    echo "built $ROOT/tools/ab/libroomnet_hip_$VARIANT.so"
else
    OUT="$ROOT/roomnet_amd/lib"
    "${LINK[@]}" $(objects "$PLAIN $VGPR_FORM") -ldl -lpthread ${RN_EXTRA_FLAGS:-} -o "$OUT/libroomnet_hip.so"
    echo "built $OUT/libroomnet_hip.so"
    AB_OBJS=()
    for o in $(objects "$PLAIN $VGPR_FORM $AB_ONLY"); do
        if has "$AB_REBUILT" "$(basename "$o" .o)"; then AB_OBJS+=("$AB/$(basename "$o")"); else AB_OBJS+=("$o"); fi
    done
    "${LINK[@]}" "${AB_OBJS[@]}" -ldl -lpthread -o "$OUT/libroomnet_hip_ab.so"
    echo "built $OUT/libroomnet_hip_ab.so"
fi
if [ -x "$ROOT/tools/spills.sh" ]; then
    for f in $REPORTED; do
        if has "$FILES" "$f"; then "$ROOT/tools/spills.sh" "$DEST/$f.o"; fi
    done | awk '$0 ~ /spills +[1-9]/ {print "  spills: " $0}' | cut -c1-70,95-200 || true
fi
