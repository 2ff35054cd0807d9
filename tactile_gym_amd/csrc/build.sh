#!/bin/bash
# Builds libtactile_gym_hip.so (the product) and libtactile_gym_hip_test.so (device self-tests, loaded by tests/ only) for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
#   tg_raster.hip, tg_scene.hip, tg_noise.hip, tg_augment.hip (the RAD translate augmentation, bit-exact specification: DESIGN.md 4.8; tg_augment_core.h holds what it shares with tg_affine.hip) and tg_rollout.hip (the device rollout buffer, bit-exact GAE: DESIGN.md 4.9), tg_replay.hip (the device replay buffer: DESIGN.md 4.10), tg_affine.hip (the general affine augmentation, bit-exact warp: DESIGN.md 4.11), tg_vecnorm.hip (the device VecNormalize, bit-exact float64 statistics: DESIGN.md 4.12), tg_action_head.hip (the device action heads, one rounding per float32 operation: DESIGN.md 4.13), tg_conv_stem.hip (the device conv stem on the f32 MFMA, one k-ordered fmaf chain per output: DESIGN.md 4.14), tg_loss_head.hip (the device loss heads, one rounding per float32 operation and double row sums in a fixed order; tg_head_core.h holds what it shares with tg_action_head.hip: DESIGN.md 4.15), tg_sac_loss.hip (SAC's device losses, the same rules; tg_loss_core.h holds the chunk sum it shares with tg_loss_head.hip: DESIGN.md 4.16), tg_mlp.hip (the device MLP towers on the f32 MFMA - SB3's policy, value and critic heads, one k-ordered fmaf chain per output: DESIGN.md 4.17), tg_conv.hip (the device NatureCNN tail - conv2, conv3 and the linear layer as one convolution family on the f32 MFMA, one k-ordered fmaf chain per output: DESIGN.md 4.21) are compiled with -ffp-contract=off (bit-exact raster specification);
#   tg_api.hip (configuration, creation, step / reset launches; + tg_api_obs.hip - the observation entries, no kernel of its own -, tg_api_state.hip, tg_api_ops.hip: the rest of the C ABI, sharing tg_ctx.hpp), tg_contact_wave.hip (wave-per-env contact solver) and tg_exchange.hip (multi-GPU payloads, integer only), tg_stack.hip (the frame stack, byte moves only) with the default contraction (FMA); tg_narrow_test.hip (GJK / EPA self-test) switches contraction off by pragma; tg_stack_test.hip (the test entry of the frame-stack launchers, no kernel of its own) needs no flag; tg_physics_test.hip (the test entry of tg_physics.hpp's helpers) keeps FMA, as tg_api.hip compiles them; tg_state_test.hip (the test entry that writes object states into a context, no kernel of its own) needs no flag; tg_fused.hip (step + render in one launch) keeps FMA for the physics and
#   takes the raster from tg_raster_dev.hpp, whose pragma switches contraction off for everything after it.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${TG_OUT:-../lib}      # TG_OUT: another output directory (audit / A-B builds: TG_EXTRA_FLAGS=... TG_OUT=../lib_audit, loaded with TG_HIP_LIBRARY)
mkdir -p "$OUT"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value ${TG_EXTRA_FLAGS:-}"
# TG_INCREMENTAL=1 (development): keep an object whose translation unit and every header are older than it
stale() {   # stale <object> <source>: 0 if the object must be rebuilt
    [ "${TG_INCREMENTAL:-0}" = "1" ] || return 0
    [ -f "$1" ] || return 0
    for f in "$2" *.hpp *.h ../../include/*.h; do [ "$f" -nt "$1" ] && return 0; done
    return 1
}
cc() {      # cc <name> <extra flags...>
    local name=$1; shift
    if stale "$OUT/$name.o" "$name.hip"; then rm -f "$OUT/$name.o"; $HIPCC $COMMON "$@" -c "$name.hip" -o "$OUT/$name.o"; fi
}
cc tg_raster -ffp-contract=off & p1=$!
cc tg_noise -ffp-contract=off & p2=$!
cc tg_api & p3=$!
cc tg_contact_wave & p4=$!
cc tg_scene -ffp-contract=off & p5=$!
cc tg_exchange & p6=$!
cc tg_narrow_test & p7=$!
cc tg_fused & p8=$!
cc tg_selftest -ffp-contract=off & p9=$!
cc tg_broadphase -ffp-contract=off & p10=$!
cc tg_api_state & p11=$!
cc tg_api_ops & p12=$!
cc tg_spin & p13=$!
cc tg_render_test & p14=$!
cc tg_stack & p15=$!
cc tg_augment -ffp-contract=off & p16=$!
cc tg_rollout -ffp-contract=off & p17=$!
cc tg_scene_test & p18=$!
cc tg_replay -ffp-contract=off & p19=$!
cc tg_affine -ffp-contract=off & p20=$!
cc tg_vecnorm -ffp-contract=off & p21=$!
cc tg_stack_test & p22=$!
cc tg_action_head -ffp-contract=off & p23=$!
cc tg_conv_stem -ffp-contract=off & p24=$!
cc tg_loss_head -ffp-contract=off & p25=$!
cc tg_sac_loss -ffp-contract=off & p26=$!
cc tg_mlp -ffp-contract=off & p27=$!
cc tg_api_obs & p28=$!
cc tg_physics_test & p29=$!
cc tg_state_test & p30=$!
cc tg_conv -ffp-contract=off & p31=$!
wait $p1; wait $p2; wait $p3; wait $p4; wait $p5; wait $p6; wait $p7; wait $p8; wait $p9; wait $p10; wait $p11; wait $p12; wait $p13; wait $p14; wait $p15; wait $p16; wait $p17; wait $p18; wait $p19; wait $p20; wait $p21; wait $p22; wait $p23; wait $p24; wait $p25; wait $p26; wait $p27; wait $p28; wait $p29; wait $p30; wait $p31    # each wait returns its job's status: a failed translation unit fails the build (set -e)
$HIPCC --offload-arch=gfx950 -shared -fPIC "$OUT/tg_raster.o" "$OUT/tg_noise.o" "$OUT/tg_api.o" "$OUT/tg_contact_wave.o" "$OUT/tg_scene.o" "$OUT/tg_exchange.o" "$OUT/tg_fused.o" "$OUT/tg_broadphase.o" "$OUT/tg_api_state.o" "$OUT/tg_api_ops.o" "$OUT/tg_spin.o" "$OUT/tg_stack.o" "$OUT/tg_augment.o" "$OUT/tg_rollout.o" "$OUT/tg_replay.o" "$OUT/tg_affine.o" "$OUT/tg_vecnorm.o" "$OUT/tg_action_head.o" "$OUT/tg_conv_stem.o" "$OUT/tg_loss_head.o" "$OUT/tg_sac_loss.o" "$OUT/tg_mlp.o" "$OUT/tg_conv.o" "$OUT/tg_api_obs.o" -o "$OUT/libtactile_gym_hip.so"
# (tg_api_obs.o, a unit without kernels, is linked last: the code objects of the units that have kernels keep the places they had in the library
#  before it existed - profiles/obs_table_rate.txt, section 3.)
# test infrastructure (include/tactile_gym_hip_test.h): device self-tests of the raster's division / block test and of the wave-mapped GJK / EPA,
# the render with a chosen kernel (with the product's own raster object), the scene camera on any triangle set (with the product's own tg_scene.o),
# the frame-stack launchers on raw buffers (tg_stack_test.hip, with the product's own tg_stack.o), the physics helpers one by one (tg_physics_test.hip),
# the state-injection entry of the step-kernel tests (tg_state_test.hip: host code over tg_ctx.hpp, nothing from the product's objects)
$HIPCC --offload-arch=gfx950 -shared -fPIC "$OUT/tg_narrow_test.o" "$OUT/tg_selftest.o" "$OUT/tg_render_test.o" "$OUT/tg_scene_test.o" "$OUT/tg_stack_test.o" "$OUT/tg_physics_test.o" "$OUT/tg_state_test.o" "$OUT/tg_raster.o" "$OUT/tg_scene.o" "$OUT/tg_stack.o" -o "$OUT/libtactile_gym_hip_test.so"
echo "built $OUT/libtactile_gym_hip.so $OUT/libtactile_gym_hip_test.so"
