// tg_stack.h - launch interface of the device frame stack and observation layout (tg_stack.hip: k_frame_stack, k_obs_stack; tg_set_frame_stack,
// tg_set_obs_layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tg {

constexpr int kStackMax = 8;      // frames per stack (tg_set_frame_stack: 1 <= n <= 8; the per-block record is one byte)

// One update of every stacked key, stable_baselines3's StackedObservations.update / reset restated per env:
//   mode kStackStep:      every stack shifts one slot toward the oldest and the new frame goes into the newest slot; an env flagged in `flag`
//                         (st.done) first has its terminal stack written (the old stack's newest n - 1 slots, then its terminal frame) when
//                         term_stack / vterm_stack are set, and its older slots are zeroed;
//   mode kStackReset:     the envs flagged in `flag` (all envs when flag is null) get zeros in every slot but the newest, which takes the frame;
//                         the others are left alone.
// Images: uint8 [num_envs][H][W] frames, stacked to [num_envs][H][W][n].  Vectors: float32 rows of `pitch` floats of which the first `dim` are
// stacked to [num_envs][dim * n] (oldest first).  rec[num_envs][blocks]: bit s = slot s of that 16 x 16 block holds the template image.
enum { kStackStep = 0, kStackReset = 1 };
struct StackVec {
    const float* src = nullptr;       // the observation after the step (post-reset rows for finished envs)
    const float* term = nullptr;      // the step's own rows (terminal frames of the finished envs); null: no terminal stack
    float* stack = nullptr;
    float* term_stack = nullptr;
    int dim = 0, pitch = 0;
};
struct StackArgs {
    int num_envs = 0, H = 0, W = 0, n = 1, mode = kStackStep, rewrite_all = 0;
    const uint8_t* flag = nullptr;    // step: st.done; reset: the reset mask (null: every env)
    const uint8_t* frame = nullptr;   // null: no image stack
    const uint8_t* term_frame = nullptr;
    const uint8_t* tmpl = nullptr;    // [H][W] the untouched sensor's image (tg_ctx.d_tile_tmpl)
    uint8_t* stack = nullptr;
    uint8_t* term_stack = nullptr;    // null: no terminal stack (auto_reset off, or a reset)
    uint8_t* rec = nullptr;
    StackVec vec[2];                  // oracle, extended_feature (dim 0: absent)
};
int launch_frame_stack(const StackArgs& a, hipStream_t stream);   // 0, or -1 for arguments the kernel is not built for

// The scene camera's images (tg_set_scene every step): uint8 [num_envs][H][W][3] frames, stacked to [num_envs][H][W][3 n] (channels last; slot s at
// bytes 3 s .. 3 s + 2 of a pixel) or [num_envs][3 n][H][W] (channels first; slot s colour c is plane 3 s + c).  Same update rules as StackArgs.
struct VisStack {
    const uint8_t* frame = nullptr;   // d_vis; null: no visual stack
    const uint8_t* term_frame = nullptr;
    uint8_t* stack = nullptr;
    uint8_t* term_stack = nullptr;    // null: no terminal stack
    int H = 0, W = 0;
};
// The stacks with a visual key or channels first (tg_set_obs_layout).  channels_first: ONE launch of k_obs_stack for the tactile image
// ([num_envs][n][H][W], n >= 2; a.frame null: none), the vectors and the visual image.  n = 1 stacks the visual image only (its planar copy): the
// tactile image [num_envs][H][W] is already [num_envs][1][H][W].  Channels last: k_frame_stack (a.n >= 2, unchanged), then k_obs_stack for the
// visual image.  0, or -1 for arguments the kernels are not built for.
int launch_obs_stack(const StackArgs& a, const VisStack& v, int channels_first, hipStream_t stream);

}  // namespace tg
