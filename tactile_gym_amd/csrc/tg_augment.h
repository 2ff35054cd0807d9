// tg_augment.h - launch interface of the RAD translate augmentation (tg_augment.hip: k_random_translate; tg_random_translate).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tg {

// One call of kornia's RandomAffine(degrees=0, translate=(ax, ay), scale=(1, 1), p) over a [B][C][H][W] (channels first) or [B][H][W][C]
// (channels last) batch of uint8 or float32 images, out of place, float32 output in the same layout.  A sample is P planes of H rows of R
// elements: channels first P = C, R = W, a horizontal tap step of S = 1 element; channels last P = 1, R = W * C, S = C.
struct TranslateArgs {
    const void* in = nullptr;
    float* out = nullptr;
    const float* params_in = nullptr;   // [B][3] (apply, tx, ty) in pixels; null: drawn from (seed, counter)
    float* params_out = nullptr;        // [B][3] written by one lane per sample; may be null
    const int64_t* rows = nullptr;      // [B] source sample of every output sample (tg_random_translate_rows); null: sample b reads sample b
    int64_t B = 0;
    int C = 0, H = 0, W = 0;
    float ax_w = 0.f, ay_h = 0.f, p = 0.f;   // (float)(ax * W), (float)(ay * H), p
    uint64_t seed = 0, counter = 0;
};
enum { kTranslateU8 = 0, kTranslateF32 = 1 };
// 0, or -1 for arguments the kernel is not built for.  Enqueued on `stream`; nothing is allocated or synchronised.
int launch_random_translate(const TranslateArgs& a, int in_dtype, int channels_first, hipStream_t stream);

}  // namespace tg
