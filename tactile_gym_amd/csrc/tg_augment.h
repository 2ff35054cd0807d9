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

constexpr int kTrChunk = 4096;    // output elements per workgroup: 4 float4 per lane
constexpr int kTrMaxRow = 8192;   // R + S of the staged path: LDS <= (4096 + 8192 + 44) * 4 B = 48.2 KiB

// How a call is launched - the one place that decides it (launch_typed; the test library reports it: tg_selftest_translate_plan).
// vec: the staged path - the plane is a multiple of 16 bytes of input and of 4 floats of output, both pointers are 16-byte aligned and
// R + S <= kTrMaxRow; else the per-element path.  One workgroup per (sample, plane, chunk); a launch holds at most 2^23 of them (grid x * 256
// lanes stays below 2^32): spl samples, 0 when one sample alone has more.
struct TranslatePlan {
    int vec, nchunk, lds_floats;
    int64_t per_sample, spl;
};
inline TranslatePlan translate_plan(int elem_bytes, bool channels_first, int C, int H, int W, uintptr_t in, uintptr_t out) {
    const int P = channels_first ? C : 1, R = channels_first ? W : W * C, S = channels_first ? 1 : C;
    const int64_t HR = (int64_t)H * R;
    const int V = 16 / elem_bytes;
    TranslatePlan p;
    p.nchunk = (int)((HR + kTrChunk - 1) / kTrChunk);
    p.vec = HR % V == 0 && !((in | out) & 15) && R + S <= kTrMaxRow;
    p.lds_floats = p.vec ? (kTrChunk + R + S + 2 * V + 12 + 3) / 4 * 4 : 0;
    p.per_sample = (int64_t)P * p.nchunk;
    p.spl = ((int64_t)1 << 23) / p.per_sample;
    return p;
}

}  // namespace tg
