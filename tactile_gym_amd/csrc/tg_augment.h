// tg_augment.h - launch interface of the RAD translate augmentation (tg_augment.hip: k_random_translate; tg_random_translate).
#pragma once
#include "tg_augment_core.h"

namespace tg {

// One call of kornia's RandomAffine(degrees=0, translate=(ax, ay), scale=(1, 1), p) over a [B][C][H][W] (channels first) or [B][H][W][C]
// (channels last) batch of uint8 or float32 images, out of place, float32 output in the same layout (planes, rows and tap step: PlaneGeom).
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
// in_dtype: TG_AUGMENT_*.  0, -1 for arguments the kernel is not built for, -2 when the launch failed.  Enqueued on `stream`; nothing is
// allocated or synchronised.
int launch_random_translate(const TranslateArgs& a, int in_dtype, int channels_first, hipStream_t stream);

constexpr int kTrMaxRow = 8192;   // R + S of the staged path: LDS <= (4096 + 8192 + 44) * 4 B = 48.2 KiB

// How a call is launched - the one place that decides it (launch_typed; the test library reports it: tg_selftest_translate_plan).
// vec: the staged path - the plane is a multiple of 16 bytes of input and of 4 floats of output, both pointers are 16-byte aligned and
// R + S <= kTrMaxRow; else the per-element path.  The workgroups and launches: ChunkPlan.
struct TranslatePlan : ChunkPlan {
    int vec, lds_floats;
};
inline TranslatePlan translate_plan(int elem_bytes, bool channels_first, int C, int H, int W, uintptr_t in, uintptr_t out) {
    const PlaneGeom g = plane_geom(channels_first, C, H, W);
    const int V = 16 / elem_bytes;
    TranslatePlan p{chunk_plan(g)};
    p.vec = g.HR % V == 0 && !((in | out) & 15) && g.R + g.S <= kTrMaxRow;
    p.lds_floats = p.vec ? (kAugChunk + g.R + g.S + 2 * V + 12 + 3) / 4 * 4 : 0;
    return p;
}

}  // namespace tg
