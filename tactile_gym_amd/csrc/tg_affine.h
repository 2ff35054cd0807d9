// tg_affine.h - launch interface of the general affine augmentation (tg_affine.hip: k_random_affine; tg_random_affine).
#pragma once
#include "tg_augment_core.h"

namespace tg {

// One call of kornia's RandomAffine(degrees, translate, scale, shear, p) - its defaults otherwise: bilinear, zero padding, align_corners=False,
// per-sample draws - over a [B][C][H][W] (channels first) or [B][H][W][C] (channels last) batch of uint8 or float32 images, out of place,
// float32 output in the same layout (planes, rows and tap step: PlaneGeom).
struct AffineArgs {
    const void* in = nullptr;
    float* out = nullptr;
    const float* params_in = nullptr;   // [B][8] (apply, tx, ty, angle, scale_x, scale_y, shear_x, shear_y); null: drawn from (seed, counter)
    float* params_out = nullptr;        // [B][8] written by one lane per sample; may be null
    const float* coeffs_in = nullptr;   // [B][6] (a00, a01, a02, a10, a11, a12) used as they are; null: computed from the parameters
    float* coeffs_out = nullptr;        // [B][6] written by one lane per sample; may be null
    const int64_t* rows = nullptr;      // [B] source sample of every output sample; null: sample b reads sample b
    int64_t B = 0;
    int C = 0, H = 0, W = 0;
    float ax_w = 0.f, ay_h = 0.f, p = 0.f;   // (float)(ax * W), (float)(ay * H), p
    float d0 = 0.f, d1 = 0.f;                // degrees
    float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
    int scale4 = 0;                          // 0: scale_y = scale_x
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;   // shear, degrees
    uint64_t seed = 0, counter = 0;
};
// in_dtype: TG_AUGMENT_*.  0, -1 for arguments the kernel is not built for, -2 when the launch failed.  Enqueued on `stream`; nothing is
// allocated or synchronised.
int launch_random_affine(const AffineArgs& a, int in_dtype, int channels_first, hipStream_t stream);

constexpr int kAfHeader = 32;           // bytes of LDS in front of the plane: the sample's coefficients, written by one lane
constexpr int kAfMaxPlane = 32 << 10;   // bytes of a plane (as stored) that the staged path keeps in LDS: five workgroups per CU at the limit

// How a call is launched - the one place that decides it (launch_typed; the test library reports it: tg_selftest_affine_plan).
//   path 2, staged: the source rows that a workgroup's 4096 outputs can reach are copied into LDS as they are stored (16-byte loads) and the taps
//           are read from there.  Needs planes that are a multiple of 16 bytes of input and of 4 floats of output, both pointers 16-byte
//           aligned, and a plane of at most kAfMaxPlane bytes.
//   path 1, gather: the taps are read from global memory, the output is stored as float4.  Needs planes that are a multiple of 4 floats and a
//           16-byte aligned output.
//   path 0, per element: anything else.
// in_vec: samples that are not applied are copied with 16-byte loads (else element loads).  The workgroups and launches: ChunkPlan.
struct AffinePlan : ChunkPlan {
    int path, in_vec, lds_bytes;
};
inline AffinePlan affine_plan(int elem_bytes, bool channels_first, int C, int H, int W, uintptr_t in, uintptr_t out) {
    const PlaneGeom g = plane_geom(channels_first, C, H, W);
    const int64_t HR = g.HR;   // 64 bits: HR * elem_bytes
    const int V = 16 / elem_bytes;
    AffinePlan p{chunk_plan(g)};
    const bool out_vec = HR % 4 == 0 && !(out & 15);
    p.in_vec = out_vec && HR % V == 0 && !(in & 15);
    p.path = p.in_vec && HR * elem_bytes <= kAfMaxPlane ? 2 : out_vec ? 1 : 0;
    p.lds_bytes = kAfHeader + (p.path == 2 ? (int)(HR * elem_bytes) : 0);
    return p;
}

}  // namespace tg
