// tg_augment_core.h - what the two image augmentations share (tg_augment.hip: k_random_translate; tg_affine.hip: k_random_affine), each once:
// the plane geometry and the chunked part of the launch plan, the launch loop, the dtype / layout dispatch and the argument checks of the C
// entries; on the device the 24-bit draw, the 16-byte convert-load, the bilinear blend, the chunk prologue and the not-applied convert-copy.
// The two warps themselves stay apart: their arithmetic specifications differ on purpose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "../../include/tactile_gym_hip.h"   // TG_AUGMENT_UINT8, TG_AUGMENT_FLOAT32: the in_dtype of the launchers and the C entries alike
#include "tg_exchange.h"                      // report_error
#include "tg_kernels.hpp"                     // counter_draw: tg_sample_actions' counter-based generator

namespace tg {

constexpr int kAugThreads = 256;                      // lanes per workgroup
constexpr int kAugChunk = 4096;                       // output elements per workgroup: 4 float4 per lane
constexpr int64_t kAugMaxGroups = (int64_t)1 << 23;   // workgroups per launch: grid x * 256 lanes stays below 2^32

// A sample is P planes of H rows of R elements, HR elements a plane, a horizontal tap step of S elements: channels first P = C, R = W, S = 1;
// channels last P = 1, R = W * C, S = C.  (C H W <= 2^30 is checked in front of every use: everything fits an int.)
struct PlaneGeom {
    int P, R, S, HR;
};
__host__ __device__ inline PlaneGeom plane_geom(bool channels_first, int C, int H, int W) {
    const int R = channels_first ? W : W * C;
    return {channels_first ? C : 1, R, channels_first ? 1 : C, H * R};
}

// The part of a launch plan that both kernels share: one workgroup per (sample, plane, chunk of kAugChunk elements); a launch holds at most
// kAugMaxGroups of them: spl samples, 0 when one sample alone has more.
struct ChunkPlan {
    int nchunk;
    int64_t per_sample, spl;
};
inline ChunkPlan chunk_plan(const PlaneGeom& g) {
    const int nchunk = (g.HR + kAugChunk - 1) / kAugChunk;
    return {nchunk, (int64_t)g.P * nchunk, kAugMaxGroups / ((int64_t)g.P * nchunk)};
}

// launch(b0, grid) for every spl samples of the batch.  0, -1 when one sample has more workgroups than a launch holds, -2 when a launch failed.
template <typename F>
inline int launch_chunks(int64_t B, const ChunkPlan& pl, F&& launch) {
    if (pl.spl < 1) return -1;
    for (int64_t b0 = 0; b0 < B; b0 += pl.spl) launch(b0, dim3((unsigned)((B - b0 < pl.spl ? B - b0 : pl.spl) * pl.per_sample)));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// What is wrong with the shape of an image batch, or nullptr (the C entries, the launchers and the test library's plan entries).
inline const char* image_shape_fault(int32_t in_dtype, int64_t B, int32_t C, int32_t H, int32_t W) {
    if (in_dtype != TG_AUGMENT_UINT8 && in_dtype != TG_AUGMENT_FLOAT32) return "unknown input dtype";
    if (B < 0 || C < 1 || H < 2 || W < 2) return "need B >= 0, C >= 1, H >= 2, W >= 2";
    if ((int64_t)C * H * W > (1 << 30)) return "more than 2^30 elements per image";
    return nullptr;
}

// typed(TIN(), std::bool_constant<channels first>()) for a batch to launch; 0 for an empty one, -1 for one the kernels are not built for.
template <typename F>
inline int dispatch_images(const void* in, const void* out, int in_dtype, int channels_first, int64_t B, int C, int H, int W, F&& typed) {
    if (image_shape_fault(in_dtype, B, C, H, W)) return -1;
    if (B == 0) return 0;
    if (!in || !out) return -1;
    if (in_dtype == TG_AUGMENT_UINT8) return channels_first ? typed(uint8_t(), std::true_type()) : typed(uint8_t(), std::false_type());
    return channels_first ? typed(float(), std::true_type()) : typed(float(), std::false_type());
}

// The argument checks that the C entries over an image batch share; `name` starts the message.  0, or the reported -1.
inline int check_image_call(const char* name, const void* in, const void* out, int32_t in_dtype, int64_t B, int32_t C, int32_t H, int32_t W,
                            double ax, double ay, float p, bool has_rows) {
    const auto bad = [name](const char* what) { return report_error(-1, (std::string(name) + ": " + what).c_str()); };
    if (const char* what = image_shape_fault(in_dtype, B, C, H, W)) return bad(what);
    if (!(ax >= 0.0 && ax <= 1.0 && ay >= 0.0 && ay <= 1.0)) return bad("translate must lie in [0, 1]");
    if (!(p >= 0.f && p <= 1.f)) return bad("p must lie in [0, 1]");
    if (B > 0 && (!in || !out)) return bad("NULL image pointer");
    const uint64_t n = (uint64_t)B * C * H * W, ib = (uint64_t)(uintptr_t)in, ob = (uint64_t)(uintptr_t)out;
    const uint64_t in_bytes = n * (in_dtype == TG_AUGMENT_UINT8 ? 1 : 4), out_bytes = n * 4;
    if (!has_rows && ib < ob + out_bytes && ob < ib + in_bytes) return bad("the output overlaps the input (out of place only)");
    return 0;
}

// The fields that TranslateArgs and AffineArgs share, from the arguments of a C entry.
template <typename A>
inline A image_args(const void* in, void* out, const float* params_in, float* params_out, const int64_t* rows, int64_t B, int C, int H, int W,
                    double ax, double ay, float p, uint64_t seed, uint64_t counter) {
    A a;
    a.in = in, a.out = (float*)out, a.params_in = params_in, a.params_out = params_out, a.rows = rows;
    a.B = B, a.C = C, a.H = H, a.W = W;
    a.ax_w = (float)(ax * W), a.ay_h = (float)(ay * H), a.p = p;
    a.seed = seed, a.counter = counter;
    return a;
}

// Uniform in [0, 1): the 24 high bits of element i of draw `counter`.
__device__ __forceinline__ float draw_u24(uint64_t seed, uint64_t counter, uint64_t i) {
    return (float)(uint32_t)(counter_draw(seed, counter, i) >> 40) * (1.0f / 16777216.0f);
}

// One aligned 16-byte load of input converted to float32 at d: 4 floats, or 16 from uint8.  (4-byte uint8 loads, which would keep every lane's
// float4 next to its neighbour's, measured 10 % slower.)
__device__ __forceinline__ void store16(float* d, const float* p) { *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void store16(float* d, const uint8_t* p) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(d + 4 * q) = make_float4((float)(w[q] & 0xffu), (float)((w[q] >> 8) & 0xffu), (float)((w[q] >> 16) & 0xffu),
                                                            (float)(w[q] >> 24));
}

// Bilinear: taps a, b on the upper row, c, d on the lower; one rounding per operation.
__device__ __forceinline__ float blend(float a, float b, float c, float d, float fx, float fy) {
    const float h0 = (1.f - fx) * a + fx * b;
    const float h1 = (1.f - fx) * c + fx * d;
    return (1.f - fy) * h0 + fy * h1;
}

// Workgroup blockIdx.x of a launch that starts at sample b0: its sample b, its index rem within the sample (0: the sample's first workgroup),
// its plane pl and its chunk [f0, fend) of the plane.
__device__ __forceinline__ void chunk_of(const PlaneGeom& g, int nchunk, int64_t b0, int64_t& b, int& rem, int& pl, int& f0, int& fend) {
    const int per_sample = g.P * nchunk;
    const int bl = (int)(blockIdx.x / (unsigned)per_sample);
    rem = (int)blockIdx.x - bl * per_sample;
    b = b0 + bl;
    pl = rem / nchunk;
    f0 = (rem - pl * nchunk) * kAugChunk;
    fend = g.HR - f0 < kAugChunk ? g.HR : f0 + kAugChunk;
}

// Plane pl of sample b of a batch.  The source sample of output sample b is rows[b] with a row table (the device buffers' minibatch gathers,
// DESIGN.md 4.9), else b: only the workgroup's source base moves.
template <typename T>
__device__ __forceinline__ T* plane_of(T* base, const int64_t* rows, int64_t b, int pl, const PlaneGeom& g) {
    return base + ((rows ? rows[b] : b) * g.P + pl) * (int64_t)g.HR;
}

// A sample that is not applied: elements [f0, fend) of the plane converted to float32.  in_vec: 16-byte loads and stores; else out_vec: element
// loads and 16-byte stores; else element by element.
template <typename TIN>
__device__ __forceinline__ void convert_copy(const TIN* in, float* out, int f0, int fend, int tid, int in_vec, int out_vec) {
    if (in_vec) {
        if (sizeof(TIN) == 1) {
            const int f = f0 + 16 * tid;
            if (f < fend) store16(out + f, in + f);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int f = f0 + 4 * tid + 1024 * k;
                if (f < fend) store16(out + f, in + f);
            }
        }
    } else if (out_vec) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = f0 + 4 * tid + 1024 * k;
            if (f < fend) *reinterpret_cast<float4*>(out + f) = make_float4((float)in[f], (float)in[f + 1], (float)in[f + 2], (float)in[f + 3]);
        }
    } else {
        for (int f = f0 + tid; f < fend; f += kAugThreads) out[f] = (float)in[f];
    }
}

}  // namespace tg
