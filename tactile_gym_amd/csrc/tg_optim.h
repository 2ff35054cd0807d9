// tg_optim.h - the device Adam (tactile_gym_amd.optim.DeviceAdam): torch.nn.utils.clip_grad_norm_ and torch.optim.Adam's step
// over every tensor of an optimiser in two launches, the plain step in one.  Included by tg_loss_head.hip alone, whose flag
// (-ffp-contract=off) makes the lines below a specification: float32 arithmetic with one rounding per operation in the order written, which
// tests/optim_ref.py restates.
//   k_optim_sumsq       one workgroup per chunk: the chunk's sum of g^2, in double, into partials[chunk]
//   k_optim_adam<CLIP>  one workgroup per chunk: (CLIP) every workgroup adds ALL the partials in index order, forms the total norm and the
//                       coefficient itself, so no launch stands between the two; then Adam on its chunk
// A chunk is TG_OPTIM_CHUNK consecutive elements of ONE tensor (the last chunk of a tensor is short); the chunks of the tensors follow each
// other in the order of the call.  The tensor table travels by value in the kernel arguments (the gradients' addresses change every
// step: nothing to keep in device memory); a workgroup finds its tensor by a search over the table's first-chunk column, wave-uniform.
// The sum of squares of a chunk: lane t of 256 adds, in double, the squares of elements 4 (256 k + t) + j of the chunk, k = 0 .. 3 outer,
// j = 0 .. 3 inner (an element past the tensor's end counts as 0); the 256 lane sums by tg_loss_core.h's tree.  That order holds whether
// the elements come as 16-byte vectors (base 16-byte aligned and four elements left) or one by one: the result depends on the sizes alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_loss_core.h"  // the 256-lane sum (slot_put, slot_get)

namespace tg {

constexpr int kOptimVec = 4;                                                   // elements of a 16-byte vector
constexpr int kOptimPasses = TG_OPTIM_CHUNK / (kLossThreads * kOptimVec);      // 4
static_assert(kOptimPasses * kLossThreads * kOptimVec == TG_OPTIM_CHUNK, "a chunk is a whole number of passes of the workgroup");

struct OptimTensor {
    float* p;                // the parameter (k_optim_sumsq reads g alone)
    const float* g;
    float* m;                // exp_avg
    float* v;                // exp_avg_sq
    int64_t n;               // elements
    int32_t first_chunk;     // of this tensor, counted over the whole call
    float ss;                // (float) (-lr / (1 - beta1^step))
    float bc2s;              // (float) sqrt(1 - beta2^step)
    int32_t reserved;
};

struct OptimTable {
    OptimTensor t[TG_OPTIM_MAX_TENSORS];
    double* partials;        // k_optim_sumsq: written at the chunk's index; k_optim_adam<true>: read, n_partials of them
    float* total_norm;       // k_optim_adam<true>: written by workgroup 0
    int64_t n_partials;
    int32_t n_tensors;       // used rows of t
    int32_t chunk_base;      // the call-wide index of this launch's first chunk
    float w1, w2, b2, eps, wd, max_norm;
};
static_assert(sizeof(OptimTable) <= 4096, "the table travels in the kernel arguments");

// The row of the table that holds `chunk`: the last one whose first_chunk is <= chunk.
__device__ __forceinline__ int optim_find(const OptimTable& tb, int chunk) {
    int lo = 0, hi = tb.n_tensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tb.t[mid].first_chunk <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Four consecutive elements from x[i ..]: one 16-byte load where `vec` (the base is 16-byte aligned) and four are left, else one by one, 0
// past the end.
__device__ __forceinline__ void optim_load4(const float* x, int64_t i, int64_t n, bool vec, float out[kOptimVec]) {
    if (vec && i + kOptimVec <= n) {
        const float4 q = *reinterpret_cast<const float4*>(x + i);
        out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
    } else {
        for (int j = 0; j < kOptimVec; ++j) out[j] = i + j < n ? x[i + j] : 0.0f;
    }
}

__device__ __forceinline__ void optim_store4(float* x, int64_t i, int64_t n, bool vec, const float in[kOptimVec]) {
    if (vec && i + kOptimVec <= n) {
        *reinterpret_cast<float4*>(x + i) = make_float4(in[0], in[1], in[2], in[3]);
    } else {
        for (int j = 0; j < kOptimVec; ++j)
            if (i + j < n) x[i + j] = in[j];
    }
}

__device__ __forceinline__ bool optim_aligned(const void* a) { return ((uintptr_t)a & 15) == 0; }

// ((0 + partials[0]) + partials[1]) + ... + partials[n - 1], the same in every lane: each wave loads 64 partials at a time, one a lane (the
// next 64 already under way), and adds them in lane order off the lanes' registers.  Past the end a lane holds +0, which leaves a sum that
// started at +0 as it is; one scalar load per partial would pay a memory latency for each.
__device__ __forceinline__ double optim_total(const double* __restrict__ partials, int64_t n) {
    const int lane = (int)threadIdx.x & 63;
    double sum = 0.0;
    double x = lane < n ? partials[lane] : 0.0;
    for (int64_t base = 0; base < n; base += 64) {
        const int64_t ahead = base + 64 + lane;
        const double next = ahead < n ? partials[ahead] : 0.0;
        const int lo = __double2loint(x), hi = __double2hiint(x);
#pragma unroll
        for (int j = 0; j < 64; ++j)
            sum = sum + __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
        x = next;
    }
    return sum;
}

__global__ __launch_bounds__(kLossThreads) void k_optim_sumsq(OptimTable tb) {
    __shared__ double lds[kLossWaves];
    const int chunk = tb.chunk_base + (int)blockIdx.x;
    const OptimTensor& T = tb.t[optim_find(tb, chunk)];
    const float* g = T.g;
    const int64_t n = T.n;
    const int64_t start = (int64_t)(chunk - T.first_chunk) * TG_OPTIM_CHUNK;
    const bool vec = optim_aligned(g);
    double acc = 0.0;
    for (int k = 0; k < kOptimPasses; ++k) {
        const int64_t i = start + (int64_t)(k * kLossThreads + (int)threadIdx.x) * kOptimVec;
        if (i >= n) break;
        float x[kOptimVec];
        optim_load4(g, i, n, vec, x);
        for (int j = 0; j < kOptimVec; ++j) acc = acc + (double)x[j] * (double)x[j];   // the product of two float32 is exact in double
    }
    slot_put(lds, 0, acc);
    __syncthreads();
    if (threadIdx.x == 0) tb.partials[chunk] = slot_get(lds, 0);
}

template <bool CLIP>
__global__ __launch_bounds__(kLossThreads) void k_optim_adam(OptimTable tb) {
    float coef = 1.0f;
    if (CLIP) {                                       // clip_grad_norm_: every workgroup forms the same bits from the same partials
        const double sum = optim_total(tb.partials, tb.n_partials);
        const float total = (float)sqrt(sum);
        const float den = total + 1e-6f;
        const float q = tb.max_norm / den;
        coef = q > 1.0f ? 1.0f : q;                   // torch.clamp(max=1.0): a NaN stays
        if (blockIdx.x == 0 && threadIdx.x == 0) *tb.total_norm = total;
    }
    const int chunk = tb.chunk_base + (int)blockIdx.x;
    const OptimTensor& T = tb.t[optim_find(tb, chunk)];
    float* p = T.p;
    const float* g = T.g;
    float* m = T.m;
    float* v = T.v;
    const int64_t n = T.n;
    const float ss = T.ss, bc2s = T.bc2s;
    const float w1 = tb.w1, w2 = tb.w2, b2 = tb.b2, eps = tb.eps, wd = tb.wd;
    const int64_t start = (int64_t)(chunk - T.first_chunk) * TG_OPTIM_CHUNK;
    const bool vec = optim_aligned(p) && optim_aligned(g) && optim_aligned(m) && optim_aligned(v);
    for (int k = 0; k < kOptimPasses; ++k) {
        const int64_t i = start + (int64_t)(k * kLossThreads + (int)threadIdx.x) * kOptimVec;
        if (i >= n) break;
        float pe[kOptimVec], ge[kOptimVec], me[kOptimVec], ve[kOptimVec];
        optim_load4(p, i, n, vec, pe);
        optim_load4(g, i, n, vec, ge);
        optim_load4(m, i, n, vec, me);
        optim_load4(v, i, n, vec, ve);
        for (int j = 0; j < kOptimVec; ++j) {
            float gj = ge[j];
            if (CLIP) gj = gj * coef;
            if (wd != 0.0f) {
                const float t = wd * pe[j];
                gj = gj + t;
            }
            const float d = gj - me[j];
            const float e = w1 * d;
            me[j] = me[j] + e;
            const float a = ve[j] * b2;
            const float gg = gj * gj;
            const float b = w2 * gg;
            ve[j] = a + b;
            const float s = (float)sqrt((double)ve[j]);   // the correctly rounded float32 root
            const float r = s / bc2s;
            const float den = r + eps;
            const float u = me[j] / den;
            const float step = ss * u;
            pe[j] = pe[j] + step;
        }
        optim_store4(m, i, n, vec, me);
        optim_store4(v, i, n, vec, ve);
        optim_store4(p, i, n, vec, pe);
    }
}

inline int64_t optim_chunks_of(int64_t count) { return (count + TG_OPTIM_CHUNK - 1) / TG_OPTIM_CHUNK; }

// The chunks of the whole call; -1 for a count < 1, -2 for a total past int32.
inline int64_t optim_chunks(int32_t n_tensors, const int64_t* counts) {
    int64_t total = 0;
    for (int32_t i = 0; i < n_tensors; ++i) {
        if (counts[i] < 1) return -1;
        total += optim_chunks_of(counts[i]);
        if (total > INT32_MAX) return -2;
    }
    return total;
}

// The launches of one call: the tensors TG_OPTIM_MAX_TENSORS at a time, each launch's grid its tensors' chunks.  fill(row, i) sets the
// pointers and factors of tensor i; `launch` enqueues the kernel on the filled table.
template <typename Fill, typename Launch>
inline void optim_launches(OptimTable& tb, int32_t n_tensors, const int64_t* counts, Fill fill, Launch launch) {
    int32_t chunk = 0;
    for (int32_t base = 0; base < n_tensors; base += TG_OPTIM_MAX_TENSORS) {
        const int32_t rows = n_tensors - base < TG_OPTIM_MAX_TENSORS ? n_tensors - base : TG_OPTIM_MAX_TENSORS;
        tb.n_tensors = rows;
        tb.chunk_base = chunk;
        for (int32_t r = 0; r < rows; ++r) {
            tb.t[r] = OptimTensor{};
            tb.t[r].n = counts[base + r];
            tb.t[r].first_chunk = chunk;
            fill(tb.t[r], base + r);
            chunk += (int32_t)optim_chunks_of(counts[base + r]);
        }
        launch(tb, (unsigned)(chunk - tb.chunk_base));
    }
}

}  // namespace tg
