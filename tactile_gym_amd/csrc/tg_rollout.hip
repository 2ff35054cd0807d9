// tg_rollout.hip - the device rollout buffer (tactile_gym_amd.rollout): stable_baselines3's RolloutBuffer / DictRolloutBuffer over
// step-major [T][N][...] storage in device memory.  Compiled with -ffp-contract=off: k_rollout_gae's arithmetic is the bit-exact specification
// the tests restate (tests/rollout_ref.py).
//
//   k_rollout_add      one launch per add(): every observation key and the per-env rows copied into slot pos (tg_rollout_add)
//   k_rollout_gae      SB3's GAE(lambda) recurrence, one lane per env, t = T-1 ... 0 (tg_rollout_gae)
//   k_rollout_gather   one launch per minibatch: rows of every non-image array gathered by storage row (tg_rollout_gather)
// The image keys of a minibatch are gathered by k_random_translate through its row table (tg_augment.hip: tg_random_translate_rows).
//
// Both copy kernels move `units` of 16, 4 or 1 bytes, four per lane and 1024 per workgroup, through a table passed by value: tg_copy_units.hpp (shared with
// tg_replay.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_copy_units.hpp"   // RoTable, move_units, which_array, RO_PICK, widest_unit, push_blocks
#include "tg_exchange.h"   // report_error

namespace tg {

constexpr int kGaeThreads = 64;
constexpr int kGaeBlock = 8;        // steps whose loads are in flight ahead of the chain

__global__ __launch_bounds__(kRoThreads) void k_rollout_add(RoTable t) {
    int64_t u0;
    const int a = which_array(t, u0);
    const uint8_t* src;
    uint8_t* dst;
    int64_t units;
    int32_t unit;
    RO_PICK(src, a, src);
    RO_PICK(dst, a, dst);
    RO_PICK(units, a, units);
    RO_PICK(unit, a, unit);
    if (unit == 0) {   // episode-start flags: uint8 (or bool) -> 0.0f / 1.0f
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t u = u0 + threadIdx.x + kRoThreads * k;
            if (u < units) reinterpret_cast<float*>(dst)[u] = src[u] ? 1.f : 0.f;
        }
        return;
    }
    const uint8_t* s[4];
    uint8_t* d[4];
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t u = u0 + threadIdx.x + kRoThreads * k;
        on[k] = u < units;
        s[k] = src + u * unit;
        d[k] = dst + u * unit;
    }
    move_units(unit, s, d, on);
}

// Output row b of every array is source row rows[b]; a unit g of the array is unit g % upr of row g / upr.
__global__ __launch_bounds__(kRoThreads) void k_rollout_gather(RoTable t, const int64_t* __restrict__ rows, int64_t B) {
    int64_t u0;
    const int a = which_array(t, u0);
    const uint8_t* src;
    uint8_t* dst;
    int64_t upr;
    int32_t unit;
    RO_PICK(src, a, src);
    RO_PICK(dst, a, dst);
    RO_PICK(units, a, upr);
    RO_PICK(unit, a, unit);
    const int64_t total = B * upr;
    const uint8_t* s[4];
    uint8_t* d[4];
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = u0 + threadIdx.x + kRoThreads * k;
        on[k] = g < total;
        const int64_t b = on[k] ? (upr == 1 ? g : g / upr) : 0;
        const int64_t u = g - b * upr;
        s[k] = src + (rows[b] * upr + u) * unit;
        d[k] = dst + g * unit;
    }
    move_units(unit, s, d, on);
}

// adv[t] = last = delta + (gl * nnt) * last, delta = (r[t] + (g * nv) * nnt) - v[t], nnt = 1 - start[t + 1], nv = v[t + 1] (t = T - 1: the caller's
// dones / last_values); ret[t] = last + v[t].  One lane per env, [T][N] arrays: every load is coalesced across the wavefront and independent of
// the chain, so the loads of the next kGaeBlock steps are issued before the current block's chain runs.  The chain itself is one multiply and one
// add per step (delta and gl * nnt do not depend on `last`).
template <typename TD>
__global__ __launch_bounds__(kGaeThreads) void k_rollout_gae(const float* __restrict__ rew, const float* __restrict__ val,
                                                             const float* __restrict__ start, const float* __restrict__ last_values,
                                                             const TD* __restrict__ dones, float* __restrict__ adv, float* __restrict__ ret,
                                                             int64_t T, int64_t N, float g, float gl) {
    // block-uniform bases + a 32-bit lane offset: every access is one scalar base and one VGPR of offset
    const int64_t n0 = (int64_t)blockIdx.x * kGaeThreads;
    const int lane = threadIdx.x;
    if (n0 + lane >= N) return;
    rew += n0; val += n0; start += n0; adv += n0; ret += n0;
    float nv = last_values[n0 + lane];
    float ns = dones[n0 + lane] != (TD)0 ? 1.f : 0.f;
    float last = 0.f;
    float r[kGaeBlock], v[kGaeBlock], s[kGaeBlock];
#pragma unroll
    for (int j = 0; j < kGaeBlock; ++j) {
        const int64_t t = T - 1 - j;
        r[j] = v[j] = s[j] = 0.f;
        if (t >= 0) { r[j] = (rew + t * N)[lane]; v[j] = (val + t * N)[lane]; s[j] = (start + t * N)[lane]; }
    }
    for (int64_t hi = T - 1; hi >= 0; hi -= kGaeBlock) {
        float rn[kGaeBlock], vn[kGaeBlock], sn[kGaeBlock];
#pragma unroll
        for (int j = 0; j < kGaeBlock; ++j) {   // the next block's loads
            const int64_t t = hi - kGaeBlock - j;
            rn[j] = vn[j] = sn[j] = 0.f;
            if (t >= 0) { rn[j] = (rew + t * N)[lane]; vn[j] = (val + t * N)[lane]; sn[j] = (start + t * N)[lane]; }
        }
#pragma unroll
        for (int j = 0; j < kGaeBlock; ++j) {
            const int64_t t = hi - j;
            if (t >= 0) {
                const float nnt = 1.f - ns;
                const float delta = (r[j] + (g * nv) * nnt) - v[j];
                last = delta + (gl * nnt) * last;
                (adv + t * N)[lane] = last;
                (ret + t * N)[lane] = last + v[j];
                nv = v[j];
                ns = s[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kGaeBlock; ++j) { r[j] = rn[j]; v[j] = vn[j]; s[j] = sn[j]; }
    }
}

}  // namespace tg

extern "C" int tg_rollout_add(int32_t n_arrays, const void* const* src_dev, void* const* dst_dev, const int64_t* bytes, const int32_t* kinds,
                              void* hip_stream) {
    using tg::report_error;
    if (n_arrays < 0 || n_arrays > TG_ROLLOUT_MAX_ARRAYS) return report_error(-1, "tg_rollout_add: between 0 and TG_ROLLOUT_MAX_ARRAYS arrays");
    if (n_arrays == 0) return 0;
    if (!src_dev || !dst_dev || !bytes || !kinds) return report_error(-1, "tg_rollout_add: NULL table");
    tg::RoTable t = {};
    int m = 0;
    for (int i = 0; i < n_arrays; ++i) {
        if (kinds[i] != TG_ROLLOUT_COPY && kinds[i] != TG_ROLLOUT_FLAG_U8) return report_error(-1, "tg_rollout_add: unknown array kind");
        if (bytes[i] < 0) return report_error(-1, "tg_rollout_add: negative byte count");
        if (bytes[i] == 0) continue;
        if (!src_dev[i] || !dst_dev[i]) return report_error(-1, "tg_rollout_add: NULL array pointer");
        const uintptr_t s = (uintptr_t)src_dev[i], d = (uintptr_t)dst_dev[i];
        const uint64_t out_bytes = (uint64_t)bytes[i] * (kinds[i] == TG_ROLLOUT_FLAG_U8 ? 4 : 1);
        if (s < d + out_bytes && d < s + (uint64_t)bytes[i]) return report_error(-1, "tg_rollout_add: a destination overlaps its source");
        if (kinds[i] == TG_ROLLOUT_FLAG_U8 && (d & 3)) return report_error(-1, "tg_rollout_add: a flag destination is not float32 aligned");
        t.src[m] = (const uint8_t*)src_dev[i];
        t.dst[m] = (uint8_t*)dst_dev[i];
        t.unit[m] = kinds[i] == TG_ROLLOUT_FLAG_U8 ? 0 : tg::widest_unit(s, d, bytes[i]);
        t.units[m] = t.unit[m] ? bytes[i] / t.unit[m] : bytes[i];
        if (!tg::push_blocks(t, m, t.units[m])) return report_error(-1, "tg_rollout_add: too many bytes for one launch");
        ++m;
    }
    if (m == 0) return 0;
    t.n = m;
    hipLaunchKernelGGL(tg::k_rollout_add, dim3(t.blk_end[m - 1]), dim3(tg::kRoThreads), 0, (hipStream_t)hip_stream, t);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_rollout_add: the kernel launch failed");
    return 0;
}

extern "C" int tg_rollout_gather(int32_t n_arrays, const void* const* src_dev, void* const* dst_dev, const int64_t* row_bytes,
                                 const int64_t* rows_dev, int64_t B, void* hip_stream) {
    using tg::report_error;
    if (n_arrays < 0 || n_arrays > TG_ROLLOUT_MAX_ARRAYS) return report_error(-1, "tg_rollout_gather: between 0 and TG_ROLLOUT_MAX_ARRAYS arrays");
    if (B < 0) return report_error(-1, "tg_rollout_gather: negative batch size");
    if (n_arrays == 0 || B == 0) return 0;
    if (!src_dev || !dst_dev || !row_bytes || !rows_dev) return report_error(-1, "tg_rollout_gather: NULL table");
    tg::RoTable t = {};
    int m = 0;
    for (int i = 0; i < n_arrays; ++i) {
        if (row_bytes[i] < 0 || row_bytes[i] > ((int64_t)1 << 40)) return report_error(-1, "tg_rollout_gather: row byte count out of range");
        if (row_bytes[i] == 0) continue;
        if (!src_dev[i] || !dst_dev[i]) return report_error(-1, "tg_rollout_gather: NULL array pointer");
        t.src[m] = (const uint8_t*)src_dev[i];
        t.dst[m] = (uint8_t*)dst_dev[i];
        t.unit[m] = tg::widest_unit((uintptr_t)src_dev[i], (uintptr_t)dst_dev[i], row_bytes[i]);
        t.units[m] = row_bytes[i] / t.unit[m];
        if (t.units[m] > (((int64_t)1 << 40) / B) || !tg::push_blocks(t, m, B * t.units[m]))
            return report_error(-1, "tg_rollout_gather: too many bytes for one launch");
        ++m;
    }
    if (m == 0) return 0;
    t.n = m;
    hipLaunchKernelGGL(tg::k_rollout_gather, dim3(t.blk_end[m - 1]), dim3(tg::kRoThreads), 0, (hipStream_t)hip_stream, t, rows_dev, B);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_rollout_gather: the kernel launch failed");
    return 0;
}

extern "C" int tg_rollout_gae(const float* rewards_dev, const float* values_dev, const float* episode_starts_dev, const float* last_values_dev,
                              const void* dones_dev, int32_t dones_dtype, float* advantages_dev, float* returns_dev, int64_t T, int64_t N,
                              double gamma, double gae_lambda, void* hip_stream) {
    using tg::report_error;
    if (dones_dtype != TG_ROLLOUT_DONES_UINT8 && dones_dtype != TG_ROLLOUT_DONES_FLOAT32) return report_error(-1, "tg_rollout_gae: unknown dones dtype");
    if (T < 1 || N < 1 || T > ((int64_t)1 << 40) / N) return report_error(-1, "tg_rollout_gae: need T >= 1, N >= 1, T N <= 2^40");
    if (!rewards_dev || !values_dev || !episode_starts_dev || !last_values_dev || !dones_dev || !advantages_dev || !returns_dev)
        return report_error(-1, "tg_rollout_gae: NULL pointer");
    const float g = (float)gamma, gl = (float)(gamma * gae_lambda);
    const int64_t blocks = (N + tg::kGaeThreads - 1) / tg::kGaeThreads;
    if (blocks >= ((int64_t)1 << 31)) return report_error(-1, "tg_rollout_gae: too many envs for one launch");
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (dones_dtype == TG_ROLLOUT_DONES_UINT8)
        hipLaunchKernelGGL(tg::k_rollout_gae<uint8_t>, dim3((unsigned)blocks), dim3(tg::kGaeThreads), 0, stream, rewards_dev, values_dev,
                           episode_starts_dev, last_values_dev, (const uint8_t*)dones_dev, advantages_dev, returns_dev, T, N, g, gl);
    else
        hipLaunchKernelGGL(tg::k_rollout_gae<float>, dim3((unsigned)blocks), dim3(tg::kGaeThreads), 0, stream, rewards_dev, values_dev,
                           episode_starts_dev, last_values_dev, (const float*)dones_dev, advantages_dev, returns_dev, T, N, g, gl);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_rollout_gae: the kernel launch failed");
    return 0;
}
