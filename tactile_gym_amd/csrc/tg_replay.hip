// tg_replay.hip - the device replay buffer (tactile_gym_amd.replay): stable_baselines3's ReplayBuffer / DictReplayBuffer (the
// off-policy buffer of the reference's SAC / RAD_SAC) over step-major [T][N][...] rings in device memory.  Compiled with -ffp-contract=off:
// k_replay_draw's dones * (1 - timeouts) is the bit-exact specification the tests restate (tests/replay_ref.py).
//
//   k_replay_add    one launch per transition batch: every array's rows copied into their slot, each row from one of two sources chosen by a
//                   per-row flag (the terminal observation where the env finished, the next observation elsewhere) (tg_replay_add)
//   k_replay_draw   one launch per sample(): the counter-based draw of B (slot, env) cells, their storage rows (and the rows of the paired
//                   next_observations), and the gathered actions, rewards and dones * (1 - timeouts) (tg_replay_draw)
// The observation keys of a minibatch are gathered by k_random_translate (images) and k_rollout_gather (vectors) through the row table the draw wrote.
//
// k_replay_add follows k_rollout_add (tg_copy_units.hpp): units of 16, 4 or 1 bytes - here the widest that divides the ROW's byte count and the
// array's three addresses, so a unit never straddles two rows and one flag decides its source - four per lane, loads before stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_copy_units.hpp"   // move_units, which_array, RO_PICK, widest_unit, push_blocks
#include "tg_exchange.h"       // report_error
#include "tg_kernels.hpp"      // mix64, kGolden: tg_sample_actions' counter-based generator

namespace tg {

constexpr int kDrawThreads = 256;

struct RpTable {
    const uint8_t* src[kRoMax];
    const uint8_t* alt[kRoMax];   // NULL: every row from src
    uint8_t* dst[kRoMax];
    int64_t units[kRoMax];        // units of one row
    int32_t unit[kRoMax];         // 16, 4 or 1 bytes; flag arrays: 0 (one uint8 flag per row in, one float32 0 / 1 out)
    uint32_t blk_end[kRoMax];     // workgroups of arrays 0 .. i
    int32_t n;
};

// Unit g of an array is unit g % upr of row g / upr; source and destination hold the rows back to back, so the offset of a unit is the same in
// src, alt and dst.  Only the chosen source of a row is read.
__global__ __launch_bounds__(kRoThreads) void k_replay_add(RpTable t, const uint8_t* __restrict__ select, int64_t n_rows) {
    int64_t u0;
    const int a = which_array(t, u0);
    const uint8_t* src;
    const uint8_t* alt;
    uint8_t* dst;
    int64_t upr;
    int32_t unit;
    RO_PICK(src, a, src);
    RO_PICK(alt, a, alt);
    RO_PICK(dst, a, dst);
    RO_PICK(units, a, upr);
    RO_PICK(unit, a, unit);
    if (unit == 0) {   // done flags: uint8 (or bool) -> 0.0f / 1.0f, one per row
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t u = u0 + threadIdx.x + kRoThreads * k;
            if (u < n_rows) {
                const uint8_t* p = (alt != nullptr && select[u]) ? alt : src;
                reinterpret_cast<float*>(dst)[u] = p[u] ? 1.f : 0.f;
            }
        }
        return;
    }
    const int64_t total = n_rows * upr;
    const bool narrow = (uint64_t)total <= 0xffffffffull;   // the same in every lane: a 32-bit division where it is enough
    const uint8_t* s[4];
    uint8_t* d[4];
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = u0 + threadIdx.x + kRoThreads * k;
        on[k] = g < total;
        const uint8_t* base = src;
        if (alt != nullptr && on[k]) {   // `alt` is the same in every lane of the workgroup
            const int64_t row = upr == 1 ? g : narrow ? (int64_t)((uint32_t)g / (uint32_t)upr) : g / upr;
            if (select[row]) base = alt;
        }
        s[k] = base + g * unit;
        d[k] = dst + g * unit;
    }
    move_units<u32x4>(unit, s, d, on);   // the register form: no LDS
}

// Sample b: h = mix64(head + G (b + 1)), head = mix64(seed + G (counter + 1)) from the host - counter_draw(seed, counter, b) (tg_kernels.hpp) in
// two stages; slot (first + ((h >> 32) M >> 32)) % T, env (h & 0xffffffff) N >> 32.
__global__ __launch_bounds__(kDrawThreads) void k_replay_draw(int64_t B, uint64_t M, int64_t first, int64_t T, uint64_t N, uint64_t head,
                                                              const float* __restrict__ actions, int32_t A, const float* __restrict__ rewards,
                                                              const float* __restrict__ dones, const float* __restrict__ timeouts,
                                                              int64_t next_offset, int64_t* __restrict__ rows, float* __restrict__ actions_out,
                                                              float* __restrict__ rewards_out, float* __restrict__ dones_out) {
    const int64_t b = (int64_t)blockIdx.x * kDrawThreads + threadIdx.x;
    if (b >= B) return;
    const uint64_t h = mix64(head + kGolden * (uint64_t)(b + 1));
    const int64_t j = (int64_t)(((h >> 32) * M) >> 32);
    int64_t slot = first + j;                                 // first < T and j < M <= T
    if (slot >= T) slot -= T;
    const int64_t env = (int64_t)(((h & 0xffffffffull) * N) >> 32);
    const int64_t row = slot * (int64_t)N + env;
    rows[b] = row;
    rows[B + b] = row + next_offset;
    if (actions != nullptr) {
        for (int32_t k = 0; k < A; ++k) actions_out[b * A + k] = actions[row * A + k];
        rewards_out[b] = rewards[row];
        dones_out[b] = dones[row] * (1.f - timeouts[row]);
    }
}

}  // namespace tg

extern "C" int tg_replay_add(int32_t n_arrays, const void* const* src_dev, const void* const* alt_dev, void* const* dst_dev, const int64_t* row_bytes,
                             const int32_t* kinds, int64_t n_rows, const void* select_dev, void* hip_stream) {
    using tg::report_error;
    if (n_arrays < 0 || n_arrays > TG_ROLLOUT_MAX_ARRAYS) return report_error(-1, "tg_replay_add: between 0 and TG_ROLLOUT_MAX_ARRAYS arrays");
    if (n_rows < 0 || n_rows > ((int64_t)1 << 40)) return report_error(-1, "tg_replay_add: row count out of range");
    if (n_arrays == 0) return 0;
    if (!src_dev || !alt_dev || !dst_dev || !row_bytes || !kinds) return report_error(-1, "tg_replay_add: NULL table");
    tg::RpTable t = {};
    int m = 0;
    for (int i = 0; i < n_arrays; ++i) {
        if (kinds[i] != TG_ROLLOUT_COPY && kinds[i] != TG_ROLLOUT_FLAG_U8) return report_error(-1, "tg_replay_add: unknown array kind");
        if (row_bytes[i] < 0 || row_bytes[i] > ((int64_t)1 << 40)) return report_error(-1, "tg_replay_add: row byte count out of range");
        if (row_bytes[i] == 0 || n_rows == 0) continue;
        const bool flag = kinds[i] == TG_ROLLOUT_FLAG_U8;
        if (flag && row_bytes[i] != 1) return report_error(-1, "tg_replay_add: a flag array has one uint8 per row");
        if (!src_dev[i] || !dst_dev[i]) return report_error(-1, "tg_replay_add: NULL array pointer");
        if (alt_dev[i] && !select_dev) return report_error(-1, "tg_replay_add: an alternative source needs select_dev");
        if (row_bytes[i] > ((int64_t)1 << 40) / n_rows) return report_error(-1, "tg_replay_add: too many bytes for one launch");
        const uintptr_t s = (uintptr_t)src_dev[i], al = (uintptr_t)alt_dev[i], d = (uintptr_t)dst_dev[i];
        const uint64_t in_bytes = (uint64_t)row_bytes[i] * (uint64_t)n_rows, out_bytes = in_bytes * (flag ? 4 : 1);
        if ((s < d + out_bytes && d < s + in_bytes) || (al && al < d + out_bytes && d < al + in_bytes))
            return report_error(-1, "tg_replay_add: a destination overlaps its source");
        if (flag && (d & 3)) return report_error(-1, "tg_replay_add: a flag destination is not float32 aligned");
        t.src[m] = (const uint8_t*)src_dev[i];
        t.alt[m] = (const uint8_t*)alt_dev[i];
        t.dst[m] = (uint8_t*)dst_dev[i];
        t.unit[m] = flag ? 0 : tg::widest_unit(s | al, d, row_bytes[i]);
        t.units[m] = flag ? 1 : row_bytes[i] / t.unit[m];
        if (!tg::push_blocks(t, m, n_rows * t.units[m])) return report_error(-1, "tg_replay_add: too many bytes for one launch");
        ++m;
    }
    if (m == 0) return 0;
    t.n = m;
    hipLaunchKernelGGL(tg::k_replay_add, dim3(t.blk_end[m - 1]), dim3(tg::kRoThreads), 0, (hipStream_t)hip_stream, t, (const uint8_t*)select_dev, n_rows);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_replay_add: the kernel launch failed");
    return 0;
}

extern "C" int tg_replay_draw(int64_t B, int64_t n_slots, int64_t first_slot, int64_t T, int64_t N, uint64_t seed, uint64_t counter,
                              const float* actions_dev, int32_t A, const float* rewards_dev, const float* dones_dev, const float* timeouts_dev,
                              int64_t next_offset, int64_t* rows_dev, float* actions_out, float* rewards_out, float* dones_out, void* hip_stream) {
    using tg::report_error;
    if (B < 0) return report_error(-1, "tg_replay_draw: negative batch size");
    if (T < 1 || N < 1 || N >= ((int64_t)1 << 31) || T > ((int64_t)1 << 40) / N) return report_error(-1, "tg_replay_draw: need T >= 1, 1 <= N < 2^31, T N <= 2^40");
    if (n_slots < 1 || n_slots > T || n_slots >= ((int64_t)1 << 31)) return report_error(-1, "tg_replay_draw: need 1 <= n_slots <= T, n_slots < 2^31");
    if (first_slot < 0 || first_slot >= T) return report_error(-1, "tg_replay_draw: first_slot outside [0, T)");
    if (next_offset < 0) return report_error(-1, "tg_replay_draw: negative next_offset");
    const int n_in = (actions_dev != nullptr) + (rewards_dev != nullptr) + (dones_dev != nullptr) + (timeouts_dev != nullptr);
    if (n_in != 0 && n_in != 4) return report_error(-1, "tg_replay_draw: actions, rewards, dones and timeouts are NULL together or not at all");
    if (n_in == 4 && (A < 1 || A > (1 << 16))) return report_error(-1, "tg_replay_draw: need 1 <= A <= 65536");
    if (B == 0) return 0;
    if (!rows_dev) return report_error(-1, "tg_replay_draw: NULL rows_dev");
    if (n_in == 4 && (!actions_out || !rewards_out || !dones_out)) return report_error(-1, "tg_replay_draw: NULL output pointer");
    const int64_t blocks = (B + tg::kDrawThreads - 1) / tg::kDrawThreads;
    if (blocks >= ((int64_t)1 << 31)) return report_error(-1, "tg_replay_draw: too many samples for one launch");
    const uint64_t head = tg::mix64(seed + tg::kGolden * (counter + 1));
    hipLaunchKernelGGL(tg::k_replay_draw, dim3((unsigned)blocks), dim3(tg::kDrawThreads), 0, (hipStream_t)hip_stream, B, (uint64_t)n_slots, first_slot, T,
                       (uint64_t)N, head, actions_dev, A, rewards_dev, dones_dev, timeouts_dev, next_offset, rows_dev, actions_out, rewards_out,
                       dones_out);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_replay_draw: the kernel launch failed");
    return 0;
}
