// tg_vecnorm.hip - the device VecNormalize (tactile_gym_amd.vecnorm): stable_baselines3's VecNormalize / RunningMeanStd over
// float32 [rows, d] device arrays, statistics in float64.  Compiled with -ffp-contract=off: every operation below rounds once, in the order
// tests/vecnorm_ref.py (device_order) restates bit for bit.  f64 division and sqrt are the correctly rounded defaults.
//
//   k_vecnorm_partial  workgroup (chunk c, column j): the 256 envs of the chunk reduce column j to (mean_c, M2_c) - two passes, each a fixed
//                      binary tree over the 256 slots (absent envs add an exact zero) - and store it.  The extra column past the table is the
//                      discounted return: returns = returns gamma + reward, written back and reduced like the others     (tg_vecnorm_update)
//   k_vecnorm_merge    one workgroup, a lane per column: the chunks merged in ascending order, then the batch merged into the running
//                      (mean, var, count); the counts are written after a barrier                                           (tg_vecnorm_update)
//   k_vecnorm_apply    (x - mean) / sqrt(var + epsilon), clipped, float32; one more row of workgroups normalises the rewards and zeroes the
//                      returns of finished envs                                                                             (tg_vecnorm_apply)
// The launch boundaries order the three; nothing is added atomically and no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error

namespace tg {

constexpr int kVnMax = TG_VECNORM_MAX_ARRAYS;
constexpr int kVnChunk = 256;          // envs per chunk = lanes per workgroup
constexpr int kVnApplyBlocks = 4096;   // k_vecnorm_apply strides over longer arrays

struct VnTable {
    const float* x[kVnMax];
    float* out[kVnMax];         // apply only
    double* stats[kVnMax];      // mean [d] | var [d] | count
    int32_t d[kVnMax];
    int32_t col_end[kVnMax];    // columns of arrays 0 .. i
    int32_t n;
    int32_t cols;               // col_end[n - 1], 0 for an empty table
};

// Table fields through selects over the by-value table (no indexed private array: no scratch).
#define VN_PICK(field, a, out)                    \
    do {                                          \
        out = t.field[0];                         \
        _Pragma("unroll") for (int i = 1; i < kVnMax; ++i) if (i == (a)) out = t.field[i]; \
    } while (0)

// The array of column `col` (< t.cols) and the column's index inside it.
__device__ __forceinline__ int column_array(const VnTable& t, int col, int& local) {
    int a = 0, first = 0;
#pragma unroll
    for (int i = 0; i < kVnMax - 1; ++i)
        if (i < t.n - 1 && col >= t.col_end[i]) { a = i + 1; first = t.col_end[i]; }
    local = col - first;
    return a;
}

// The sum of the workgroup's 256 values in a fixed order: within each wavefront lane l adds lane l + s for s = 32, 16 ... 1, then
// (w0 + w1) + (w2 + w3).  Every lane returns the sum.
__device__ __forceinline__ double chunk_sum(double v, double* wave_sums) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
    __syncthreads();   // wave_sums is written again by the second pass
    return r;
}

__device__ __forceinline__ int chunk_rows(int c, int N) {
    const int left = N - c * kVnChunk;
    return left < kVnChunk ? left : kVnChunk;
}

// scratch: [column][chunk] pairs (mean_c, M2_c)
__global__ __launch_bounds__(kVnChunk) void k_vecnorm_partial(VnTable t, int32_t N, int32_t C, double* __restrict__ returns,
                                                              const float* __restrict__ rewards, double gamma, double* __restrict__ scratch) {
    __shared__ double wave_sums[4];
    const int c = blockIdx.x, col = blockIdx.y;
    const int i = c * kVnChunk + threadIdx.x;
    const bool present = i < N;
    double v = 0.0;
    if (col < t.cols) {
        int local;
        const int a = column_array(t, col, local);
        const float* x;
        int32_t d;
        VN_PICK(x, a, x);
        VN_PICK(d, a, d);
        if (present) v = (double)x[(int64_t)i * d + local];
    } else if (present) {
        v = returns[i] * gamma + (double)rewards[i];
        returns[i] = v;
    }
    const double mean = chunk_sum(v, wave_sums) / (double)chunk_rows(c, N);
    const double dev = present ? v - mean : 0.0;
    const double m2 = chunk_sum(dev * dev, wave_sums);
    if (threadIdx.x == 0) {
        double* p = scratch + 2 * ((int64_t)col * C + c);
        p[0] = mean;
        p[1] = m2;
    }
}

__global__ __launch_bounds__(kVnChunk) void k_vecnorm_merge(VnTable t, int32_t N, int32_t C, int32_t with_returns, double* __restrict__ ret_stats,
                                                            const double* __restrict__ scratch) {
    const int total = t.cols + (with_returns ? 1 : 0);
    for (int col = threadIdx.x; col < total; col += kVnChunk) {
        const double* p = scratch + 2 * (int64_t)col * C;
        double n = (double)chunk_rows(0, N), mean = p[0], m2 = p[1];
        for (int c = 1; c < C; ++c) {
            const double nc = (double)chunk_rows(c, N), delta = p[2 * c] - mean, tot = n + nc;
            // a chunk mean that is not finite: np.mean's sum, inf + x = inf, where the step's inf - inf would be NaN (opposite infinities still are)
            mean = delta - delta == 0.0 ? mean + delta * nc / tot : mean + p[2 * c];
            m2 = m2 + p[2 * c + 1] + delta * delta * n * nc / tot;
            n = tot;
        }
        const double bv = m2 / n;
        double *mean_p, *var_p;
        double count;
        if (col < t.cols) {
            int local;
            const int a = column_array(t, col, local);
            double* st;
            int32_t d;
            VN_PICK(stats, a, st);
            VN_PICK(d, a, d);
            mean_p = st + local;
            var_p = st + d + local;
            count = st[2 * d];
        } else {
            mean_p = ret_stats;
            var_p = ret_stats + 1;
            count = ret_stats[2];
        }
        const double old = *mean_p, delta = mean - old, tot = count + n;
        *mean_p = old + delta * n / tot;
        *var_p = (*var_p * count + bv * n + delta * delta * count * n / tot) / tot;
    }
    __syncthreads();   // every column has read its count
    if ((int)threadIdx.x < t.n) {
        double* st;
        int32_t d;
        VN_PICK(stats, (int)threadIdx.x, st);
        VN_PICK(d, (int)threadIdx.x, d);
        st[2 * d] = st[2 * d] + (double)N;
    }
    if (threadIdx.x == kVnMax && with_returns) ret_stats[2] = ret_stats[2] + (double)N;
}

__device__ __forceinline__ double clipped(double y, double clip) { return y < -clip ? -clip : (y > clip ? clip : y); }   // a NaN passes, as np.clip

__global__ __launch_bounds__(kVnChunk) void k_vecnorm_apply(VnTable t, int64_t R, double clip_obs, double epsilon, const float* rewards,
                                                            float* rewards_out, int64_t n_rewards, const double* __restrict__ ret_stats,
                                                            double clip_reward, double* returns, const uint8_t* __restrict__ dones,
                                                            int64_t n_reset) {
    const int64_t first = (int64_t)blockIdx.x * kVnChunk + threadIdx.x, stride = (int64_t)gridDim.x * kVnChunk;
    const int a = blockIdx.y;
    if (a < t.n) {
        const float* x;
        float* out;
        const double* st;
        int32_t d;
        VN_PICK(x, a, x);
        VN_PICK(out, a, out);
        VN_PICK(stats, a, st);
        VN_PICK(d, a, d);
        const int64_t total = R * d;
        const bool narrow = (uint64_t)total <= 0xffffffffull;   // the same in every lane: a 32-bit remainder where it is enough
        for (int64_t e = first; e < total; e += stride) {
            const int64_t col = narrow ? (int64_t)((uint32_t)e % (uint32_t)d) : e % d;
            const double y = ((double)x[e] - st[col]) / sqrt(st[d + col] + epsilon);
            out[e] = (float)clipped(y, clip_obs);
        }
        return;
    }
    if (rewards != nullptr) {
        const double scale = sqrt(ret_stats[1] + epsilon);
        for (int64_t e = first; e < n_rewards; e += stride) rewards_out[e] = (float)clipped((double)rewards[e] / scale, clip_reward);
    }
    if (returns != nullptr)
        for (int64_t e = first; e < n_reset; e += stride)
            if (dones == nullptr || dones[e]) returns[e] = 0.0;
}

// The checked table of an entry: 0, or the error already reported.
static int fill_table(VnTable& t, const char* who, int32_t n_arrays, const float* const* x_dev, float* const* out_dev, const int32_t* widths,
                      double* const* stats_dev, char* msg, size_t msg_len) {
    auto fail = [&](const char* what) {
        snprintf(msg, msg_len, "%s: %s", who, what);
        return report_error(-1, msg);
    };
    if (n_arrays < 0 || n_arrays > kVnMax) return fail("between 0 and TG_VECNORM_MAX_ARRAYS arrays");
    if (n_arrays > 0 && (!x_dev || !widths || !stats_dev)) return fail("NULL table");
    int32_t cols = 0;
    for (int i = 0; i < n_arrays; ++i) {
        if (widths[i] < 1 || widths[i] > TG_VECNORM_MAX_WIDTH || cols + widths[i] > TG_VECNORM_MAX_WIDTH)
            return fail("widths must be positive and add up to at most TG_VECNORM_MAX_WIDTH");
        if (!x_dev[i] || !stats_dev[i] || (out_dev && !out_dev[i])) return fail("NULL array pointer");
        cols += widths[i];
        t.x[i] = x_dev[i];
        t.out[i] = out_dev ? out_dev[i] : nullptr;
        t.stats[i] = stats_dev[i];
        t.d[i] = widths[i];
        t.col_end[i] = cols;
    }
    t.n = n_arrays;
    t.cols = cols;
    return 0;
}

}  // namespace tg

extern "C" int tg_vecnorm_update(int32_t n_arrays, const float* const* x_dev, const int32_t* widths, double* const* stats_dev, int64_t N,
                                 double* returns_dev, const float* rewards_dev, double gamma, double* ret_stats_dev, double* scratch_dev,
                                 void* hip_stream) {
    using tg::report_error;
    char msg[160];
    tg::VnTable t = {};
    if (const int rc = tg::fill_table(t, "tg_vecnorm_update", n_arrays, x_dev, nullptr, widths, stats_dev, msg, sizeof msg)) return rc;
    if (N < 1 || N > TG_VECNORM_MAX_ROWS) return report_error(-1, "tg_vecnorm_update: need 1 <= N <= TG_VECNORM_MAX_ROWS");
    const int n_ret = (returns_dev != nullptr) + (rewards_dev != nullptr) + (ret_stats_dev != nullptr);
    if (n_ret != 0 && n_ret != 3) return report_error(-1, "tg_vecnorm_update: returns, rewards and ret_stats are NULL together or not at all");
    if (!(gamma == gamma)) return report_error(-1, "tg_vecnorm_update: gamma is not a number");
    const int total = t.cols + (n_ret ? 1 : 0);
    if (total == 0) return 0;
    if (!scratch_dev) return report_error(-1, "tg_vecnorm_update: NULL scratch_dev");
    const int32_t C = (int32_t)((N + tg::kVnChunk - 1) / tg::kVnChunk);
    hipLaunchKernelGGL(tg::k_vecnorm_partial, dim3(C, total), dim3(tg::kVnChunk), 0, (hipStream_t)hip_stream, t, (int32_t)N, C, returns_dev,
                       rewards_dev, gamma, scratch_dev);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_vecnorm_update: the kernel launch failed");
    hipLaunchKernelGGL(tg::k_vecnorm_merge, dim3(1), dim3(tg::kVnChunk), 0, (hipStream_t)hip_stream, t, (int32_t)N, C, n_ret ? 1 : 0, ret_stats_dev,
                       scratch_dev);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_vecnorm_update: the kernel launch failed");
    return 0;
}

extern "C" int tg_vecnorm_apply(int32_t n_arrays, const float* const* x_dev, float* const* out_dev, const int32_t* widths,
                                const double* const* stats_dev, int64_t R, double clip_obs, double epsilon, const float* rewards_dev,
                                float* rewards_out, int64_t n_rewards, const double* ret_stats_dev, double clip_reward, double* returns_dev,
                                const uint8_t* dones_dev, int64_t n_reset, void* hip_stream) {
    using tg::report_error;
    char msg[160];
    tg::VnTable t = {};
    if (n_arrays > 0 && !out_dev) return report_error(-1, "tg_vecnorm_apply: NULL table");
    if (const int rc = tg::fill_table(t, "tg_vecnorm_apply", n_arrays, x_dev, out_dev, widths, const_cast<double* const*>(stats_dev), msg, sizeof msg))
        return rc;
    if (n_arrays > 0 && (R < 1 || R > TG_VECNORM_MAX_APPLY_ROWS)) return report_error(-1, "tg_vecnorm_apply: need 1 <= R <= TG_VECNORM_MAX_APPLY_ROWS");
    if (!(clip_obs >= 0.0) || !(clip_reward >= 0.0) || !(epsilon >= 0.0))
        return report_error(-1, "tg_vecnorm_apply: clip_obs, clip_reward and epsilon must not be negative");
    if (n_rewards < 0 || n_rewards > TG_VECNORM_MAX_APPLY_ROWS || n_reset < 0 || n_reset > TG_VECNORM_MAX_APPLY_ROWS)
        return report_error(-1, "tg_vecnorm_apply: n_rewards and n_reset must lie in [0, TG_VECNORM_MAX_APPLY_ROWS]");
    const bool with_rewards = rewards_dev != nullptr && n_rewards > 0, with_reset = returns_dev != nullptr && n_reset > 0;
    if (rewards_dev && (!rewards_out || !ret_stats_dev)) return report_error(-1, "tg_vecnorm_apply: rewards need rewards_out and ret_stats_dev");
    if (dones_dev && !returns_dev) return report_error(-1, "tg_vecnorm_apply: dones_dev without returns_dev");
    const bool tail = with_rewards || with_reset;
    if (t.n == 0 && !tail) return 0;
    int64_t longest = 1;
    for (int i = 0; i < t.n; ++i) longest = R * t.d[i] > longest ? R * t.d[i] : longest;
    if (with_rewards && n_rewards > longest) longest = n_rewards;
    if (with_reset && n_reset > longest) longest = n_reset;
    int64_t blocks = (longest + tg::kVnChunk - 1) / tg::kVnChunk;
    if (blocks > tg::kVnApplyBlocks) blocks = tg::kVnApplyBlocks;
    hipLaunchKernelGGL(tg::k_vecnorm_apply, dim3((unsigned)blocks, t.n + (tail ? 1 : 0)), dim3(tg::kVnChunk), 0, (hipStream_t)hip_stream, t, R, clip_obs,
                       epsilon, with_rewards ? rewards_dev : nullptr, rewards_out, n_rewards, ret_stats_dev, clip_reward,
                       with_reset ? returns_dev : nullptr, dones_dev, n_reset);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_vecnorm_apply: the kernel launch failed");
    return 0;
}
