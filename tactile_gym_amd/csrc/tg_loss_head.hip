// tg_loss_head.hip - the device loss heads (tactile_gym_amd.loss_head): what stable_baselines3 does between the network's output
// and the scalar loss, with the gradients at the head's inputs.
//   tg_ppo_loss            PPO.train from evaluate_actions to `loss` on float32 [B][A], and dloss / d(mean, log_std, values)
//   tg_squashed_rsample    SAC's actor.action_log_prob: k_action_head<TG_HEAD_SQUASHED>'s arithmetic (tg_head_core.h) at (seed, counter)
//   tg_squashed_rsample_bwd  its backward pass
// Compiled with -ffp-contract=off: float32 arithmetic with one rounding per operation in the order written below, which tests/loss_head_ref.py
// (device_order) restates; exp, tanh and log are evaluated in double on the float32 argument and rounded once.  Every sum over rows is taken in
// double: rows in chunks of 256 consecutive rows (one row per lane), inside a chunk the shuffle tree of tg_loss_core.h (offsets 32 .. 1 inside
// each wave, then the four wave sums in wave order), the chunk sums added in ascending order.  No atomics: the same inputs give the same bits.
//
//   k_ppo_one      one workgroup: advantage statistics, every chunk in turn, the finish.  B <= 4096 (path 1).
//   k_ppo_stats    one workgroup: the advantage statistics into the workspace's head                   }
//   k_ppo_chunks   one workgroup per chunk: the rows' outputs, the chunk's sums into the workspace     } path 2, the same device functions
//   k_ppo_finish   one workgroup: the chunk sums in ascending order, the finish                        }
// The work is latency bound; what the calls buy is the dozens of torch launches they replace.
//   tg_optim_workspace, tg_optim_sumsq, tg_optim_adam   the device Adam (tactile_gym_amd.optim) over tg_optim.h's kernels
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error
#include "tg_head_core.h"  // the draw and the per-element chains, shared with tg_action_head.hip
#include "tg_loss_core.h"  // the chunk and its sum (wave_sum, slot_put, slot_get), shared with tg_sac_loss.hip
#include "tg_optim.h"      // the device Adam's kernels: under this unit's flag, their entries at the end of this file

namespace tg {

constexpr int kLossStats = 5;                     // slots 0 .. 4: the surrogate, the value loss, the entropy, the KL term, the clip indicator
constexpr int kLossSlots = kLossStats + TG_HEAD_MAX_ACT;   // slots 5 .. 5 + A - 1: the columns of dlog_std [A]
constexpr int kLossHeadBytes = 16;                // the workspace's head: adv_mean, adv_std (float32), then padding

struct PpoArgs {
    const float* mean;          // [B][A]
    const float* log_std;       // [A] (stride 0) or [B][A] (stride A)
    const float* values;        // [B]
    const float* actions;       // [B][A]
    const float* old_log_prob;  // [B]
    const float* advantages;    // [B]
    const float* returns;       // [B]
    const float* old_values;    // [B], read when clip_vf >= 0
    float* stats;               // [8]
    float* log_prob;            // nullable [B]
    float* dmean;               // nullable [B][A]
    float* dls;                 // nullable [A] or [B][A]
    float* dvalues;             // nullable [B]
    double* chunk_sums;         // path 2: [chunks][5 + A]
    float* adv_stats;           // path 2: the workspace's head
    int64_t B;
    int32_t A;
    int32_t ls_stride;
    int32_t normalize;          // already 0 when B == 1
    float clip, clip_vf, ent_coef, vf_coef;
};

// One value per row summed over all rows, chunk by chunk, by the whole workgroup: every thread returns the total.
template <typename F>
__device__ __forceinline__ double all_rows_sum(int64_t B, double* lds, F value) {
    double total = 0.0;
    for (int64_t base = 0; base < B; base += kLossThreads) {
        const int64_t i = base + threadIdx.x;
        slot_put(lds, 0, i < B ? value(i) : 0.0);
        __syncthreads();
        total = total + slot_get(lds, 0);
        __syncthreads();
    }
    return total;
}

// SB3: (adv - adv.mean()) / (adv.std() + 1e-8), the mean and the unbiased variance in double, each rounded to float32 once.
__device__ __forceinline__ void adv_statistics(const PpoArgs& a, double* lds, float* adv_mean, float* adv_std) {
    if (!a.normalize) {
        *adv_mean = 0.0f;
        *adv_std = 1.0f;
        return;
    }
    const float* adv = a.advantages;
    const double mean = all_rows_sum(a.B, lds, [&](int64_t i) { return (double)adv[i]; }) / (double)a.B;
    const double ss = all_rows_sum(a.B, lds, [&](int64_t i) { const double c = (double)adv[i] - mean; return c * c; });
    *adv_mean = (float)mean;
    *adv_std = (float)sqrt(ss / (double)(a.B - 1));
}

// Rows chunk * 256 .. + 255: every per-row output, and for thread t < 5 (+ A with dlog_std [A]) the chunk's sum of slot t.
__device__ __forceinline__ double chunk_pass(const PpoArgs& a, int64_t chunk, float adv_mean, float adv_std, double* lds) {
    const int64_t i = chunk * kLossThreads + threadIdx.x;
    const bool valid = i < a.B;
    const int A = a.A;
    const float fB = (float)a.B;
    const bool cols = a.dls && a.ls_stride == 0;      // dlog_std [A]: a sum over rows per column
    double s_pol = 0.0, s_val = 0.0, s_ent = 0.0, s_kl = 0.0, s_cf = 0.0;
    float coef = 0.0f;                                // dloss / dlog_prob of this row
    if (valid) {
        float lp = 0.0f, ent = 0.0f;
        for (int j = 0; j < A; ++j) {
            const int64_t e = i * A + j;
            const float ls = a.log_std[a.ls_stride ? e : (int64_t)j];
            const float sigma = head_sigma(ls);
            const float d = a.actions[e] - a.mean[e];
            lp = lp + head_gaussian_term(d, sigma, ls);
            const float h = 1.4189385332046727f + ls;  // DiagGaussianDistribution.entropy: 0.5 + 0.5 log(2 pi) + log_std
            ent = ent + h;
        }
        if (a.log_prob) a.log_prob[i] = lp;
        float adv = a.advantages[i];
        if (a.normalize) {
            const float c = adv - adv_mean;
            const float den = adv_std + 1e-8f;
            adv = c / den;
        }
        const float lr = lp - a.old_log_prob[i];
        const float ratio = (float)exp((double)lr);
        const float lo = 1.0f - a.clip, hi = 1.0f + a.clip;
        const float p1 = adv * ratio;
        const float rc = ratio < lo ? lo : (ratio > hi ? hi : ratio);
        const float p2 = adv * rc;
        const float pm = p2 < p1 ? p2 : p1;           // torch.min
        const bool inside = ratio >= lo && ratio <= hi;
        // autograd: the clamp passes inside (inclusive); outside only the unclipped product, when it is the smaller.  torch.min hands a NaN
        // product the gradient as well, and the zero of a blocked row still meets adv and ratio on its way back: 0 inf = NaN
        const float g = p1 / fB;
        if (inside || !(p1 >= p2)) coef = -g;
        else if (p1 > p2) coef = (0.0f * fabsf(adv)) * ratio;
        else coef = 0.0f - g;                         // equal outside the clip: adv is 0, or infinite with half the gradient
        const float v = a.values[i];
        float vp = v;
        bool vpass = true;
        if (a.clip_vf >= 0.0f) {
            const float ov = a.old_values[i];
            const float dv = v - ov;
            const float nc = -a.clip_vf;
            const float dc = dv < nc ? nc : (dv > a.clip_vf ? a.clip_vf : dv);
            vp = ov + dc;
            vpass = dv >= nc && dv <= a.clip_vf;
        }
        const float diff = a.returns[i] - vp;
        const float sq = diff * diff;
        if (a.dvalues) {                              // d(vf_coef mean (returns - values_pred)^2) / dvalues
            const float t2 = 2.0f * diff;
            const float t3 = t2 * a.vf_coef;
            const float t4 = t3 / fB;
            a.dvalues[i] = vpass ? -t4 : 0.0f;
        }
        const float r1 = ratio - 1.0f;
        const float kl = r1 - lr;
        s_pol = (double)pm;
        s_val = (double)sq;
        s_ent = (double)ent;
        s_kl = (double)kl;
        s_cf = fabsf(r1) > a.clip ? 1.0 : 0.0;
    }
    slot_put(lds, 0, s_pol);
    slot_put(lds, 1, s_val);
    slot_put(lds, 2, s_ent);
    slot_put(lds, 3, s_kl);
    slot_put(lds, 4, s_cf);
    if (a.dmean || a.dls) {
        const float ge = a.ent_coef / fB;             // the entropy's share of dlog_std: -ent_coef / B per column
        const float lost_row = coef - coef;           // 0, or NaN for a coef that is not finite
        for (int j = 0; j < A; ++j) {
            float gl = 0.0f;
            if (valid) {
                const int64_t e = i * A + j;
                const float ls = a.log_std[a.ls_stride ? e : (int64_t)j];
                const float sigma = head_sigma(ls);
                const float d = a.actions[e] - a.mean[e];
                const float var = sigma * sigma;
                if (a.dmean) {                        // dlog_prob / dmean = d / sigma^2
                    const float dm = d / var;
                    a.dmean[e] = coef * dm;
                }
                const float q = d * d;                // dlog_prob / dlog_std = d^2 / sigma^2 - 1
                const float qs = q / var;
                const float dl = qs - 1.0f;
                // autograd reaches log_std on two paths, coef d^2 / sigma^2 through sigma and -coef beside it: with a coef or a sigma that
                // is not finite they give inf - inf or 0 inf, a NaN, where the factored product would be finite or infinite.  sigma itself
                // is asked, not its float32 square: a finite sigma whose square overflows gives the finite -coef, in torch as here
                const float lost = lost_row + (sigma - sigma);
                const float cl = lost == 0.0f ? coef * dl : lost;
                gl = cl - ge;
                if (a.dls && a.ls_stride) a.dls[e] = gl;
            }
            if (cols) slot_put(lds, kLossStats + j, (double)gl);
        }
    }
    __syncthreads();
    const int slots = kLossStats + (cols ? A : 0);
    const double mine = (int)threadIdx.x < slots ? slot_get(lds, threadIdx.x) : 0.0;
    __syncthreads();
    return mine;
}

// Thread t < 5 + A holds the total of slot t: the eight stats and dlog_std [A].
__device__ __forceinline__ void finish(const PpoArgs& a, double total, float adv_mean, float adv_std, double* lds) {
    const int t = threadIdx.x;
    if (t < kLossSlots) lds[t] = total;
    __syncthreads();
    const double dB = (double)a.B;
    if (t == 0) {
        const float policy_loss = (float)(-(lds[0] / dB));
        const float value_loss = (float)(lds[1] / dB);
        const float entropy_loss = (float)(-(lds[2] / dB));
        const float e1 = a.ent_coef * entropy_loss;
        const float v1 = a.vf_coef * value_loss;
        const float l1 = policy_loss + e1;
        a.stats[0] = l1 + v1;
        a.stats[1] = policy_loss;
        a.stats[2] = value_loss;
        a.stats[3] = entropy_loss;
        a.stats[4] = (float)(lds[3] / dB);
        a.stats[5] = (float)(lds[4] / dB);
        a.stats[6] = adv_mean;
        a.stats[7] = adv_std;
    }
    if (a.dls && a.ls_stride == 0 && t >= kLossStats && t < kLossStats + a.A) a.dls[t - kLossStats] = (float)lds[t];
}

__global__ __launch_bounds__(kLossThreads) void k_ppo_one(PpoArgs a) {
    __shared__ double lds[kLossSlots * kLossWaves];
    float adv_mean, adv_std;
    adv_statistics(a, lds, &adv_mean, &adv_std);
    const int64_t chunks = (a.B + kLossThreads - 1) / kLossThreads;
    double total = 0.0;
    for (int64_t c = 0; c < chunks; ++c) total = total + chunk_pass(a, c, adv_mean, adv_std, lds);
    finish(a, total, adv_mean, adv_std, lds);
}

__global__ __launch_bounds__(kLossThreads) void k_ppo_stats(PpoArgs a) {
    __shared__ double lds[kLossWaves];
    float adv_mean, adv_std;
    adv_statistics(a, lds, &adv_mean, &adv_std);
    if (threadIdx.x == 0) {
        a.adv_stats[0] = adv_mean;
        a.adv_stats[1] = adv_std;
    }
}

__global__ __launch_bounds__(kLossThreads) void k_ppo_chunks(PpoArgs a) {
    __shared__ double lds[kLossSlots * kLossWaves];
    const double mine = chunk_pass(a, (int64_t)blockIdx.x, a.adv_stats[0], a.adv_stats[1], lds);
    const int slots = kLossStats + a.A;
    if ((int)threadIdx.x < slots) a.chunk_sums[(int64_t)blockIdx.x * slots + threadIdx.x] = mine;
}

__global__ __launch_bounds__(kLossThreads) void k_ppo_finish(PpoArgs a) {
    __shared__ double lds[kLossSlots];
    const int64_t chunks = (a.B + kLossThreads - 1) / kLossThreads;
    const int slots = kLossStats + a.A;
    double total = 0.0;
    if ((int)threadIdx.x < slots)
        for (int64_t c = 0; c < chunks; ++c) total = total + a.chunk_sums[c * slots + threadIdx.x];
    finish(a, total, a.adv_stats[0], a.adv_stats[1], lds);
}

// ---------------------------------------------------------------------------------------------------------------- SAC's rsample
struct RsampleArgs {
    const float* mean;       // [B][A]
    const float* log_std;    // [A] or [B][A]
    const float* noise_in;   // nullable [B][A]
    float* actions;          // [B][A]
    float* log_prob;         // [B]
    float* eps_out;          // nullable [B][A]: saved for the backward
    float* sigma_out;        // nullable [B][A]
    int64_t B;
    int32_t A;
    int32_t ls_stride;
    float ls_min, ls_max;
    uint64_t seed, counter;
};

__global__ __launch_bounds__(kLossThreads) void k_squashed_rsample(RsampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (i >= a.B) return;
    float gsum = 0.0f, csum = 0.0f;
    for (int j = 0; j < a.A; ++j) {                   // k_action_head<TG_HEAD_SQUASHED>, operation for operation
        const int64_t e = i * a.A + j;
        const float mean = a.mean[e];
        const float ls = head_clamp(a.log_std[a.ls_stride ? e : (int64_t)j], a.ls_min, a.ls_max);
        const float sigma = head_sigma(ls);
        const float eps = a.noise_in ? a.noise_in[e] : head_normal(a.seed, a.counter, (uint64_t)e);
        const float se = sigma * eps;
        const float x = mean + se;
        const float d = x - mean;
        gsum = gsum + head_gaussian_term(d, sigma, ls);
        const float act = head_tanh(x);
        a.actions[e] = act;
        // saved as the backward needs it: with a mean that is not finite x - mean is NaN and autograd's gradients with it, which the
        // backward, that never sees mean, reads off a NaN here
        if (a.eps_out) a.eps_out[e] = mean - mean == 0.0f ? eps : mean - mean;
        if (a.sigma_out) a.sigma_out[e] = sigma;
        csum = csum + head_squash_term(act);
    }
    a.log_prob[i] = gsum - csum;
}

struct RsampleBwdArgs {
    const float* g_a;        // nullable [B][A]
    const float* g_lp;       // nullable [B]
    const float* actions;    // [B][A]: a
    const float* eps;        // [B][A]
    const float* sigma;      // [B][A]
    const float* log_std;    // the forward's, for the clamp's mask
    float* dmean;            // nullable [B][A]
    float* dls;              // nullable [B][A]
    int64_t B;
    int32_t A;
    int32_t ls_stride;
    float ls_min, ls_max;
};

__global__ __launch_bounds__(kLossThreads) void k_squashed_rsample_bwd(RsampleBwdArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    if (i >= a.B) return;
    const float glp = a.g_lp ? a.g_lp[i] : 0.0f;
    for (int j = 0; j < a.A; ++j) {
        const int64_t e = i * a.A + j;
        const float act = a.actions[e];
        const float aa = act * act;
        const float om = 1.0f - aa;                   // da / dx
        const float w = om + 1e-6f;
        float s = 0.0f;
        if (a.g_a) s = a.g_a[e] * om;
        if (a.g_lp) {                                 // d(-log w) / dx = 2 a (1 - a^2) / w
            const float n1 = 2.0f * act;
            const float n2 = n1 * om;
            const float n3 = n2 / w;
            const float n4 = glp * n3;
            s = s + n4;
            // the Gaussian sum's gradient is taken analytically (0 to mean): autograd sends G = g_lp d / sigma^2 to x and -G to mean, and
            // with a G that is not finite (g_lp, eps or sigma infinite, sigma 0) their sum is NaN, not 0
            const float se = a.sigma[e] * a.eps[e];
            const float var = a.sigma[e] * a.sigma[e];
            const float G = glp * (se / var);
            const float lost = G - G;
            if (!(lost == 0.0f)) s = lost;
        }
        if (a.dmean) a.dmean[e] = s;
        if (a.dls) {                                  // x = mean + sigma eps; the Gaussian sum's own share is -1 per column
            const float ls = a.log_std[a.ls_stride ? e : (int64_t)j];
            const bool inside = ls >= a.ls_min && ls <= a.ls_max;   // torch.clamp's gradient: inclusive, 0 for a NaN
            const float u1 = s * a.sigma[e];
            const float u2 = u1 * a.eps[e];
            const float u3 = u2 - glp;
            a.dls[e] = inside ? u3 : 0.0f;
        }
    }
}

inline int64_t ppo_workspace_bytes(int64_t B, int32_t A) {
    const int64_t chunks = (B + kLossThreads - 1) / kLossThreads;
    return kLossHeadBytes + chunks * (kLossStats + A) * (int64_t)sizeof(double);
}

}  // namespace tg

extern "C" int64_t tg_ppo_loss_workspace(int64_t B, int32_t A) {
    if (A < 1 || A > TG_HEAD_MAX_ACT) return tg::report_error(-1, "tg_ppo_loss_workspace: need 1 <= A <= TG_HEAD_MAX_ACT");
    if (B < 1 || B > TG_HEAD_MAX_ROWS) return tg::report_error(-1, "tg_ppo_loss_workspace: need 1 <= B <= TG_HEAD_MAX_ROWS");
    return tg::ppo_workspace_bytes(B, A);
}

extern "C" int tg_ppo_loss(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, const float* values_dev,
                           const float* actions_dev, const float* old_log_prob_dev, const float* advantages_dev, const float* returns_dev,
                           const float* old_values_dev, int64_t B, int32_t A, float clip_range, float clip_range_vf, float ent_coef, float vf_coef,
                           int32_t normalize_advantage, int32_t path, float* stats_out, float* log_prob_out, float* dmean_out,
                           float* dlog_std_out, float* dvalues_out, void* workspace_dev, int64_t workspace_bytes, void* hip_stream) {
    using tg::report_error;
    if (!mean_dev || !log_std_dev || !values_dev || !actions_dev || !old_log_prob_dev || !advantages_dev || !returns_dev)
        return report_error(-1, "tg_ppo_loss: NULL input");
    if (!stats_out) return report_error(-1, "tg_ppo_loss: NULL stats_out");
    if (A < 1 || A > TG_HEAD_MAX_ACT) return report_error(-1, "tg_ppo_loss: need 1 <= A <= TG_HEAD_MAX_ACT");
    if (log_std_stride != 0 && log_std_stride != A) return report_error(-1, "tg_ppo_loss: log_std_stride must be 0 or A");
    if (B < 1 || B > TG_HEAD_MAX_ROWS) return report_error(-1, "tg_ppo_loss: need 1 <= B <= TG_HEAD_MAX_ROWS");
    if (!(clip_range >= 0.0f)) return report_error(-1, "tg_ppo_loss: need clip_range >= 0");
    if (clip_range_vf != clip_range_vf) return report_error(-1, "tg_ppo_loss: clip_range_vf is a NaN (negative means none)");
    if (clip_range_vf >= 0.0f && !old_values_dev) return report_error(-1, "tg_ppo_loss: clip_range_vf needs old_values_dev");
    if (path != TG_LOSS_PATH_AUTO && path != TG_LOSS_PATH_ONE && path != TG_LOSS_PATH_GRID)
        return report_error(-1, "tg_ppo_loss: path must be TG_LOSS_PATH_AUTO, TG_LOSS_PATH_ONE or TG_LOSS_PATH_GRID");
    if (path == TG_LOSS_PATH_ONE && B > TG_LOSS_ONE_MAX_ROWS) return report_error(-1, "tg_ppo_loss: TG_LOSS_PATH_ONE needs B <= TG_LOSS_ONE_MAX_ROWS");
    const bool grid = path == TG_LOSS_PATH_GRID || (path == TG_LOSS_PATH_AUTO && B > TG_LOSS_ONE_MAX_ROWS);
    if (grid && (!workspace_dev || workspace_bytes < tg::ppo_workspace_bytes(B, A)))
        return report_error(-1, "tg_ppo_loss: the grid path needs a workspace of tg_ppo_loss_workspace(B, A) bytes");
    tg::PpoArgs a = {};
    a.mean = mean_dev;
    a.log_std = log_std_dev;
    a.values = values_dev;
    a.actions = actions_dev;
    a.old_log_prob = old_log_prob_dev;
    a.advantages = advantages_dev;
    a.returns = returns_dev;
    a.old_values = old_values_dev;
    a.stats = stats_out;
    a.log_prob = log_prob_out;
    a.dmean = dmean_out;
    a.dls = dlog_std_out;
    a.dvalues = dvalues_out;
    a.B = B;
    a.A = A;
    a.ls_stride = log_std_stride;
    a.normalize = (normalize_advantage && B > 1) ? 1 : 0;
    a.clip = clip_range;
    a.clip_vf = clip_range_vf >= 0.0f ? clip_range_vf : -1.0f;
    a.ent_coef = ent_coef;
    a.vf_coef = vf_coef;
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 block(tg::kLossThreads);
    if (!grid) {
        hipLaunchKernelGGL(tg::k_ppo_one, dim3(1), block, 0, s, a);
    } else {
        a.adv_stats = (float*)workspace_dev;
        a.chunk_sums = (double*)((char*)workspace_dev + tg::kLossHeadBytes);
        const int64_t chunks = (B + tg::kLossThreads - 1) / tg::kLossThreads;
        hipLaunchKernelGGL(tg::k_ppo_stats, dim3(1), block, 0, s, a);
        hipLaunchKernelGGL(tg::k_ppo_chunks, dim3((unsigned)chunks), block, 0, s, a);
        hipLaunchKernelGGL(tg::k_ppo_finish, dim3(1), block, 0, s, a);
    }
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_ppo_loss: a kernel launch failed");
    return 0;
}

extern "C" int tg_squashed_rsample(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, int64_t B, int32_t A, float log_std_min,
                                   float log_std_max, uint64_t seed, uint64_t counter, const float* noise_in_dev, float* actions_out,
                                   float* log_prob_out, float* eps_out, float* sigma_out, void* hip_stream) {
    using tg::report_error;
    if (!mean_dev || !log_std_dev) return report_error(-1, "tg_squashed_rsample: NULL mean_dev or log_std_dev");
    if (!actions_out || !log_prob_out) return report_error(-1, "tg_squashed_rsample: NULL actions_out or log_prob_out");
    if (A < 1 || A > TG_HEAD_MAX_ACT) return report_error(-1, "tg_squashed_rsample: need 1 <= A <= TG_HEAD_MAX_ACT");
    if (log_std_stride != 0 && log_std_stride != A) return report_error(-1, "tg_squashed_rsample: log_std_stride must be 0 or A");
    if (B < 1 || B > TG_HEAD_MAX_ROWS) return report_error(-1, "tg_squashed_rsample: need 1 <= B <= TG_HEAD_MAX_ROWS");
    if (!(log_std_min <= log_std_max)) return report_error(-1, "tg_squashed_rsample: need log_std_min <= log_std_max");
    tg::RsampleArgs a = {};
    a.mean = mean_dev;
    a.log_std = log_std_dev;
    a.noise_in = noise_in_dev;
    a.actions = actions_out;
    a.log_prob = log_prob_out;
    a.eps_out = eps_out;
    a.sigma_out = sigma_out;
    a.B = B;
    a.A = A;
    a.ls_stride = log_std_stride;
    a.ls_min = log_std_min;
    a.ls_max = log_std_max;
    a.seed = seed;
    a.counter = counter;
    const dim3 grid((unsigned)((B + tg::kLossThreads - 1) / tg::kLossThreads)), block(tg::kLossThreads);
    hipLaunchKernelGGL(tg::k_squashed_rsample, grid, block, 0, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_squashed_rsample: the kernel launch failed");
    return 0;
}

extern "C" int tg_squashed_rsample_bwd(const float* g_actions_dev, const float* g_log_prob_dev, const float* actions_dev, const float* eps_dev,
                                       const float* sigma_dev, const float* log_std_dev, int32_t log_std_stride, int64_t B, int32_t A,
                                       float log_std_min, float log_std_max, float* dmean_out, float* dlog_std_out, void* hip_stream) {
    using tg::report_error;
    if (!actions_dev || !eps_dev || !sigma_dev || !log_std_dev) return report_error(-1, "tg_squashed_rsample_bwd: NULL saved tensor or log_std_dev");
    if (A < 1 || A > TG_HEAD_MAX_ACT) return report_error(-1, "tg_squashed_rsample_bwd: need 1 <= A <= TG_HEAD_MAX_ACT");
    if (log_std_stride != 0 && log_std_stride != A) return report_error(-1, "tg_squashed_rsample_bwd: log_std_stride must be 0 or A");
    if (B < 1 || B > TG_HEAD_MAX_ROWS) return report_error(-1, "tg_squashed_rsample_bwd: need 1 <= B <= TG_HEAD_MAX_ROWS");
    if (!(log_std_min <= log_std_max)) return report_error(-1, "tg_squashed_rsample_bwd: need log_std_min <= log_std_max");
    if (!dmean_out && !dlog_std_out) return 0;
    tg::RsampleBwdArgs a = {};
    a.g_a = g_actions_dev;
    a.g_lp = g_log_prob_dev;
    a.actions = actions_dev;
    a.eps = eps_dev;
    a.sigma = sigma_dev;
    a.log_std = log_std_dev;
    a.dmean = dmean_out;
    a.dls = dlog_std_out;
    a.B = B;
    a.A = A;
    a.ls_stride = log_std_stride;
    a.ls_min = log_std_min;
    a.ls_max = log_std_max;
    const dim3 grid((unsigned)((B + tg::kLossThreads - 1) / tg::kLossThreads)), block(tg::kLossThreads);
    hipLaunchKernelGGL(tg::k_squashed_rsample_bwd, grid, block, 0, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_squashed_rsample_bwd: the kernel launch failed");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the device Adam (tg_optim.h)
extern "C" int64_t tg_optim_workspace(int64_t n_chunks) {
    if (n_chunks < 1 || n_chunks > INT32_MAX) return tg::report_error(-1, "tg_optim_workspace: need 1 <= n_chunks <= 2^31 - 1");
    return n_chunks * (int64_t)sizeof(double);
}

extern "C" int tg_optim_sumsq(int32_t n_tensors, const float* const* grads_dev, const int64_t* counts, double* partials_dev,
                              int64_t workspace_bytes, void* hip_stream) {
    using tg::report_error;
    if (n_tensors < 1) return report_error(-1, "tg_optim_sumsq: need n_tensors >= 1");
    if (!grads_dev || !counts) return report_error(-1, "tg_optim_sumsq: NULL grads_dev or counts");
    for (int32_t i = 0; i < n_tensors; ++i)
        if (!grads_dev[i]) return report_error(-1, "tg_optim_sumsq: NULL tensor in grads_dev");
    const int64_t chunks = tg::optim_chunks(n_tensors, counts);
    if (chunks == -1) return report_error(-1, "tg_optim_sumsq: need every count >= 1");
    if (chunks < 0) return report_error(-1, "tg_optim_sumsq: more than 2^31 - 1 chunks");
    if (!partials_dev || workspace_bytes < chunks * (int64_t)sizeof(double))
        return report_error(-1, "tg_optim_sumsq: partials_dev needs tg_optim_workspace(chunks) bytes");
    hipStream_t s = (hipStream_t)hip_stream;
    tg::OptimTable tb = {};
    tb.partials = partials_dev;
    tg::optim_launches(
        tb, n_tensors, counts, [&](tg::OptimTensor& row, int32_t i) { row.g = grads_dev[i]; },
        [&](const tg::OptimTable& t, unsigned grid) { hipLaunchKernelGGL(tg::k_optim_sumsq, dim3(grid), dim3(tg::kLossThreads), 0, s, t); });
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_optim_sumsq: a kernel launch failed");
    return 0;
}

extern "C" int tg_optim_adam(int32_t n_tensors, float* const* params_dev, const float* const* grads_dev, float* const* exp_avg_dev,
                             float* const* exp_avg_sq_dev, const int64_t* counts, const float* step_size, const float* bias_corr2_sqrt,
                             double beta1, double beta2, float eps, float weight_decay, int32_t clip, float max_norm,
                             const double* partials_dev, int64_t n_partials, float* total_norm_out, void* hip_stream) {
    using tg::report_error;
    if (n_tensors < 1) return report_error(-1, "tg_optim_adam: need n_tensors >= 1");
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev) return report_error(-1, "tg_optim_adam: NULL pointer array");
    if (!counts || !step_size || !bias_corr2_sqrt) return report_error(-1, "tg_optim_adam: NULL counts, step_size or bias_corr2_sqrt");
    for (int32_t i = 0; i < n_tensors; ++i)
        if (!params_dev[i] || !grads_dev[i] || !exp_avg_dev[i] || !exp_avg_sq_dev[i]) return report_error(-1, "tg_optim_adam: NULL tensor");
    const int64_t chunks = tg::optim_chunks(n_tensors, counts);
    if (chunks == -1) return report_error(-1, "tg_optim_adam: need every count >= 1");
    if (chunks < 0) return report_error(-1, "tg_optim_adam: more than 2^31 - 1 chunks");
    if (clip) {
        if (!(max_norm >= 0.0f)) return report_error(-1, "tg_optim_adam: need max_norm >= 0");
        if (!partials_dev || n_partials < 1) return report_error(-1, "tg_optim_adam: the clip needs partials_dev and n_partials >= 1");
        if (!total_norm_out) return report_error(-1, "tg_optim_adam: the clip needs total_norm_out");
    }
    hipStream_t s = (hipStream_t)hip_stream;
    tg::OptimTable tb = {};
    tb.partials = const_cast<double*>(partials_dev);
    tb.total_norm = total_norm_out;
    tb.n_partials = clip ? n_partials : 0;
    tb.w1 = (float)(1.0 - beta1);
    tb.w2 = (float)(1.0 - beta2);
    tb.b2 = (float)beta2;
    tb.eps = eps;
    tb.wd = weight_decay;
    tb.max_norm = max_norm;
    tg::optim_launches(
        tb, n_tensors, counts,
        [&](tg::OptimTensor& row, int32_t i) {
            row.p = params_dev[i];
            row.g = grads_dev[i];
            row.m = exp_avg_dev[i];
            row.v = exp_avg_sq_dev[i];
            row.ss = step_size[i];
            row.bc2s = bias_corr2_sqrt[i];
        },
        [&](const tg::OptimTable& t, unsigned grid) {
            if (clip) hipLaunchKernelGGL(tg::k_optim_adam<true>, dim3(grid), dim3(tg::kLossThreads), 0, s, t);
            else hipLaunchKernelGGL(tg::k_optim_adam<false>, dim3(grid), dim3(tg::kLossThreads), 0, s, t);
        });
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_optim_adam: a kernel launch failed");
    return 0;
}
