// tg_action_head.hip - the device action heads (tactile_gym_amd.action_head): what stable_baselines3 does between the policy
// network's output and venv.step() for use_sde=False - DiagGaussianDistribution (PPO: sample, log-prob summed over the action axis, the clip
// for the env only), SquashedDiagGaussianDistribution (SAC: tanh, the corrected log-prob, unscale_action) and SAC's uniform warm-up - as ONE
// launch over float32 [N][A].  Compiled with -ffp-contract=off: float32 arithmetic with one rounding per operation in the order written
// below, which tests/action_head_ref.py (device_order) restates; exp, tanh, log and the Box-Muller draw are evaluated in double on the float32
// argument and rounded to float32 once.
//
//   k_action_head<MODE>  one lane per env (row i), 256-lane workgroups, the A columns in ascending order inside the lane: the row sums of the
//                        log-prob stay in one lane in a fixed order.  lo / hi travel in the kernel arguments.  No LDS, no scratch.
// The launch moves a few tens of KB and is latency bound; what it buys is the ten-odd torch launches it replaces.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error
#include "tg_head_core.h"  // the draw and the per-element chains, shared with tg_loss_head.hip

namespace tg {

constexpr int kHeadThreads = 256;

struct HeadArgs {
    const float* mean;        // [N][A]
    const float* log_std;     // [A] (stride 0) or [N][A] (stride A)
    const float* noise_in;    // nullable [N][A]: used in place of the draws
    float* actions;           // nullable outputs
    float* env;
    float* gauss;
    float* log_prob;
    float* noise_out;
    int64_t N;
    int32_t A;
    int32_t ls_stride;
    int32_t deterministic;
    float ls_min, ls_max;
    uint64_t seed, counter;
    float lo[TG_HEAD_MAX_ACT];
    float hi[TG_HEAD_MAX_ACT];
};

template <int MODE>
__global__ __launch_bounds__(kHeadThreads) void k_action_head(HeadArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kHeadThreads + threadIdx.x;
    if (i >= a.N) return;
    const int A = a.A;
    if (MODE == TG_HEAD_UNIFORM) {
        for (int j = 0; j < A; ++j) {
            const int64_t e = i * A + j;
            const float lo = a.lo[j], hi = a.hi[j];
            const float u = a.noise_in ? a.noise_in[e] : (float)head_bits24(a.seed, a.counter, (uint64_t)e) * (1.0f / 16777216.0f);
            const float span = hi - lo;
            const float scaled = span * u;
            float env = lo + scaled;                             // tg_sample_actions' lo + (hi - lo) u
            env = env > hi ? hi : env;                           // the sum can round one neighbour past hi when hi - lo is inexact
            if (a.noise_out) a.noise_out[e] = u;
            if (a.env) a.env[e] = env;
            if (a.actions) {                                     // SB3's scale_action: 2 ((env - lo) / (hi - lo)) - 1
                const float off = env - lo;
                const float frac = off / span;
                const float twice = 2.0f * frac;
                a.actions[e] = twice - 1.0f;
            }
        }
        return;
    }
    float gsum = 0.0f, csum = 0.0f;
    for (int j = 0; j < A; ++j) {
        const int64_t e = i * A + j;
        const float mean = a.mean[e];
        float ls = a.log_std[a.ls_stride ? e : (int64_t)j];
        ls = head_clamp(ls, a.ls_min, a.ls_max);                                   // a NaN passes, as torch.clamp
        const float sigma = head_sigma(ls);
        const float eps = a.noise_in ? a.noise_in[e] : (a.deterministic ? 0.0f : head_normal(a.seed, a.counter, (uint64_t)e));
        // deterministic is SB3's mode(), mean itself: no product with sigma, whose 0 inf or 0 NaN would make a NaN of a finite mean
        const float se = (a.deterministic && !a.noise_in) ? 0.0f : sigma * eps;
        const float x = mean + se;
        if (a.noise_out) a.noise_out[e] = eps;
        if (a.gauss) a.gauss[e] = x;
        // torch's Normal.log_prob with log_std for log(exp(log_std)): -(x - mean)^2 / (2 sigma^2) - log_std - log sqrt(2 pi)
        const float d = x - mean;
        const float term = head_gaussian_term(d, sigma, ls);
        gsum = gsum + term;
        if (MODE == TG_HEAD_GAUSSIAN) {
            if (a.actions) a.actions[e] = x;
            if (a.env) {                                          // np.clip: min(max(x, lo), hi), a NaN passes
                const float lo = a.lo[j], hi = a.hi[j];
                const float up = x < lo ? lo : x;
                a.env[e] = up > hi ? hi : up;
            }
        } else {
            const float act = head_tanh(x);
            if (a.actions) a.actions[e] = act;
            if (a.env) {                                          // SB3's unscale_action: lo + (0.5 (a + 1) (hi - lo))
                const float lo = a.lo[j], hi = a.hi[j];
                const float p1 = act + 1.0f;
                const float half = 0.5f * p1;
                const float span = hi - lo;
                const float scaled = half * span;
                const float un = lo + scaled;
                const float up = un < lo ? lo : un;               // at a = +-1 the formula can leave [lo, hi] by one rounding when hi - lo
                a.env[e] = up > hi ? hi : up;                     // is inexact: the env is never handed an action outside its space
            }
            const float c = head_squash_term(act);                // log(1 - a^2 + 1e-6)
            csum = csum + c;
        }
    }
    if (a.log_prob) a.log_prob[i] = MODE == TG_HEAD_GAUSSIAN ? gsum : gsum - csum;
}

}  // namespace tg

extern "C" int tg_action_head(const float* mean_dev, const float* log_std_dev, int32_t log_std_stride, int64_t N, int32_t A, const float* lo,
                              const float* hi, float log_std_min, float log_std_max, int32_t mode, int32_t deterministic, uint64_t seed,
                              uint64_t counter, const float* noise_in_dev, float* actions_out, float* env_actions_out, float* gaussian_out,
                              float* log_prob_out, float* noise_out, void* hip_stream) {
    using tg::report_error;
    if (mode != TG_HEAD_GAUSSIAN && mode != TG_HEAD_SQUASHED && mode != TG_HEAD_UNIFORM)
        return report_error(-1, "tg_action_head: mode must be TG_HEAD_GAUSSIAN, TG_HEAD_SQUASHED or TG_HEAD_UNIFORM");
    const bool gaussian = mode != TG_HEAD_UNIFORM;
    if (gaussian && !mean_dev) return report_error(-1, "tg_action_head: NULL mean_dev");
    if (gaussian && !log_std_dev) return report_error(-1, "tg_action_head: NULL log_std_dev");
    if (A < 1 || A > TG_HEAD_MAX_ACT) return report_error(-1, "tg_action_head: need 1 <= A <= TG_HEAD_MAX_ACT");
    if (log_std_stride != 0 && log_std_stride != A) return report_error(-1, "tg_action_head: log_std_stride must be 0 or A");
    if (N < 0 || N > TG_HEAD_MAX_ROWS) return report_error(-1, "tg_action_head: need 0 <= N <= TG_HEAD_MAX_ROWS");
    if (!lo || !hi) return report_error(-1, "tg_action_head: NULL lo or hi");
    for (int j = 0; j < A; ++j) {
        if (!(lo[j] <= hi[j])) return report_error(-1, "tg_action_head: need lo[j] <= hi[j]");
        if (mode != TG_HEAD_GAUSSIAN && lo[j] == hi[j])
            return report_error(-1, "tg_action_head: lo[j] == hi[j] in the squashed or uniform mode (scale_action would divide by zero)");
    }
    if (!(log_std_min <= log_std_max)) return report_error(-1, "tg_action_head: need log_std_min <= log_std_max");
    if (N == 0) return 0;
    if (!actions_out && !env_actions_out && !gaussian_out && !log_prob_out && !noise_out) return 0;
    tg::HeadArgs a = {};
    a.mean = mean_dev;
    a.log_std = log_std_dev;
    a.noise_in = noise_in_dev;
    a.actions = actions_out;
    a.env = env_actions_out;
    a.gauss = gaussian ? gaussian_out : nullptr;
    a.log_prob = gaussian ? log_prob_out : nullptr;
    a.noise_out = noise_out;
    a.N = N;
    a.A = A;
    a.ls_stride = log_std_stride;
    a.deterministic = deterministic ? 1 : 0;
    a.ls_min = log_std_min;
    a.ls_max = log_std_max;
    a.seed = seed;
    a.counter = counter;
    for (int j = 0; j < A; ++j) {
        a.lo[j] = lo[j];
        a.hi[j] = hi[j];
    }
    const dim3 grid((unsigned)((N + tg::kHeadThreads - 1) / tg::kHeadThreads)), block(tg::kHeadThreads);
    hipStream_t s = (hipStream_t)hip_stream;
    if (mode == TG_HEAD_GAUSSIAN)
        hipLaunchKernelGGL(tg::k_action_head<TG_HEAD_GAUSSIAN>, grid, block, 0, s, a);
    else if (mode == TG_HEAD_SQUASHED)
        hipLaunchKernelGGL(tg::k_action_head<TG_HEAD_SQUASHED>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(tg::k_action_head<TG_HEAD_UNIFORM>, grid, block, 0, s, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_action_head: the kernel launch failed");
    return 0;
}
