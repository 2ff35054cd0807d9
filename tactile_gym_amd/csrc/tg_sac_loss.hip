// tg_sac_loss.hip - SAC's device losses (tactile_gym_amd.loss_head): what stable_baselines3's SAC.train does between the
// networks' outputs and its scalar losses, with the gradients at those outputs.
//   tg_sac_critic_loss   from the target networks' outputs to critic_loss: the TD target, one mse per critic, dloss / dq_cur_i
//   tg_sac_actor_loss    actor_loss and ent_coef_loss: dloss / d(log_prob, q_pi_i, log_ent_coef)
// Compiled with -ffp-contract=off: float32 arithmetic with one rounding per operation in the order written below, which tests/sac_loss_ref.py
// (*_device_order) restates; exp is evaluated in double on the float32 argument and rounded once.  Every mean over rows is accumulated in double
// in the order of tg_loss_core.h (chunks of 256 consecutive rows, the lane tree, the four wave sums in wave order, the chunk sums ascending) and
// rounded to float32 once.  No atomics: the same inputs give the same bits.
// One workgroup of 256 lanes walks the chunks in turn for every B <= TG_SAC_MAX_ROWS: SAC's minibatches are 64 .. 256 rows, one or two chunks,
// and the work is latency bound; what the calls buy is the dozens of torch launches they replace.  The critics' outputs are separate tensors
// (a cat would be a launch): their pointers travel by value in the kernel's arguments and every loop over them is unrolled, so the critic index
// is a constant in every access.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error
#include "tg_loss_core.h"  // the chunk and its sum, shared with tg_loss_head.hip

namespace tg {

constexpr int kSacCritics = TG_SAC_MAX_CRITICS;
constexpr int kCriticSlots = kSacCritics + 2;     // slots 0 .. 3: the critics' squared errors; 4: the target; 5: min_i q_next_i
constexpr int kActorSlots = 5;                    // the actor's row term, log_ent_coef (log_prob + target_entropy), log_prob + target_entropy, log_prob, min_i q_pi_i

struct SacIn { const float* p[kSacCritics]; };    // [n][B]
struct SacOut { float* p[kSacCritics]; };         // each nullable

// SB3's ent_coef: exp(log_ent_coef.detach()), or the fixed ent_coef_tensor
__device__ __forceinline__ float sac_alpha(const float* log_ent_coef, float ent_coef) {
    return log_ent_coef ? (float)exp((double)*log_ent_coef) : ent_coef;
}

// torch.min: a NaN in either operand is the minimum (fminf alone returns the other operand)
__device__ __forceinline__ float min_keeps_nan(float a, float b) {
    return a != a ? a : (b != b ? b : fminf(a, b));
}

struct SacCriticArgs {
    SacIn q_cur, q_next;
    SacOut dq_cur;
    const float* next_log_prob;  // [B]
    const float* rewards;        // [B]
    const float* dones;          // [B]
    const float* log_ent_coef;   // nullable scalar
    float* stats;                // [8]
    float* target;               // nullable [B]
    int32_t B, n;
    float gamma, ent_coef;
};

__global__ __launch_bounds__(kLossThreads) void k_sac_critic(SacCriticArgs a) {
    __shared__ double lds[kCriticSlots * kLossWaves];
    const int t = threadIdx.x;
    const float alpha = sac_alpha(a.log_ent_coef, a.ent_coef);
    const float fB = (float)a.B;
    double total = 0.0;                               // thread t < 6: the total of slot t
    for (int base = 0; base < a.B; base += kLossThreads) {
        const int i = base + t;
        const bool valid = i < a.B;
        float m = 0.0f, target = 0.0f;
        if (valid) {
            m = a.q_next.p[0][i];
#pragma unroll
            for (int c = 1; c < kSacCritics; ++c)
                if (c < a.n) m = min_keeps_nan(m, a.q_next.p[c][i]);
            const float t1 = alpha * a.next_log_prob[i];
            const float y = m - t1;
            const float nd = 1.0f - a.dones[i];
            const float g = nd * a.gamma;
            const float t2 = g * y;
            target = a.rewards[i] + t2;
            if (a.target) a.target[i] = target;
        }
#pragma unroll
        for (int c = 0; c < kSacCritics; ++c) {
            double sq = 0.0;
            if (c < a.n && valid) {
                const float e = a.q_cur.p[c][i] - target;
                const float s = e * e;
                sq = (double)s;
                if (a.dq_cur.p[c]) a.dq_cur.p[c][i] = e / fB;     // autograd's 0.5 * 2 (q - target) / B
            }
            slot_put(lds, c, sq);
        }
        slot_put(lds, kSacCritics, (double)target);
        slot_put(lds, kSacCritics + 1, (double)m);
        __syncthreads();
        if (t < kCriticSlots) total = total + slot_get(lds, t);
        __syncthreads();
    }
    if (t < kCriticSlots) lds[t] = total;
    __syncthreads();
    if (t == 0) {
        const double dB = (double)a.B;
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < kSacCritics; ++c) {
            const float mse = c < a.n ? (float)(lds[c] / dB) : 0.0f;
            if (c < a.n) sum = sum + mse;
            a.stats[4 + c] = mse;
        }
        a.stats[0] = 0.5f * sum;
        a.stats[1] = alpha;
        a.stats[2] = (float)(lds[kSacCritics] / dB);
        a.stats[3] = (float)(lds[kSacCritics + 1] / dB);
    }
}

struct SacActorArgs {
    SacIn q_pi;
    SacOut dq_pi;
    const float* log_prob;       // [B]
    const float* log_ent_coef;   // nullable scalar
    float* stats;                // [8]
    float* dlog_prob;            // nullable [B]
    int32_t B, n;
    int32_t want_ent;            // the entropy-coefficient loss is asked (log_ent_coef is then not null)
    float ent_coef, target_entropy;
};

__global__ __launch_bounds__(kLossThreads) void k_sac_actor(SacActorArgs a) {
    __shared__ double lds[kActorSlots * kLossWaves];
    const int t = threadIdx.x;
    const float alpha = sac_alpha(a.log_ent_coef, a.ent_coef);
    const float lec = a.want_ent ? *a.log_ent_coef : 0.0f;
    const float fB = (float)a.B;
    const float dlp = alpha / fB;
    const float dq = -1.0f / fB;
    double total = 0.0;                               // thread t < 5: the total of slot t
    for (int base = 0; base < a.B; base += kLossThreads) {
        const int i = base + t;
        const bool valid = i < a.B;
        double s_a = 0.0, s_p = 0.0, s_c = 0.0, s_lp = 0.0, s_m = 0.0;
        if (valid) {
            const float lp = a.log_prob[i];
            float m = a.q_pi.p[0][i];
            int k = 0;                                // torch.min(dim): the lowest index that attains the minimum takes the gradient;
                                                      // a NaN is the minimum, at the lowest index that holds one
#pragma unroll
            for (int c = 1; c < kSacCritics; ++c)
                if (c < a.n) {
                    const float q = a.q_pi.p[c][i];
                    if (q < m || (q != q && m == m)) {
                        m = q;
                        k = c;
                    }
                }
            const float t1 = alpha * lp;
            const float row = t1 - m;
            s_a = (double)row;
            s_lp = (double)lp;
            s_m = (double)m;
            if (a.want_ent) {
                const float c1 = lp + a.target_entropy;
                const float p = lec * c1;
                s_p = (double)p;
                s_c = (double)c1;
            }
            if (a.dlog_prob) a.dlog_prob[i] = dlp;
#pragma unroll
            for (int c = 0; c < kSacCritics; ++c)
                if (c < a.n && a.dq_pi.p[c]) a.dq_pi.p[c][i] = c == k ? dq : 0.0f;
        }
        slot_put(lds, 0, s_a);
        slot_put(lds, 1, s_p);
        slot_put(lds, 2, s_c);
        slot_put(lds, 3, s_lp);
        slot_put(lds, 4, s_m);
        __syncthreads();
        if (t < kActorSlots) total = total + slot_get(lds, t);
        __syncthreads();
    }
    if (t < kActorSlots) lds[t] = total;
    __syncthreads();
    if (t == 0) {
        const double dB = (double)a.B;
        a.stats[0] = (float)(lds[0] / dB);
        a.stats[1] = a.want_ent ? -(float)(lds[1] / dB) : 0.0f;
        a.stats[2] = alpha;
        a.stats[3] = (float)(lds[3] / dB);
        a.stats[4] = (float)(lds[4] / dB);
        a.stats[5] = a.want_ent ? -(float)(lds[2] / dB) : 0.0f;
        a.stats[6] = 0.0f;
        a.stats[7] = 0.0f;
    }
}

}  // namespace tg

extern "C" int tg_sac_critic_loss(const float* const* q_cur_dev, const float* const* q_next_dev, int32_t n_critics, const float* next_log_prob_dev,
                                  const float* rewards_dev, const float* dones_dev, int64_t B, float gamma, const float* log_ent_coef_dev,
                                  float ent_coef, float* stats_out, float* target_out, float* const* dq_cur_out, void* hip_stream) {
    using tg::report_error;
    if (n_critics < 1 || n_critics > TG_SAC_MAX_CRITICS) return report_error(-1, "tg_sac_critic_loss: need 1 <= n_critics <= TG_SAC_MAX_CRITICS");
    if (B < 1 || B > TG_SAC_MAX_ROWS) return report_error(-1, "tg_sac_critic_loss: need 1 <= B <= TG_SAC_MAX_ROWS");
    if (!q_cur_dev || !q_next_dev || !next_log_prob_dev || !rewards_dev || !dones_dev) return report_error(-1, "tg_sac_critic_loss: NULL input");
    for (int c = 0; c < n_critics; ++c)
        if (!q_cur_dev[c] || !q_next_dev[c]) return report_error(-1, "tg_sac_critic_loss: NULL critic output");
    if (!stats_out) return report_error(-1, "tg_sac_critic_loss: NULL stats_out");
    tg::SacCriticArgs a = {};
    for (int c = 0; c < n_critics; ++c) {
        a.q_cur.p[c] = q_cur_dev[c];
        a.q_next.p[c] = q_next_dev[c];
        a.dq_cur.p[c] = dq_cur_out ? dq_cur_out[c] : nullptr;
    }
    a.next_log_prob = next_log_prob_dev;
    a.rewards = rewards_dev;
    a.dones = dones_dev;
    a.log_ent_coef = log_ent_coef_dev;
    a.stats = stats_out;
    a.target = target_out;
    a.B = (int32_t)B;
    a.n = n_critics;
    a.gamma = gamma;
    a.ent_coef = ent_coef;
    hipLaunchKernelGGL(tg::k_sac_critic, dim3(1), dim3(tg::kLossThreads), 0, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_sac_critic_loss: the kernel launch failed");
    return 0;
}

extern "C" int tg_sac_actor_loss(const float* log_prob_dev, const float* const* q_pi_dev, int32_t n_critics, int64_t B, const float* log_ent_coef_dev,
                                 float ent_coef, float target_entropy, int32_t want_ent_coef_loss, float* stats_out, float* dlog_prob_out,
                                 float* const* dq_pi_out, void* hip_stream) {
    using tg::report_error;
    if (n_critics < 1 || n_critics > TG_SAC_MAX_CRITICS) return report_error(-1, "tg_sac_actor_loss: need 1 <= n_critics <= TG_SAC_MAX_CRITICS");
    if (B < 1 || B > TG_SAC_MAX_ROWS) return report_error(-1, "tg_sac_actor_loss: need 1 <= B <= TG_SAC_MAX_ROWS");
    if (!log_prob_dev || !q_pi_dev) return report_error(-1, "tg_sac_actor_loss: NULL input");
    for (int c = 0; c < n_critics; ++c)
        if (!q_pi_dev[c]) return report_error(-1, "tg_sac_actor_loss: NULL critic output");
    if (!stats_out) return report_error(-1, "tg_sac_actor_loss: NULL stats_out");
    if (want_ent_coef_loss && !log_ent_coef_dev) return report_error(-1, "tg_sac_actor_loss: the entropy-coefficient loss needs log_ent_coef_dev");
    tg::SacActorArgs a = {};
    for (int c = 0; c < n_critics; ++c) {
        a.q_pi.p[c] = q_pi_dev[c];
        a.dq_pi.p[c] = dq_pi_out ? dq_pi_out[c] : nullptr;
    }
    a.log_prob = log_prob_dev;
    a.log_ent_coef = log_ent_coef_dev;
    a.stats = stats_out;
    a.dlog_prob = dlog_prob_out;
    a.B = (int32_t)B;
    a.n = n_critics;
    a.want_ent = want_ent_coef_loss ? 1 : 0;
    a.ent_coef = ent_coef;
    a.target_entropy = target_entropy;
    hipLaunchKernelGGL(tg::k_sac_actor, dim3(1), dim3(tg::kLossThreads), 0, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_sac_actor_loss: the kernel launch failed");
    return 0;
}
