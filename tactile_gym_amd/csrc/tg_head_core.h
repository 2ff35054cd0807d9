// tg_head_core.h - what tg_action_head.hip (the device action heads) and tg_loss_head.hip (the device loss heads)
// share: the draw and the per-element float32 chains of the Gaussian log-prob and of the tanh correction, one copy.  Both translation units are
// compiled with -ffp-contract=off: every line below is one float32 operation with one rounding, in the order written; exp, tanh, log and the
// Box-Muller draw are evaluated in double on the float32 argument and rounded to float32 once.  tests/action_head_ref.py (device_order)
// restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tg_kernels.hpp"  // counter_draw: tg_sample_actions' counter-based generator

namespace tg {

// The 24 random bits of element e of draw `counter`: tg_sample_actions' integers.
__device__ __forceinline__ uint32_t head_bits24(uint64_t seed, uint64_t counter, uint64_t e) {
    return (uint32_t)(counter_draw(seed, counter, e) >> 40);
}

// Box-Muller on elements 2 e and 2 e + 1, all in double: u1 in (0, 1], u2 in [0, 1); |result| <= sqrt(-2 ln 2^-24) = 5.768
__device__ __forceinline__ float head_normal(uint64_t seed, uint64_t counter, uint64_t e) {
    const double u1 = (double)(head_bits24(seed, counter, 2 * e) + 1u) * (1.0 / 16777216.0);
    const double u2 = (double)head_bits24(seed, counter, 2 * e + 1) * (1.0 / 16777216.0);
    const double r = sqrt(-2.0 * log(u1));
    const double c = cos(6.283185307179586 * u2);
    return (float)(r * c);
}

// torch.clamp(ls, ls_min, ls_max): a NaN passes
__device__ __forceinline__ float head_clamp(float ls, float ls_min, float ls_max) {
    return ls < ls_min ? ls_min : (ls > ls_max ? ls_max : ls);
}

__device__ __forceinline__ float head_sigma(float ls) { return (float)exp((double)ls); }

// One column of torch's Normal.log_prob with log_std for log(exp(log_std)), d = x - mean:  -d^2 / (2 sigma^2) - log_std - log sqrt(2 pi)
__device__ __forceinline__ float head_gaussian_term(float d, float sigma, float ls) {
    const float q = d * d;
    const float var = sigma * sigma;
    const float den = 2.0f * var;
    const float t = q / den;
    const float t1 = -t - ls;
    return t1 - 0.9189385332046727f;
}

__device__ __forceinline__ float head_tanh(float x) { return (float)tanh((double)x); }

// One column of SquashedDiagGaussianDistribution's correction: log(1 - a^2 + 1e-6)
__device__ __forceinline__ float head_squash_w(float act) {
    const float aa = act * act;
    const float om = 1.0f - aa;
    return om + 1e-6f;
}

__device__ __forceinline__ float head_squash_term(float act) { return (float)log((double)head_squash_w(act)); }

}  // namespace tg
