// tg_conv_stem.hip - the device conv stem (tactile_gym_amd.torch_layers): the first stage of stable_baselines3's NatureCNN on
// this project's observations - preprocess_obs (obs.float() / 255), Conv2d(C, 32, kernel_size=8, stride=4), ReLU - as ONE launch that reads the
// uint8 (or float32) image once and writes the activated float32 output once, and its backward pass for the weight and the bias (the input is
// data and gets no gradient).  Compiled with -ffp-contract=off; the only fused multiply-adds are the ones written: the MFMA's and __builtin_fmaf.
//
// Specification per output element, k = (c 8 + ky) 8 + kx (torch's [32][Cn][8][8] weight, flattened), K = 64 Cn:
//     acc = 0;  for k = 0 .. K-1 ascending: acc = fmaf((float) x_k, w[co][k], acc);  z = fmaf(acc, scale, bias[co]);  y = relu(z)
// relu(z) = z > 0 ? z : (z != z ? z : 0): fmaxf(z, 0)'s bits for every number, and a NaN stays a NaN as in torch.relu.
// v_mfma_f32_32x32x2_f32 is bit for bit that chain (two k per instruction, the lower first), so every output element has ONE arithmetic order,
// whatever the batch it sits in and wherever its tile falls.
//
//   k_conv_stem<T, CF>      one 256-lane workgroup per region: one image, up to 128 output positions (R output rows x Cv <= 128 output columns,
//                           flattened r Cv + cx), one 32-position tile per wavefront.  Channel by channel (k ascending) the workgroup stages
//                           the channel's 32 x 64 weights ([k][co], padded rows) and the (4 R + 4) x (4 Cv + 4) input elements the region reads
//                           in LDS in the input's own type; lane l of a wave then feeds A = w[co = l & 31][k = 2 s + (l >> 5)] and
//                           B = (float) x[k][position l & 31], converted on the LDS read, to 32 MFMAs on ONE accumulator tile: D[co][position],
//                           position on the lane (C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so the stores
//                           of one register are 32 consecutive floats of one output channel.  Lanes past the region's last position compute on
//                           position 0 and store nothing.
//   k_conv_stem_bwd<T, CF>  grid (G, Cn): workgroup g of channel c walks regions g, g + G, ... in ascending order; it stages
//                           g = dy (y > 0) of the region as [position][co] and the channel's input elements, and accumulates
//                           D[co][k] += sum over positions of g[co][position] (float) x[position][k] (A = g, B = x, two positions per MFMA):
//                           wave (kt, ph) owns k tile kt of the channel's 64 and positions ph 64 .. ph 64 + 63 of every region.  Partials
//                           [G][2][32][K] and, from the c = 0 workgroups, bias partials [G][8][32] go to the caller's workspace.
//   k_conv_stem_reduce      four lanes per dweight / dbias element sum a quarter of its partials each in ascending order, the four are added
//                           as (q0 + q1) + (q2 + q3) and scaled: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error

namespace tg {

constexpr int kStemThreads = 256;
constexpr int kStemPos = 128;                        // output positions of a region: 4 waves x one 32-wide tile
constexpr int kStemXs = 16 * (kStemPos + kStemPos + 2);   // max (4 R + 4)(4 Cv + 4) = 16 (R Cv + R + Cv + 1) over R Cv <= 128
constexpr int kStemWPitch = TG_STEM_OUT + 1;         // [k][co] rows padded: the transposing writes hit 64 banks
constexpr int kStemBwdGroups = 256;                  // G: partial sums per weight = 2 G
constexpr int kStemBiasParts = 8;
constexpr int64_t kStemMaxRegions = (1ll << 24) - 1;  // one launch: 256 lanes x regions stays below 2^32

typedef float f32x16 __attribute__((ext_vector_type(16)));

// How an image's OH x OW output positions are cut into regions of at most kStemPos: column chunks of Cw, strips of R rows.
struct StemGeom {
    int32_t OH, OW, Cw, n_chunks, R, n_strips;
    int64_t regions;                                 // B n_strips n_chunks
};

__host__ __device__ inline StemGeom stem_geom(int64_t B, int32_t H, int32_t W) {
    StemGeom g;
    g.OH = (H - TG_STEM_KERNEL) / TG_STEM_STRIDE + 1;
    g.OW = (W - TG_STEM_KERNEL) / TG_STEM_STRIDE + 1;
    g.Cw = g.OW < kStemPos ? g.OW : kStemPos;
    g.n_chunks = (g.OW + g.Cw - 1) / g.Cw;
    g.R = kStemPos / g.Cw;
    if (g.R > g.OH) g.R = g.OH;
    g.n_strips = (g.OH + g.R - 1) / g.R;
    g.regions = B * g.n_strips * g.n_chunks;
    return g;
}

struct StemArgs {
    const void* x;            // T [B][Cn][H][W] (CF) or [B][H][W][Cn]
    const float* w;           // [32][K]
    const float* bias;        // [32]
    float* y;                 // forward: out [B][32][OH][OW]
    const float* yin;         // backward: the forward's output
    const float* dy;
    float* ws;                // backward partials
    float* wsb;
    int64_t B;
    int32_t Cn, H, W;
    float scale;
    StemGeom g;
};

struct StemRegion {
    int64_t b;
    int32_t oy0, ox0, Rv, Cv, npos, ncols, nelem;
};

__device__ __forceinline__ StemRegion stem_region(const StemGeom& g, int64_t region) {
    StemRegion r;
    const int32_t chunk = (int32_t)(region % g.n_chunks);
    region /= g.n_chunks;
    const int32_t strip = (int32_t)(region % g.n_strips);
    r.b = region / g.n_strips;
    r.oy0 = strip * g.R;
    r.ox0 = chunk * g.Cw;
    r.Rv = g.OH - r.oy0 < g.R ? g.OH - r.oy0 : g.R;
    r.Cv = g.OW - r.ox0 < g.Cw ? g.OW - r.ox0 : g.Cw;
    r.npos = r.Rv * r.Cv;
    r.ncols = TG_STEM_STRIDE * r.Cv + 4;
    r.nelem = (TG_STEM_STRIDE * r.Rv + 4) * r.ncols;             // <= kStemXs
    return r;
}

// Channel c's input elements of the region, rows 4 oy0 .. 4 (oy0 + Rv) + 3 and columns 4 ox0 .. 4 (ox0 + Cv) + 3 (all inside the image), as read.
template <typename T, bool CF>
__device__ __forceinline__ void stem_stage_x(const StemArgs& a, const StemRegion& r, int32_t c, T* xs, int tid) {
    const T* x = (const T*)a.x;
    for (int32_t idx = tid; idx < r.nelem; idx += kStemThreads) {
        const int32_t row = idx / r.ncols, col = idx - row * r.ncols;
        const int64_t yy = TG_STEM_STRIDE * r.oy0 + row, xx = TG_STEM_STRIDE * r.ox0 + col;
        const int64_t gi = CF ? ((r.b * a.Cn + c) * a.H + yy) * a.W + xx : ((r.b * a.H + yy) * a.W + xx) * a.Cn + c;
        xs[idx] = x[gi];
    }
}

template <typename T, bool CF>
__global__ __launch_bounds__(kStemThreads) void k_conv_stem(StemArgs a) {
    __shared__ float wl[64 * kStemWPitch];
    __shared__ T xs[kStemXs];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const StemRegion r = stem_region(a.g, (int64_t)blockIdx.x);
    const int32_t K = 64 * a.Cn;
    const int32_t m = wave * 32 + j;
    const bool valid = m < r.npos, active = wave * 32 < r.npos;           // active: the same for the whole wave
    const int32_t mm = valid ? m : 0;
    const int32_t ry = mm / r.Cv, cx = mm - ry * r.Cv;
    const int32_t xoff = TG_STEM_STRIDE * ry * r.ncols + TG_STEM_STRIDE * cx + h;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int32_t c = 0; c < a.Cn; ++c) {
        if (c) __syncthreads();
        for (int32_t idx = tid; idx < TG_STEM_OUT * 64; idx += kStemThreads) {
            const int32_t co = idx >> 6, k = idx & 63;
            wl[k * kStemWPitch + co] = a.w[(int64_t)co * K + c * 64 + k];
        }
        stem_stage_x<T, CF>(a, r, c, xs, tid);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int s = 0; s < 32; ++s) {                                 // k = 2 s + h: ky = s >> 2, kx = 2 (s & 3) + h
                const float wa = wl[(2 * s + h) * kStemWPitch + j];
                const float xb = (float)xs[xoff + (s >> 2) * r.ncols + 2 * (s & 3)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, xb, acc, 0, 0, 0);
            }
        }
    }
    if (active && valid) {
        const int64_t plane = (int64_t)a.g.OH * a.g.OW;
        const int64_t at = (int64_t)(r.oy0 + ry) * a.g.OW + r.ox0 + cx;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int32_t co = (i & 3) + 8 * (i >> 2) + 4 * h;
            const float z = __builtin_fmaf(acc[i], a.scale, a.bias[co]);
            a.y[(r.b * TG_STEM_OUT + co) * plane + at] = z > 0.0f ? z : (z != z ? z : 0.0f);   // torch.relu: a NaN stays a NaN
        }
    }
}

template <typename T, bool CF>
__global__ __launch_bounds__(kStemThreads) void k_conv_stem_bwd(StemArgs a) {
    __shared__ float gs[kStemPos * kStemWPitch];
    __shared__ T xs[kStemXs];
    __shared__ int32_t poff[kStemPos];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t grp = blockIdx.x, G = gridDim.x, c = blockIdx.y;
    const int32_t K = 64 * a.Cn;
    const int32_t kt = wave & 1, ph = wave >> 1;
    const int32_t k = kt * 32 + j, ky = k >> 3, kx = k & 7;
    const int32_t bco = tid & 31, bpart = tid >> 5;                        // the bias sums: channel, sixteen positions of the 128
    const int64_t plane = (int64_t)a.g.OH * a.g.OW;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    float bsum = 0.0f;
    for (int64_t region = grp; region < a.g.regions; region += G) {
        const StemRegion r = stem_region(a.g, region);
        if (region != grp) __syncthreads();
        for (int32_t idx = tid; idx < TG_STEM_OUT * kStemPos; idx += kStemThreads) {
            const int32_t co = idx >> 7, m = idx & (kStemPos - 1);
            float v = 0.0f;
            if (m < r.npos) {
                const int32_t ry = m / r.Cv, cx = m - ry * r.Cv;
                const int64_t gi = (r.b * TG_STEM_OUT + co) * plane + (int64_t)(r.oy0 + ry) * a.g.OW + r.ox0 + cx;
                v = a.yin[gi] > 0.0f ? a.dy[gi] : 0.0f;
            }
            gs[m * kStemWPitch + co] = v;
        }
        if (tid < kStemPos) {
            const int32_t ry = tid / r.Cv, cx = tid - ry * r.Cv;
            poff[tid] = tid < r.npos ? TG_STEM_STRIDE * ry * r.ncols + TG_STEM_STRIDE * cx : -1;
        }
        stem_stage_x<T, CF>(a, r, c, xs, tid);
        __syncthreads();
        if (ph * 64 < r.npos) {
            const int32_t koff = ky * r.ncols + kx;
#pragma unroll 8
            for (int s = 0; s < 32; ++s) {                                 // positions ph 64 + 2 s + h: past the region g = 0 and x = 0
                const int32_t m = ph * 64 + 2 * s + h;
                const float ga = gs[m * kStemWPitch + j];
                const int32_t po = poff[m];
                const float xv = (float)xs[(po < 0 ? 0 : po) + koff];
                const float xb = po < 0 ? 0.0f : xv;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, xb, acc, 0, 0, 0);
            }
        }
        if (c == 0) {
            for (int i = 0; i < kStemPos / kStemBiasParts; ++i) bsum = bsum + gs[(bpart * (kStemPos / kStemBiasParts) + i) * kStemWPitch + bco];
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int32_t co = (i & 3) + 8 * (i >> 2) + 4 * h;
        a.ws[(((int64_t)grp * 2 + ph) * TG_STEM_OUT + co) * K + c * 64 + k] = acc[i];
    }
    if (c == 0) a.wsb[((int64_t)grp * kStemBiasParts + bpart) * TG_STEM_OUT + bco] = bsum;
}

constexpr int kStemReduceOut = 64;                   // outputs of a reduction workgroup, each summed by 256 / 64 = 4 lanes

__global__ __launch_bounds__(kStemThreads) void k_conv_stem_reduce(const float* ws, const float* wsb, int32_t G, int32_t K, float scale,
                                                                    float* dweight, float* dbias) {
    __shared__ float part[kStemThreads / kStemReduceOut][kStemReduceOut];
    const int32_t tl = threadIdx.x % kStemReduceOut, ps = threadIdx.x / kStemReduceOut;
    const int32_t t = blockIdx.x * kStemReduceOut + tl, nw = TG_STEM_OUT * K;
    const bool is_w = t < nw, live = t < nw + TG_STEM_OUT;
    float s = 0.0f;
    if (live) {                                          // lane ps sums the ps-th quarter of the partials, ascending
        const float* src = is_w ? ws + t : wsb + (t - nw);
        const int64_t stride = is_w ? nw : TG_STEM_OUT;
        const int32_t P = is_w ? 2 * G : kStemBiasParts * G;
        const int32_t p0 = (int32_t)((int64_t)P * ps / 4), p1 = (int32_t)((int64_t)P * (ps + 1) / 4);
#pragma unroll 8
        for (int32_t p = p0; p < p1; ++p) s = s + src[p * stride];
    }
    part[ps][tl] = s;
    __syncthreads();
    if (live && ps == 0) {
        const float lo = part[0][tl] + part[1][tl], hi = part[2][tl] + part[3][tl];
        const float r = lo + hi;
        if (is_w) dweight[t] = scale * r;
        else dbias[t - nw] = r;
    }
}

static int32_t stem_groups(const StemGeom& g) { return (int32_t)(g.regions < kStemBwdGroups ? g.regions : kStemBwdGroups); }

static int64_t stem_workspace(const StemGeom& g, int32_t Cn) {
    const int64_t G = stem_groups(g);
    return (G * 2 * TG_STEM_OUT * 64 * Cn + G * kStemBiasParts * TG_STEM_OUT) * (int64_t)sizeof(float);
}

// The checks the three calls share; 0 or the error's code.
static int stem_check(const char* who, int64_t B, int32_t Cn, int32_t H, int32_t W) {
    static thread_local char msg[160];
    const char* what = nullptr;
    if (Cn < 1 || Cn > TG_STEM_MAX_CIN) what = "need 1 <= Cn <= TG_STEM_MAX_CIN";
    else if (H < TG_STEM_KERNEL || W < TG_STEM_KERNEL) what = "need H >= 8 and W >= 8";
    else if (B < 0) what = "need B >= 0";
    else if (stem_geom(B, H, W).regions > kStemMaxRegions) what = "too many output positions for one launch";
    if (!what) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return report_error(-1, msg);
}

}  // namespace tg

extern "C" int tg_conv_stem(const void* x_dev, int32_t x_is_float, int32_t channels_first, int64_t B, int32_t Cn, int32_t H, int32_t W,
                            const float* weight_dev, const float* bias_dev, float scale, float* y_dev, void* hip_stream) {
    using namespace tg;
    if (!x_dev || !weight_dev || !bias_dev || !y_dev) return report_error(-1, "tg_conv_stem: NULL x_dev, weight_dev, bias_dev or y_dev");
    if (int rc = stem_check("tg_conv_stem", B, Cn, H, W)) return rc;
    if (B == 0) return 0;
    StemArgs a = {};
    a.x = x_dev;
    a.w = weight_dev;
    a.bias = bias_dev;
    a.y = y_dev;
    a.B = B;
    a.Cn = Cn;
    a.H = H;
    a.W = W;
    a.scale = scale;
    a.g = stem_geom(B, H, W);
    const dim3 grid((unsigned)a.g.regions), block(kStemThreads);
    hipStream_t s = (hipStream_t)hip_stream;
    if (x_is_float) {
        if (channels_first) hipLaunchKernelGGL((k_conv_stem<float, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_conv_stem<float, false>), grid, block, 0, s, a);
    } else {
        if (channels_first) hipLaunchKernelGGL((k_conv_stem<uint8_t, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_conv_stem<uint8_t, false>), grid, block, 0, s, a);
    }
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_stem: the kernel launch failed");
    return 0;
}

extern "C" int64_t tg_conv_stem_bwd_workspace(int64_t B, int32_t Cn, int32_t H, int32_t W) {
    using namespace tg;
    if (int rc = stem_check("tg_conv_stem_bwd_workspace", B, Cn, H, W)) return rc;
    return stem_workspace(stem_geom(B, H, W), Cn);
}

extern "C" int tg_conv_stem_bwd(const void* x_dev, int32_t x_is_float, int32_t channels_first, int64_t B, int32_t Cn, int32_t H, int32_t W,
                                const float* y_dev, const float* dy_dev, float scale, float* dweight_dev, float* dbias_dev, void* workspace_dev,
                                int64_t workspace_bytes, void* hip_stream) {
    using namespace tg;
    if (!x_dev || !y_dev || !dy_dev || !dweight_dev || !dbias_dev)
        return report_error(-1, "tg_conv_stem_bwd: NULL x_dev, y_dev, dy_dev, dweight_dev or dbias_dev");
    if (int rc = stem_check("tg_conv_stem_bwd", B, Cn, H, W)) return rc;
    if (B == 0) return 0;
    StemArgs a = {};
    a.g = stem_geom(B, H, W);
    if (!workspace_dev) return report_error(-1, "tg_conv_stem_bwd: NULL workspace_dev");
    if (workspace_bytes < stem_workspace(a.g, Cn))
        return report_error(-1, "tg_conv_stem_bwd: the workspace is smaller than tg_conv_stem_bwd_workspace's size");
    const int32_t G = stem_groups(a.g), K = 64 * Cn;
    a.x = x_dev;
    a.yin = y_dev;
    a.dy = dy_dev;
    a.ws = (float*)workspace_dev;
    a.wsb = a.ws + (int64_t)G * 2 * TG_STEM_OUT * K;
    a.B = B;
    a.Cn = Cn;
    a.H = H;
    a.W = W;
    a.scale = scale;
    const dim3 grid((unsigned)G, (unsigned)Cn), block(kStemThreads);
    hipStream_t s = (hipStream_t)hip_stream;
    if (x_is_float) {
        if (channels_first) hipLaunchKernelGGL((k_conv_stem_bwd<float, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_conv_stem_bwd<float, false>), grid, block, 0, s, a);
    } else {
        if (channels_first) hipLaunchKernelGGL((k_conv_stem_bwd<uint8_t, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_conv_stem_bwd<uint8_t, false>), grid, block, 0, s, a);
    }
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_stem_bwd: the kernel launch failed");
    const int32_t n_out = TG_STEM_OUT * K + TG_STEM_OUT;
    hipLaunchKernelGGL(k_conv_stem_reduce, dim3((unsigned)((n_out + kStemReduceOut - 1) / kStemReduceOut)), block, 0, s, a.ws, a.wsb, G, K, scale,
                       dweight_dev, dbias_dev);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_stem_bwd: the reduction's launch failed");
    return 0;
}
