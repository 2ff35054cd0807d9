// tg_conv.hip - the device NatureCNN tail (tactile_gym_amd.torch_layers): a valid (unpadded) strided convolution with bias and
// ReLU on float32 [B][Cin][H][W], torch's [Cout][Cin][KH][KW] weight and [Cout] bias, every size a runtime parameter.  NatureCNN's
// Conv2d(32, 64, 4, 2), Conv2d(64, 64, 3, 1) and Flatten + Linear(64 h w, F) (a convolution of conv3's [64][h][w] output with an h x w
// kernel: OH = OW = 1, K = 64 h w; nn.Linear's [F][64 h w] weight is that kernel, flattened) are three instances of it.  Compiled with
// -ffp-contract=off; the only fused multiply-adds are the MFMA's.
//
// Specification per output element, k = (c KH + ky) KW + kx, K = Cin KH KW (even):
//     acc = 0;  for k = 0 .. K-1 ascending: acc = fmaf(x_k, w[co][k], acc);  z = acc + b[co];  y = z > 0 ? z : (z != z ? z : 0)
// ONE chain for every shape (no K segmentation: S = 1 everywhere).  v_mfma_f32_32x32x2_f32 on one accumulator tile is bit for bit that chain
// (two k per instruction, the lower first; operand and C/D lane maps as in tg_conv_stem.hip's header), so an element's arithmetic order is a
// function of the layer's shape alone: never of B, of the row's index or of where its tile falls.
// Backward, g = dy (y > 0):  dbias[co] = sum_m g[m][co],  dweight[co][k] = sum_m g[m][co] x[m][k]  (m = (b OH + oy) OW + ox ascending inside
// a workgroup's walk, the workgroups' partials added ascending), and
//     dx[b][c][iy][ix] = one chain over j = (co KH + ky) KW + kx ascending of g[b][co][oy][ox] w[co][c][ky][kx],  oy = (iy - ky) / stride,
//     ox = (ix - kx) / stride; a term whose division is inexact or whose (oy, ox) lies outside the output is fed as 0 w or skipped (a
//     whole MFMA is skipped when none of its 2 x 32 terms exists; with finite w the bits are the same: the accumulator is never -0).
//
//   k_conv_fwd     one 256-lane workgroup per (position block, channel block).  Output positions are flattened OVER THE BATCH,
//                  m = (b OH + oy) OW + ox, and cut into 32-position tiles; a workgroup's four waves are PT position tiles x CTW channel tiles
//                  (CTW = 4, 2, 1 for Cout >= 128, 64, 32; PT = 4 / CTW).  In chunks of 32 k the workgroup stages w as [k][co] and the
//                  gathered x as [k][position] in LDS (rows padded to 129 floats, as kStemWPitch: conflict-free transposing writes), lanes
//                  along k on the global reads (contiguous for the linear layer, runs of KW for a convolution); lane l of a wave feeds
//                  A = w[co = l & 31][k = 2 s + (l >> 5)], B = x[k][position l & 31] to 16 MFMAs on ONE accumulator tile D[co][position].
//                  The per-k input offsets of the next chunk are computed while this one is staged (two tables, no third barrier).
//                  Lanes past the last position compute on position 0 and store nothing.
//   k_conv_bwd     grid (channel-pair x k-pair blocks, P): workgroup p walks the 64-position chunks p, p + P, ... in ascending order, stages
//                  g as [position][co] (64 channels) and x as [position][k] (64 k) and accumulates D[co][k] += sum over positions
//                  (A = g, B = x, two positions per MFMA), one 32 x 32 tile per wave, carried in registers over the walk.  Partials
//                  [P][Cout][K] and, from the k-block-0 workgroups, bias partials [P][4][Cout] go to the caller's workspace.
//                  P = max(1, min(ceil(M / 256), 64, 2^25 / (Cout K))): sized by M = B OH OW (one partial for the linear layer at
//                  M = 64), and capped so that the partials never pass 128 MiB.
//   k_conv_reduce  one lane per dweight / dbias element adds its P (4 P) partials ascending: no atomics, the same bits on every run.
//   k_conv_lin_fwd, k_conv_lin_dx   the linear layer (H = KH and W = KW: x[b] is the window itself and every dx term exists): the same two
//                  chains with no LDS and no barrier - one wave per 32 x 32 tile, the operands read from global memory as each lane needs
//                  them, a batch of sixteen MFMAs' operands in flight while the batch before runs (forward: 16-byte vectors along k, taken
//                  when K % 32 == 0 and the bases are 16-byte aligned; dx: D[b][k], chain over co).  Which kernel runs changes no bit: the chain per element is the same.
//   k_conv_dx      input positions flattened over the batch, n = (b H + iy) W + ix, 32-position tiles x 32-channel tiles of Cin, A = w read
//                  transposed ([j][c]), B = g gathered as [j][position] (an absent term is 0), chunks of 32 j; a ballot at staging time
//                  records per (j, tile) whether any term exists and the MFMA of a pair (j, j + 1) without one is skipped.
// Worst-case workspace at NatureCNN's shapes (128 x 128 observation, features_dim 512), bytes = 4 P (Cout K + 4 Cout):
//     B = 64:    conv2 P = 49: 6 472 704    conv3 P = 36: 5 345 280    linear P = 1: 18 882 560
//     B = 1024:  conv2 P = 64: 8 454 144    conv3 P = 64: 9 502 720    linear P = 4: 75 530 240
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error

namespace tg {

constexpr int kConvThreads = 256;
constexpr int kConvChunk = 32;                       // k (forward) or j (dx) staged at a time: 16 MFMAs
constexpr int kConvPitch = 129;                      // LDS rows of up to 128 floats, padded: the transposing writes spread over the banks
constexpr int kConvBwdPos = 64;                      // positions of a backward chunk: 32 MFMAs
constexpr int kConvBwdPitch = 65;
constexpr int kConvBwdShare = 256;                   // positions per workgroup that size P
constexpr int kConvBwdMaxParts = 64;
constexpr int64_t kConvBwdMaxFloats = 1ll << 25;     // P Cout K stays at or below this: 128 MiB of weight partials
constexpr int kConvBiasParts = 4;
constexpr int64_t kConvMaxPos = TG_CONV_MAX_POSITIONS;   // 2^29 - 32, for B OH OW and B H W: 32-position tiles x 256 lanes stay below 2^32 in one launch

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    const float* x;           // [B][Cin][H][W]
    const float* w;           // [Cout][K]
    const float* bias;        // [Cout]
    float* y;                 // forward: out [B][Cout][OH][OW]
    const float* yin;         // backward: the forward's output
    const float* dy;
    float* dx;                // [B][Cin][H][W]
    float* ws;                // backward partials [P][Cout][K]
    float* wsb;               // [P][4][Cout]
    int64_t B, M, N;          // M = B OH OW, N = B H W
    int32_t Cin, H, W, Cout, KH, KW, stride, OH, OW, K, J, P;
};

__device__ __forceinline__ float conv_relu(float z) { return z > 0.0f ? z : (z != z ? z : 0.0f); }   // torch.relu: a NaN stays a NaN

// offset of element k = (c KH + ky) KW + kx inside an image's window: (c H + ky) W + kx
__device__ __forceinline__ int64_t conv_koff(const ConvArgs& a, int32_t k) {
    const int32_t khw = a.KH * a.KW, c = k / khw, r = k - c * khw, ky = r / a.KW, kx = r - ky * a.KW;
    return ((int64_t)c * a.H + ky) * a.W + kx;
}

// offset of the window of output position m = (b OH + oy) OW + ox in x
__device__ __forceinline__ int64_t conv_pbase(const ConvArgs& a, int64_t m) {
    const int32_t ohw = a.OH * a.OW;
    const int64_t b = m / ohw;
    const int32_t p = (int32_t)(m - b * ohw), oy = p / a.OW, ox = p - oy * a.OW;
    return ((b * a.Cin * a.H) + (int64_t)oy * a.stride) * a.W + (int64_t)ox * a.stride;
}

__global__ __launch_bounds__(kConvThreads) void k_conv_fwd(ConvArgs a, int32_t cl) {
    __shared__ float wl[kConvChunk * kConvPitch];
    __shared__ float xs[kConvChunk * kConvPitch];
    __shared__ int64_t koff[2][kConvChunk];
    __shared__ int64_t pbase[128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t CTW = 1 << cl, MP = (4 >> cl) * 32, CW = CTW * 32;
    const int32_t ctl = wave & (CTW - 1), pt = wave >> cl;
    const int64_t m0 = (int64_t)blockIdx.x * MP;
    const int32_t co0 = blockIdx.y * CW;
    const int32_t K = a.K;
    const bool active = m0 + pt * 32 < a.M && co0 + ctl * 32 < a.Cout;        // the same for the whole wave
    if (tid < MP) pbase[tid] = conv_pbase(a, m0 + tid < a.M ? m0 + tid : 0);
    if (tid < kConvChunk && tid < K) koff[0][tid] = conv_koff(a, tid);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    const int32_t wcol = ctl * 32 + j, xcol = pt * 32 + j;
    for (int32_t k0 = 0, cur = 0; k0 < K; k0 += kConvChunk, cur ^= 1) {
        const int32_t kn = K - k0 < kConvChunk ? K - k0 : kConvChunk;          // even, as K is
        __syncthreads();
        for (int32_t idx = tid; idx < kConvChunk * CW; idx += kConvThreads) {
            const int32_t kk = idx & 31, col = idx >> 5, co = co0 + col;
            if (kk < kn) wl[kk * kConvPitch + col] = co < a.Cout ? a.w[(int64_t)co * K + k0 + kk] : 0.0f;
        }
        for (int32_t idx = tid; idx < kConvChunk * MP; idx += kConvThreads) {
            const int32_t kk = idx & 31, mm = idx >> 5;
            if (kk < kn) xs[kk * kConvPitch + mm] = a.x[pbase[mm] + koff[cur][kk]];
        }
        if (tid < kConvChunk && k0 + kConvChunk + tid < K) koff[cur ^ 1][tid] = conv_koff(a, k0 + kConvChunk + tid);
        __syncthreads();
        if (active) {
            if (kn == kConvChunk) {
#pragma unroll
                for (int s = 0; s < kConvChunk / 2; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + h) * kConvPitch + wcol], xs[(2 * s + h) * kConvPitch + xcol], acc, 0, 0, 0);
            } else {
                for (int s = 0; s < kn / 2; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + h) * kConvPitch + wcol], xs[(2 * s + h) * kConvPitch + xcol], acc, 0, 0, 0);
            }
        }
    }
    const int64_t m = m0 + pt * 32 + j;
    if (active && m < a.M) {
        const int64_t ohw = (int64_t)a.OH * a.OW, b = m / ohw, p = m - b * ohw;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int32_t co = co0 + ctl * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            a.y[(b * a.Cout + co) * ohw + p] = conv_relu(acc[i] + a.bias[co]);
        }
    }
}

__global__ __launch_bounds__(kConvThreads) void k_conv_bwd(ConvArgs a, int32_t n_kblocks) {
    __shared__ float gs[kConvBwdPos * kConvBwdPitch];
    __shared__ float xs[kConvBwdPos * kConvBwdPitch];
    __shared__ int64_t pb[2][kConvBwdPos];                                    // the position's window in x; -1 past the last position
    __shared__ int64_t gb[2][kConvBwdPos];                                    // its channel-0 element in y and dy
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t kblock = blockIdx.x % n_kblocks, cblock = blockIdx.x / n_kblocks, p = blockIdx.y, P = a.P;
    const int32_t co0 = cblock * 64, kb0 = kblock * 64, K = a.K;
    const int32_t ctl = wave & 1, ktl = wave >> 1;
    const int64_t ohw = (int64_t)a.OH * a.OW;
    const int64_t n_chunks = (a.M + kConvBwdPos - 1) / kConvBwdPos;
    const bool active = co0 + ctl * 32 < a.Cout && kb0 + ktl * 32 < K;
    const int32_t sk = kb0 + lane;                                            // the k this lane stages
    const bool sk_ok = sk < K;
    const int64_t sk_off = sk_ok ? conv_koff(a, sk) : 0;
    const int32_t srow = tid >> 6;                                            // staging: rows srow, srow + 4, ...
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    float bsum = 0.0f;
    auto positions = [&](int64_t chunk, int32_t buf) {
        const int64_t m = chunk * kConvBwdPos + tid;
        if (m < a.M) {
            const int64_t b = m / ohw;
            pb[buf][tid] = conv_pbase(a, m);
            gb[buf][tid] = b * a.Cout * ohw + (m - b * ohw);
        } else {
            pb[buf][tid] = -1;
            gb[buf][tid] = -1;
        }
    };
    if (tid < kConvBwdPos) positions(p, 0);
    int32_t cur = 0;
    for (int64_t chunk = p; chunk < n_chunks; chunk += P, cur ^= 1) {
        __syncthreads();
        {                                                                      // g: lanes along the positions, 64 channels
            const int64_t base = gb[cur][lane];
#pragma unroll 4
            for (int32_t col = srow; col < 64; col += 4) {
                const int32_t co = co0 + col;
                float v = 0.0f;
                if (base >= 0 && co < a.Cout) {
                    const int64_t gi = base + co * ohw;
                    v = a.yin[gi] > 0.0f ? a.dy[gi] : 0.0f;
                }
                gs[lane * kConvBwdPitch + col] = v;
            }
        }
#pragma unroll 4
        for (int32_t mm = srow; mm < kConvBwdPos; mm += 4) {                   // x: lanes along k, 64 positions
            const int64_t base = pb[cur][mm];
            xs[mm * kConvBwdPitch + lane] = base >= 0 && sk_ok ? a.x[base + sk_off] : 0.0f;
        }
        if (tid < kConvBwdPos && chunk + P < n_chunks) positions(chunk + P, cur ^ 1);
        __syncthreads();
        if (active) {
#pragma unroll 8
            for (int s = 0; s < kConvBwdPos / 2; ++s)                          // positions 2 s + h of the chunk: past the last g = 0 and x = 0
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[(2 * s + h) * kConvBwdPitch + ctl * 32 + j],
                                                           xs[(2 * s + h) * kConvBwdPitch + ktl * 32 + j], acc, 0, 0, 0);
        }
        if (kblock == 0) {
            for (int i = 0; i < kConvBwdPos / kConvBiasParts; ++i) bsum = bsum + gs[(srow * (kConvBwdPos / kConvBiasParts) + i) * kConvBwdPitch + lane];
        }
    }
    if (active) {
        const int32_t k = kb0 + ktl * 32 + j;
        if (k < K) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int32_t co = co0 + ctl * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                a.ws[((int64_t)p * a.Cout + co) * K + k] = acc[i];
            }
        }
    }
    if (kblock == 0 && co0 + lane < a.Cout) a.wsb[((int64_t)p * kConvBiasParts + srow) * a.Cout + co0 + lane] = bsum;
}

__global__ __launch_bounds__(kConvThreads) void k_conv_reduce(const float* ws, const float* wsb, int32_t P, int64_t nw, int32_t Cout, float* dweight,
                                                               float* dbias) {
    const int64_t t = (int64_t)blockIdx.x * kConvThreads + threadIdx.x;
    if (t >= nw + Cout) return;
    const bool is_w = t < nw;
    const float* src = is_w ? ws + t : wsb + (t - nw);
    const int64_t step = is_w ? nw : Cout;
    const int32_t n = is_w ? P : kConvBiasParts * P;
    float s = 0.0f;
    for (int32_t q = 0; q < n; ++q) s = s + src[q * step];
    if (is_w) dweight[t] = s;
    else dbias[t - nw] = s;
}

__global__ __launch_bounds__(kConvThreads) void k_conv_dx(ConvArgs a, int32_t cl) {
    __shared__ float wl[kConvChunk * kConvBwdPitch];                          // [j][c], 64 channels
    __shared__ float gs[kConvChunk * kConvPitch];                             // [j][position]
    __shared__ int32_t jt[2][kConvChunk];                                     // co | ky / stride << 10 | ky % stride << 14 | kx / stride << 16 | kx % stride << 20
    __shared__ int32_t jw[2][kConvChunk];                                     // (co Cin KH + ky) KW + kx: w's element of channel 0
    __shared__ int32_t any[kConvChunk][4];                                    // whether a term of (j, position tile) exists
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t CT = 1 << cl, NP = (4 >> cl) * 32;
    const int32_t ctl = wave & (CT - 1), pt = wave >> cl;
    const int64_t n0 = (int64_t)blockIdx.x * NP;
    const int32_t khw = a.KH * a.KW, J = a.J;
    const int64_t ohw = (int64_t)a.OH * a.OW, hw = (int64_t)a.H * a.W;
    const bool active = n0 + pt * 32 < a.N && ctl * 32 < a.Cin;
    // the position this thread stages, for every j
    const int32_t sn = tid & (NP - 1), sj0 = tid / NP, sjstep = kConvThreads / NP;
    const bool sn_ok = n0 + sn < a.N;
    const int64_t snn = sn_ok ? n0 + sn : 0, sb = snn / hw;
    const int32_t sq = (int32_t)(snn - sb * hw), siy = sq / a.W, six = sq - siy * a.W;
    const int32_t qy = siy / a.stride, ry = siy - qy * a.stride, qx = six / a.stride, rx = six - qx * a.stride;
    const int64_t sgb = sb * a.Cout * ohw;
    auto tables = [&](int32_t jj, int32_t buf) {
        const int32_t co = jj / khw, r = jj - co * khw, ky = r / a.KW, kx = r - ky * a.KW;
        jt[buf][tid] = co | (ky / a.stride) << 10 | (ky % a.stride) << 14 | (kx / a.stride) << 16 | (kx % a.stride) << 20;
        jw[buf][tid] = co * a.Cin * khw + r;
    };
    if (tid < kConvChunk) tables(tid, 0);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int32_t j0 = 0, cur = 0; j0 < J; j0 += kConvChunk, cur ^= 1) {      // J = Cout KH KW is a multiple of 32, as Cout is
        __syncthreads();
        for (int32_t idx = tid; idx < kConvChunk * 64; idx += kConvThreads) {
            const int32_t jj = idx & 31, c = idx >> 5;
            wl[jj * kConvBwdPitch + c] = c < a.Cin ? a.w[jw[cur][jj] + c * khw] : 0.0f;
        }
        for (int32_t jj = sj0; jj < kConvChunk; jj += sjstep) {
            const int32_t e = jt[cur][jj];
            const int32_t co = e & 1023, oy = qy - ((e >> 10) & 15), ox = qx - ((e >> 16) & 15);
            const bool ok = sn_ok && ry == ((e >> 14) & 3) && rx == ((e >> 20) & 3) && oy >= 0 && oy < a.OH && ox >= 0 && ox < a.OW;
            float v = 0.0f;
            if (ok) {
                const int64_t gi = sgb + ((int64_t)co * a.OH + oy) * a.OW + ox;
                v = a.yin[gi] > 0.0f ? a.dy[gi] : 0.0f;
            }
            gs[jj * kConvPitch + sn] = v;
            const unsigned long long mask = __ballot(ok);
            if (lane == 0) {                                                   // a wave stages two neighbouring tiles of one j
                any[jj][sn >> 5] = (uint32_t)mask != 0u;
                any[jj][(sn >> 5) + 1] = (uint32_t)(mask >> 32) != 0u;
            }
        }
        if (tid < kConvChunk && j0 + kConvChunk < J) tables(j0 + kConvChunk + tid, cur ^ 1);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int s = 0; s < kConvChunk / 2; ++s) {
                if (any[2 * s][pt] | any[2 * s + 1][pt])                       // the same for the whole wave
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wl[(2 * s + h) * kConvBwdPitch + ctl * 32 + j], gs[(2 * s + h) * kConvPitch + pt * 32 + j],
                                                               acc, 0, 0, 0);
            }
        }
    }
    const int64_t n = n0 + pt * 32 + j;
    if (active && n < a.N) {
        const int64_t b = n / hw, q = n - b * hw;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int32_t c = ctl * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (c < a.Cin) a.dx[(b * a.Cin + c) * hw + q] = acc[i];
        }
    }
}

// The linear layer (H = KH, W = KW: one output position an image, x[b] IS the window, every dx term exists) without LDS and without
// barriers: each wave owns one 32 x 32 tile and reads its operands straight from global memory.  The same chains.
__global__ __launch_bounds__(kConvThreads) void k_conv_lin_fwd(ConvArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t ct = blockIdx.y * 4 + wave, K = a.K;
    if (ct * 32 >= a.Cout) return;
    const int64_t b = (int64_t)blockIdx.x * 32 + j;
    const float4* wp = (const float4*)(a.w + (int64_t)(ct * 32 + j) * K);      // K % 32 == 0 and 16-byte aligned bases: the launcher's condition
    const float4* xp = (const float4*)(a.x + (b < a.B ? b : 0) * K);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    constexpr int kV = 8;                                                      // 16-byte vectors a side and batch: 16 MFMAs
    float wa[kV], wb[kV], wc[kV], wd[kV], xa[kV], xb[kV], xc[kV], xd[kV];
#pragma unroll
    for (int u = 0; u < kV; ++u) {
        const float4 wv = wp[u], xv = xp[u];
        wa[u] = wv.x, wb[u] = wv.y, wc[u] = wv.z, wd[u] = wv.w;
        xa[u] = xv.x, xb[u] = xv.y, xc[u] = xv.z, xd[u] = xv.w;
    }
    for (int32_t t = 0; t < K / 4; t += kV) {
        float w0[kV], w1[kV], x0[kV], x1[kV];                                  // k = 4 t + h, then 4 t + 2 + h: the lower half-wave the lower k
#pragma unroll
        for (int u = 0; u < kV; ++u) {
            w0[u] = h ? wb[u] : wa[u];
            w1[u] = h ? wd[u] : wc[u];
            x0[u] = h ? xb[u] : xa[u];
            x1[u] = h ? xd[u] : xc[u];
        }
        const int32_t tn = t + kV < K / 4 ? t + kV : t;                        // the next batch's loads are issued before this batch's MFMAs
#pragma unroll                                                                 // (in the last batch: a reload that nobody uses)
        for (int u = 0; u < kV; ++u) {
            const float4 wv = wp[tn + u], xv = xp[tn + u];
            wa[u] = wv.x, wb[u] = wv.y, wc[u] = wv.z, wd[u] = wv.w;
            xa[u] = xv.x, xb[u] = xv.y, xc[u] = xv.z, xd[u] = xv.w;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kV; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[u], x0[u], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[u], x1[u], acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (b < a.B) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int32_t co = ct * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            a.y[b * a.Cout + co] = conv_relu(acc[i] + a.bias[co]);
        }
    }
}

// dx[b][k] = chain over co ascending of g[b][co] w[co][k]: D[b][k], A = g, B = w, the stores of one register 32 consecutive k of one image.
__global__ __launch_bounds__(kConvThreads) void k_conv_lin_dx(ConvArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t kt = blockIdx.y * 4 + wave, K = a.K;
    if (kt * 32 >= K) return;
    const int64_t b0 = (int64_t)blockIdx.x * 32, b = b0 + j;
    const int32_t k = kt * 32 + j;
    const bool b_ok = b < a.B, k_ok = k < K;
    const float* yp = a.yin + (b_ok ? b : 0) * a.Cout + h;
    const float* gp = a.dy + (b_ok ? b : 0) * a.Cout + h;
    const float* wp = a.w + (int64_t)h * K + (k_ok ? k : 0);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    constexpr int kV = 16;                                                     // co = 2 s + h; Cout / 2 is a multiple of 16
    float yn[kV], gn[kV], wn[kV];
#pragma unroll
    for (int u = 0; u < kV; ++u) {
        yn[u] = yp[2 * u];
        gn[u] = gp[2 * u];
        wn[u] = wp[(int64_t)2 * u * K];
    }
    for (int32_t s0 = 0; s0 < a.Cout / 2; s0 += kV) {
        float ga[kV], wb[kV];
#pragma unroll
        for (int u = 0; u < kV; ++u) {
            ga[u] = b_ok && yn[u] > 0.0f ? gn[u] : 0.0f;
            wb[u] = k_ok ? wn[u] : 0.0f;
        }
        const int32_t sn = s0 + kV < a.Cout / 2 ? s0 + kV : s0;                // the next batch's loads are issued before this batch's MFMAs
#pragma unroll                                                                 // (in the last batch: a reload that nobody uses)
        for (int u = 0; u < kV; ++u) {
            yn[u] = yp[2 * (sn + u)];
            gn[u] = gp[2 * (sn + u)];
            wn[u] = wp[(int64_t)2 * (sn + u) * K];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kV; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[u], wb[u], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (k_ok) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t bi = b0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (bi < a.B) a.dx[bi * K + k] = acc[i];
        }
    }
}

static bool conv_is_linear(const ConvArgs& a) { return a.H == a.KH && a.W == a.KW; }

static int32_t conv_parts(int64_t M, int32_t Cout, int32_t K) {
    int64_t P = (M + kConvBwdShare - 1) / kConvBwdShare;
    if (P > kConvBwdMaxParts) P = kConvBwdMaxParts;
    const int64_t cap = kConvBwdMaxFloats / ((int64_t)Cout * K);
    if (P > cap) P = cap;
    return (int32_t)(P < 1 ? 1 : P);
}

static int64_t conv_workspace(int64_t M, int32_t Cout, int32_t K) {
    return (int64_t)conv_parts(M, Cout, K) * ((int64_t)Cout * K + kConvBiasParts * Cout) * (int64_t)sizeof(float);
}

// The checks the three calls share; 0 or the error's code.  Fills the sizes of `a`.
static int conv_check(const char* who, ConvArgs& a, int64_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t KH, int32_t KW,
                      int32_t stride) {
    static thread_local char msg[200];
    const char* what = nullptr;
    if (Cin < 1 || Cin > TG_CONV_MAX_CIN) what = "need 1 <= Cin <= TG_CONV_MAX_CIN (64)";
    else if (Cout < TG_CONV_COUT_STEP || Cout > TG_CONV_MAX_COUT || Cout % TG_CONV_COUT_STEP)
        what = "need Cout a multiple of TG_CONV_COUT_STEP (32), at most TG_CONV_MAX_COUT (512)";
    else if (KH < 1 || KW < 1 || KH > TG_CONV_MAX_KERNEL || KW > TG_CONV_MAX_KERNEL) what = "need 1 <= KH, KW <= TG_CONV_MAX_KERNEL (16)";
    else if (KH > H || KW > W) what = "need KH <= H and KW <= W";
    else if (stride < 1 || stride > TG_CONV_MAX_STRIDE) what = "need 1 <= stride <= TG_CONV_MAX_STRIDE (4)";
    else if ((Cin * KH * KW) % 2) what = "need K = Cin KH KW even";
    else if (B < 0) what = "need B >= 0";
    else {
        a.B = B;
        a.Cin = Cin;
        a.H = H;
        a.W = W;
        a.Cout = Cout;
        a.KH = KH;
        a.KW = KW;
        a.stride = stride;
        a.OH = (H - KH) / stride + 1;
        a.OW = (W - KW) / stride + 1;
        a.K = Cin * KH * KW;
        a.J = Cout * KH * KW;
        if (B > kConvMaxPos / ((int64_t)H * W)) what = "too many positions (B H W) for one launch";
        else {
            a.M = B * a.OH * a.OW;
            a.N = B * H * W;
            a.P = conv_parts(a.M, Cout, a.K);
        }
    }
    if (!what) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return report_error(-1, msg);
}

}  // namespace tg

extern "C" int tg_conv_relu(const float* x_dev, int64_t B, int32_t Cin, int32_t H, int32_t W, const float* weight_dev, const float* bias_dev,
                            int32_t Cout, int32_t KH, int32_t KW, int32_t stride, float* y_dev, void* hip_stream) {
    using namespace tg;
    if (!x_dev || !weight_dev || !bias_dev || !y_dev) return report_error(-1, "tg_conv_relu: NULL x_dev, weight_dev, bias_dev or y_dev");
    ConvArgs a = {};
    if (int rc = conv_check("tg_conv_relu", a, B, Cin, H, W, Cout, KH, KW, stride)) return rc;
    if (B == 0) return 0;
    a.x = x_dev;
    a.w = weight_dev;
    a.bias = bias_dev;
    a.y = y_dev;
    const dim3 block(kConvThreads);
    if (conv_is_linear(a) && a.K % 32 == 0 && ((uintptr_t)x_dev | (uintptr_t)weight_dev) % 16 == 0) {
        hipLaunchKernelGGL(k_conv_lin_fwd, dim3((unsigned)((B + 31) / 32), (unsigned)((Cout + 127) / 128)), block, 0, (hipStream_t)hip_stream, a);
    } else {
        const int32_t cl = Cout >= 128 ? 2 : (Cout >= 64 ? 1 : 0), MP = (4 >> cl) * 32, CW = 32 << cl;
        const dim3 grid((unsigned)((a.M + MP - 1) / MP), (unsigned)((Cout + CW - 1) / CW));
        hipLaunchKernelGGL(k_conv_fwd, grid, block, 0, (hipStream_t)hip_stream, a, cl);
    }
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_relu: the kernel launch failed");
    return 0;
}

extern "C" int64_t tg_conv_relu_bwd_workspace(int64_t B, int32_t Cin, int32_t H, int32_t W, int32_t Cout, int32_t KH, int32_t KW, int32_t stride) {
    using namespace tg;
    ConvArgs a = {};
    if (int rc = conv_check("tg_conv_relu_bwd_workspace", a, B, Cin, H, W, Cout, KH, KW, stride)) return rc;
    return conv_workspace(a.M, Cout, a.K);
}

extern "C" int tg_conv_relu_bwd(const float* x_dev, int64_t B, int32_t Cin, int32_t H, int32_t W, const float* weight_dev, const float* y_dev,
                                const float* dy_dev, int32_t Cout, int32_t KH, int32_t KW, int32_t stride, float* dweight_dev, float* dbias_dev,
                                float* dx_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream) {
    using namespace tg;
    if (!x_dev || !weight_dev || !y_dev || !dy_dev || !dweight_dev || !dbias_dev)
        return report_error(-1, "tg_conv_relu_bwd: NULL x_dev, weight_dev, y_dev, dy_dev, dweight_dev or dbias_dev");
    ConvArgs a = {};
    if (int rc = conv_check("tg_conv_relu_bwd", a, B, Cin, H, W, Cout, KH, KW, stride)) return rc;
    if (B == 0) return 0;
    if (!workspace_dev) return report_error(-1, "tg_conv_relu_bwd: NULL workspace_dev");
    if (workspace_bytes < conv_workspace(a.M, Cout, a.K))
        return report_error(-1, "tg_conv_relu_bwd: the workspace is smaller than tg_conv_relu_bwd_workspace's size");
    a.x = x_dev;
    a.w = weight_dev;
    a.yin = y_dev;
    a.dy = dy_dev;
    a.dx = dx_dev;
    a.ws = (float*)workspace_dev;
    a.wsb = a.ws + (int64_t)a.P * Cout * a.K;
    hipStream_t s = (hipStream_t)hip_stream;
    const dim3 block(kConvThreads);
    const int32_t n_kblocks = (a.K + 63) / 64, n_cblocks = (Cout + 63) / 64;
    hipLaunchKernelGGL(k_conv_bwd, dim3((unsigned)(n_kblocks * n_cblocks), (unsigned)a.P), block, 0, s, a, n_kblocks);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_relu_bwd: the kernel launch failed");
    const int64_t nw = (int64_t)Cout * a.K;
    hipLaunchKernelGGL(k_conv_reduce, dim3((unsigned)((nw + Cout + kConvThreads - 1) / kConvThreads)), block, 0, s, a.ws, a.wsb, a.P, nw, Cout,
                       dweight_dev, dbias_dev);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_relu_bwd: the reduction's launch failed");
    if (dx_dev) {
        if (conv_is_linear(a)) {
            hipLaunchKernelGGL(k_conv_lin_dx, dim3((unsigned)((B + 31) / 32), (unsigned)((a.K + 127) / 128)), block, 0, s, a);
        } else {
            const int32_t cl = Cin > 32 ? 1 : 0, NP = (4 >> cl) * 32;
            hipLaunchKernelGGL(k_conv_dx, dim3((unsigned)((a.N + NP - 1) / NP)), block, 0, s, a, cl);
        }
        if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_conv_relu_bwd: the input gradient's launch failed");
    }
    return 0;
}
