// tg_mlp.hip - the device MLP towers (tactile_gym_amd.mlp): stable_baselines3's MlpExtractor with action_net and value_net, SAC's
// actor (latent_pi, mu, log_std) and its ContinuousCritic (qf0, qf1, ...) as ONE forward launch and at most TWO backward launches for every tower
// of a call.  Compiled with -ffp-contract=off; the only fused multiply-adds are the MFMA's.
//
// Specification per output element (W torch's [out][in]):
//     acc = 0;  for k = 0 .. in-1 ascending: acc = fmaf(h_{l-1}[row][k], W[co][k], acc);  z = acc + b[co];  h = act(z)
// (ReLU: z > 0 ? z : (z != z ? z : 0) - a NaN stays a NaN, as in torch.relu.)
// v_mfma_f32_32x32x2_f32 is bit for bit that chain (two k per instruction, the lower first), so an output has ONE arithmetic order,
// whatever the batch it sits in, wherever its tile falls and whatever other towers run beside it.  The k tail (in odd, or no multiple of the
// 32-wide staging chunk) is finished with the operand pair (-0.0, +0.0): the product is -0.0 and acc + (-0.0) has acc's bits for EVERY acc, where
// (0, 0) would turn an accumulator of -0.0 into +0.0 (tests/mlp_ref.py shows both).
//
//   k_mlp_fwd     grid (row tiles of 32, T), 512 lanes: wave w owns output columns 32 w .. 32 w + 31 of every layer, D[row][co] with co on the lane
//                 (C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so a register's stores are 32 consecutive floats
//                 of one row.  Chunk by chunk of 32 k the workgroup stages W[co][k] (and, for the first layer, the input's columns) in LDS, eight
//                 loads a lane issued together at addresses clamped into the arrays; lane l
//                 feeds A = h[row = l & 31][k = 2 s + (l >> 5)] and B = W[co = l & 31][k] to 16 MFMAs per chunk on ONE accumulator tile.  The
//                 activated tile goes to LDS ([row][256], column ^ row: conflict free for the row-strided A reads) for the next layer, and to
//                 global memory where the caller asked.
//   k_mlp_bwd     grid (G <= 64, T): workgroup g of tower t walks row tiles g, g + G, ... in ascending order.  Per tile and layer, last first:
//                 g = dh act'(h) in LDS; dbias and dweight[co][k] += sum over the tile's rows of g[row][co] h_{l-1}[row][k] (A = g, B = h_{l-1}
//                 straight from global memory, k on the lane; the accumulator tile starts from the workgroup's own partial of the previous
//                 tile, so a workgroup's sum is ONE chain over its rows); dh_{l-1}[row][k] = chain over co of g[row][co] W[co][k] (A = g,
//                 B = W straight from global memory, k on the lane).  With G = 1 the sums go to the caller's buffers, else to the workgroup's
//                 slab of the workspace.  dh_0 goes to dx (T = 1) or to the tower's slab.
//   k_mlp_reduce  one lane per output element adds the G slabs (the T towers' dh_0) in ascending order: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tactile_gym_hip.h"
#include "tg_exchange.h"   // report_error

namespace tg {

constexpr int kMlpThreads = 512;
constexpr int kMlpWaves = kMlpThreads / 64;
constexpr int kMlpRows = 32;                         // rows of a tile
constexpr int kMlpChunk = 32;                        // k of a staging chunk
constexpr int kMlpPitch = TG_MLP_MAX_WIDTH;          // LDS rows of the activations; element (r, c) at r * 256 + (c ^ r)
constexpr int kMlpGroups = 64;                       // G: backward workgroups (partial sums) per tower
constexpr int kMlpSegs = 2 * TG_MLP_MAX_TOWERS * TG_MLP_MAX_LAYERS;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MlpArgs {
    tg_mlp_tower tw[TG_MLP_MAX_TOWERS];
    int64_t slab_off[TG_MLP_MAX_TOWERS][TG_MLP_MAX_LAYERS];   // floats into a slab: the layer's dweight [out + out2][in], then dbias [out + out2]
    const float* x0;
    const float* x1;
    float* dx0;
    float* dx1;
    float* ws;                // backward: G slabs (G > 1)
    float* dxs;               // backward: T slabs [B][K0] (T > 1)
    int64_t B, slab_floats, n_tiles;
    int32_t Ka, Kb, save_all, want_dx;
};

__device__ __forceinline__ int mlp_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// torch.relu: fmaxf's bits for every number (-0.0 -> +0.0 included), and a NaN stays a NaN where fmaxf would return 0
__device__ __forceinline__ float mlp_relu(float z) { return z > 0.0f ? z : (z != z ? z : 0.0f); }

__device__ __forceinline__ const float* mlp_input_at(const MlpArgs& a, int64_t row, int32_t k) {
    return k < a.Ka ? a.x0 + row * a.Ka + k : a.x1 + row * a.Kb + (k - a.Ka);
}

__global__ __launch_bounds__(kMlpThreads) void k_mlp_fwd(MlpArgs a) {
    __shared__ float hs[kMlpRows * kMlpPitch];
    __shared__ float wl[TG_MLP_MAX_WIDTH * kMlpChunk];                    // element (co, k) at co * 32 + (k ^ (co & 31))
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const tg_mlp_tower& tw = a.tw[blockIdx.y];
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;
    const int32_t K0 = a.Ka + a.Kb, co0 = wave * 32;
    for (int32_t l = 0; l < tw.n_layers; ++l) {
        const tg_mlp_layer& ly = tw.layer[l];
        const int32_t in = ly.in, out = ly.out, outT = ly.out + ly.out2;
        const int32_t staged = ((outT + 31) >> 5) << 5;                   // rows of W in a chunk, zeros past outT
        const bool active = co0 < outT;                                   // the same for the whole wave
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int32_t k0 = 0; k0 < in; k0 += kMlpChunk) {
            __syncthreads();                                              // the previous chunk is read, the previous layer's tile is written
            {   // every load is issued before the first is used: the addresses are clamped into the arrays, what lies outside is replaced
                const int32_t k = tid & 31, kc = k0 + k < in ? k0 + k : in - 1;
                float xv[2];
                if (l == 0) {                                             // the input's columns k0 .. k0 + 31, as a [32][32] image at the head of hs
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int64_t row = row0 + (tid >> 5) + 16 * i;
                        xv[i] = *mlp_input_at(a, row < a.B ? row : a.B - 1, kc);
                    }
                }
                for (int32_t c0 = 0; c0 < staged; c0 += 128) {            // 128 rows of W at a time: eight loads a lane, then their LDS writes
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int32_t co = c0 + (tid >> 5) + 16 * i, cc = co < outT ? co : outT - 1;
                        v[i] = (cc < out ? ly.weight + (int64_t)cc * in : ly.weight2 + (int64_t)(cc - out) * in)[kc];
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int32_t co = c0 + (tid >> 5) + 16 * i;
                        if (co < staged) wl[co * kMlpChunk + (k ^ (co & 31))] = (co < outT && k0 + k < in) ? v[i] : 0.0f;
                    }
                }
                if (l == 0) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int32_t r = (tid >> 5) + 16 * i;
                        hs[r * kMlpChunk + (k ^ r)] = (row0 + r < a.B && k0 + k < K0) ? xv[i] : -0.0f;
                    }
                }
            }
            __syncthreads();
            if (active) {
                const float* ap = l == 0 ? hs + j * kMlpChunk : hs + j * kMlpPitch + k0;   // k0 is a multiple of 32: (k0 + kk) ^ j = k0 + (kk ^ j)
                const float* bp = wl + (co0 + j) * kMlpChunk;
#pragma unroll
                for (int s = 0; s < kMlpChunk / 2; ++s) {
                    const int kk = (2 * s + h) ^ j;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc, 0, 0, 0);
                }
            }
        }
        __syncthreads();                                                  // every wave has read the layer's input
        if (active) {
            const int32_t co = co0 + j;
            const bool store = (l == tw.n_layers - 1 || a.save_all) && co < outT;
            float bias = 0.0f;
            if (co < outT) bias = co < out ? ly.bias[co] : ly.bias2[co - out];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int32_t r = mlp_row(i, h);
                float v = -0.0f;                                          // past the layer's width: the next layer's k tail
                if (co < outT) {
                    const float z = acc[i] + bias;
                    v = ly.act == TG_MLP_ACT_RELU ? mlp_relu(z) : ly.act == TG_MLP_ACT_TANH ? (float)tanh((double)z) : z;
                }
                hs[r * kMlpPitch + (co ^ r)] = v;
                const int64_t row = row0 + r;
                if (store && row < a.B) {
                    if (co < out) ly.h[row * out + co] = v;
                    else ly.h2[row * ly.out2 + (co - out)] = v;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kMlpThreads) void k_mlp_bwd(MlpArgs a) {
    __shared__ float gs[kMlpRows * kMlpPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, j = lane & 31;
    const int32_t t = blockIdx.y, grp = blockIdx.x, G = gridDim.x, T = gridDim.y;
    const tg_mlp_tower& tw = a.tw[t];
    const int32_t L = tw.n_layers, K0 = a.Ka + a.Kb;
    float* slab = G > 1 ? a.ws + (int64_t)grp * a.slab_floats : nullptr;
    bool first = true;
    for (int64_t tile = grp; tile < a.n_tiles; tile += G, first = false) {
        const int64_t row0 = tile * kMlpRows;
        {
            const tg_mlp_layer& ly = tw.layer[L - 1];
            const int32_t out = ly.out, outT = ly.out + ly.out2;
            __syncthreads();                                              // the previous tile is read
            for (int32_t idx = tid; idx < kMlpRows * kMlpPitch; idx += kMlpThreads) {
                const int32_t r = idx >> 8, co = idx & 255;
                const int64_t row = row0 + r;
                float v = 0.0f;
                if (row < a.B && co < outT) {
                    if (co < out) v = tw.dy ? tw.dy[row * out + co] : 0.0f;
                    else v = tw.dy2 ? tw.dy2[row * ly.out2 + (co - out)] : 0.0f;
                }
                gs[r * kMlpPitch + (co ^ r)] = v;
            }
        }
        for (int32_t l = L - 1; l >= 0; --l) {
            const tg_mlp_layer& ly = tw.layer[l];
            const int32_t in = ly.in, out = ly.out, outT = ly.out + ly.out2;
            const float* hprev = l ? tw.layer[l - 1].h : nullptr;
            float* sw = slab ? slab + a.slab_off[t][l] : nullptr;
            float* sb = slab ? sw + (int64_t)outT * in : nullptr;
            // g = dh act'(h), in place: each lane rewrites the elements it reads.  Past the batch and past the layer's width: -0.0
            for (int32_t idx = tid; idx < kMlpRows * kMlpPitch; idx += kMlpThreads) {
                const int32_t r = idx >> 8, co = idx & 255;
                const int64_t row = row0 + r;
                const int32_t at = r * kMlpPitch + (co ^ r);
                float g = -0.0f;
                if (row < a.B && co < outT) {
                    const float dh = gs[at];
                    const float hv = co < out ? ly.h[row * out + co] : ly.h2[row * ly.out2 + (co - out)];
                    if (ly.act == TG_MLP_ACT_TANH) {
                        const float tt = hv * hv;
                        const float u = 1.0f - tt;
                        g = dh * u;
                    } else if (ly.act == TG_MLP_ACT_RELU) {
                        g = hv > 0.0f ? dh : 0.0f;
                    } else {
                        g = dh;
                    }
                }
                gs[at] = g;
            }
            __syncthreads();
            const bool want_b = ly.dbias || ly.dbias2, want_w = ly.dweight || ly.dweight2;   // a frozen layer's sums are not taken
            if (want_b && tid < outT) {                                   // dbias: the tile's rows in ascending order, on the workgroup's partial
                const int32_t co = tid;
                float* dst = slab ? sb + co : co < out ? (ly.dbias ? ly.dbias + co : nullptr) : (ly.dbias2 ? ly.dbias2 + (co - out) : nullptr);
                if (dst) {
                    float s = first ? 0.0f : *dst;
                    for (int r = 0; r < kMlpRows; ++r) s = s + gs[r * kMlpPitch + (co ^ r)];
                    *dst = s;
                }
            }
            if (want_w) {                                                 // dweight: 32 x 32 tiles (co, k), dealt to the waves
                const int32_t nkt = (in + 31) >> 5, nt = ((outT + 31) >> 5) * nkt;
                for (int32_t ti = wave; ti < nt; ti += kMlpWaves) {
                    const int32_t c0 = (ti / nkt) * 32, k = (ti % nkt) * 32 + j;
                    f32x16 acc;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int32_t co = c0 + mlp_row(i, h);
                        acc[i] = (!first && co < outT && k < in) ? sw[(int64_t)co * in + k] : 0.0f;
                    }
#pragma unroll 4
                    for (int s = 0; s < kMlpRows / 2; ++s) {
                        const int32_t r = 2 * s + h;
                        const int64_t row = row0 + r;
                        const float ga = gs[r * kMlpPitch + ((c0 + j) ^ r)];
                        float xb = 0.0f;
                        if (row < a.B && k < in) xb = l ? hprev[row * in + k] : *mlp_input_at(a, row, k);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, xb, acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int32_t co = c0 + mlp_row(i, h);
                        if (co < outT && k < in) {
                            if (slab) sw[(int64_t)co * in + k] = acc[i];
                            else if (co < out) { if (ly.dweight) ly.dweight[(int64_t)co * in + k] = acc[i]; }
                            else if (ly.dweight2) ly.dweight2[(int64_t)(co - out) * in + k] = acc[i];
                        }
                    }
                }
            }
            if (l == 0 && !a.want_dx) break;
            // dh_{l-1}[row][k] = chain over co ascending of g[row][co] W[co][k]: 32-wide k tiles
            const int32_t nkt = (in + 31) >> 5, nsteps = (outT + 1) >> 1;
            f32x16 keep;
#pragma unroll
            for (int i = 0; i < 16; ++i) keep[i] = 0.0f;
            for (int32_t kt = wave; kt < nkt; kt += kMlpWaves) {
                const int32_t k = kt * 32 + j;
                if (l == 0 && T == 1 && ((!a.dx0 && kt * 32 + 32 <= a.Ka) || (!a.dx1 && kt * 32 >= a.Ka))) continue;   // no column of the tile is asked for
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
                for (int s0 = 0; s0 < nsteps; s0 += 4) {                      // four steps at a time; steps past outT add (-0.0, +0.0)
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int32_t co = 2 * (s0 + s) + h;
                        const float ga = gs[j * kMlpPitch + (co ^ j)];
                        float wb = 0.0f;
                        if (co < outT && k < in) wb = co < out ? ly.weight[(int64_t)co * in + k] : ly.weight2[(int64_t)(co - out) * in + k];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, wb, acc, 0, 0, 0);
                    }
                }
                if (l) {
                    keep = acc;                                           // in <= 256: one tile per wave
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int64_t row = row0 + mlp_row(i, h);
                        if (row < a.B && k < K0) {
                            if (T > 1) a.dxs[((int64_t)t * a.B + row) * K0 + k] = acc[i];
                            else if (k < a.Ka) { if (a.dx0) a.dx0[row * a.Ka + k] = acc[i]; }
                            else if (a.dx1) a.dx1[row * a.Kb + (k - a.Ka)] = acc[i];
                        }
                    }
                }
            }
            if (l) {
                __syncthreads();                                          // g is read
                if (wave < nkt) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int32_t r = mlp_row(i, h);
                        gs[r * kMlpPitch + ((wave * 32 + j) ^ r)] = keep[i];
                    }
                }
                __syncthreads();
            }
        }
    }
}

struct MlpSeg {
    float* d0;                // elements [0, n0)
    float* d1;                // elements [n0, n): the second row block
    int64_t off;              // floats into a slab
    int32_t n0, n;
};

struct MlpReduceArgs {
    MlpSeg seg[kMlpSegs];
    const float* ws;
    const float* dxs;
    float* dx0;
    float* dx1;
    int64_t slab_floats, B;
    int32_t G, n_seg, Ka, Kb, T;
};

__global__ __launch_bounds__(256) void k_mlp_reduce(MlpReduceArgs a) {
    const int64_t stride = (int64_t)gridDim.x * 256, e0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((int32_t)blockIdx.y < a.n_seg) {
        const MlpSeg& sg = a.seg[blockIdx.y];
        for (int64_t e = e0; e < sg.n; e += stride) {
            float* dst = e < sg.n0 ? (sg.d0 ? sg.d0 + e : nullptr) : (sg.d1 ? sg.d1 + (e - sg.n0) : nullptr);
            if (!dst) continue;
            const float* src = a.ws + sg.off + e;
            float s = src[0];
            for (int32_t g = 1; g < a.G; ++g) s = s + src[g * a.slab_floats];
            *dst = s;
        }
    } else {                                                              // dx: the towers' dh_0, tower 0 first
        const int32_t K0 = a.Ka + a.Kb;
        const int64_t n = a.B * K0;
        for (int64_t e = e0; e < n; e += stride) {
            const int64_t row = e / K0;
            const int32_t k = (int32_t)(e - row * K0);
            float* dst = k < a.Ka ? (a.dx0 ? a.dx0 + row * a.Ka + k : nullptr) : (a.dx1 ? a.dx1 + row * a.Kb + (k - a.Ka) : nullptr);
            if (!dst) continue;
            float s = a.dxs[e];
            for (int32_t t = 1; t < a.T; ++t) s = s + a.dxs[t * n + e];
            *dst = s;
        }
    }
}

enum { kMlpShapes = 0, kMlpForward = 1, kMlpBackward = 2 };

// The checks the three calls share; 0 or the error's code.  what: the shapes alone, or the pointers of the forward / backward call as well.
static int mlp_check(const char* who, int what, const float* x0, int32_t Ka, const float* x1, int32_t Kb, int64_t B, const tg_mlp_tower* towers,
                     int32_t T, int32_t save_all) {
    static thread_local char msg[200];
    const char* bad = nullptr;
    int32_t bt = 0, bl = 0;
    if (!towers) bad = "NULL towers";
    else if (T < 1 || T > TG_MLP_MAX_TOWERS) bad = "need 1 <= T <= TG_MLP_MAX_TOWERS";
    else if (Ka < 1 || Kb < 0 || (int64_t)Ka + Kb > TG_MLP_MAX_IN) bad = "need Ka >= 1, Kb >= 0 and Ka + Kb <= TG_MLP_MAX_IN (1024)";
    else if (B < 0 || B > TG_MLP_MAX_ROWS) bad = "need 0 <= B <= TG_MLP_MAX_ROWS";
    else if (what != kMlpShapes && (!x0 || (Kb > 0 && !x1))) bad = "NULL x0_dev or x1_dev";
    for (int32_t t = 0; !bad && t < T; ++t) {
        const tg_mlp_tower& tw = towers[t];
        bt = t;
        bl = 0;
        if (tw.n_layers < 1 || tw.n_layers > TG_MLP_MAX_LAYERS) { bad = "need 1 <= n_layers <= TG_MLP_MAX_LAYERS"; break; }
        for (int32_t l = 0; !bad && l < tw.n_layers; ++l) {
            const tg_mlp_layer& ly = tw.layer[l];
            const bool last = l == tw.n_layers - 1;
            bl = l;
            if (ly.out < 1 || ly.out > TG_MLP_MAX_WIDTH || ly.out2 < 0 || (int64_t)ly.out + ly.out2 > TG_MLP_MAX_WIDTH)
                bad = "a layer's width (out, out + out2) must lie in 1 .. TG_MLP_MAX_WIDTH (256): wider layers are not built";
            else if (ly.out2 > 0 && !last) bad = "only a tower's last layer may have a second row block";
            else if (ly.in != (l ? tw.layer[l - 1].out : Ka + Kb)) bad = "in must be the previous layer's out (Ka + Kb for the first layer)";
            else if (ly.act != TG_MLP_ACT_NONE && ly.act != TG_MLP_ACT_TANH && ly.act != TG_MLP_ACT_RELU) bad = "unknown activation";
            else if (what == kMlpShapes) continue;
            else if (!ly.weight || !ly.bias || (ly.out2 > 0 && (!ly.weight2 || !ly.bias2))) bad = "NULL weight or bias";
            else if ((what == kMlpBackward || last || save_all) && (!ly.h || (ly.out2 > 0 && !ly.h2))) bad = "NULL h (or h2)";
        }
    }
    if (!bad) return 0;
    snprintf(msg, sizeof msg, "%s: tower %d layer %d: %s", who, bt, bl, bad);
    return report_error(-1, msg);
}

struct MlpPlan {
    int64_t n_tiles, slab_floats, ws_floats, dxs_floats;
    int32_t G;
};

static MlpPlan mlp_plan(int64_t B, int32_t Ka, int32_t Kb, const tg_mlp_tower* towers, int32_t T, int64_t (*off)[TG_MLP_MAX_LAYERS]) {
    MlpPlan p;
    p.n_tiles = (B + kMlpRows - 1) / kMlpRows;
    p.G = (int32_t)(p.n_tiles < kMlpGroups ? p.n_tiles : kMlpGroups);
    p.slab_floats = 0;
    for (int32_t t = 0; t < T; ++t)
        for (int32_t l = 0; l < towers[t].n_layers; ++l) {
            const tg_mlp_layer& ly = towers[t].layer[l];
            if (off) off[t][l] = p.slab_floats;
            p.slab_floats += (int64_t)(ly.out + ly.out2) * (ly.in + 1);
        }
    p.ws_floats = p.G > 1 ? p.G * p.slab_floats : 0;
    p.dxs_floats = T > 1 ? T * B * (Ka + Kb) : 0;
    return p;
}

static void mlp_fill(MlpArgs& a, const float* x0, int32_t Ka, const float* x1, int32_t Kb, int64_t B, const tg_mlp_tower* towers, int32_t T) {
    for (int32_t t = 0; t < T; ++t) a.tw[t] = towers[t];
    a.x0 = x0;
    a.x1 = x1;
    a.Ka = Ka;
    a.Kb = Kb;
    a.B = B;
}

}  // namespace tg

extern "C" int tg_mlp_forward(const float* x0_dev, int32_t Ka, const float* x1_dev, int32_t Kb, int64_t B, const tg_mlp_tower* towers, int32_t T,
                              int32_t save_all, void* hip_stream) {
    using namespace tg;
    if (int rc = mlp_check("tg_mlp_forward", kMlpForward, x0_dev, Ka, x1_dev, Kb, B, towers, T, save_all)) return rc;
    if (B == 0) return 0;
    MlpArgs a = {};
    mlp_fill(a, x0_dev, Ka, x1_dev, Kb, B, towers, T);
    a.save_all = save_all;
    a.n_tiles = (B + kMlpRows - 1) / kMlpRows;
    hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned)a.n_tiles, (unsigned)T), dim3(kMlpThreads), 0, (hipStream_t)hip_stream, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_mlp_forward: the kernel launch failed");
    return 0;
}

extern "C" int64_t tg_mlp_backward_workspace(int64_t B, int32_t Ka, int32_t Kb, const tg_mlp_tower* towers, int32_t T) {
    using namespace tg;
    if (int rc = mlp_check("tg_mlp_backward_workspace", kMlpShapes, nullptr, Ka, nullptr, Kb, B, towers, T, 0)) return rc;
    const MlpPlan p = mlp_plan(B, Ka, Kb, towers, T, nullptr);
    return (p.ws_floats + p.dxs_floats) * (int64_t)sizeof(float);
}

extern "C" int tg_mlp_backward(const float* x0_dev, int32_t Ka, const float* x1_dev, int32_t Kb, int64_t B, const tg_mlp_tower* towers, int32_t T,
                               float* dx0_dev, float* dx1_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream) {
    using namespace tg;
    if (int rc = mlp_check("tg_mlp_backward", kMlpBackward, x0_dev, Ka, x1_dev, Kb, B, towers, T, 1)) return rc;
    if (B == 0) return 0;
    MlpArgs a = {};
    const MlpPlan p = mlp_plan(B, Ka, Kb, towers, T, a.slab_off);
    const int64_t need = (p.ws_floats + p.dxs_floats) * (int64_t)sizeof(float);
    if (need > 0 && !workspace_dev) return report_error(-1, "tg_mlp_backward: NULL workspace_dev");
    if (workspace_bytes < need) return report_error(-1, "tg_mlp_backward: the workspace is smaller than tg_mlp_backward_workspace's size");
    mlp_fill(a, x0_dev, Ka, x1_dev, Kb, B, towers, T);
    if (Kb == 0) dx1_dev = nullptr;
    a.dx0 = dx0_dev;
    a.dx1 = dx1_dev;
    a.want_dx = dx0_dev || dx1_dev;
    a.ws = (float*)workspace_dev;
    a.dxs = a.ws + p.ws_floats;
    a.slab_floats = p.slab_floats;
    a.n_tiles = p.n_tiles;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_mlp_bwd, dim3((unsigned)p.G, (unsigned)T), dim3(kMlpThreads), 0, s, a);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_mlp_backward: the kernel launch failed");
    const bool sum_dx = T > 1 && a.want_dx;
    if (p.G == 1 && !sum_dx) return 0;                                    // one row tile holds the batch: the sums are in place
    MlpReduceArgs r = {};
    int64_t widest = sum_dx ? B * (Ka + Kb) : 0;
    if (p.G > 1) {
        for (int32_t t = 0; t < T; ++t)
            for (int32_t l = 0; l < towers[t].n_layers; ++l) {
                const tg_mlp_layer& ly = towers[t].layer[l];
                MlpSeg& w = r.seg[r.n_seg++];
                w = {ly.dweight, ly.dweight2, a.slab_off[t][l], ly.out * ly.in, (ly.out + ly.out2) * ly.in};
                MlpSeg& b = r.seg[r.n_seg++];
                b = {ly.dbias, ly.dbias2, a.slab_off[t][l] + (int64_t)(ly.out + ly.out2) * ly.in, ly.out, ly.out + ly.out2};
                if (w.n > widest) widest = w.n;
            }
    }
    r.ws = a.ws;
    r.dxs = a.dxs;
    r.dx0 = dx0_dev;
    r.dx1 = dx1_dev;
    r.slab_floats = p.slab_floats;
    r.B = B;
    r.G = p.G;
    r.Ka = Ka;
    r.Kb = Kb;
    r.T = T;
    int64_t blocks = (widest + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_mlp_reduce, dim3((unsigned)blocks, (unsigned)(r.n_seg + (sum_dx ? 1 : 0))), dim3(256), 0, s, r);
    if (hipGetLastError() != hipSuccess) return report_error(-2, "tg_mlp_backward: the reduction's launch failed");
    return 0;
}
