// tg_affine.hip - the general 2-D affine warp of the image augmentation: kornia's RandomAffine(degrees, translate, scale, shear, p) with its
// defaults (bilinear, zero padding, align_corners=False, per-sample draws) over uint8 or float32 image batches (tg_random_affine).  Compiled with
// -ffp-contract=off: the arithmetic below is the specification the tests restate (tests/affine_ref.py), in three stages.
//
// (a) Draws, float32, one rounding per operation: u_k = element 8 b + k of tg_sample_actions' generator at (seed, counter); apply = u0 < p,
//     tx = (float)(ax W)(2 u1 - 1), ty likewise with u2, angle = d0 + (d1 - d0) u3, scale_x = s0 + (s1 - s0) u4, scale_y = scale_x or
//     s2 + (s3 - s2) u5, shear_x = h0 + (h1 - h0) u6, shear_y = h2 + (h3 - h2) u7 (or the caller's [B][8]).
// (b) Coefficients, double, rounded once to float32: the forward map is M(q) = L Sh (q - c) + c + t about the centre c = ((W-1)/2, (H-1)/2),
//     L = R(angle) diag(scale_x, scale_y), Sh = [[1, -tan shx], [-tan shy, 1 + tan shx tan shy]]; output pixel (j, i) samples the input at
//     src = K M^-1(P (j + 1/2, i + 1/2)) - 1/2 with P = diag((W-1)/W, (H-1)/H), K = P^-1 - kornia's warp_affine normalises with n - 1 and
//     grid_sample unnormalises with n.  Folded: src_x = a00 j + a01 i + a02, src_y = a10 j + a11 i + a12 (or the caller's [B][6]).
// (c) Warp, float32: sx = (a00 (float)j + a01 (float)i) + a02, sy likewise.  A coordinate outside (-1, W) x (-1, H), or not finite, gives 0:
//     there every tap is outside the image or has weight 0, and inside that range floor(sx) lies in [-1, W - 1], so the conversion to int is
//     exact and defined.  x0 = floor(sx), fx = sx - x0, the same in y; the four taps are 0 outside the image; h0 = (1 - fx) a + fx b, h1
//     likewise, out = (1 - fy) h0 + fy h1.  Every channel of a sample uses the same coefficients; a sample that is not applied is the input
//     converted to float32.
//
// Mapping: one workgroup per (sample, plane, 4096 output elements), as k_random_translate.  Lane 0 draws the parameters and computes the
// coefficients - the double-precision trigonometry runs in one wavefront, not four - writes params_out / coeffs_out for the sample's first
// workgroup and hands the six floats to the workgroup through 32 bytes of LDS; every lane then holds them in scalar registers.  Every lane
// writes 4 x 16 bytes of output (each wavefront store 1 KiB contiguous).  The taps of an output tile lie in a parallelogram of the source:
// the staged path (affine_plan: path 2) copies the source ROWS that the chunk's corners reach - sy is monotone in j and in i also after
// rounding, so the corners bound it - into LDS as they are stored, with aligned 16-byte loads, and reads the taps from there; the gather path
// (1) reads them from global memory; the per-element path (0) also stores element by element.  All three run the same arithmetic (affine_px).
#include "tg_affine.h"   // + tg_augment_core.h: what k_random_translate shares (the draw, store16, blend, the chunk prologue, the convert-copy)

namespace tg {

// Stage (a): prm[8] of sample b.
__device__ __forceinline__ void af_params(const AffineArgs& a, int64_t b, float prm[8]) {
    if (a.params_in) {
#pragma unroll
        for (int k = 0; k < 8; ++k) prm[k] = a.params_in[8 * b + k];
        prm[0] = prm[0] != 0.f ? 1.f : 0.f;
        return;
    }
    const uint64_t i = 8 * (uint64_t)b;
    float u[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = draw_u24(a.seed, a.counter, i + k);
    prm[0] = u[0] < a.p ? 1.f : 0.f;
    prm[1] = a.ax_w * (2.f * u[1] - 1.f);
    prm[2] = a.ay_h * (2.f * u[2] - 1.f);
    prm[3] = a.d0 + (a.d1 - a.d0) * u[3];
    prm[4] = a.s0 + (a.s1 - a.s0) * u[4];
    prm[5] = a.scale4 ? a.s2 + (a.s3 - a.s2) * u[5] : prm[4];
    prm[6] = a.h0 + (a.h1 - a.h0) * u[6];
    prm[7] = a.h2 + (a.h3 - a.h2) * u[7];
}

__device__ __forceinline__ double af_tan_deg(double d) { return d == 0.0 ? 0.0 : sinpi(d / 180.0) / cospi(d / 180.0); }

// Stage (b): A^-1 = Sh^-1 L^-1 in closed form (det Sh = 1), then the fold with P, K, the centre and the half-pixel offsets.
__device__ __forceinline__ void af_coeffs(const float prm[8], int H, int W, float co[6]) {
    const double tx = prm[1], ty = prm[2], scx = prm[4], scy = prm[5];
    const double c = cospi((double)prm[3] / 180.0), s = sinpi((double)prm[3] / 180.0);
    const double tsx = af_tan_deg(prm[6]), tsy = af_tan_deg(prm[7]);
    const double l00 = c / scx, l01 = s / scx, l10 = -s / scy, l11 = c / scy;           // L^-1 = diag(1 / scale) R^T
    const double g = 1.0 + tsx * tsy;                                                  // Sh^-1 = [[g, tsx], [tsy, 1]]
    const double i00 = g * l00 + tsx * l10, i01 = g * l01 + tsx * l11, i10 = tsy * l00 + l10, i11 = tsy * l01 + l11;
    const double cx = (W - 1) / 2.0, cy = (H - 1) / 2.0;
    const double px = (W - 1.0) / W, py = (H - 1.0) / H, kx = W / (W - 1.0), ky = H / (H - 1.0);
    const double ux = 0.5 * px - cx - tx, uy = 0.5 * py - cy - ty;
    co[0] = (float)i00;
    co[1] = (float)(kx * i01 * py);
    co[2] = (float)(kx * (i00 * ux + i01 * uy + cx) - 0.5);
    co[3] = (float)(ky * i10 * px);
    co[4] = (float)i11;
    co[5] = (float)(ky * (i10 * ux + i11 * uy + cy) - 0.5);
}

struct AfCo {
    float a00, a01, a02, a10, a11, a12;
};

__device__ __forceinline__ float af_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// Stage (c) for one output element: pixel column j, row i, channel offset cc of a plane `src` of H rows of R elements, tap step S.
template <typename TSRC>
__device__ __forceinline__ float affine_px(const TSRC* __restrict__ src, const AfCo& k, int j, int i, int cc, int H, int W, int R, int S) {
    const float jf = (float)j, yf = (float)i;
    const float sx = (k.a00 * jf + k.a01 * yf) + k.a02;
    const float sy = (k.a10 * jf + k.a11 * yf) + k.a12;
    if (!(sx > -1.f && sx < (float)W && sy > -1.f && sy < (float)H)) return 0.f;   // far out or not finite; inside, the floors convert exactly
    const float flx = floorf(sx), fly = floorf(sy);
    const int x0 = (int)flx, y0 = (int)fly;                                         // [-1, W - 1], [-1, H - 1]
    const float fx = sx - flx, fy = sy - fly;
    const bool c0 = x0 >= 0, c1 = x0 + 1 < W, r0 = y0 >= 0, r1 = y0 + 1 < H;
    const int t = y0 * R + x0 * S + cc;
    const float va = r0 && c0 ? (float)src[t] : 0.f, vb = r0 && c1 ? (float)src[t + S] : 0.f;
    const float vc = r1 && c0 ? (float)src[t + R] : 0.f, vd = r1 && c1 ? (float)src[t + R + S] : 0.f;
    return blend(va, vb, vc, vd, fx, fy);
}

// Four consecutive elements from f (a multiple of 4; they may run on into the next row) as one float4 store.
template <bool CF, typename TSRC>
__device__ __forceinline__ void affine_quad(const TSRC* __restrict__ src, float* __restrict__ out, const AfCo& k, int f, int C, int H, int W, int R,
                                            int S) {
    int y = f / R;
    const int e = f - y * R;
    int j = CF ? e : e / C, cc = CF ? 0 : e - j * C;
    float o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o[q] = affine_px(src, k, j, y, cc, H, W, R, S);
        if (CF || ++cc == C) {
            cc = 0;
            if (++j == W) { j = 0; ++y; }
        }
    }
    *reinterpret_cast<float4*>(out + f) = make_float4(o[0], o[1], o[2], o[3]);
}

template <typename TIN, bool CF>
__global__ __launch_bounds__(kAugThreads) void k_random_affine(AffineArgs a, int64_t b0, int nchunk, int path, int in_vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float* const head = reinterpret_cast<float*>(lds_raw);
    TIN* const plane = reinterpret_cast<TIN*>(lds_raw + kAfHeader);
    const PlaneGeom g = plane_geom(CF, a.C, a.H, a.W);
    const int R = g.R, S = g.S, H = a.H, W = a.W, C = a.C;
    int64_t b;
    int rem, pl, f0, fend;
    chunk_of(g, nchunk, b0, b, rem, pl, f0, fend);
    const int tid = threadIdx.x;

    if (tid == 0) {   // one lane: stages (a) and (b); the sample's first workgroup reports them
        float prm[8], co[6];
        af_params(a, b, prm);
        if (a.coeffs_in) {
#pragma unroll
            for (int q = 0; q < 6; ++q) co[q] = a.coeffs_in[6 * b + q];
        } else if (prm[0] != 0.f || (rem == 0 && a.coeffs_out)) {
            af_coeffs(prm, H, W, co);
        } else {
#pragma unroll
            for (int q = 0; q < 6; ++q) co[q] = 0.f;
        }
        if (rem == 0) {
            if (a.params_out) {
#pragma unroll
                for (int q = 0; q < 8; ++q) a.params_out[8 * b + q] = prm[q];
            }
            if (a.coeffs_out) {
#pragma unroll
                for (int q = 0; q < 6; ++q) a.coeffs_out[6 * b + q] = co[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) head[q] = co[q];
        head[6] = prm[0];
    }
    __syncthreads();
    const bool apply = af_uniform(head[6]) != 0.f;
    AfCo k;
    k.a00 = af_uniform(head[0]), k.a01 = af_uniform(head[1]), k.a02 = af_uniform(head[2]);
    k.a10 = af_uniform(head[3]), k.a11 = af_uniform(head[4]), k.a12 = af_uniform(head[5]);

    const TIN* __restrict__ in = plane_of(reinterpret_cast<const TIN*>(a.in), a.rows, b, pl, g);
    float* __restrict__ out = plane_of(a.out, nullptr, b, pl, g);

    if (!apply) {
        convert_copy(in, out, f0, fend, tid, in_vec, path);   // paths 1 and 2 store float4: the output is aligned
        return;
    }

    if (path == 0) {   // per element
        for (int f = f0 + tid; f < fend; f += kAugThreads) {
            const int y = f / R, e = f - y * R;
            const int j = CF ? e : e / C, cc = CF ? 0 : e - j * C;
            out[f] = affine_px(in, k, j, y, cc, H, W, R, S);
        }
        return;
    }

    if (path == 1) {   // taps from global memory
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = f0 + 4 * tid + 1024 * q;
            if (f < fend) affine_quad<CF>(in, out, k, f, C, H, W, R, S);
        }
        return;
    }

    // Staged: the source rows [ylo, yhi] that this chunk's outputs (rows y0 .. y1, every column) can reach, at their own offsets in `plane`.
    // sy at the four corners bounds sy over the chunk (each rounding is monotone); a NaN at a corner (an infinite coefficient) stages every row.
    {
        const float y0f = (float)(f0 / R), y1f = (float)((fend - 1) / R), w1 = (float)(W - 1);
        const float s00 = (k.a10 * 0.f + k.a11 * y0f) + k.a12, s01 = (k.a10 * w1 + k.a11 * y0f) + k.a12;
        const float s10 = (k.a10 * 0.f + k.a11 * y1f) + k.a12, s11 = (k.a10 * w1 + k.a11 * y1f) + k.a12;
        int ylo = 0, yhi = H - 1;
        if (s00 == s00 && s01 == s01 && s10 == s10 && s11 == s11) {
            const float lo = fminf(fminf(s00, s01), fminf(s10, s11)), hi = fmaxf(fmaxf(s00, s01), fmaxf(s10, s11));
            ylo = (int)fminf(fmaxf(floorf(lo), 0.f), (float)(H - 1));
            yhi = (int)fminf(fmaxf(floorf(hi) + 1.f, 0.f), (float)(H - 1));
        }
        constexpr int V = 16 / (int)sizeof(TIN);
        const int a_lo = ylo * R / V * V, a_hi = ((yhi + 1) * R + V - 1) / V * V;   // HR is a multiple of V: a_hi <= HR
        for (int v = a_lo + V * tid; v < a_hi; v += V * kAugThreads)
            *reinterpret_cast<uint4*>(plane + v) = *reinterpret_cast<const uint4*>(in + v);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f = f0 + 4 * tid + 1024 * q;
        if (f < fend) affine_quad<CF>(plane, out, k, f, C, H, W, R, S);
    }
}

template <typename TIN, bool CF>
static int launch_typed(const AffineArgs& a, hipStream_t stream) {
    const AffinePlan pl = affine_plan((int)sizeof(TIN), CF, a.C, a.H, a.W, (uintptr_t)a.in, (uintptr_t)a.out);
    return launch_chunks(a.B, pl, [&](int64_t b0, dim3 grid) {
        hipLaunchKernelGGL((k_random_affine<TIN, CF>), grid, dim3(kAugThreads), (size_t)pl.lds_bytes, stream, a, b0, pl.nchunk, pl.path, pl.in_vec);
    });
}

int launch_random_affine(const AffineArgs& a, int in_dtype, int channels_first, hipStream_t stream) {
    return dispatch_images(a.in, a.out, in_dtype, channels_first, a.B, a.C, a.H, a.W,
                           [&](auto t, auto cf) { return launch_typed<decltype(t), decltype(cf)::value>(a, stream); });
}

}  // namespace tg

static bool af_range(double lo, double hi) { return lo <= hi && lo - lo == 0.0 && hi - hi == 0.0; }   // ordered and finite

extern "C" int tg_random_affine_rows(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H,
                                     int32_t W, double ax, double ay, float d0, float d1, float s0, float s1, float s2, float s3, float h0,
                                     float h1, float h2, float h3, float p, uint64_t seed, uint64_t counter, const float* params_in_dev,
                                     float* params_out_dev, const float* coeffs_in_dev, float* coeffs_out_dev, const int64_t* rows_dev,
                                     void* hip_stream) {
    using tg::report_error;
    if (const int bad = tg::check_image_call("tg_random_affine", in_dev, out_dev, in_dtype, B, C, H, W, ax, ay, p, rows_dev != nullptr)) return bad;
    if (!af_range(d0, d1)) return report_error(-1, "tg_random_affine: degrees must be a finite range d0 <= d1");
    if (!af_range(s0, s1) || !(s0 > 0.f)) return report_error(-1, "tg_random_affine: scale must be a finite range 0 < s0 <= s1");
    const bool scale4 = !(s2 == 0.f && s3 == 0.f);
    if (scale4 && (!af_range(s2, s3) || !(s2 > 0.f)))
        return report_error(-1, "tg_random_affine: the scale of y must be a finite range 0 < s2 <= s3, or s2 = s3 = 0 for scale_y = scale_x");
    if (!af_range(h0, h1) || !af_range(h2, h3)) return report_error(-1, "tg_random_affine: shear must be finite ranges h0 <= h1, h2 <= h3");
    if (B == 0) return 0;
    tg::AffineArgs a = tg::image_args<tg::AffineArgs>(in_dev, out_dev, params_in_dev, params_out_dev, rows_dev, B, C, H, W, ax, ay, p, seed, counter);
    a.coeffs_in = coeffs_in_dev;
    a.coeffs_out = coeffs_out_dev;
    a.d0 = d0, a.d1 = d1;
    a.s0 = s0, a.s1 = s1, a.s2 = s2, a.s3 = s3;
    a.scale4 = scale4;
    a.h0 = h0, a.h1 = h1, a.h2 = h2, a.h3 = h3;
    const int rc = tg::launch_random_affine(a, in_dtype, channels_first, (hipStream_t)hip_stream);
    if (rc == -2) return report_error(-2, "tg_random_affine: the kernel launch failed");
    if (rc) return report_error(rc, "tg_random_affine: arguments the kernel is not built for");
    return 0;
}

extern "C" int tg_random_affine(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H, int32_t W,
                                double ax, double ay, float d0, float d1, float s0, float s1, float s2, float s3, float h0, float h1, float h2,
                                float h3, float p, uint64_t seed, uint64_t counter, const float* params_in_dev, float* params_out_dev,
                                const float* coeffs_in_dev, float* coeffs_out_dev, void* hip_stream) {
    return tg_random_affine_rows(in_dev, out_dev, in_dtype, channels_first, B, C, H, W, ax, ay, d0, d1, s0, s1, s2, s3, h0, h1, h2, h3, p, seed,
                                 counter, params_in_dev, params_out_dev, coeffs_in_dev, coeffs_out_dev, nullptr, hip_stream);
}
