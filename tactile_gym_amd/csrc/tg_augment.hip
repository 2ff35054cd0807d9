// tg_augment.hip - RAD's image augmentation on the device: kornia's RandomAffine(degrees=0, translate=(ax, ay), scale=(1, 1), p) with its
// defaults (bilinear, zero padding, align_corners=False) over uint8 or float32 image batches (tg_random_translate).  Compiled with
// -ffp-contract=off: the arithmetic below is the bit-exact specification the tests restate (tests/augment_ref.py).
//
// Per sample b: apply = u0 < p, tx = (float)(ax W) (2 u1 - 1), ty = (float)(ay H) (2 u2 - 1), u_k = 24 bits of tg_sample_actions' generator at
// element 3 b + k of draw `counter` (or the caller's [B][3] (apply, tx, ty)).  kornia's warp_affine normalises with W - 1 and grid_sample
// unnormalises with W, so the shift in pixels is sx = tx W / (W - 1): out[y][x] = bilinear(in, x - sx, y - sy) with every tap outside the image 0.
// With o = floor(-s) and f = -s - o that is a 2 x 2 stencil of constant weights at a constant integer offset per sample.
//
// Mapping: a sample is P planes of H rows of R elements (channels first: P = C, R = W, the right-hand tap one element on; channels last: P = 1,
// R = W C, the right-hand tap C elements on).  One workgroup per (sample, plane, 4096 output elements): the parameters are computed once per
// workgroup, the source span that the chunk's four taps can reach - one contiguous range of the plane, the chunk plus one row and one tap -
// is staged into LDS as float32 with aligned 16-byte loads, and every lane then writes 4 x 16 bytes of output (aligned, each wavefront store
// 1 KiB contiguous) from aligned 16-byte LDS reads.  The column offset of a tap is the same for every lane of the launch modulo 4, so the
// unaligned window is two aligned float4 reads and a selection by that uniform remainder.  Samples that are not applied take a plain
// convert-copy.  Shapes whose planes are not 16-byte multiples, or rows too long for the LDS span, take a per-element path with the same
// arithmetic.  tg_random_translate_rows gives the source a row table (sample b reads source sample rows[b]: the minibatch gather of the device
// rollout buffer): the workgroup's source base is the only thing that changes.
#include "tg_augment.h"   // + tg_augment_core.h: what k_random_affine shares (the draw, store16, blend, the chunk prologue, the convert-copy)

namespace tg {

struct TrSample {
    bool apply;
    int ox, oy;
    float fx, fy;
};

// o = floor(-s), f = (float)(-s - o) for s = t n / (n - 1).  -s is clamped to [-(n + 2), n + 2] first (NaN goes to -(n + 2)): beyond that
// every tap is outside the image whatever f is.
__device__ __forceinline__ void split_shift(float t, int n, int& o, float& f) {
    const double s = (double)t * n / (n - 1);
    const double m = fmin(fmax(-s, -(double)(n + 2)), (double)(n + 2));
    const double fl = floor(m);
    o = (int)fl;
    f = (float)(m - fl);
}

__device__ __forceinline__ TrSample sample_params(const TranslateArgs& a, int64_t b, bool write) {
    bool apply;
    float tx, ty;
    if (a.params_in) {
        apply = a.params_in[3 * b] != 0.f;
        tx = a.params_in[3 * b + 1];
        ty = a.params_in[3 * b + 2];
    } else {
        const uint64_t i = 3 * (uint64_t)b;
        apply = draw_u24(a.seed, a.counter, i) < a.p;
        tx = a.ax_w * (2.f * draw_u24(a.seed, a.counter, i + 1) - 1.f);
        ty = a.ay_h * (2.f * draw_u24(a.seed, a.counter, i + 2) - 1.f);
    }
    if (write && a.params_out && threadIdx.x == 0) {   // one lane of one workgroup per sample
        a.params_out[3 * b] = apply ? 1.f : 0.f;
        a.params_out[3 * b + 1] = tx;
        a.params_out[3 * b + 2] = ty;
    }
    TrSample s;
    s.apply = apply;
    split_shift(tx, a.W, s.ox, s.fx);
    split_shift(ty, a.H, s.oy, s.fy);
    return s;
}

// Element k of the 8 floats (w0, w1) from position r + k, r in 0..3 the same in every lane (selects, no indexed register array).
__device__ __forceinline__ float pick(const float4& w0, const float4& w1, int r, int k) {
    const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    return r == 0 ? w[k] : r == 1 ? w[k + 1] : r == 2 ? w[k + 2] : w[k + 3];
}

// The two aligned float4 of LDS that hold floats [al, al + 8); al = local - r clamped into the allocation (lanes whose taps are all outside
// the image read something harmless; a tap inside the image never needs the clamp).
__device__ __forceinline__ void window(const float* lds, int local, int r, int lds_floats, float4& w0, float4& w1) {
    int al = local - r;
    al = al < 0 ? 0 : (al > lds_floats - 8 ? lds_floats - 8 : al);
    w0 = *reinterpret_cast<const float4*>(lds + al);
    w1 = *reinterpret_cast<const float4*>(lds + al + 4);
}

// vec: the plane is a multiple of 16 bytes of input and of 4 floats of output, both pointers are 16-byte aligned and R + S <= kTrMaxRow.
template <typename TIN, bool CF>
__global__ __launch_bounds__(kAugThreads) void k_random_translate(TranslateArgs a, int64_t b0, int nchunk, int vec, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const PlaneGeom g = plane_geom(CF, a.C, a.H, a.W);
    const int R = g.R, S = CF ? 1 : g.S, HR = g.HR, H = a.H;   // CF: S as the literal 1 (the same code as before plane_geom)
    int64_t b;
    int rem, pl, f0, fend;
    chunk_of(g, nchunk, b0, b, rem, pl, f0, fend);
    const TrSample sp = sample_params(a, b, rem == 0);
    const TIN* __restrict__ in = plane_of(reinterpret_cast<const TIN*>(a.in), a.rows, b, pl, g);
    float* __restrict__ out = plane_of(a.out, nullptr, b, pl, g);
    const int tid = threadIdx.x;

    if (!sp.apply) {
        convert_copy(in, out, f0, fend, tid, vec, vec);
        return;
    }

    const int dx = sp.ox * S, oy = sp.oy;
    const float fx = sp.fx, fy = sp.fy;
    if (!vec) {   // per element, taps read from global memory
        for (int f = f0 + tid; f < fend; f += kAugThreads) {
            const int y = f / R, j = f - y * R;
            const int ya = y + oy, xa = j + dx;
            const bool r0 = ya >= 0 && ya < H, r1 = ya + 1 >= 0 && ya + 1 < H;
            const bool c0 = xa >= 0 && xa < R, c1 = xa + S >= 0 && xa + S < R;
            const int64_t t = (int64_t)ya * R + xa;
            const float va = r0 && c0 ? (float)in[t] : 0.f, vb = r0 && c1 ? (float)in[t + S] : 0.f;
            const float vc = r1 && c0 ? (float)in[t + R] : 0.f, vd = r1 && c1 ? (float)in[t + R + S] : 0.f;
            out[f] = blend(va, vb, vc, vd, fx, fy);
        }
        return;
    }

    // Stage the source span [s_lo, s_hi) of the plane (clamped to it, widened to 16-byte vectors) at lds[src - a_lo + 4].
    constexpr int V = 16 / (int)sizeof(TIN);
    const int D = oy * R + dx;                                       // |oy| <= H + 2, |dx| <= (W + 2) S: fits, the span ends may not
    const int64_t lo64 = (int64_t)f0 + D, hi64 = (int64_t)fend + D + R + S;
    const int lo = lo64 < 0 ? 0 : (lo64 > HR ? HR : (int)lo64), hi = hi64 > HR ? HR : (hi64 < 0 ? 0 : (int)hi64);
    const int a_lo = lo / V * V;
    if (lo < hi) {
        const int a_hi = (hi + V - 1) / V * V;
        for (int v = a_lo + V * tid; v < a_hi; v += V * kAugThreads) store16(lds + (v - a_lo + 4), in + v);
    }
    __syncthreads();

    // Tap shifts: a at D, b at D + S, c at D + R, d at D + R + S; the window remainder of each is the shift mod 4 (f and a_lo are multiples of 4).
    const int ra = D & 3, rc = (D + R) & 3, rb = (D + S) & 3, rd = (D + R + S) & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int f = f0 + 4 * tid + 1024 * k;
        if (f >= fend) break;
        const int local = f - a_lo + 4;
        float4 a0, a1, c0, c1, b0w, b1w, d0w, d1w;
        window(lds, local + D, ra, lds_floats, a0, a1);
        window(lds, local + D + R, rc, lds_floats, c0, c1);
        if (!CF) {
            window(lds, local + D + S, rb, lds_floats, b0w, b1w);
            window(lds, local + D + R + S, rd, lds_floats, d0w, d1w);
        }
        int y = f / R, j = f - y * R;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i > 0 && ++j == R) { j = 0; ++y; }
            const int ya = y + oy, xa = j + dx;
            const bool r0 = ya >= 0 && ya < H, r1 = ya + 1 >= 0 && ya + 1 < H;
            const bool cl0 = xa >= 0 && xa < R, cl1 = xa + S >= 0 && xa + S < R;
            const float ea = pick(a0, a1, ra, i), ec = pick(c0, c1, rc, i);
            const float eb = CF ? pick(a0, a1, ra, i + 1) : pick(b0w, b1w, rb, i);
            const float ed = CF ? pick(c0, c1, rc, i + 1) : pick(d0w, d1w, rd, i);
            o[i] = blend(r0 && cl0 ? ea : 0.f, r0 && cl1 ? eb : 0.f, r1 && cl0 ? ec : 0.f, r1 && cl1 ? ed : 0.f, fx, fy);
        }
        *reinterpret_cast<float4*>(out + f) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <typename TIN, bool CF>
static int launch_typed(const TranslateArgs& a, hipStream_t stream) {
    const TranslatePlan pl = translate_plan((int)sizeof(TIN), CF, a.C, a.H, a.W, (uintptr_t)a.in, (uintptr_t)a.out);
    return launch_chunks(a.B, pl, [&](int64_t b0, dim3 grid) {
        hipLaunchKernelGGL((k_random_translate<TIN, CF>), grid, dim3(kAugThreads), (size_t)pl.lds_floats * 4, stream, a, b0, pl.nchunk, pl.vec,
                           pl.lds_floats);
    });
}

int launch_random_translate(const TranslateArgs& a, int in_dtype, int channels_first, hipStream_t stream) {
    return dispatch_images(a.in, a.out, in_dtype, channels_first, a.B, a.C, a.H, a.W,
                           [&](auto t, auto cf) { return launch_typed<decltype(t), decltype(cf)::value>(a, stream); });
}

}  // namespace tg

extern "C" int tg_random_translate_rows(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H,
                                        int32_t W, double ax, double ay, float p, uint64_t seed, uint64_t counter, const float* params_in_dev,
                                        float* params_out_dev, const int64_t* rows_dev, void* hip_stream) {
    using tg::report_error;
    if (const int bad = tg::check_image_call("tg_random_translate", in_dev, out_dev, in_dtype, B, C, H, W, ax, ay, p, rows_dev != nullptr)) return bad;
    if (B == 0) return 0;
    const tg::TranslateArgs a = tg::image_args<tg::TranslateArgs>(in_dev, out_dev, params_in_dev, params_out_dev, rows_dev, B, C, H, W, ax, ay, p,
                                                                  seed, counter);
    const int rc = tg::launch_random_translate(a, in_dtype, channels_first, (hipStream_t)hip_stream);
    if (rc == -2) return report_error(-2, "tg_random_translate: the kernel launch failed");
    if (rc) return report_error(rc, "tg_random_translate: arguments the kernel is not built for");
    return 0;
}

extern "C" int tg_random_translate(const void* in_dev, void* out_dev, int32_t in_dtype, int32_t channels_first, int64_t B, int32_t C, int32_t H,
                                   int32_t W, double ax, double ay, float p, uint64_t seed, uint64_t counter, const float* params_in_dev,
                                   float* params_out_dev, void* hip_stream) {
    return tg_random_translate_rows(in_dev, out_dev, in_dtype, channels_first, B, C, H, W, ax, ay, p, seed, counter, params_in_dev, params_out_dev,
                                    nullptr, hip_stream);
}
