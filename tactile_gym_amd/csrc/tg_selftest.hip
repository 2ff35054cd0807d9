// tg_selftest.hip - libtactile_gym_hip_test.so: device self-tests of pieces of the product's kernels against brute force / the compiler's own
// arithmetic.  TEST INFRASTRUCTURE: built next to the product library from the same headers (tg_raster_dev.hpp, tg_narrowphase.hpp), linked
// into nothing that ships; include/tactile_gym_hip_test.h declares its three entry points, tests/ are its only callers
// (tests/test_gpu_parity.py, tests/test_gpu_narrowphase.py).  Until round 4 these lived in libtactile_gym_hip.so and its ABI.
// Compiled with -ffp-contract=off like tg_raster.hip (the raster's expressions are the subject).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tactile_gym_hip_test.h"
#include "tg_augment.h"      // translate_plan: the launch decision of tg_random_translate (host only)
#include "tg_affine.h"       // affine_plan: the launch decision of tg_random_affine (host only)
#include "tg_ctx.hpp"        // fail: the message behind tg_selftest_last_error
#include "tg_raster_dev.hpp"

namespace tg {

// tg_selftest_division: the refinement above against the compiler's correctly rounded `/` on pseudo-random operand pairs with exponents in
// 2^-40 .. 2^24 (a superset of what a covered pixel produces); counts the pairs whose quotient bits differ.
__global__ void k_selftest_division(long long n, unsigned long long seed, unsigned long long* mismatches) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    for (long long i = i0; i < n; i += stride) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        const unsigned ea = 127u - 40u + (unsigned)((z >> 46) & 0xff) % 65u, eb = 127u - 40u + (unsigned)((z >> 54) & 0xff) % 65u;
        const float a = __uint_as_float(((unsigned)(z >> 63) << 31) | (ea << 23) | ((unsigned)z & 0x7fffffu));
        const float b = __uint_as_float(((unsigned)((z >> 62) & 1) << 31) | (eb << 23) | ((unsigned)(z >> 23) & 0x7fffffu));
        bad += __float_as_uint(div_mid_range(a, b)) != __float_as_uint(a / b);
    }
    if (bad) atomicAdd(mismatches, bad);
}
int selftest_division(long long n, unsigned long long seed, long long* mismatches_host) {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 8) != hipSuccess) return -1;
    (void)hipMemset(d, 0, 8);
    hipLaunchKernelGGL(k_selftest_division, dim3(2048), dim3(256), 0, 0, n, seed, d);
    const hipError_t e = hipMemcpy(mismatches_host, d, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}

// tg_selftest_penetration_division: t_s_camera's (penetration / 0.05) - the division of tactile_sensor.py:284-289 as the kernels evaluate it since
// round 5, div_mid_range(cl, 0.05f) - against the correctly rounded `/` for EVERY float a penetration can be: 0 and all of [1e-4, 0.05].
__global__ void k_selftest_penetration_division(unsigned long long* mismatches) {
    const unsigned lo = __float_as_uint(1e-4f), hi = __float_as_uint(0.05f);
    const unsigned long long n = (unsigned long long)(hi - lo) + 2ull, stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float a = i == n - 1 ? 0.0f : __uint_as_float(lo + (unsigned)i);
        const float max_pen = 0.05f;
        bad += __float_as_uint(div_mid_range(a, max_pen)) != __float_as_uint(a / max_pen);
    }
    if (bad) atomicAdd(mismatches, bad);
}
int selftest_penetration_division(long long* mismatches_host) {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 8) != hipSuccess) return -1;
    (void)hipMemset(d, 0, 8);
    hipLaunchKernelGGL(k_selftest_penetration_division, dim3(4096), dim3(256), 0, 0, d);
    const hipError_t e = hipMemcpy(mismatches_host, d, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}

// tg_selftest_edge_exclusion: edges_exclude_rect against brute force.  Pseudo-random triangles in window coordinates - image-sized, slivers
// (third vertex a hair off the line of the other two), huge (coordinates up to 1e4), vertices snapped onto pixel centres - and rectangles
// as the kernels pass them (16 x 16 blocks, 32 x 8 cells, at pixel-centre coordinates within 256 x 256); every pixel centre of the rectangle
// is put through the pixel loops' own edge expressions.  out[0] = cases where the rule excluded a rectangle that holds a pixel with all three
// edge functions >= 0 or all <= 0 (must be 0: a superset of `hit`), out[1] = rectangles excluded, out[2] = rectangles that held no such pixel.
// Round 5, edges_cover_rect (the renders' "this block is wholly inside the triangle: no coverage test per pixel"): out[3] = rectangles it called
// covered in which some pixel fails the pixel loops' coverage predicate (must be 0), out[4] = rectangles called covered, out[5] = rectangles
// whose every pixel passes the predicate.
__global__ void k_selftest_edge_exclusion(long long n, unsigned long long seed, unsigned long long* out) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, excl = 0, empty = 0, bad_cov = 0, n_cov = 0, n_full = 0;
    for (long long i = i0; i < n; i += stride) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
        auto next = [&]() { z += 0x9E3779B97F4A7C15ull; unsigned long long r = z; r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull; r = (r ^ (r >> 27)) * 0x94D049BB133111EBull; return r ^ (r >> 31); };
        auto unif = [&](float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); };
        const int kind = (int)(next() % 5);
        const float span = kind == 2 ? 1.0e4f : 356.0f, off = kind == 2 ? -5.0e3f : -50.0f;
        float x0 = off + unif(0.0f, span), y0 = off + unif(0.0f, span), x1 = off + unif(0.0f, span), y1 = off + unif(0.0f, span);
        float x2 = off + unif(0.0f, span), y2 = off + unif(0.0f, span);
        if (kind == 1) { const float t = unif(-0.5f, 1.5f), eps = unif(-1e-3f, 1e-3f); x2 = x0 + t * (x1 - x0) + eps; y2 = y0 + t * (y1 - y0) - eps; }   // sliver
        if (kind == 3) { x0 = floorf(x0) + 0.5f; y0 = floorf(y0) + 0.5f; x1 = floorf(x1) + 0.5f; y2 = floorf(y2) + 0.5f; }                          // on pixel centres
        if (kind == 4) { x1 = x0 + unif(-24.0f, 24.0f); y1 = y0 + unif(-24.0f, 24.0f); x2 = x0 + unif(-24.0f, 24.0f); y2 = y0 + unif(-24.0f, 24.0f); }   // heightfield-sized
        const bool cell = (next() & 1ull) != 0;
        const int w = cell ? 32 : 16, h = cell ? 8 : 16;
        const float X0 = (float)((int)(next() % (256 / w)) * w) + 0.5f, Y0 = (float)((int)(next() % (256 / h)) * h) + 0.5f;
        const float X1 = X0 + (float)(w - 1), Y1 = Y0 + (float)(h - 1);
        const bool ex = edges_exclude_rect(x0, y0, x1, y1, x2, y2, X0, X1, Y0, Y1);
        const bool cov = edges_cover_rect(x0, y0, x1, y1, x2, y2, X0, X1, Y0, Y1);
        const float bxl = fminf(x0, fminf(x1, x2)), bxh = fmaxf(x0, fmaxf(x1, x2)), byl = fminf(y0, fminf(y1, y2)), byh = fmaxf(y0, fmaxf(y1, y2));
        bool covered = false, all_hit = true;
        for (int py = 0; py < h; ++py) {
            const float fy = Y0 + (float)py;
            const float a0 = y2 - fy, a1 = y1 - fy, a2 = y0 - fy;
            for (int px = 0; px < w; ++px) {
                const float fx = X0 + (float)px;
                const float e0 = (x1 - fx) * a0 - (x2 - fx) * a1;
                const float e1 = (x2 - fx) * a2 - (x0 - fx) * a0;
                const float e2 = (x0 - fx) * a1 - (x1 - fx) * a2;
                const bool pos = (e0 >= 0.0f) & (e1 >= 0.0f) & (e2 >= 0.0f), neg = (e0 <= 0.0f) & (e1 <= 0.0f) & (e2 <= 0.0f);
                covered = covered | pos | neg;
                // the pixel loops' whole coverage predicate (bounding box, same-signed edge functions, non-degenerate)
                all_hit = all_hit & ((fx >= bxl) & (fx <= bxh) & (fy >= byl) & (fy <= byh) & (pos | neg) & (((e0 + e1) + e2) != 0.0f));
            }
        }
        bad += (ex && covered) ? 1 : 0;
        excl += ex ? 1 : 0;
        empty += covered ? 0 : 1;
        bad_cov += (cov && !all_hit) ? 1 : 0;
        n_cov += cov ? 1 : 0;
        n_full += all_hit ? 1 : 0;
    }
    if (bad) atomicAdd(out, bad);
    atomicAdd(out + 1, excl);
    atomicAdd(out + 2, empty);
    if (bad_cov) atomicAdd(out + 3, bad_cov);
    atomicAdd(out + 4, n_cov);
    atomicAdd(out + 5, n_full);
}
int selftest_edge_exclusion(long long n, unsigned long long seed, long long* out_host /*[6]*/) {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 48) != hipSuccess) return -1;
    (void)hipMemset(d, 0, 48);
    hipLaunchKernelGGL(k_selftest_edge_exclusion, dim3(2048), dim3(256), 0, 0, n, seed, d);
    const hipError_t e = hipMemcpy(out_host, d, 48, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}

// tg_selftest_pixel_predicate: the block kernel's hit predicate (pixel_hit, tg_raster_dev.hpp) against the chained compares it replaced, both
// fed the pixel loop's own e0..e2, s and d.  A case is a record - window coordinates, depths, and the bounding box as emit() makes it - and
// one quad of four pixel centres with the depths z it holds.  Even kinds are random: image-sized triangles, slivers, coordinates up to 1e4,
// vertices on pixel centres.  Odd kinds (half of the cases) force the specials: zero-area triangles in front of z (s == +-0); an edge through
// the pixel centre or a vertex on it (e_k == +0, e_k == -0); the bounding box's edge on the pixel centre (fx == xmin, fx == xmax); +-inf and
// NaN coordinates, one or all of the three x among them.  out[0] = pixels whose (hit, new z) differ between the forms (must be 0), out[1] =
// pixels hit, out[2] = pixels where the coverage booleans alone - box & (pos | neg) & (s != 0) against box & (lo >= 0 | hi <= 0) - differ
// (the cases the identity argument is about: d must be NaN there), out[3] = pixels of forced specials.
__global__ void k_selftest_pixel_predicate(long long n, unsigned long long seed, unsigned long long* out) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, hits = 0, cov_diff = 0, specials = 0;
    for (long long i = i0; i < n; i += stride) {
        unsigned long long zz = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
        auto next = [&]() { zz += 0x9E3779B97F4A7C15ull; unsigned long long r = zz; r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull; r = (r ^ (r >> 27)) * 0x94D049BB133111EBull; return r ^ (r >> 31); };
        auto unif = [&](float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); };
        const int kind = (int)(next() % 8);
        const int qx = 4 * (int)(next() % 64), qy = (int)(next() % 256);           // the quad: pixels qx .. qx + 3 of row qy, 256 x 256 image
        const float fy = (float)qy + 0.5f, cxp = (float)(qx + (int)(next() % 4)) + 0.5f;   // (cxp: one of its pixel centres, for the specials)
        const float span = kind == 4 ? 1.0e4f : 356.0f, off = kind == 4 ? -5.0e3f : -50.0f;
        float x0 = off + unif(0.0f, span), y0 = off + unif(0.0f, span), x1 = off + unif(0.0f, span), y1 = off + unif(0.0f, span);
        float x2 = off + unif(0.0f, span), y2 = off + unif(0.0f, span);
        if (kind == 0 && (next() & 1ull)) {                                        // a small triangle about the quad: most of the hits
            x0 = cxp + unif(-12.0f, 12.0f); y0 = fy + unif(-12.0f, 12.0f); x1 = cxp + unif(-12.0f, 12.0f); y1 = fy + unif(-12.0f, 12.0f);
            x2 = cxp + unif(-12.0f, 12.0f); y2 = fy + unif(-12.0f, 12.0f);
        }
        if (kind == 2) { const float t = unif(-0.5f, 1.5f), eps = unif(-1e-3f, 1e-3f); x2 = x0 + t * (x1 - x0) + eps; y2 = y0 + t * (y1 - y0) - eps; }   // sliver
        if (kind == 6) { x0 = floorf(x0) + 0.5f; y0 = floorf(y0) + 0.5f; x1 = floorf(x1) + 0.5f; y2 = floorf(y2) + 0.5f; }                          // on pixel centres
        float d0 = unif(0.01f, 0.05f), d1 = unif(0.01f, 0.05f), d2 = unif(0.01f, 0.05f);
        float z[4] = {unif(0.0f, 0.06f), unif(0.0f, 0.06f), unif(0.0f, 0.06f), unif(0.0f, 0.06f)};
        if (kind == 1) {               // zero area, exactly, in front of z: two vertices equal / three on a line of whole steps through the pixel centre / all equal
            const int sub = (int)(next() % 3);
            const float dx = (float)((int)(next() % 9) - 4), dy = (float)((int)(next() % 9) - 4);
            if (sub == 0) { x2 = x1; y2 = y1; }
            if (sub == 1) { x0 = cxp - 3.0f * dx; y0 = fy - 3.0f * dy; x1 = cxp + 2.0f * dx; y1 = fy + 2.0f * dy; x2 = cxp + 5.0f * dx; y2 = fy + 5.0f * dy; }
            if (sub == 2) { x0 = cxp; y0 = fy; x1 = cxp; y1 = fy; x2 = cxp; y2 = fy; }
            d0 = d1 = d2 = 0.001f;
            z[0] = z[1] = z[2] = z[3] = 0.05f;
        }
        if (kind == 3) {               // e_k == +-0: an edge through the pixel centre (whole steps: the products are exact), or a vertex on it
            const float dx = (float)((int)(next() % 9) - 4), dy = (float)((int)(next() % 9) - 4);
            const int sub = (int)(next() % 4);
            if (sub == 0) { x0 = cxp - 2.0f * dx; y0 = fy - 2.0f * dy; x1 = cxp + 3.0f * dx; y1 = fy + 3.0f * dy; }
            if (sub == 1) { x1 = cxp - 2.0f * dx; y1 = fy - 2.0f * dy; x2 = cxp + 3.0f * dx; y2 = fy + 3.0f * dy; }
            if (sub == 2) { x0 = cxp; y0 = fy; }
            if (sub == 3) { x1 = cxp; y1 = fy; x2 = cxp + dx; y2 = fy + dy; }
            z[0] = z[1] = z[2] = z[3] = 0.06f;
        }
        if (kind == 5) {               // the bounding box's edge on a pixel centre
            const float w = unif(0.0f, 40.0f), h = unif(1.0f, 40.0f);
            const bool left = (next() & 1ull) != 0;
            x0 = cxp; y0 = fy - h; x1 = left ? cxp + w : cxp - w; y1 = fy + unif(-1.0f, 1.0f); x2 = cxp; y2 = fy + h;
            if (next() & 1ull) { x2 = x1; x1 = cxp; }
            z[0] = z[1] = z[2] = z[3] = 0.06f;
        }
        if (kind == 7) {               // +-inf and NaN coordinates and depths
            const float inf = __uint_as_float(0x7f800000u), nan = __uint_as_float(0x7fc00000u);
            const unsigned long long w = next();
            float* c[9] = {&x0, &y0, &x1, &y1, &x2, &y2, &d0, &d1, &d2};
            const int sub = (int)(w % 4);
            const float v = ((w >> 8) % 3) == 0 ? nan : (((w >> 8) % 3) == 1 ? inf : -inf);
            if (sub == 0) *c[(w >> 16) % 9] = v;
            if (sub == 1) { x0 = v; x1 = v; x2 = v; }
            if (sub == 2) { *c[(w >> 16) % 9] = v; *c[(w >> 24) % 9] = ((w >> 32) & 1ull) ? nan : -v; }
            if (sub == 3) { x0 = ((w >> 16) & 1ull) ? inf : -inf; x1 = ((w >> 17) & 1ull) ? inf : nan; x2 = v; }
        }
        TriRec r;
        r.x0 = x0; r.y0 = y0; r.d0 = d0; r.x1 = x1; r.y1 = y1; r.d1 = d1; r.x2 = x2; r.y2 = y2; r.d2 = d2;
        r.xmin = fminf(r.x0, fminf(r.x1, r.x2)); r.xmax = fmaxf(r.x0, fmaxf(r.x1, r.x2));      // (emit())
        const float a0 = r.y2 - fy, a1 = r.y1 - fy, a2 = r.y0 - fy;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float fx = (float)(qx + p) + 0.5f;
            const float e0 = (r.x1 - fx) * a0 - (r.x2 - fx) * a1;
            const float e1 = (r.x2 - fx) * a2 - (r.x0 - fx) * a0;
            const float e2 = (r.x0 - fx) * a1 - (r.x1 - fx) * a2;
            const float s = (e0 + e1) + e2;
            const float d = div_mid_range((e0 * r.d0 + e1 * r.d1) + e2 * r.d2, s);
            // the chained form, as the other pixel loops have it
            const bool box = (fx >= r.xmin) & (fx <= r.xmax);
            const bool pos = (e0 >= 0.0f) & (e1 >= 0.0f) & (e2 >= 0.0f), neg = (e0 <= 0.0f) & (e1 <= 0.0f) & (e2 <= 0.0f);
            const bool hit_a = box & (pos | neg) & (s != 0.0f) & (d < z[p]);
            const float z_a = hit_a ? d : z[p];
            const bool hit_b = pixel_hit(fx, r.xmin, r.xmax, e0, e1, e2, d, z[p]);
            const float z_b = hit_b ? d : z[p];
            bad += (hit_a != hit_b) | (__float_as_uint(z_a) != __float_as_uint(z_b));
            hits += hit_a;
            // the same two forms without the depth test: z = +inf passes every d that is not NaN (and not +inf)
            const bool cov_a = box & (pos | neg) & (s != 0.0f), cov_b = pixel_hit(fx, r.xmin, r.xmax, e0, e1, e2, 0.0f, 1.0f);
            cov_diff += cov_a != cov_b;
            bad += (cov_a != cov_b) & !(d != d);          // where the booleans differ d must be NaN
            specials += kind & 1;
        }
    }
    if (bad) atomicAdd(out, bad);
    atomicAdd(out + 1, hits);
    atomicAdd(out + 2, cov_diff);
    atomicAdd(out + 3, specials);
}
int selftest_pixel_predicate(long long n, unsigned long long seed, long long* out_host /*[4]*/) {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 32) != hipSuccess) return -1;
    (void)hipMemset(d, 0, 32);
    hipLaunchKernelGGL(k_selftest_pixel_predicate, dim3(2048), dim3(256), 0, 0, n, seed, d);
    const hipError_t e = hipMemcpy(out_host, d, 32, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return e == hipSuccess ? 0 : -1;
}

}  // namespace tg

extern "C" int tg_selftest_pixel_predicate(int64_t n, uint64_t seed, int64_t* out) {
    if (!out || n < 0) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -2;
    long long m[4] = {-1, -1, -1, -1};
    if (tg::selftest_pixel_predicate((long long)n, (unsigned long long)seed, m) != 0) return -3;
    for (int k = 0; k < 4; ++k) out[k] = m[k];
    return 0;
}

extern "C" int tg_selftest_division(int64_t n, uint64_t seed, int64_t* mismatches) {
    if (!mismatches || n < 0) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -2;
    long long m = 0;
    if (tg::selftest_division((long long)n, (unsigned long long)seed, &m) != 0) return -3;
    *mismatches = (int64_t)m;
    return 0;
}

extern "C" int tg_selftest_edge_exclusion(int64_t n, uint64_t seed, int64_t* out) {
    if (!out || n < 0) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -2;
    long long m[6] = {-1, -1, -1, -1, -1, -1};
    if (tg::selftest_edge_exclusion((long long)n, (unsigned long long)seed, m) != 0) return -3;
    for (int k = 0; k < 6; ++k) out[k] = m[k];
    return 0;
}

extern "C" int tg_selftest_penetration_division(int64_t* mismatches) {
    if (!mismatches) return -1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -2;
    long long m = 0;
    if (tg::selftest_penetration_division(&m) != 0) return -3;
    *mismatches = (int64_t)m;
    return 0;
}

// The launch decision of tg_random_translate for a call of that shape and those addresses, by the launcher's own function (tg_augment.h:
// translate_plan).  The argument checks in front of it are tg_random_translate_rows' own predicate (tg_augment_core.h: image_shape_fault).
// Host only.
extern "C" int tg_selftest_translate_plan(int32_t in_dtype, int32_t channels_first, int32_t C, int32_t H, int32_t W, int64_t B, uint64_t in_addr,
                                          uint64_t out_addr, int32_t* path, int32_t* chunks, int32_t* lds_bytes, int64_t* launches) {
    using tg::fail;
    if (!path || !chunks || !lds_bytes || !launches) return fail(-1, "NULL argument");
    if (const char* what = tg::image_shape_fault(in_dtype, B, C, H, W)) return fail(-1, what);
    const tg::TranslatePlan p = tg::translate_plan(in_dtype == TG_AUGMENT_UINT8 ? 1 : 4, channels_first != 0, C, H, W, (uintptr_t)in_addr, (uintptr_t)out_addr);
    if (p.spl < 1) return fail(-1, "one sample has more workgroups than a launch holds");
    *path = p.vec;
    *chunks = p.nchunk;
    *lds_bytes = p.lds_floats * 4;
    *launches = (B + p.spl - 1) / p.spl;
    return 0;
}

// The launch decision of tg_random_affine, by the launcher's own function (tg_affine.h: affine_plan); argument checks as above.  Host only.
extern "C" int tg_selftest_affine_plan(int32_t in_dtype, int32_t channels_first, int32_t C, int32_t H, int32_t W, int64_t B, uint64_t in_addr,
                                       uint64_t out_addr, int32_t* path, int32_t* in_vec, int32_t* chunks, int32_t* lds_bytes, int64_t* launches) {
    using tg::fail;
    if (!path || !in_vec || !chunks || !lds_bytes || !launches) return fail(-1, "NULL argument");
    if (const char* what = tg::image_shape_fault(in_dtype, B, C, H, W)) return fail(-1, what);
    const tg::AffinePlan p = tg::affine_plan(in_dtype == TG_AUGMENT_UINT8 ? 1 : 4, channels_first != 0, C, H, W, (uintptr_t)in_addr, (uintptr_t)out_addr);
    if (p.spl < 1) return fail(-1, "one sample has more workgroups than a launch holds");
    *path = p.path;
    *in_vec = p.in_vec;
    *chunks = p.nchunk;
    *lds_bytes = p.lds_bytes;
    *launches = (B + p.spl - 1) / p.spl;
    return 0;
}
