// tg_physics_test.hip - libtactile_gym_hip_test.so: the device helpers of tg_physics.hpp (and rot_error of tg_kernels.hpp) called one by one on
// caller-supplied cases (tg_selftest_physics).  TEST INFRASTRUCTURE (include/tactile_gym_hip_test.h), not part of the product library; compiled
// with the default contraction (FMA), as tg_api.hip compiles the same headers.  Case i runs in lane i % 64 of the one-wavefront workgroup
// i / 64, so the caller decides which cases vote together in the helpers' __any / __all tests.  tests/physics_cases.py holds the tables,
// tests/physics_ref.py the reference, tests/test_gpu_physics_primitives.py calls it.
#include "../../include/tactile_gym_hip_test.h"
#include "tg_ctx.hpp"        // tg_kernels.hpp (rot_error) -> tg_physics.hpp; fail, DevBuf, need_device

namespace tg {
namespace {

enum {
    OP_QUAT_FROM_EULER = 0, OP_EULER_FROM_QUAT, OP_MAT_FROM_QUAT, OP_QUAT_FROM_MAT, OP_QUAT_MUL, OP_AXIS_ANGLE, OP_ROT_ERROR, OP_PLANE_SPACE,
    OP_TRSQRT, OP_TRCP, OP_TSQRT_FAST, OP_INVERSE_S3, OP_FRICTION_CLAMP, OP_SINCOS_SMALL, OP_TRIG_ADVANCE, OP_INTEGRATE_ROTATION,
    OP_SOLVE6, OP_SOLVE8, OP_PINV8,
    OP_PGS_UNCLAMPED6, OP_PGS_BLOCKS6, OP_PGS_CLAMPED6, OP_PGS_THRESHOLD6,
    OP_PGS_UNCLAMPED8, OP_PGS_BLOCKS8, OP_PGS_CLAMPED8, OP_PGS_THRESHOLD8,
    OP_COUNT
};
constexpr int kTrigN = 6, kTrigMaxK = 24, kRotMaxK = 240;
// widths of a case and of its result, in doubles; uniform >= 0: the input column that must be equal in the 64 lanes of a wavefront (a
// loop count around a wave vote)
struct OpShape { int in_w, out_w, uniform; };
constexpr OpShape kShape[OP_COUNT] = {
    {3, 4, -1}, {4, 3, -1}, {4, 9, -1}, {9, 4, -1}, {8, 4, -1}, {4, 9, -1}, {18, 3, -1}, {3, 6, -1},
    {1, 1, -1}, {1, 1, -1}, {1, 1, -1}, {6, 6, -1}, {4, 2, -1}, {1, 2, -1},
    {1 + kTrigN + kTrigMaxK * kTrigN, 3 * kTrigN, 0},   // k, q[6], dq[24][6] -> s[6], c[6], q[6]
    {14, 9, 0},                                          // k, R[9], w[3], dt -> R[9]
    {42, 6, -1}, {72, 8, -1}, {54, 8, -1},
    {51, 7, 48}, {51, 7, 48}, {51, 7, 48}, {51, 7, 48},  // Minv[N][N], rimp[N], jdi[N], iters, maximp, res_thr -> dv[N], the integer result
    {83, 9, 80}, {83, 9, 80}, {83, 9, 80}, {83, 9, 80},
};

template <typename T, int N, int KIND> __device__ __forceinline__ void run_pgs(const double* __restrict__ in, double* __restrict__ out) {
    T Minv[N][N], rimp[N], jdi[N], dv[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) Minv[r][c] = (T)in[r * N + c];
        rimp[r] = (T)in[N * N + r];
        jdi[r] = (T)in[N * N + N + r];
        dv[r] = T(0);
    }
    const int iters = (int)in[N * N + 2 * N];
    const T maximp = (T)in[N * N + 2 * N + 1], res_thr = (T)in[N * N + 2 * N + 2];
    int ret = 0;
    if (KIND == 0) ret = pgs_unclamped<T, N>(Minv, rimp, jdi, iters, dv);
    else if (KIND == 1) ret = pgs_unclamped_blocks<T, N>(Minv, rimp, jdi, iters, dv);
    else if (KIND == 2) pgs_clamped<T, N>(Minv, rimp, jdi, maximp, iters, dv);
    else ret = pgs_threshold<T, N>(Minv, rimp, jdi, maximp, iters, res_thr, dv);
#pragma unroll
    for (int r = 0; r < N; ++r) out[r] = (double)dv[r];
    out[N] = (double)ret;
}

template <typename T, int N> __device__ __forceinline__ void run_solve(const double* __restrict__ in, double* __restrict__ out) {
    T A[N][N], b[N], x[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
#pragma unroll
        for (int c = 0; c < N; ++c) A[r][c] = (T)in[r * N + c];
        b[r] = (T)in[N * N + r];
        x[r] = T(0);
    }
    solve_pivoted<T, N>(A, b, x);
#pragma unroll
    for (int r = 0; r < N; ++r) out[r] = (double)x[r];
}

template <typename T, int OP> __global__ __launch_bounds__(64) void k_physics_test(const double* __restrict__ in_all, double* __restrict__ out_all) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const double* __restrict__ in = in_all + i * kShape[OP].in_w;
    double* __restrict__ out = out_all + i * kShape[OP].out_w;
    if constexpr (OP == OP_QUAT_FROM_EULER) {
        const Q4<T> q = quat_from_euler<T>((T)in[0], (T)in[1], (T)in[2]);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else if constexpr (OP == OP_EULER_FROM_QUAT) {
        T r, p, y;
        euler_from_quat<T>(Q4<T>{(T)in[0], (T)in[1], (T)in[2], (T)in[3]}, r, p, y);
        out[0] = r; out[1] = p; out[2] = y;
    } else if constexpr (OP == OP_MAT_FROM_QUAT) {
        const M3<T> R = mat_from_quat<T>(Q4<T>{(T)in[0], (T)in[1], (T)in[2], (T)in[3]});
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = R.m[k];
    } else if constexpr (OP == OP_QUAT_FROM_MAT) {
        M3<T> R;
#pragma unroll
        for (int k = 0; k < 9; ++k) R.m[k] = (T)in[k];
        const Q4<T> q = quat_from_mat<T>(R);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else if constexpr (OP == OP_QUAT_MUL) {
        const Q4<T> q = quat_mul<T>(Q4<T>{(T)in[0], (T)in[1], (T)in[2], (T)in[3]}, Q4<T>{(T)in[4], (T)in[5], (T)in[6], (T)in[7]});
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else if constexpr (OP == OP_AXIS_ANGLE) {
        const M3<T> R = axis_angle<T>(mk<T>((T)in[0], (T)in[1], (T)in[2]), (T)in[3]);
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = R.m[k];
    } else if constexpr (OP == OP_ROT_ERROR) {
        M3<T> Rt, R;
#pragma unroll
        for (int k = 0; k < 9; ++k) { Rt.m[k] = (T)in[k]; R.m[k] = (T)in[9 + k]; }
        const V3<T> e = rot_error<T>(Rt, R);
        out[0] = e.x; out[1] = e.y; out[2] = e.z;
    } else if constexpr (OP == OP_PLANE_SPACE) {
        V3<T> t1, t2;
        plane_space<T>(mk<T>((T)in[0], (T)in[1], (T)in[2]), t1, t2);
        out[0] = t1.x; out[1] = t1.y; out[2] = t1.z; out[3] = t2.x; out[4] = t2.y; out[5] = t2.z;
    } else if constexpr (OP == OP_TRSQRT) {
        out[0] = trsqrt((T)in[0]);
    } else if constexpr (OP == OP_TRCP) {
        out[0] = trcp((T)in[0]);
    } else if constexpr (OP == OP_TSQRT_FAST) {
        out[0] = tsqrt_fast<T>((T)in[0]);
    } else if constexpr (OP == OP_INVERSE_S3) {
        const S3<T> B = inverse<T>(S3<T>{(T)in[0], (T)in[1], (T)in[2], (T)in[3], (T)in[4], (T)in[5]});
        out[0] = B.xx; out[1] = B.xy; out[2] = B.xz; out[3] = B.yy; out[4] = B.yz; out[5] = B.zz;
    } else if constexpr (OP == OP_FRICTION_CLAMP) {
        T s1 = (T)in[0], s2 = (T)in[1];
        friction_clamp<T>(s1, s2, (T)in[2], in[3] != 0.0);
        out[0] = s1; out[1] = s2;
    } else if constexpr (OP == OP_SINCOS_SMALL) {
        T s, c;
        sincos_small<T>((T)in[0], &s, &c);
        out[0] = s; out[1] = c;
    } else if constexpr (OP == OP_TRIG_ADVANCE) {
        const int k = (int)in[0];                      // equal in the wavefront's lanes (checked on the host)
        T q[kTrigN];
#pragma unroll
        for (int j = 0; j < kTrigN; ++j) q[j] = (T)in[1 + j];
        JointTrig<T, kTrigN> t;
        trig_init<T, kTrigN>(q, t);
        for (int step = 0; step < k; ++step) {
            T dq[kTrigN];
#pragma unroll
            for (int j = 0; j < kTrigN; ++j) { dq[j] = (T)in[1 + kTrigN + step * kTrigN + j]; q[j] += dq[j]; }   // as sim_tick: q += dq, then the pair
            trig_advance<T, kTrigN>(q, dq, t);
        }
#pragma unroll
        for (int j = 0; j < kTrigN; ++j) { out[j] = t.s[j]; out[kTrigN + j] = t.c[j]; out[2 * kTrigN + j] = q[j]; }
    } else if constexpr (OP == OP_INTEGRATE_ROTATION) {
        const int k = (int)in[0];
        M3<T> R;
#pragma unroll
        for (int j = 0; j < 9; ++j) R.m[j] = (T)in[1 + j];
        const V3<T> w = mk<T>((T)in[10], (T)in[11], (T)in[12]);
        const T dt = (T)in[13];
        for (int step = 0; step < k; ++step) integrate_rotation<T>(R, w, dt);
#pragma unroll
        for (int j = 0; j < 9; ++j) out[j] = R.m[j];
    } else if constexpr (OP == OP_SOLVE6) {
        run_solve<T, 6>(in, out);
    } else if constexpr (OP == OP_SOLVE8) {
        run_solve<T, 8>(in, out);
    } else if constexpr (OP == OP_PINV8) {
        T J[6][8], b[6], x[8];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 8; ++c) J[r][c] = (T)in[r * 8 + c];
            b[r] = (T)in[48 + r];
        }
        pinv_apply<T, 8>(J, b, x);
#pragma unroll
        for (int c = 0; c < 8; ++c) out[c] = (double)x[c];
    } else if constexpr (OP >= OP_PGS_UNCLAMPED6 && OP <= OP_PGS_THRESHOLD6) {
        run_pgs<T, 6, OP - OP_PGS_UNCLAMPED6>(in, out);
    } else {
        run_pgs<T, 8, OP - OP_PGS_UNCLAMPED8>(in, out);
    }
}

template <typename T, int OP = 0> void launch_physics_test(int op, int n, const double* in, double* out) {
    if constexpr (OP < OP_COUNT) {
        if (op == OP) k_physics_test<T, OP><<<dim3(n / 64), dim3(64)>>>(in, out);
        else launch_physics_test<T, OP + 1>(op, n, in, out);
    }
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int tg_selftest_physics(int32_t op, int32_t dtype, int32_t n, int32_t in_w, const double* in, int32_t out_w, double* out) {
    if (op < 0 || op >= OP_COUNT) return fail(-1, "unknown op");
    if (dtype != 0 && dtype != 1) return fail(-1, "unknown dtype (0: double, 1: float)");
    if (!in || !out) return fail(-1, "NULL argument");
    if (n < 64 || n % 64) return fail(-1, "n must be a positive multiple of 64: every lane of a wavefront holds a case");
    const OpShape sh = kShape[op];
    if (in_w != sh.in_w || out_w != sh.out_w) return fail(-1, "the op expects other widths");
    if (sh.uniform >= 0) {
        const int cap = op == OP_TRIG_ADVANCE ? kTrigMaxK : (op == OP_INTEGRATE_ROTATION ? kRotMaxK : 1024);
        for (int i = 0; i < n; ++i) {
            const double k = in[(size_t)i * in_w + sh.uniform];
            if (!(k >= -cap && k <= cap) || k != (double)(int)k || (k < 0 && op <= OP_INTEGRATE_ROTATION)) return fail(-1, "loop count out of range");
            if (k != in[(size_t)(i - i % 64) * in_w + sh.uniform]) return fail(-1, "the loop count must be equal in the lanes of a wavefront");
        }
    }
    if (int rc = need_device()) return rc;
    DevBuf din, dout;
    const size_t ib = (size_t)n * in_w * sizeof(double), ob = (size_t)n * out_w * sizeof(double);
    if (din.alloc(ib) || dout.alloc(ob)) return fail(-2, "hipMalloc failed");
    TG_HIP(hipMemcpy(din.p, in, ib, hipMemcpyHostToDevice));
    TG_HIP(hipMemset(dout.p, 0, ob));
    if (dtype == 0) launch_physics_test<double>(op, n, (const double*)din.p, (double*)dout.p);
    else launch_physics_test<float>(op, n, (const double*)din.p, (double*)dout.p);
    if (hipGetLastError() != hipSuccess) return fail(-3, "launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail(-3, "kernel failed");
    TG_HIP(hipMemcpy(out, dout.p, ob, hipMemcpyDeviceToHost));
    return 0;
}
