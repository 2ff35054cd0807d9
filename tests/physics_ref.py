"""Plain numpy restatement of the device helpers of csrc/tg_physics.hpp and of rot_error (csrc/tg_kernels.hpp).  TEST INFRASTRUCTURE, not
collected by pytest: tests/test_physics_cases_cpu.py and tests/test_gpu_physics_primitives.py import it.

Every function takes a batch of cases X [n][in_w] (the layout of tg_selftest_physics, include/tactile_gym_hip_test.h), a working dtype `dt`
and the kernel's dtype `T`, and returns [n][out_w] in `dt`:
  dt = np.longdouble (80-bit on x86, eps 1.08e-19) is THE REFERENCE;
  dt = T (np.float64 / np.float32) is "the plain restatement in T": the same text evaluated in the kernel's own number format, which the
  CPU test holds to half the kernel's margin and which measures the iterative solvers' e_T.
`T` only rounds the literals the header writes as T(...), e.g. the 1e-30 of tsqrt_fast, which differs between float and double.

Where Bullet or PyBullet fixes the rule the restatement follows it: the branch thresholds (0.99999, 1/sqrt 2, 0.001, the tie rules of
btMatrix3x3::getRotation), the Gram-Schmidt step after the exponential map, the literal dv-form Gauss-Seidel with reverse row order on even
sweeps.  What the kernels do differently on purpose is NOT restated: the Taylor pairs (exact sin / cos here), the seed + Newton reciprocals
(exact division here), the residual form and the P^4 blocks of the motor solver (sweep by sweep here), the one-sided Jacobi SVD (np.linalg.pinv
is the reference of pinv_apply; the Jacobi loop is restated only as `pinv_jacobi`, to measure e_T).
"""
import numpy as np

LD = np.longdouble
OPS = ["quat_from_euler", "euler_from_quat", "mat_from_quat", "quat_from_mat", "quat_mul", "axis_angle", "rot_error", "plane_space",
       "trsqrt", "trcp", "tsqrt_fast", "inverse_s3", "friction_clamp", "sincos_small", "trig_advance", "integrate_rotation",
       "solve6", "solve8", "pinv8",
       "pgs_unclamped6", "pgs_blocks6", "pgs_clamped6", "pgs_threshold6", "pgs_unclamped8", "pgs_blocks8", "pgs_clamped8", "pgs_threshold8"]
OP_ID = {name: i for i, name in enumerate(OPS)}
TRIG_N, TRIG_MAX_K = 6, 24
#        in_w, out_w
SHAPE = {"quat_from_euler": (3, 4), "euler_from_quat": (4, 3), "mat_from_quat": (4, 9), "quat_from_mat": (9, 4), "quat_mul": (8, 4),
         "axis_angle": (4, 9), "rot_error": (18, 3), "plane_space": (3, 6), "trsqrt": (1, 1), "trcp": (1, 1), "tsqrt_fast": (1, 1),
         "inverse_s3": (6, 6), "friction_clamp": (4, 2), "sincos_small": (1, 2), "trig_advance": (1 + TRIG_N + TRIG_MAX_K * TRIG_N, 3 * TRIG_N),
         "integrate_rotation": (14, 9), "solve6": (42, 6), "solve8": (72, 8), "pinv8": (54, 8)}
for _n in (6, 8):
    for _k in ("unclamped", "blocks", "clamped", "threshold"):
        SHAPE[f"pgs_{_k}{_n}"] = (_n * _n + 2 * _n + 3, _n + 1)
# input columns that are counts or flags: never moved by the conditioning rule
FIXED = {"friction_clamp": [3], "trig_advance": [0], "integrate_rotation": [0]}
for _n in (6, 8):
    for _k in ("unclamped", "blocks", "clamped", "threshold"):
        FIXED[f"pgs_{_k}{_n}"] = [_n * _n + 2 * _n, _n * _n + 2 * _n + 1, _n * _n + 2 * _n + 2]


def eps(T):
    return float(np.finfo(T).eps)


def _k(v, dt, T):
    """The literal T(v) of the header, in the working dtype."""
    return dt(T(v))


def _cols(X):
    return [X[:, j] for j in range(X.shape[1])]


# ------------------------------------------------------------------------------------------------ rotation helpers
def quat_from_euler(X, dt, T):
    r, p, y = _cols(X)
    h = dt(0.5)
    sr, cr, sp, cp, sy, cy = np.sin(h * r), np.cos(h * r), np.sin(h * p), np.cos(h * p), np.sin(h * y), np.cos(h * y)
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=1)
    return q / np.sqrt((q * q).sum(axis=1, dtype=dt))[:, None]


def euler_sarg(X, dt):
    x, y, z, w = _cols(X)
    return dt(-2) * (x * z - w * y)


def euler_from_quat(X, dt, T):
    x, y, z, w = _cols(X)
    sqx, sqy, sqz, sqw = x * x, y * y, z * z, w * w
    sarg = dt(-2) * (x * z - w * y)
    half_pi = np.arccos(dt(0)) if dt is LD else dt(1.5707963267948966)
    lo, hi = sarg <= _k(-0.99999, dt, T), sarg >= _k(0.99999, dt, T)
    r = np.arctan2(dt(2) * (y * z + w * x), sqw - sqx - sqy + sqz)
    p = np.arcsin(np.clip(sarg, dt(-1), dt(1)))
    yy = np.arctan2(dt(2) * (x * y + w * z), sqw + sqx - sqy - sqz)
    zero = np.zeros_like(r)
    r = np.where(lo | hi, zero, r)
    p = np.where(lo, -half_pi, np.where(hi, half_pi, p))
    yy = np.where(lo, dt(2) * np.arctan2(x, -y), np.where(hi, dt(2) * np.arctan2(-x, y), yy))
    return np.stack([r, p, yy], axis=1)


def mat_from_quat(X, dt, T):
    x, y, z, w = _cols(X)
    d = x * x + y * y + z * z + w * w
    s = dt(2) / d
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz, xx, xy, xz, yy, yz, zz = w * xs, w * ys, w * zs, x * xs, x * ys, x * zs, y * ys, y * zs, z * zs
    one = dt(1)
    return np.stack([one - (yy + zz), xy - wz, xz + wy, xy + wz, one - (xx + zz), yz - wx, xz - wy, yz + wx, one - (xx + yy)], axis=1)


def quat_from_mat_branch(X):
    """0: trace > 0; 1, 2, 3: the largest diagonal element is R00, R11, R22 by btMatrix3x3::getRotation's tie rules."""
    R = X.reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    i = np.where(R[:, 0, 0] >= R[:, 1, 1], 0, 1)
    i = np.where(R[:, 2, 2] > R[np.arange(len(R)), i, i], 2, i)
    return np.where(tr > 0, 0, i + 1)


def quat_from_mat(X, dt, T):
    R = X.reshape(-1, 3, 3)
    n = len(R)
    br = quat_from_mat_branch(X)
    q = np.zeros((n, 4), dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] + dt(1))
        s2 = dt(0.5) / s
        q0 = np.stack([(R[:, 2, 1] - R[:, 1, 2]) * s2, (R[:, 0, 2] - R[:, 2, 0]) * s2, (R[:, 1, 0] - R[:, 0, 1]) * s2, dt(0.5) * s], axis=1)
        q[br == 0] = q0[br == 0]
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            s = np.sqrt(R[:, i, i] - R[:, j, j] - R[:, k, k] + dt(1))
            s2 = dt(0.5) / s
            qi = np.zeros((n, 4), dtype=dt)
            qi[:, i] = dt(0.5) * s
            qi[:, 3] = (R[:, k, j] - R[:, j, k]) * s2
            qi[:, j] = (R[:, j, i] + R[:, i, j]) * s2
            qi[:, k] = (R[:, k, i] + R[:, i, k]) * s2
            q[br == i + 1] = qi[br == i + 1]
    return q


def quat_mul(X, dt, T):
    ax, ay, az, aw, bx, by, bz, bw = _cols(X)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], axis=1)


def axis_angle(X, dt, T):
    ax, ay, az, q = _cols(X)
    s, c = np.sin(q), np.cos(q)
    v = dt(1) - c
    return np.stack([c + ax * ax * v, ax * ay * v - az * s, ax * az * v + ay * s, ay * ax * v + az * s, c + ay * ay * v, ay * az * v - ax * s,
                     az * ax * v - ay * s, az * ay * v + ax * s, c + az * az * v], axis=1)


def rot_error(X, dt, T):
    """Rotation vector of Rt R^T: axis from the skew part (norm 2 sin), angle by atan2; below s = 1e-12 the small-angle form 0.5 * ax."""
    Rt, R = X[:, :9].reshape(-1, 3, 3), X[:, 9:].reshape(-1, 3, 3)
    E = np.einsum("nik,njk->nij", Rt, R)
    cosang = dt(0.5) * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - dt(1))
    ax = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)
    s = np.sqrt((ax * ax).sum(axis=1))
    ang = np.arctan2(dt(0.5) * s, cosang)
    small = s < _k(1e-12, dt, T)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(small, dt(0.5), ang / np.where(small, dt(1), s))
    return f[:, None] * ax


def plane_space(X, dt, T):
    """btPlaneSpace1."""
    nx, ny, nz = _cols(X)
    up = np.abs(nz) > _k(0.7071067811865475244, dt, T)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = ny * ny + nz * nz
        k = dt(1) / np.sqrt(a)
        t1a = np.stack([np.zeros_like(nx), -nz * k, ny * k], axis=1)
        t2a = np.stack([a * k, -nx * t1a[:, 2], nx * t1a[:, 1]], axis=1)
        b = nx * nx + ny * ny
        kb = dt(1) / np.sqrt(b)
        t1b = np.stack([-ny * kb, nx * kb, np.zeros_like(nx)], axis=1)
        t2b = np.stack([-nz * t1b[:, 1], nz * t1b[:, 0], b * kb], axis=1)
    return np.where(up[:, None], np.concatenate([t1a, t2a], axis=1), np.concatenate([t1b, t2b], axis=1))


# ------------------------------------------------------------------------------------------------ fast arithmetic
def trsqrt(X, dt, T):
    return dt(1) / np.sqrt(X)


def trcp(X, dt, T):
    return dt(1) / X


def tsqrt_fast(X, dt, T):
    """x / sqrt(max(x, T(1e-30))): sqrt(x) from 1e-30 up, 0 at 0, x * 1e15 between (the header's clamp, part of the function)."""
    return X / np.sqrt(np.maximum(X, _k(1e-30, dt, T)))


def inverse_s3(X, dt, T):
    xx, xy, xz, yy, yz, zz = _cols(X)
    c00, c01, c02 = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    det = xx * c00 + xy * c01 + xz * c02
    return np.stack([c00, c01, c02, xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy], axis=1) / det[:, None]


def friction_clamp(X, dt, T):
    s1, s2, lim, cone = _cols(X)
    tot2 = s1 * s1 + s2 * s2
    over = tot2 > lim * lim
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(over, lim / np.sqrt(np.where(over, tot2, dt(1))), dt(1))
    p1, p2 = np.minimum(np.maximum(s1, -lim), lim), np.minimum(np.maximum(s2, -lim), lim)
    c = cone != 0
    return np.stack([np.where(c, s1 * f, p1), np.where(c, s2 * f, p2)], axis=1)


# ------------------------------------------------------------------------------------------------ small-angle trigonometry
def sincos_small(X, dt, T):
    return np.stack([np.sin(X[:, 0]), np.cos(X[:, 0])], axis=1)


def trig_q(X, T):
    """q after the k additions q += dq in T, as sim_tick forms it: [n][6] in T (plain IEEE additions, the kernel's own bits)."""
    k = X[:, 0].astype(int)
    q = X[:, 1:1 + TRIG_N].astype(T)
    dq = X[:, 1 + TRIG_N:].astype(T).reshape(-1, TRIG_MAX_K, TRIG_N)
    for step in range(TRIG_MAX_K):
        q = np.where((step < k)[:, None], (q + dq[:, step]).astype(T), q)
    return q


def trig_advance(X, dt, T):
    """sin / cos of the angle the recurrence stands for: the anchor q0 plus the exact sum of the dq since - or, once some lane of the case's
    wavefront (64 consecutive cases) has held |dq| > 0.02 in a step, the q that step re-anchored on (q as accumulated in T) plus the dq since."""
    n = len(X)
    k = X[:, 0].astype(int)
    dq = X[:, 1 + TRIG_N:].reshape(-1, TRIG_MAX_K, TRIG_N)
    qT = X[:, 1:1 + TRIG_N].astype(T)
    ang = X[:, 1:1 + TRIG_N].astype(dt)
    for step in range(TRIG_MAX_K):
        on = step < k
        dT = dq[:, step].astype(T)
        qT = np.where(on[:, None], (qT + dT).astype(T), qT)
        big = (np.abs(dT).max(axis=1) > T(0.02)) & on
        anchor = np.repeat(big.reshape(-1, 64).any(axis=1), 64) & on if n % 64 == 0 else big
        ang = np.where(anchor[:, None], qT.astype(dt), np.where(on[:, None], ang + dT.astype(dt), ang))
    return np.concatenate([np.sin(ang), np.cos(ang), qT.astype(dt)], axis=1)


def trig_recurrence(X, dt, T):
    """The recurrence itself (degree-7/6 Taylor pair, angle addition) in dt - the plain restatement of trig_advance."""
    n = len(X)
    k = X[:, 0].astype(int)
    dq = X[:, 1 + TRIG_N:].reshape(-1, TRIG_MAX_K, TRIG_N)
    qT = X[:, 1:1 + TRIG_N].astype(T)
    s, c = np.sin(qT.astype(dt)), np.cos(qT.astype(dt))
    for step in range(TRIG_MAX_K):
        on = (step < k)[:, None]
        dT = dq[:, step].astype(T)
        qT = np.where(on, (qT + dT).astype(T), qT)
        big = (np.abs(dT).max(axis=1) > T(0.02)) & on[:, 0]
        anchor = (np.repeat(big.reshape(-1, 64).any(axis=1), 64) & on[:, 0])[:, None]
        d = dT.astype(dt)
        d2 = d * d
        cd = dt(1) + d2 * (dt(-0.5) + d2 * (dt(T(1.0 / 24.0)) + d2 * dt(T(-1.0 / 720.0))))
        sd = d * (dt(1) + d2 * (dt(T(-1.0 / 6.0)) + d2 * (dt(T(1.0 / 120.0)) + d2 * dt(T(-1.0 / 5040.0)))))
        s1, c1 = s * cd + c * sd, c * cd - s * sd
        s = np.where(anchor, np.sin(qT.astype(dt)), np.where(on, s1, s))
        c = np.where(anchor, np.cos(qT.astype(dt)), np.where(on, c1, c))
    return np.concatenate([s, c, qT.astype(dt)], axis=1)


def integrate_rotation(X, dt, T):
    """k ticks of btTransformUtil::integrateTransform's orientation part on a rotation matrix: exponential map with Bullet's small-angle branch
    (|w| < 0.001: k = dt/2 - dt^3 / 48 |w|^2), the quaternion normalised, then Gram-Schmidt on the columns (c0, c1; c2 = c0 x c1)."""
    kk = X[:, 0].astype(int)
    R = X[:, 1:10].reshape(-1, 3, 3).astype(dt)
    w = X[:, 10:13]
    h = X[:, 13]
    ang = np.sqrt((w * w).sum(axis=1))
    half = ang * h * dt(0.5)
    small = ang < _k(0.001, dt, T)
    with np.errstate(invalid="ignore", divide="ignore"):
        kf = np.where(small, dt(0.5) * h - (h * h * h) * _k(0.020833333333, dt, T) * ang * ang, np.sin(half) / np.where(small, dt(1), ang))
    a = kf[:, None] * w
    qw = np.cos(half)
    nrm = dt(1) / np.sqrt((a * a).sum(axis=1) + qw * qw)
    x, y, z, ww = a[:, 0] * nrm, a[:, 1] * nrm, a[:, 2] * nrm, qw * nrm
    one, two = dt(1), dt(2)
    dR = np.stack([one - two * (y * y + z * z), two * (x * y - z * ww), two * (x * z + y * ww), two * (x * y + z * ww), one - two * (x * x + z * z),
                   two * (y * z - x * ww), two * (x * z - y * ww), two * (y * z + x * ww), one - two * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    for step in range(int(kk.max()) if len(kk) else 0):
        Rn = np.einsum("nij,njk->nik", dR, R)
        c0, c1 = Rn[:, :, 0], Rn[:, :, 1]
        c0 = c0 / np.sqrt((c0 * c0).sum(axis=1))[:, None]
        c1 = c1 - (c0 * c1).sum(axis=1)[:, None] * c0
        c1 = c1 / np.sqrt((c1 * c1).sum(axis=1))[:, None]
        c2 = np.cross(c0, c1)
        R = np.where((step < kk)[:, None, None], np.stack([c0, c1, c2], axis=2), R)
    return R.reshape(-1, 9)


# ------------------------------------------------------------------------------------------------ small solves
def solve_gauss(A, b, dt, log=None):
    """Gaussian elimination with partial pivoting, batched; a pivot that is exactly zero eliminates nothing and its unknown is 0 (the
    kernel's rule).  On a regular system this is np.linalg.solve (the CPU test compares them).  log (a list) receives per column
    (rows were exchanged [n], the pivot is exactly zero [n])."""
    A, b = A.astype(dt).copy(), b.astype(dt).copy()
    n, N = A.shape[0], A.shape[1]
    for c in range(N):
        swapped = np.zeros(n, bool)
        for r in range(c + 1, N):      # the kernel's conditional swaps, row by row: the same rows end up in the same places
            sw = np.abs(A[:, r, c]) > np.abs(A[:, c, c])
            swapped |= sw
            Ac, Ar = A[:, c].copy(), A[:, r].copy()
            A[:, c], A[:, r] = np.where(sw[:, None], Ar, Ac), np.where(sw[:, None], Ac, Ar)
            bc, br = b[:, c].copy(), b[:, r].copy()
            b[:, c], b[:, r] = np.where(sw, br, bc), np.where(sw, bc, br)
        piv = A[:, c, c]
        if log is not None:
            log.append((swapped, piv == 0))
        with np.errstate(invalid="ignore", divide="ignore"):
            inv = np.where(piv != 0, dt(1) / np.where(piv != 0, piv, dt(1)), dt(0))
        for r in range(c + 1, N):
            f = A[:, r, c] * inv
            A[:, r, c + 1:] -= f[:, None] * A[:, c, c + 1:]
            b[:, r] -= f * b[:, c]
    x = np.zeros((n, N), dtype=dt)
    for r in range(N - 1, -1, -1):
        s = b[:, r] - (A[:, r, r + 1:] * x[:, r + 1:]).sum(axis=1)
        piv = A[:, r, r]
        x[:, r] = np.where(piv != 0, s / np.where(piv != 0, piv, dt(1)), dt(0))
    return x


def _solve(N):
    def f(X, dt, T):
        return solve_gauss(X[:, :N * N].reshape(-1, N, N), X[:, N * N:], dt)
    return f


solve6, solve8 = _solve(6), _solve(8)


def pinv8(X, dt, T):
    """np.linalg.pinv(J, rcond=1e-15) @ b in float64 (mg400.py:105-107), whatever dt: THE reference of pinv_apply."""
    J = X[:, :48].reshape(-1, 6, 8).astype(np.float64)
    b = X[:, 48:].astype(np.float64)
    return np.stack([np.linalg.pinv(J[i], rcond=1e-15) @ b[i] for i in range(len(J))]).astype(dt) if len(J) else np.zeros((0, 8), dt)


def pinv_jacobi(X, dt, T, sweeps=10):
    """The plain restatement of pinv_apply in dt: one-sided (Hestenes) Jacobi on the rows, ten sweeps, the rotation skip test, the cut at
    s2 > 1e-30 s2max."""
    A = X[:, :48].reshape(-1, 6, 8).astype(dt).copy()
    b = X[:, 48:].astype(dt)
    n = len(A)
    U = np.tile(np.eye(6, dtype=dt), (n, 1, 1))
    one = dt(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for _ in range(sweeps):
            for p in range(5):
                for q in range(p + 1, 6):
                    al, be, ga = (A[:, p] * A[:, p]).sum(axis=1), (A[:, q] * A[:, q]).sum(axis=1), (A[:, p] * A[:, q]).sum(axis=1)
                    rot = (np.abs(ga) > _k(1e-300, dt, T)) & (ga * ga > (al * be) * _k(1e-32, dt, T))
                    zeta = np.where(rot, (be - al) / np.where(rot, dt(2) * ga, one), dt(0))
                    tt = np.where(rot, np.where(zeta >= 0, one, -one) / (np.abs(zeta) + np.sqrt(one + zeta * zeta)), dt(0))
                    cs = one / np.sqrt(one + tt * tt)
                    sn = cs * tt
                    for M in (A, U):
                        mp, mq = M[:, p].copy(), M[:, q].copy()
                        M[:, p] = cs[:, None] * mp - sn[:, None] * mq
                        M[:, q] = sn[:, None] * mp + cs[:, None] * mq
        s2 = (A * A).sum(axis=2)
        ub = np.einsum("nrc,nc->nr", U, b)
        keep = s2 > s2.max(axis=1)[:, None] * _k(1e-30, dt, T)
        wgt = np.where(keep, ub / np.where(keep, s2, one), dt(0))
    return np.einsum("nrc,nr->nc", A, wgt)


# ------------------------------------------------------------------------------------------------ motor solver
def _pgs_unpack(X, N, dt):
    Minv = X[:, :N * N].reshape(-1, N, N).astype(dt)
    rimp, jdi = X[:, N * N:N * N + N].astype(dt), X[:, N * N + N:N * N + 2 * N].astype(dt)
    iters = X[:, N * N + 2 * N].astype(int)
    return Minv, rimp, jdi, iters, X[:, N * N + 2 * N + 1].astype(dt), X[:, N * N + 2 * N + 2].astype(dt)


def pgs_literal(X, N, dt, n_sweeps, clamp, threshold=False):
    """btMultiBodyConstraintSolver's row update on the motor rows, literally, in dv form: delta = rhs_i - dv_i jdi_i; the accumulated impulse
    clamped to +-maximp when `clamp`; dv += Minv[:, i] delta.  Sweep s (from 0) runs the rows in reverse order when s is even.  n_sweeps [n]
    per case.  threshold: a case stops after the sweep whose largest squared (delta Minv_ii) is <= res_thr.  Returns dv, the sweeps run, the
    residual of each sweep [n][max sweeps] (nan where a case no longer ran) and the accumulated impulses."""
    Minv, rimp, jdi, _, maximp, res_thr = _pgs_unpack(X, N, dt)
    n = len(X)
    dv, lam = np.zeros((n, N), dt), np.zeros((n, N), dt)
    live = n_sweeps > 0
    ran = np.zeros(n, int)
    S = int(n_sweeps.max()) if n else 0
    resid = np.full((n, S), np.nan)
    for s in range(S):
        live = live & (s < n_sweeps)
        res = np.zeros(n, dt)
        for i in (range(N - 1, -1, -1) if s % 2 == 0 else range(N)):
            t = rimp[:, i] - dv[:, i] * jdi[:, i]
            tot = lam[:, i] + t
            sc = np.minimum(np.maximum(tot, -maximp), maximp) if clamp else tot
            delta = np.where(live, np.where(sc == tot, t, sc - lam[:, i]), dt(0))
            lam[:, i] = np.where(live, sc, lam[:, i])
            dv += Minv[:, :, i] * delta[:, None]
            dvel = delta * Minv[:, i, i]
            res = np.maximum(res, dvel * dvel)
        ran += live
        resid[live, s] = res[live].astype(np.float64)
        if threshold:
            live = live & ~(res <= res_thr)
    return dv, ran, resid, lam


def pgs_residual_form(X, N, dt, n_sweeps):
    """max_j |r_j| after every sweep of the unclamped iteration in the residual form r_j = rimp_j - dv_j jdi_j (the quantity the kernels' exit
    tests read): [n][max sweeps + 1], column s = after s sweeps."""
    Minv, rimp, jdi, _, _, _ = _pgs_unpack(X, N, dt)
    G = Minv * jdi[:, :, None]
    r = rimp.copy()
    S = int(n_sweeps.max()) if len(X) else 0
    out = np.zeros((len(X), S + 1), dt)
    out[:, 0] = np.abs(r).max(axis=1)
    for s in range(S):
        for i in (range(N - 1, -1, -1) if s % 2 == 0 else range(N)):
            r = r - G[:, :, i] * r[:, i][:, None]
        out[:, s + 1] = np.abs(r).max(axis=1)
    return out


def pgs_exit_thr(X, N, T):
    _, rimp, _, _, _, _ = _pgs_unpack(X, N, LD)
    return np.abs(rimp).max(axis=1) * LD(2.0 ** -56 if T is np.float64 else 2.0 ** -27)


def pgs_exit_checks(kind, iters):
    """The sweep counts after which the kernel tests its exit: pgs_unclamped after every block of four sweeps that fits; pgs_unclamped_blocks
    after its lead pairs + every block of eight."""
    if iters < 0:
        return []
    if kind == "unclamped":
        return list(range(4, iters + 1, 4))
    pairs = iters // 2
    return [2 * (pairs & 3) + 8 * (b + 1) for b in range(pairs >> 2)]


def pgs_exit(kind, X, N, T, margin=None):
    """The kernels' integer result: the first check (pgs_exit_checks) at which every case of the wavefront (64 consecutive cases) has
    max|r| <= thr, or -1.  margin (a list) receives, for every check of every wavefront, the factor between max|r| and thr of every case."""
    iters = _pgs_unpack(X, N, LD)[3]
    res = pgs_residual_form(X, N, LD, np.abs(iters))
    thr = pgs_exit_thr(X, N, T)
    out = np.full(len(X), -1, int)
    for w0 in range(0, len(X), 64):
        sl = slice(w0, w0 + 64)
        for chk in pgs_exit_checks(kind, int(iters[w0])):
            ratio = res[sl, chk] / thr[sl]
            if margin is not None:
                margin.extend(float(v) for v in ratio)
            if (ratio <= 1).all():
                out[sl] = chk
                break
    return out


def _pgs(kind, N):
    def f(X, dt, T):
        iters = _pgs_unpack(X, N, dt)[3]
        n_sw = np.abs(iters)
        if kind == "blocks":
            n_sw = 2 * (n_sw // 2)
        dv, ran, _, _ = pgs_literal(X, N, dt, n_sw, clamp=kind in ("clamped", "threshold"), threshold=kind == "threshold")
        if kind in ("unclamped", "blocks"):
            ret = pgs_exit(kind, X, N, T) if len(X) % 64 == 0 else np.full(len(X), -1)
        else:
            ret = ran if kind == "threshold" else np.zeros(len(X), int)
        return np.concatenate([dv, ret.astype(dt)[:, None]], axis=1)
    return f


pgs_unclamped6, pgs_blocks6, pgs_clamped6, pgs_threshold6 = (_pgs(k, 6) for k in ("unclamped", "blocks", "clamped", "threshold"))
pgs_unclamped8, pgs_blocks8, pgs_clamped8, pgs_threshold8 = (_pgs(k, 8) for k in ("unclamped", "blocks", "clamped", "threshold"))


def run(op, X, dt, T):
    """The reference (dt = LD) or the plain restatement (dt = T) of op on the cases X [n][in_w] (any float dtype; converted to dt)."""
    return globals()[op](np.asarray(X).astype(dt), dt, T)


def restate(op, X, T):
    """The plain restatement in T; for trig_advance the recurrence, for pinv8 the Jacobi loop."""
    X = np.asarray(X).astype(T)
    if op == "trig_advance":
        return trig_recurrence(X, T, T)
    if op == "pinv8":
        return pinv_jacobi(X, T, T)
    return globals()[op](X, T, T)


def ulp_neighbours(X, T, fixed=()):
    """The inputs with one component moved by +1 or -1 ulp of T (zeros stay: they are structure, not roundings): yields [n][in_w] arrays."""
    XT = np.asarray(X).astype(T)
    for j in range(XT.shape[1]):
        if j in fixed or not np.any(XT[:, j] != 0):
            continue
        for sgn in (np.inf, -np.inf):
            Y = XT.copy()
            Y[:, j] = np.where(XT[:, j] != 0, np.nextafter(XT[:, j], T(sgn)), XT[:, j])
            yield Y


def spread(op, X, T, ref=None):
    """The conditioning rule's `spread` per case: the largest change of any output of the reference when one input moves by one ulp of T."""
    ref = run(op, X, LD, T) if ref is None else ref
    sp = np.zeros(len(ref), LD)
    with np.errstate(invalid="ignore"):
        for Y in ulp_neighbours(X, T, FIXED.get(op, ())):
            d = np.abs(run(op, Y, LD, T) - ref)
            sp = np.maximum(sp, np.where(np.isfinite(d), d, 0).max(axis=1))
    return sp
