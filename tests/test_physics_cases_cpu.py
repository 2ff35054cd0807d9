"""What tests/test_gpu_physics_primitives.py rests on, proved on the CPU with the reference alone (tests/physics_ref.py, tests/physics_cases.py):
every case is in the branch or on the path its label names, with the margins the tables promise; the reference agrees with oracle/pb_math.py
and with np.linalg.solve; the float32 pinv cases are well posed; the plain restatement of every helper in its own number format passes the
kernel's tolerance with half the margin; and the iterative solvers' e_T are what physics_cases.py's docstring quotes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import physics_cases as pc  # noqa: E402
import physics_ref as pr  # noqa: E402

LD = np.longdouble
BOTH = pytest.mark.parametrize("dtype", ["f64", "f32"])
PGS_OPS = [op for op in pr.OPS if op.startswith("pgs_")]


def ulps_from(value, threshold, T):
    """Signed distance of value from T(threshold) in ulps of T at the threshold."""
    thr = T(threshold)
    return (np.asarray(value, np.float64) - float(thr)) / float(np.spacing(thr))


@pytest.mark.parametrize("op", pr.OPS)
@BOTH
def test_tables_are_well_formed(op, dtype):
    t = pc.table(op, dtype)
    T = pc.DTYPES[dtype]
    assert t.X.shape[1] == pr.SHAPE[op][0] and len(t.X) % 64 == 0 and len(t.X) <= 4096 and len(t.labels) == len(t.X)
    assert np.array_equal(t.X, t.X.astype(T).astype(np.float64)), "a value that T does not hold"
    assert np.isfinite(t.X).all()
    assert pc.reference(op, dtype).shape == (len(t.X), pr.SHAPE[op][1])
    pad = t.labels == "pad"                                  # a pad is a copy of the case before it
    assert not pad[0] and all(np.array_equal(t.X[i], t.X[i - 1]) for i in np.nonzero(pad)[0])


@BOTH
def test_euler_cases_are_in_their_branch(dtype):
    """sarg evaluated in T - with and without the contraction of its two products into one FMA, which moves it by an ulp - lies at least
    4 ulp of T on the side of +-0.99999 the label names."""
    T = pc.DTYPES[dtype]
    t = pc.table("euler_from_quat", dtype)
    x, y, z, w = (t.X[:, j].astype(T) for j in range(4))
    plain = np.abs(T(-2) * (x * z - w * y))
    fused = np.abs((T(-2) * (x.astype(LD) * z.astype(LD) - (w * y).astype(LD)).astype(T)))       # fma(x, z, -(w y)): one rounding less
    for sarg in (plain, fused):
        d = ulps_from(sarg, pc.GIMBAL, T)
        inside = t.sel("ordinary", "non-unit small", "gimbal + inside", "gimbal - inside")
        outside = t.sel("gimbal + outside", "gimbal - outside", "gimbal + at 1", "gimbal - at 1")
        assert (d[inside] <= -4).all() and (d[outside] >= 4).all()
        m = t.sel("gimbal + inside 0.99995", "gimbal - inside 0.99995")     # between 0.9999 and 0.99999: a moved threshold shows here
        assert m.sum() == 4 and (ulps_from(sarg[m], 0.9999, T) >= 4).all()
        big = t.sel("non-unit large")
        assert (np.abs(d[big]) >= 4).all() and (d[big] > 0).any() and (sarg[big] > 1).any()
    assert (np.sign(pr.euler_sarg(t.X, np.float64))[t.sel("gimbal -")] < 0).all() and (pr.euler_sarg(t.X, np.float64)[t.sel("gimbal +")] > 0).all()
    at1 = ulps_from(plain[t.sel("gimbal + at 1", "gimbal - at 1")], 1.0, T)
    assert (np.abs(at1) <= 4).all()
    norm = np.linalg.norm(t.X, axis=1)
    assert (np.abs(norm[t.sel("non-unit")] - 1) > 0.09).all() and (np.abs(norm[t.sel("ordinary", "gimbal")] - 1) < 1e-6).all()


@BOTH
def test_quat_from_mat_cases_are_in_their_branch(dtype):
    t = pc.table("quat_from_mat", dtype)
    br = pr.quat_from_mat_branch(t.X)
    R = t.X.reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    for b, name in enumerate(("trace > 0", "R00 largest", "R11 largest", "R22 largest")):
        m = t.sel(name)
        assert m.sum() >= 8 and (br[m] == b).all()
    m = t.sel("tie R00 == R11 >= R22")
    assert m.sum() == 1 and (R[m, 0, 0] == R[m, 1, 1]).all() and (R[m, 0, 0] > R[m, 2, 2]).all() and (tr[m] < 0).all() and (br[m] == 1).all()
    m = t.sel("tie R11 == R22 > R00")
    assert m.sum() == 1 and (R[m, 1, 1] == R[m, 2, 2]).all() and (R[m, 1, 1] > R[m, 0, 0]).all() and (tr[m] < 0).all() and (br[m] == 2).all()
    m = t.sel("trace 0")
    assert m.sum() == 2 and (tr[m] == 0).all() and (br[m] == 1).all()
    m = t.sel("half turn")
    assert sorted(br[m]) == [1, 2, 3] and (tr[m] == -1).all()


@BOTH
def test_rot_error_cases_have_their_angle(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("rot_error", dtype)
    X = t.X.astype(LD)
    E = np.einsum("nik,njk->nij", X[:, :9].reshape(-1, 3, 3), X[:, 9:].reshape(-1, 3, 3))
    s = np.sqrt(((E - E.transpose(0, 2, 1)) ** 2).sum(axis=(1, 2)) / 2)        # 2 sin(angle)
    ang = np.arctan2(0.5 * s, 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1))
    for a in pc.ROT_ERROR_ANGLES:
        m = t.labels == f"angle {a:.3g}"
        assert m.sum() == 7
        assert np.allclose(ang[m].astype(float), a, rtol=0, atol=max(64 * pr.eps(T), 1e-3 * a if a < 1e-5 and T is np.float32 else 0) + 16 * pr.eps(T) / max(a, 1e-3))
    assert (s[t.labels == "angle 0"] < 1e-12 / 4).all()                             # the 0.5 * ax branch ...
    if T is np.float64:
        assert (s[t.labels == "angle 1e-09"] > 4e-12).all()                         # ... and just above it
    m = t.sel("angle pi")
    assert m.sum() == 7 and (np.abs(ang[m] - np.pi) < 1e-3).all()


@BOTH
def test_plane_space_cases_are_in_their_branch(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("plane_space", dtype)
    d = ulps_from(np.abs(t.X[:, 2]), 0.7071067811865475244, T)
    assert (d[t.sel("|n.z| above")] >= 4).all() and (d[t.sel("|n.z| below")] <= -4).all() and (d[t.sel("|n.z| above")] <= 12).any()
    assert t.sel("|n.z| above").sum() == 6 and t.sel("|n.z| below").sum() == 6
    ax = t.X[t.sel("axes")]
    assert len(ax) == 6 and (np.abs(ax).sum(axis=1) == 1).all() and len({tuple(a) for a in ax}) == 6
    assert (np.abs(d[t.sel("ordinary")]) >= 4).all()
    assert (np.abs(np.linalg.norm(t.X, axis=1) - 1) < 4 * pr.eps(T)).all()


@BOTH
def test_fast_arithmetic_cases(dtype):
    T = pc.DTYPES[dtype]
    for op in pc.ULP_OPS:
        t = pc.table(op, dtype)
        x = t.X[:, 0]
        assert set(2.0 ** np.arange(-40, 41)) <= set(x[t.sel("powers of two")])
        near = x[t.sel("next to 1")]
        assert float(np.nextafter(T(1), T(2))) in near and float(np.nextafter(T(1), T(0))) in near
        rnd = x[t.sel("random")]
        e = np.floor(np.log2(np.abs(rnd)))
        assert len(rnd) >= 1900 and e.min() == -40 and e.max() == 40
    t = pc.table("tsqrt_fast", dtype)
    x = t.X[:, 0]
    assert (x[t.sel("zero")] == 0).all() and (x[t.sel("below 1e-30")] < float(T(1e-30))).all() and (x[t.sel("above 1e-30")] > float(T(1e-30))).all()
    assert t.sel("below 1e-30").sum() == 4 and t.sel("above 1e-30").sum() == 4


@BOTH
def test_friction_cases_are_in_their_branch(dtype):
    t = pc.table("friction_clamp", dtype)
    s1, s2, lim, cone = t.X.T
    tot2 = s1 * s1 + s2 * s2
    for name, c in (("cone", 1), ("pyramid", 0)):
        over, inside = t.sel(f"{name} over"), t.sel(f"{name} inside")
        assert over.sum() >= 20 and inside.sum() >= 20 and (cone[over | inside] == c).all()
        assert (tot2[over] > lim[over] ** 2 * (1 + 1e-3)).all() and (tot2[inside] < lim[inside] ** 2 * (1 - 1e-3)).all()
    p = t.sel("pyramid over", "pyramid inside")
    assert (np.abs(np.abs(t.X[p, :2]) - lim[p, None]) > 1e-3).all()
    assert (np.abs(t.X[p, :2]) > lim[p, None]).any() and (np.abs(t.X[p, :2]) < lim[p, None]).any()


@BOTH
def test_sincos_wavefronts(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("sincos_small", dtype)
    x = np.abs(t.X[:, 0]).reshape(-1, 64)
    lab = t.labels.reshape(-1, 64)
    lim = float(T(0.05))
    taylor = np.array([(row == "taylor").any() for row in lab])
    assert taylor.sum() == 2
    assert (x[taylor] <= lim).all()                                            # no lane out of range: the polynomial
    assert ((x[~taylor] > lim).sum(axis=1) >= 1).all()                         # some lane out of range: the library call for all
    mixed = np.array([(row == "library: a neighbour holds 0.06").any() for row in lab])
    assert mixed.sum() == 2 and ((x[mixed] > lim).sum(axis=1) == 1).all()
    for a, b in zip(np.nonzero(taylor)[0], np.nonzero(mixed)[0]):               # the same 63 values both ways
        assert np.array_equal(t.X.reshape(-1, 64)[a, :63], t.X.reshape(-1, 64)[b, :63])
    v = t.X[t.sel("taylor"), 0]
    assert lim in v and -lim in v and 0.0 in v and float(np.nextafter(T(0.05), T(0))) in v and len(np.unique(v)) >= 120
    out = t.X[t.sel("library: outside"), 0]
    assert float(np.nextafter(T(0.05), T(1))) in out and 0.06 in np.round(out.astype(np.float64), 7)


@BOTH
def test_trig_wavefronts(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("trig_advance", dtype)
    k = t.X[:, 0].astype(int).reshape(-1, 64)
    assert (k == k[:, :1]).all()
    dq = np.abs(t.X[:, 1 + pr.TRIG_N:]).reshape(-1, 64, pr.TRIG_MAX_K, pr.TRIG_N)
    big = dq > float(T(0.02))
    lab = t.labels.reshape(-1, 64)[:, 0]
    for w in range(len(k)):
        assert (dq[w, :, k[w, 0]:] == 0).all()
        if "re-anchored" in lab[w]:
            step = k[w, 0] - 1 if "last" in lab[w] else 4
            assert big[w].sum() == 1 and big[w, 5, step, 2] and np.isclose(dq[w, 5, step, 2], 0.021)
        else:
            assert not big[w].any()
    assert sorted(set(k[:, 0])) == [0, 1, 23, 24]
    for kk in pc.TRIG_KS:
        for name in ("+0.02", "-0.02", "random"):
            m = t.sel(f"k={kk} {name}")
            assert m.sum() >= 16
        m = t.sel(f"k={kk} +0.02")
        assert (t.X[m, 1 + pr.TRIG_N:1 + pr.TRIG_N + kk * pr.TRIG_N] == float(T(0.02))).all()
    q0 = t.X[:, 1:1 + pr.TRIG_N]
    assert q0.min() < -3 and q0.max() > 3 and (np.abs(q0) <= np.pi).all()


@BOTH
def test_integrate_rotation_cases_are_in_their_branch(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("integrate_rotation", dtype)
    w, dt, k = t.X[:, 10:13], t.X[:, 13], t.X[:, 0].astype(int)
    ang = np.sqrt((w.astype(LD) ** 2).sum(axis=1)).astype(np.float64)
    half = ang * dt / 2
    assert (ang[t.sel("w = 0", "240 ticks, w = 0")] == 0).all()
    assert (ang[t.sel("ang below 0.001", "240 ticks, ang below")] < 0.001 * (1 - 1e-3)).all() and (ang[t.sel("ang above 0.001")] > 0.001 * (1 + 1e-3)).all()
    assert (ang[t.sel("ang below 0.001")] >= 0.00099 * (1 - 1e-6)).any() and (ang[t.sel("ang above 0.001")] <= 0.00101 * (1 + 1e-6)).any()
    m = t.sel("ang below 0.001, dt 50")                      # the cubic term of the small-angle branch is 1e-5 .. 1e-4 of the linear one
    cubic = dt[m] ** 2 / 24 * ang[m] ** 2
    assert m.sum() == 8 and (cubic > 4e-6).all() and (cubic.max() > 8e-5)
    assert (half[t.sel("|w| dt / 2 below 0.05")] < 0.05 * (1 - 1e-4)).all() and (half[t.sel("|w| dt / 2 below 0.05")] > 0.0499).any()
    assert (half[t.sel("|w| dt / 2 above 0.05")] > 0.05 * (1 + 1e-3)).all() and (half[t.sel("|w| dt / 2 above 0.05")] < 0.0503).any()
    assert np.allclose(ang[t.sel("100 rad/s", "240 ticks, 100 rad/s")], 100.0)
    R = t.X[:, 1:10].reshape(-1, 3, 3)
    off = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(axis=(1, 2))
    m = t.sel("start off orthonormal", "240 ticks, start off")
    assert (off[m] > 1e-7).all() and (off[m] < 1e-5).all() and (off[~m & (t.labels != "pad")] < 8 * pr.eps(T)).all()
    waves_half, waves_lab, waves_k = half.reshape(-1, 64), t.labels.reshape(-1, 64), k.reshape(-1, 64)
    assert (waves_k == waves_k[:, :1]).all() and sorted(set(k)) == [1, 240]
    assert (waves_half[0] <= float(T(0.05)) * (1 - 1e-4)).all()                # the first wavefront: every lane takes the polynomials
    assert (waves_half[1] > 0.05).any()                                        # the second: the same cases beside lanes out of range
    n_in = int(np.sum(["neighbour" in lb for lb in waves_lab[1]]))
    assert n_in >= 40 and np.array_equal(t.X.reshape(-1, 64, 14)[0, :n_in], t.X.reshape(-1, 64, 14)[1, :n_in])
    assert (waves_half[2] <= 0.05 * (1 - 1e-4)).all() and (waves_k[2] == 240).all()
    assert (waves_half[3] > 0.05).all() and (waves_k[3] == 240).all()


@pytest.mark.parametrize("N", [6, 8])
@BOTH
def test_solve_cases_are_what_they_claim(N, dtype):
    T = pc.DTYPES[dtype]
    t = pc.table(f"solve{N}", dtype)
    A, b = t.X[:, :N * N].reshape(-1, N, N), t.X[:, N * N:]
    for dt in (LD, T):
        log = []
        pr.solve_gauss(A, b, dt, log)
        swapped = np.stack([s for s, _ in log], axis=1)
        zero = np.stack([z for _, z in log], axis=1)
        m = t.sel("a row swap at every column")
        assert m.sum() == 5 and swapped[m][:, :N - 1].all()
        m = t.sel("zero column")
        assert m.sum() == 3 and (zero[m].sum(axis=1) == 1).all() and sorted(np.argmax(zero[m], axis=1)) == [0, 2, N - 1]
        assert not zero[~m].any()
    assert (np.abs(A[t.sel("zero column")]).min(axis=1) == 0).any(axis=1).all()
    cond = np.array([np.linalg.cond(a) for a in A[t.sel("well conditioned", "a row swap")]])
    assert cond.max() < 50
    m = t.sel("diag 1e-6 .. 1e6")
    d = np.abs(A[m]).max(axis=1)
    assert m.sum() == 10 and (d.max(axis=1) / d.min(axis=1) > 1e11).all()     # the columns' scales
    if N == 6:
        J = pc.arm("ur5")[0]
        m = t.sel("UR5 TCP Jacobian at rest")
        assert m.sum() == 4 and np.array_equal(A[m][0], J.astype(T).astype(np.float64)) and J.shape == (6, 6)
    # on the regular systems the reference is np.linalg.solve, to the conditioning rule's own half margin
    reg = ~t.sel("zero column")
    ref = pc.reference(f"solve{N}", dtype)
    lin = np.stack([np.linalg.solve(a, v) for a, v in zip(A[reg], b[reg])])
    bound = 4 * pc.case_spread(f"solve{N}", "f64" if T is np.float64 else dtype)[reg][:, None] + 4 * pr.eps(np.float64) * np.maximum(1, np.abs(ref[reg]))
    assert (np.abs(lin - ref[reg]) <= bound.astype(np.float64) + 64 * pr.eps(np.float64) * np.abs(ref[reg]).max(axis=1)[:, None] * np.array([np.linalg.cond(a) for a in A[reg]])[:, None]).all()


@BOTH
def test_pinv_cases_are_what_they_claim(dtype):
    T = pc.DTYPES[dtype]
    t = pc.table("pinv8", dtype)
    J, b = t.X[:, :48].reshape(-1, 6, 8), t.X[:, 48:]
    sv = np.array([np.linalg.svd(j, compute_uv=False) for j in J])
    rank = (sv > 1e-15 * np.maximum(sv[:, :1], 1e-300)).sum(axis=1)
    assert (rank[t.sel("full rank")] == 6).all() and (sv[t.sel("full rank"), 5] / sv[t.sel("full rank"), 0] > 0.2).all()
    for name in ("MG400 at rest", "three zero columns, rank 5"):
        m = t.sel(name)
        assert m.sum() == 8 and (J[m][:, :, 5:] == 0).all() and (rank[m] == 5).all() and (sv[m, 4] / sv[m, 0] > 1e-3).all()
        inside, outside = t.sel(name + ", b in the range"), t.sel(name + ", b outside the range")
        ref = pc.reference("pinv8", dtype).astype(np.float64)
        res = np.abs(np.einsum("nrc,nc->nr", J, ref) - b).max(axis=1)
        assert (res[inside] < 1e-5 if T is np.float32 else res[inside] < 1e-13).all() and (res[outside] > 1e-3).all()
    m = t.sel("zero rows")
    assert (np.abs(J[m]).max(axis=2) == 0).sum(axis=1).min() == 2 and (rank[m] == 4).all()
    m = t.sel("duplicated columns")
    assert (J[m] == np.round(J[m])).all() and (np.abs(J[m]) <= 3).all() and (J[m][:, :, 3] == J[m][:, :, 0]).all() and (rank[m] <= 6).all()
    m = t.sel("zero matrix")
    assert m.sum() == 1 and (J[m] == 0).all()
    if T is np.float64:
        for ratio in (1e-3, 1e-6, 1e-9, 1e-12, 1e-14, 1e-16):
            m = t.sel(f"sigma_min / sigma_max = {ratio:g}")
            assert m.sum() >= 3 and np.allclose(sv[m, 5] / sv[m, 0], ratio, rtol=1e-2 if ratio > 1e-13 else 1e-9)
            assert (rank[m] == (6 if ratio > 1e-15 else 5)).all()                # both sides of numpy's cut ...
        m = t.sel("sigma_min / sigma_max = 1e-14", "sigma_min / sigma_max = 1e-16")
        assert ((J[m] != 0).sum(axis=2)[:, 3] == 1).all() and ((J[m] != 0).sum(axis=1)[:, 5] == 1).all()   # ... on a row and a column of its own


def test_f32_pinv_cases_are_well_posed():
    """After rounding to float32 every singular value is either at least eps_f32 / 0.01 of the largest (condition number x eps_f32 < 0.01)
    or zero by the matrix's structure (below 1e-15 of the largest in float64: an exact rank deficiency)."""
    t = pc.table("pinv8", "f32")
    for j, lb in zip(t.X[:, :48].reshape(-1, 6, 8), t.labels):
        s = np.linalg.svd(j, compute_uv=False)
        if s[0] == 0:
            continue
        r = s / s[0]
        assert ((r > pr.eps(np.float32) / 0.01) | (r < 1e-15)).all(), (lb, r)


@pytest.mark.parametrize("op", PGS_OPS)
@BOTH
def test_pgs_cases_are_what_they_claim(op, dtype):
    T = pc.DTYPES[dtype]
    N, kind = int(op[-1]), op[4:-1]
    t = pc.table(op, dtype)
    X = t.X
    iters = X[:, N * N + 2 * N].astype(int)
    assert (iters.reshape(-1, 64) == iters.reshape(-1, 64)[:, :1]).all()
    want = pc.PGS_BLOCK_ITERS if kind == "blocks" else pc.PGS_ITERS
    assert set(want) <= set(iters)
    for i in np.nonzero(np.arange(len(X)) % 16 == 0)[0]:                          # the contraction a label names, on a sample
        lb = t.labels[i]
        if "contraction" in lb or "lane" in lb:
            target = 0.94 if ("0.94" in lb) else 0.5
            A = X[i, :N * N].reshape(N, N)
            assert np.allclose(A, A.T) and np.linalg.eigvalsh(A).min() > 0
            assert abs(pc.pgs_contraction(A, X[i, N * N + N:N * N + 2 * N]) - target) < 0.02, lb
    if kind in ("unclamped", "clamped") or op == "pgs_blocks8":
        name = "UR5" if N == 6 else "MG400"
        A = X[t.sel(f"iters=150 {name}")][0, :N * N].reshape(N, N)
        assert abs(pc.pgs_contraction(A, 1 / np.diag(A)) - (0.52 if N == 6 else 0.94)) < 0.01          # the header's 0.94 for the MG400
    lab = t.labels.reshape(-1, 64)
    mixed = np.array([(row == "iters=150 one lane 0.94").sum() == 1 and (row == "iters=150 63 lanes 0.5").sum() == 63 for row in lab])
    assert mixed.sum() == 1
    ref = pc.reference(op, dtype)
    ret = ref[:, -1].astype(int).reshape(-1, 64)
    if kind in ("unclamped", "blocks"):
        assert (pc.exit_margin(kind, X, N, T) >= 2).all()
        assert (ret == ret[:, :1]).all()
        fired = np.array([(row == f"iters={it} all lanes 0.5").all() for row in lab for it in [150]]).reshape(-1)
        assert fired.sum() == 1 and (ret[fired] > 0).all() and (ret[fired] < 100).all()        # the exit fires where every lane converges fast ...
        assert (ret[mixed] == -1).all()                                                          # ... and one slow lane holds 63 fast ones in the loop
        own = pr.pgs_residual_form(X[mixed.repeat(64)].astype(LD), N, LD, np.array([150])) / pr.pgs_exit_thr(X[mixed.repeat(64)], N, T)[:, None]
        assert ((own[:, 144] <= 0.5).sum() == 63)
        short = ret[[(it < 4 if kind == "unclamped" else it < 8) for it in iters.reshape(-1, 64)[:, 0]]]
        assert (short == -1).all()
    if kind in ("clamped", "threshold"):
        sat = pc.pgs_saturated(X, N, T)
        one, every = t.sel("maximp: one row saturates"), t.sel("maximp: every row saturates")
        assert one.sum() == 64 and every.sum() == 64
        assert (sat[every] == N).all() and (sat[one] >= 1).all() and (sat[one] < N).all() and (sat[~(one | every) & (t.labels != "pad")] == 0).all()
        huge = X[:, N * N + 2 * N + 1] == float(T(1e30))
        assert (huge == ~(one | every)).all()
    if kind == "threshold":
        assert (pc.threshold_margin(X, N, T) >= 2).all()
        assert (X[:, -1] > 0).all()
        assert (ret.min(axis=1) != ret.max(axis=1)).sum() >= 10                 # wavefronts whose lanes stop at different sweeps
        assert (ret[mixed].max() - ret[mixed].min()) >= 10
        stopped = ref[:, -1] < np.abs(iters)
        assert stopped.sum() > 300 and (~stopped).sum() > 50


@pytest.mark.parametrize("op", ["quat_from_euler", "euler_from_quat", "mat_from_quat", "quat_from_mat", "quat_mul"])
def test_reference_agrees_with_pb_math(op):
    """The float64 evaluation of physics_ref is oracle/pb_math.py: the same branch on every case, values to 4 ulp of their size (numpy's and
    libm's sin / atan2 differ in the last bit); the reference itself agrees with both to the conditioning rule's half margin."""
    from oracle import pb_math
    t = pc.table(op, "f64")
    fn = {"quat_from_euler": lambda r: pb_math.quat_from_euler(r), "euler_from_quat": pb_math.euler_from_quat, "mat_from_quat": lambda r: pb_math.mat_from_quat(r).reshape(9),
          "quat_from_mat": lambda r: pb_math.quat_from_mat(r.reshape(3, 3)), "quat_mul": lambda r: pb_math.quat_mul(r[:4], r[4:])}[op]
    pb = np.stack([np.asarray(fn(row), np.float64) for row in t.X])
    f64 = pr.run(op, t.X, np.float64, np.float64)
    scale = np.maximum(1, np.abs(pb).max(axis=1))[:, None]
    slope = 1.0
    if op == "euler_from_quat":                      # asin next to the gimbal threshold: d asin = d sarg / sqrt(1 - sarg^2)
        slope = 1 / np.sqrt(np.maximum(1 - np.minimum(np.abs(pr.euler_sarg(t.X, np.float64)), 1) ** 2, 1e-6))[:, None]
    assert (np.abs(f64 - pb) <= 4 * pr.eps(np.float64) * scale * slope).all()
    assert (np.abs(pb - pc.reference(op, "f64")) <= pc.general_bound(op, "f64", 4)).all()


@pytest.mark.parametrize("op", pr.OPS)
@BOTH
def test_plain_restatement_passes_with_half_the_margin(op, dtype):
    fails, figs = pc.check(op, dtype, pr.restate(op, pc.table(op, dtype).X, pc.DTYPES[dtype]), margin=0.5)
    print(f"{op} {dtype}: " + "; ".join(figs))
    assert not fails, "\n".join(fails)


def test_iterative_margins():
    """e_T per iterative solver, printed (physics_cases.py's docstring quotes them); each is a few roundings per unit of the error measure -
    were one large, 4 e_T would check nothing."""
    for op in pc.ITERATIVE_OPS:
        for dtype, T in pc.DTYPES.items():
            e = pc.measured_e(op, dtype) / pr.eps(T)
            print(f"e_T {op} {dtype}: {e:.2f} eps")
            assert 0.25 <= e <= 32, (op, dtype, e)


def test_trig_advance_drift_is_what_the_header_says():
    """The header's figure for the recurrence: a few eps per advance, inside 3 k eps; NOT below 1e-15 over an env step's 24 ticks, as its comment
    once said - the plain float64 restatement passes 1e-15 at 23 advances of +-0.02."""
    for dtype, T in pc.DTYPES.items():
        t, ref = pc.table("trig_advance", dtype), pc.reference("trig_advance", dtype)
        got = pr.restate("trig_advance", t.X, T)
        m = t.sel("k=23 +0.02", "k=23 -0.02", "k=23 random", "k=24 +0.02", "k=24 -0.02", "k=24 random")
        err = float(np.abs(got[m, :12] - ref[m, :12]).max())
        print(f"trig_advance {dtype}: worst drift after 23 / 24 advances {err:.3g} = {err / pr.eps(T):.2f} eps")
        assert err <= 1.5 * 24 * pr.eps(T)
        if T is np.float64:
            assert err > 0.9e-15
