"""The device helpers of csrc/tg_physics.hpp (and rot_error) one by one against a longdouble reference, at every branch and path.

tg_selftest_physics (include/tactile_gym_hip_test.h) runs case i in lane i % 64 of wavefront i // 64; tests/physics_cases.py lays the tables out
wavefront by wavefront, so the helpers' __any / __all votes are decided by the table: all lanes in range, one lane out of range, one lane
that converges slowly among 63 that converge fast.  tests/physics_ref.py is the reference; the tolerances are derived in physics_cases.py's
docstring and held by physics_cases.check, the function tests/test_physics_cases_cpu.py holds the plain restatement to at half the margin.
One launch per (op, dtype).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import physics_cases as pc  # noqa: E402
import physics_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


def run_device(op, dtype, X):
    from tactile_gym_amd import _capi
    L = _capi.test_lib()
    X = np.ascontiguousarray(X, np.float64)
    in_w, out_w = pr.SHAPE[op]
    out = np.full((len(X), out_w), np.nan)
    rc = L.tg_selftest_physics(pr.OP_ID[op], {"f64": 0, "f32": 1}[dtype], len(X), in_w, X.ctypes.data_as(_dp), out_w, out.ctypes.data_as(_dp))
    assert rc == 0, L.tg_selftest_last_error().decode()
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("op", pr.OPS)
def test_primitive(op, dtype):
    got = run_device(op, dtype, pc.table(op, dtype).X)
    fails, figs = pc.check(op, dtype, got)
    print(f"{op} {dtype}: " + "; ".join(figs))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sincos_small_votes_as_a_wavefront(dtype):
    """Where one lane of the wavefront is out of range, EVERY lane takes the library call: each lane's result carries the bits of the device's
    own sincos of its x (axis_angle about z hands those out unchanged: R[0] = c + 0 * v, R[3] = 0 * v + 1 * s).  Both paths are accurate to
    2 eps, so the value check cannot tell a wavefront's vote from a lane's own choice; this does.  And the vote is needed at all: in the
    all-in-range wavefronts some lane's Taylor result differs from the library's in the last bit (else the table could not see the path)."""
    t = pc.table("sincos_small", dtype)
    got = run_device("sincos_small", dtype, t.X)
    lib = run_device("axis_angle", dtype, pc.library_axis_angle_rows(t.X[:, 0]))[:, [3, 0]]
    voted = t.sel("library")
    assert voted.sum() >= 128 and (~voted).sum() >= 128
    bad = np.nonzero(voted & (got != lib).any(axis=1))[0]
    assert len(bad) == 0, f"lanes of a wavefront with a lane out of range that did not take the library call: x = {t.X[bad[:8], 0]}"
    assert (got[~voted] != lib[~voted]).any(), "the Taylor pair equals the library call on every in-range case: the table cannot tell the paths apart"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_integrate_rotation_stays_orthonormal(dtype):
    """After 240 ticks R^T R = I to 32 eps_T whatever the start: every tick ends in a Gram-Schmidt step whose two normalisations go through
    trsqrt (2 ulp: a column's squared norm is off by at most 5 eps plus the 2 eps of its own dot product), the projection leaves c0 . c1 at a
    few eps, and c2 = c0 x c1 inherits both - 32 eps covers the sum with a factor 2, independent of the number of ticks."""
    t = pc.table("integrate_rotation", dtype)
    rows = t.sel("240 ticks")
    R = run_device("integrate_rotation", dtype, t.X)[rows].reshape(-1, 3, 3)
    err = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(axis=(1, 2))
    print(f"integrate_rotation {dtype}: max |R^T R - I| after 240 ticks = {err.max() / pr.eps(pc.DTYPES[dtype]):.2f} eps")
    assert (err <= 32 * pr.eps(pc.DTYPES[dtype])).all(), (err.max(), t.labels[rows][np.argmax(err)])


def test_error_returns():
    """Unknown op or dtype, NULL, n no multiple of 64, a width the op does not expect, a loop count that differs inside a wavefront: -1, no launch
    (the output keeps what it held)."""
    from tactile_gym_amd import _capi
    L = _capi.test_lib()
    X = np.ones((64, 3))
    out = np.full((64, 4), 7.0)
    pin, pout = X.ctypes.data_as(_dp), out.ctypes.data_as(_dp)
    null = _dp()
    assert L.tg_selftest_physics(len(pr.OPS), 0, 64, 3, pin, 4, pout) == -1
    assert L.tg_selftest_physics(-1, 0, 64, 3, pin, 4, pout) == -1
    assert L.tg_selftest_physics(0, 2, 64, 3, pin, 4, pout) == -1
    assert L.tg_selftest_physics(0, 0, 64, 3, null, 4, pout) == -1
    assert L.tg_selftest_physics(0, 0, 64, 3, pin, 4, null) == -1
    for n in (0, 1, 63, 65, -64):
        assert L.tg_selftest_physics(0, 0, n, 3, pin, 4, pout) == -1
    assert L.tg_selftest_physics(0, 0, 64, 4, pin, 4, pout) == -1
    assert L.tg_selftest_physics(0, 0, 64, 3, pin, 3, pout) == -1
    assert b"width" in L.tg_selftest_last_error()
    op = "integrate_rotation"
    Y = pc.table(op, "f64").X[:64].copy()
    res = np.full((64, 9), 7.0)
    Y[3, 0] = 2.0                                    # one lane's tick count differs
    assert L.tg_selftest_physics(pr.OP_ID[op], 0, 64, 14, Y.ctypes.data_as(_dp), 9, res.ctypes.data_as(_dp)) == -1
    Y[:, 0] = 241.0                                  # above the op's limit
    assert L.tg_selftest_physics(pr.OP_ID[op], 0, 64, 14, Y.ctypes.data_as(_dp), 9, res.ctypes.data_as(_dp)) == -1
    assert (out == 7.0).all() and (res == 7.0).all()
    assert L.tg_selftest_physics(0, 0, 64, 3, pin, 4, pout) == 0 and np.isfinite(out).all() and not (out == 7.0).all()
