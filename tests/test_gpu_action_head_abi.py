"""tg_action_head (csrc/tg_action_head.hip) called directly on raw pointers: row counts round the 64-lane wavefront and the 256-lane workgroup,
every action width up to the limit, both log_std strides, every mode, deterministic on and off, the clamp on and off, every subset of the
nullable outputs, a saturated case and the error returns that take no launch.  Every output sits between guard bytes inside a larger buffer.

What has no transcendental function on its path is compared with tests/action_head_ref.py (device_order) bit for bit; everything else with the
float64 formulas (exact_*) evaluated at the kernel's own output of the stage before, noise -> gaussian -> actions -> log_prob, within the bounds
that the restatement's docstring derives."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import action_head_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402
from action_head_device import OUTPUTS, _bits, _bounds, _call, _lib, f32  # noqa: E402

ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)
WIDTHS = (1, 2, 3, 6, 16)


def _inputs(rng, N, A, per_row):
    mean = rng.uniform(-1.5, 1.5, (N, A)).astype(f32)
    ls = rng.uniform(-3.0, -1.5, (N, A) if per_row else (A,)).astype(f32)
    return mean, ls


def _within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (what, float((err / bound).max()))


def _check_chain(mode, got, mean, ls, lo, hi, noise):
    """The outputs of one Gaussian / squashed call against the restatement, each stage at the kernel's own output of the stage before."""
    N, A = mean.shape
    ls = np.broadcast_to(ls, (N, A))
    assert _bits(got["noise"], noise)
    x = got["gaussian"]
    _within(x, ref.exact_x(mean, ls, noise), ref.bound_x(mean, ls, noise), "gaussian")
    if mode == ref.GAUSSIAN:
        assert _bits(got["actions"], x) and _bits(got["env"], ref.clip_f32(x, lo, hi)) and _bits(got["env"], np.clip(x, lo, hi))
        _within(got["log_prob"], ref.exact_log_prob(x, mean, ls), ref.bound_gaussian_sum(x, mean, ls), "log_prob")
    else:
        a = got["actions"]
        _within(a, ref.exact_tanh(x), ref.bound_tanh(x), "actions")
        assert _bits(got["env"], ref.unscale_env_f32(a, lo, hi))
        _within(got["env"], ref.exact_unscale(a, lo, hi), ref.bound_unscale(a, lo, hi), "env")
        _within(got["log_prob"], ref.exact_log_prob(x, mean, ls, a), ref.bound_squashed_sum(x, mean, ls, a), "log_prob")


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("N", ROWS)
def test_every_mode_stride_and_switch_at_this_shape(N, A):
    rng = np.random.default_rng(100 * N + A)
    lo, hi = _bounds(A)
    noise = rng.standard_normal((N, A)).astype(f32)
    for mode, per_row, clamp in itertools.product((ref.GAUSSIAN, ref.SQUASHED), (False, True), ((-np.inf, np.inf), (-2.5, -2.0))):
        mean, ls = _inputs(rng, N, A, per_row)
        ls.flat[0], ls.flat[-1] = (-3.0, -1.5) if mode == ref.GAUSSIAN else (-1.5, -3.0)   # outside the clamp whatever was drawn
        clamped = ref.clamp(ls, *clamp)
        assert clamp[0] == -np.inf or ((clamped != ls).any() and (clamped >= f32(-2.5)).all() and (clamped <= f32(-2.0)).all())
        # the noise given: the chain of stages
        got = _call(mode, N, A, mean, ls, clamp=clamp, noise_in=noise, seed=5, counter=9)
        _check_chain(mode, got, mean, clamped, lo, hi, noise)
        assert _bits(got["noise"], _call(mode, N, A, mean, ls, clamp=clamp, noise_in=noise, deterministic=True)["noise"])      # the given noise wins
        # deterministic: eps = 0, x = mean; in the Gaussian mode only the log-prob has a transcendental function (exp) on its path
        det = _call(mode, N, A, mean, ls, clamp=clamp, deterministic=True, seed=5, counter=9)
        want = ref.device_order(mode, mean, ls, lo, hi, *clamp, deterministic=True)
        assert _bits(det["noise"], np.zeros((N, A), f32)) and _bits(det["gaussian"], mean)
        if mode == ref.GAUSSIAN:
            assert _bits(det["actions"], want["actions"]) and _bits(det["env"], want["env"]) and _bits(det["actions"], mean)
        _check_chain(mode, det, mean, clamped, lo, hi, np.zeros((N, A), f32))
        # drawn: the noise within one float32 neighbour of the restatement's, the rest chained from the kernel's own noise
        drawn = _call(mode, N, A, mean, ls, clamp=clamp, seed=5, counter=9)
        eps = ref.normal_draws(5, 9, N * A).reshape(N, A)
        assert (np.abs(drawn["noise"] - eps) <= np.spacing(np.maximum(np.abs(drawn["noise"]), np.abs(eps)))).all()
        print(f"N={N} A={A} mode={mode}: {np.mean(drawn['noise'] == eps):.4f} of the draws bit-equal to numpy's")
        _check_chain(mode, drawn, mean, clamped, lo, hi, drawn["noise"])
    # uniform: no transcendental function anywhere; drawn, and with u given
    got = _call(ref.UNIFORM, N, A, outputs=("actions", "env", "noise"), seed=3, counter=4)
    want = ref.device_order(ref.UNIFORM, None, None, lo, hi, seed=3, counter=4, shape=(N, A))
    assert _bits(got["env"], want["env"]) and _bits(got["actions"], want["actions"]) and _bits(got["noise"], want["noise"])
    u = rng.uniform(0, 1, (N, A)).astype(f32)
    got = _call(ref.UNIFORM, N, A, outputs=("actions", "env", "noise"), noise_in=u, stride=A)
    want = ref.device_order(ref.UNIFORM, None, None, lo, hi, noise=u, shape=(N, A))
    assert _bits(got["env"], want["env"]) and _bits(got["actions"], want["actions"]) and _bits(got["noise"], u)


@pytest.mark.parametrize("mode", [ref.GAUSSIAN, ref.SQUASHED, ref.UNIFORM])
def test_every_subset_of_the_outputs(mode):
    N, A = 257, 3
    rng = np.random.default_rng(7)
    mean, ls = _inputs(rng, N, A, True)
    names = OUTPUTS if mode != ref.UNIFORM else ("actions", "env", "noise")
    full = _call(mode, N, A, mean, ls, seed=2, counter=1, outputs=names)
    for r in range(len(names)):                                               # the full set is `full`; the empty one launches nothing
        for subset in itertools.combinations(names, r):
            got = _call(mode, N, A, mean, ls, seed=2, counter=1, outputs=subset)
            assert set(got) == set(subset) and all(_bits(got[k], full[k]) for k in subset), subset
    if mode == ref.UNIFORM:                                                   # gaussian_out and log_prob_out are not written in this mode
        capi, L = _lib()
        lo, hi = _bounds(A)
        extra = [Guarded(4 * N * A), Guarded(4 * N)]
        p = C.c_void_p
        capi.check(L.tg_action_head(p(None), p(None), 0, N, A, (C.c_float * A)(*lo.tolist()), (C.c_float * A)(*hi.tolist()), -np.inf, np.inf, mode, 0,
                                    2, 1, p(None), p(None), p(None), p(extra[0].ptr), p(extra[1].ptr), p(None),
                                    p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert all(bool((g.buf == PATTERN).all()) for g in extra)


def test_nothing_to_do_launches_nothing():
    mean, ls = np.zeros((4, 2), f32), np.zeros(2, f32)
    assert _call(ref.GAUSSIAN, 4, 2, mean, ls, outputs=()) == {}
    capi, L = _lib()
    out = Guarded(64)
    lo, hi = _bounds(2)
    p = C.c_void_p
    capi.check(L.tg_action_head(p(out.ptr), p(out.ptr), 0, 0, 2, (C.c_float * 2)(*lo.tolist()), (C.c_float * 2)(*hi.tolist()), -np.inf, np.inf, 0, 0,
                                0, 0, p(None), p(out.ptr), p(out.ptr), p(out.ptr), p(out.ptr), p(out.ptr), p(None)))         # N = 0
    torch.cuda.synchronize()
    assert bool((out.buf == PATTERN).all())


def test_saturated_inputs_stay_finite_and_inside_the_space():
    N, A = 300, 6
    rng = np.random.default_rng(11)
    lo, hi = _bounds(A)
    mean = rng.uniform(-20, 20, (N, A)).astype(f32)
    mean[:4] = [[20.0] * A, [-20.0] * A, [19.5, -19.5] * 3, [0.0] * A]
    ls = rng.uniform(-20, 2, (N, A)).astype(f32)
    got = _call(ref.SQUASHED, N, A, mean, ls, clamp=(-20.0, 2.0), deterministic=True)
    assert all(np.isfinite(v).all() for v in got.values())
    assert (np.abs(got["actions"]) <= 1).all() and (got["env"] >= lo).all() and (got["env"] <= hi).all()
    assert (np.abs(got["actions"][:2]) == 1).all()                            # tanh(+-20) rounds to +-1: log(1e-6) in the correction, not log(0)
    got = _call(ref.SQUASHED, N, A, mean, ls, clamp=(-20.0, 2.0), seed=1, counter=2)
    assert all(np.isfinite(v).all() for v in got.values())
    assert (np.abs(got["actions"]) <= 1).all() and (got["env"] >= lo).all() and (got["env"] <= hi).all()
    got = _call(ref.GAUSSIAN, N, A, mean, ls, clamp=(-20.0, 2.0), seed=1, counter=2)
    assert all(np.isfinite(v).all() for v in got.values()) and (got["env"] >= lo).all() and (got["env"] <= hi).all()
    assert _bits(got["env"], np.clip(got["actions"], lo, hi))


def test_clip_on_the_bounds_and_infinities():
    lo, hi = np.array([-0.25, -1.0, 0.0], f32), np.array([0.25, 2.0, 0.0], f32)
    mean = np.array([[-0.25, 2.0, 0.0], [0.25, -1.0, 1e-30], [np.inf, -np.inf, -1e-30], [-np.inf, np.inf, 0.5], [0.1, 0.5, 3.0],
                     [np.nextafter(f32(0.25), f32(1)), np.nextafter(f32(-1), f32(-2)), 0.0]], f32)
    got = _call(ref.GAUSSIAN, 6, 3, mean, np.zeros(3, f32), lo=lo, hi=hi, deterministic=True, outputs=("actions", "env"))
    assert _bits(got["actions"], mean) and _bits(got["env"], np.clip(mean, lo, hi))


def test_error_returns_take_no_launch_and_write_nothing():
    N, A = 70, 3
    rng = np.random.default_rng(2)
    mean, ls = _inputs(rng, N, A, True)
    lo, hi = _bounds(A)
    bad = lambda mode=ref.GAUSSIAN, **kw: _call(mode, kw.pop("N", N), kw.pop("A", A), kw.pop("mean", mean), kw.pop("log_std", ls),   # noqa: E731
                                                expect_error=True, **kw)
    for mode in (ref.GAUSSIAN, ref.SQUASHED):
        bad(mode, mean=None)
        bad(mode, log_std=None)
    for width in (0, -1):
        bad(A=width, lo=np.zeros(17, f32), hi=np.ones(17, f32), outputs=())   # no output can be sized: the error return itself is the check
    bad(A=17, lo=np.zeros(17, f32), hi=np.ones(17, f32), stride=0)
    for stride in (1, 2, 4, -3, 6):
        bad(stride=stride)
        bad(ref.UNIFORM, stride=stride)
    upside = hi.copy(), lo.copy()
    for mode in (ref.GAUSSIAN, ref.SQUASHED, ref.UNIFORM):
        bad(mode, lo=upside[0], hi=upside[1])
        one = hi.copy()
        one[1] = np.nextafter(lo[1], f32(-9))                                 # one dimension upside down by one float32 neighbour
        bad(mode, lo=lo, hi=one)
        bad(mode, lo=np.array([0, np.nan, 0], f32), hi=np.ones(3, f32))
    flat = hi.copy()
    flat[2] = lo[2]
    for mode in (ref.SQUASHED, ref.UNIFORM):
        bad(mode, lo=lo, hi=flat)
    ok = _call(ref.GAUSSIAN, N, A, mean, ls, lo=lo, hi=flat, deterministic=True)                      # a degenerate dimension clips to its value
    assert (ok["env"][:, 2] == lo[2]).all()
    bad(clamp=(1.0, 0.5))
    bad(clamp=(np.nan, 0.5))
    for mode in (-1, 3, 99):
        bad(mode)
    bad(N=-1, outputs=())
