"""tg_ppo_loss, tg_squashed_rsample and tg_squashed_rsample_bwd (csrc/tg_loss_head.hip) called directly on raw pointers between guard bytes: row
counts round the wavefront, the 256-row chunk and the 4096-row switch between the two paths, action widths up to the limit, both log_std
strides, the value clip and the normalisation on and off.  Every stat and gradient against the float64 composition of tests/loss_head_ref.py
within the bounds its docstring derives (no row left out, the input conditions asserted), the two paths bit for bit, every subset of the
nullable outputs, the workspace to the byte, the error returns, and the exact case: the head's own sample gives ratio == 1."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import action_head_ref as head  # noqa: E402
import loss_head_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from loss_device import AUTO, GRID, INPUTS, ONE, OUTPUTS, _bits, _head, _lib, _ppo, _rsample, _rsample_bwd, _upload, f32  # noqa: E402

ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 5000)
WIDTHS = (1, 2, 6, 16)
CLIP, CLIP_VF, ENT, VF = 0.2, 0.2, 0.01, 0.5


def _named(got):
    out = dict(zip(ref.STATS, got["stats"].astype(np.float64)))
    out.update({k: v for k, v in got.items() if k != "stats"})
    return out


def _within(got, ex, bounds, names, what):
    for k in names:
        err = np.abs(np.asarray(got[k], np.float64) - ex[k])
        bad = err > np.broadcast_to(bounds[k], err.shape)
        assert not bad.any(), (what, k, float(err.max()), float(np.max(bounds[k])))


def _case(B, A, per_row, clip_vf, normalize):
    inp = ref.ppo_inputs(B, A, per_row, seed=1000 * B + 10 * A + per_row, clip_range=CLIP, clip_range_vf=clip_vf)
    return inp, dict(clip_range=CLIP, clip_range_vf=clip_vf, ent_coef=ENT, vf_coef=VF, normalize_advantage=normalize)


@pytest.mark.parametrize("A", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_stats_and_gradients_within_bounds_and_both_paths_bit_equal(B, A):
    """Both strides, each with the value clip and the normalisation on and off (the two diagonals alternate from shape to shape)."""
    pairs = ((CLIP_VF, True), (None, False)) if (ROWS.index(B) + WIDTHS.index(A)) % 2 else ((CLIP_VF, False), (None, True))
    for per_row, (clip_vf, normalize) in itertools.product((False, True), pairs):
        inp, kw = _case(B, A, per_row, clip_vf, normalize)
        ex = ref.ppo_exact(**inp, **kw)
        assert ref.conditions_hold(ex, inp, CLIP, clip_vf)
        bounds = ref.ppo_bounds(ex, **inp, **kw)
        dev = _upload(inp)
        got = _ppo(inp, dev, kw)
        what = (B, A, per_row, clip_vf, normalize)
        _within(_named(got), ex, bounds, ref.STATS + ("log_prob", "dmean", "dlog_std", "dvalues"), what)
        if B == 1 or not normalize:
            assert got["stats"][6] == 0 and got["stats"][7] == 1              # not applied
        grid = _ppo(inp, dev, kw, path=GRID)                                  # a second call, and the other path wherever both apply
        assert all(_bits(got[k], grid[k]) for k in OUTPUTS), what
        if B <= 4096:
            one = _ppo(inp, dev, kw, path=ONE)
            assert all(_bits(got[k], one[k]) for k in OUTPUTS), what
        else:
            _ppo(inp, dev, kw, path=ONE, expect_error=True)


@pytest.mark.parametrize("B", [257, 4097])
def test_every_subset_of_the_nullable_outputs(B):
    for per_row in (False, True):
        inp, kw = _case(B, 6, per_row, CLIP_VF, True)
        dev = _upload(inp)
        full = _ppo(inp, dev, kw)
        names = OUTPUTS[1:]
        for r in range(len(names)):
            for subset in itertools.combinations(names, r):
                got = _ppo(inp, dev, kw, outputs=("stats",) + subset)
                assert all(_bits(got[k], full[k]) for k in got), subset


def test_the_grid_path_takes_a_workspace_of_exactly_the_queried_size():
    capi, L = _lib()
    inp, kw = _case(4097, 6, False, CLIP_VF, True)
    dev = _upload(inp)
    need = int(L.tg_ppo_loss_workspace(4097, 6))
    assert need == 16 + 8 * 17 * 11
    got = _ppo(inp, dev, kw, path=GRID, workspace_bytes=need)                 # _ppo puts the workspace between guards, to the byte
    ex = ref.ppo_exact(**inp, **kw)
    _within(_named(got), ex, ref.ppo_bounds(ex, **inp, **kw), ref.STATS + ("log_prob", "dmean", "dlog_std", "dvalues"), "4097 grid")
    _ppo(inp, dev, kw, path=GRID, workspace_bytes=need - 1, expect_error=True)
    _ppo(inp, dev, kw, path=AUTO, workspace_bytes=need - 1, expect_error=True)
    _ppo(inp, dev, kw, path=GRID, no_workspace=True, expect_error=True)
    assert L.tg_ppo_loss_workspace(4097, 0) < 0 and L.tg_ppo_loss_workspace(4097, 17) < 0 and L.tg_ppo_loss_workspace(0, 6) < 0
    small, kws = _case(64, 2, False, None, True)                              # one workgroup needs none
    devs = _upload(small)
    a, b = _ppo(small, devs, kws, no_workspace=True, workspace_bytes=0), _ppo(small, devs, kws)
    assert all(_bits(a[k], b[k]) for k in OUTPUTS)


def test_error_returns_write_nothing():
    inp, kw = _case(70, 3, True, CLIP_VF, True)
    dev = _upload(inp)
    bad = lambda **over: _ppo(inp, dev, over.pop("kw", kw), expect_error=True, path=over.pop("path", AUTO), **over)   # noqa: E731
    for name in INPUTS:
        bad(**{name: None})                                                   # old_values: needed with the value clip
    bad(outputs=OUTPUTS[1:])                                                  # NULL stats_out
    for width in (0, -1, 17):
        bad(A=width, stride=0)
    for stride in (1, 2, 4, -3, 6):
        bad(stride=stride)
    for rows in (0, -1):
        bad(B=rows)
    bad(clip_range=-0.1)
    bad(clip_range=float("nan"))
    bad(kw=dict(kw, clip_range_vf=float("nan")))
    for path in (-1, 3, 99):
        bad(path=path)
    ok = _ppo(inp, dev, dict(kw, clip_range_vf=None), old_values=None)        # without the clip old_values may be NULL
    assert np.isfinite(ok["stats"]).all()


@pytest.mark.parametrize("B,A,per_row", [(64, 2, False), (257, 6, False), (1000, 16, True), (4097, 3, False)])
def test_the_heads_own_sample_gives_ratio_one_exactly(B, A, per_row):
    """tg_action_head's Gaussian sample and log_prob fed back as actions and old_log_prob: the log-prob chain gives the head's bits, so
    ratio == 1 in every row, approx_kl == 0 and clip_fraction == 0 - a chain that merely agrees to rounding would not."""
    rng = np.random.default_rng(B + A)
    mean = rng.uniform(-1.5, 1.5, (B, A)).astype(f32)
    ls = rng.uniform(-3.0, 0.5, (B, A) if per_row else (A,)).astype(f32)
    actions, log_prob, _ = _head(head.GAUSSIAN, mean, ls, seed=11, counter=B)
    inp = dict(mean=mean, log_std=ls, values=rng.standard_normal(B).astype(f32), actions=actions, old_log_prob=log_prob,
               advantages=rng.standard_normal(B).astype(f32), returns=rng.standard_normal(B).astype(f32), old_values=None)
    kw = dict(clip_range=CLIP, clip_range_vf=None, ent_coef=ENT, vf_coef=VF, normalize_advantage=True)
    for path in (AUTO, GRID):
        got = _ppo(inp, _upload(inp), kw, path=path)
        assert _bits(got["log_prob"], log_prob)
        assert got["stats"][4] == 0 and got["stats"][5] == 0                  # approx_kl, clip_fraction
        # ratio == 1: the policy loss is -mean(adv_n), the gradient at log_prob -adv_n / B in every row
        same = dict(inp, old_log_prob=ref.ppo_exact(**inp, **kw)["log_prob"])    # the float64 composition's own ratio == 1
        ex = ref.ppo_exact(**same, **kw)
        assert (ex["ratio"] == 1).all()
        _within(_named(got), ex, ref.ppo_bounds(ex, **same, **kw), ("policy_loss", "value_loss", "entropy_loss", "loss", "dmean", "dvalues"), "exact")
    got = _ppo(inp, _upload(inp), dict(kw, clip_range=0.0))                   # 1 <= ratio <= 1: inside the clamp, nothing counted as clipped
    assert got["stats"][5] == 0 and np.abs(got["dmean"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------- tg_squashed_rsample
@pytest.mark.parametrize("B,A", [(1, 1), (2, 2), (64, 2), (255, 6), (257, 16), (1000, 6)])
def test_rsample_is_the_heads_squashed_mode_and_its_backward_stays_within_bounds(B, A):
    inp = ref.rsample_inputs(B, A, seed=B + A)
    mean, ls = inp["mean"], inp["log_std"]
    for noise in (None, inp["eps"]):
        for log_std in (ls, ls[0].copy()):                                    # [B, A] and [A]
            want = _head(head.SQUASHED, mean, log_std, seed=5, counter=9, clamp=(-20.0, 2.0), noise_in=noise)
            fwd = _rsample(mean, log_std, seed=5, counter=9, noise_in=noise)
            assert _bits(fwd["actions"], want[0]) and _bits(fwd["log_prob"], want[1]) and _bits(fwd["eps"], want[2])
            bare = _rsample(mean, log_std, seed=5, counter=9, noise_in=noise, save=False)
            assert _bits(bare["actions"], fwd["actions"]) and _bits(bare["log_prob"], fwd["log_prob"])
    fwd = _rsample(mean, ls, seed=5, counter=9)
    eps = fwd["eps"]                                                          # the kernel's own draw is the point of evaluation
    full = _rsample_bwd(fwd, ls, inp["g_a"], inp["g_lp"])
    for g_a, g_lp in ((inp["g_a"], inp["g_lp"]), (inp["g_a"], None), (None, inp["g_lp"])):
        got = _rsample_bwd(fwd, ls, g_a, g_lp)
        ex, bounds = ref.rsample_exact(mean, ls, eps, g_a, g_lp), ref.rsample_bounds(mean, ls, eps, g_a, g_lp)
        _within(got, ex, bounds, ("dmean", "dlog_std"), (B, A, g_a is None, g_lp is None))
        inside = (ls >= -20) & (ls <= 2)
        assert (got["dlog_std"][~inside] == 0).all()
        if g_lp is not None:
            assert (got["dlog_std"][(ls == -20) | (ls == 2)] != 0).all()      # the mask is inclusive
    for name in ("dmean", "dlog_std"):                                        # each output alone
        assert _bits(_rsample_bwd(fwd, ls, inp["g_a"], inp["g_lp"], outputs=(name,))[name], full[name])
    assert _bits(_rsample_bwd(fwd, ls, inp["g_a"], inp["g_lp"])["dlog_std"], full["dlog_std"])       # a second call


def test_rsample_saturated_stays_finite():
    B, A = 300, 6
    inp = ref.rsample_inputs(B, A, seed=17, saturated=True)
    inp["mean"][:3] = [[20.0] * A, [-20.0] * A, [19.5, -19.5] * 3]
    fwd = _rsample(inp["mean"], inp["log_std"], seed=1, counter=2)
    assert all(np.isfinite(v).all() for v in fwd.values()) and (np.abs(fwd["actions"]) <= 1).all() and (np.abs(fwd["actions"][:2]) == 1).all()
    got = _rsample_bwd(fwd, inp["log_std"], inp["g_a"], inp["g_lp"])
    assert all(np.isfinite(v).all() for v in got.values())                    # no NaN, no infinity: w >= 1e-6
    assert (got["dmean"][:2] == 0).all()                                      # 1 - a^2 == 0 at a = +-1


def test_rsample_error_returns_write_nothing():
    inp = ref.rsample_inputs(70, 3, seed=2)
    mean, ls = inp["mean"], inp["log_std"]
    for over in (dict(null=("mean",)), dict(null=("ls",)), dict(null=("actions",)), dict(null=("log_prob",)), dict(A=0), dict(A=17),
                 dict(stride=1), dict(stride=6), dict(B=0), dict(B=-1)):
        _rsample(mean, ls, expect_error=True, **over)
    _rsample(mean, ls, clamp=(1.0, 0.5), expect_error=True)
    fwd = _rsample(mean, ls)
    for over in (dict(null=("actions",)), dict(null=("eps",)), dict(null=("sigma",)), dict(null=("ls",)), dict(A=0), dict(A=17), dict(stride=2),
                 dict(B=0)):
        _rsample_bwd(fwd, ls, inp["g_a"], inp["g_lp"], expect_error=True, **over)
    _rsample_bwd(fwd, ls, inp["g_a"], inp["g_lp"], clamp=(float("nan"), 0.5), expect_error=True)
