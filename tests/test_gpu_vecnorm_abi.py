"""tg_vecnorm_update and tg_vecnorm_apply (csrc/tg_vecnorm.hip) called directly on raw pointers: row counts round the 64-lane wavefront and the
256-row chunk, every table size and the total-width limit, an apply over a row count of its own, the returns recurrence under every done
pattern, and the error returns that take no launch.  Every output sits between guard bytes inside a larger buffer.

Statistics, returns and outputs are compared with tests/vecnorm_ref.py (device_order) bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vecnorm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import Guarded  # noqa: E402
from vecnorm_device import Device, _bits, _done_pattern, _lib, _ptrs, _stream  # noqa: E402

ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000)
TABLES = ((1,), (3, 10), (34, 68, 1), (68, 34, 10, 3))       # every width, one to four arrays
DONES = ("none", "all", "alternating", "first", "last")


def _batch(rng, rows, widths):
    """float32 [rows, d] per array: every column with a scale and an offset of its own (metres, radians per second, angles)."""
    return [((rng.standard_normal((rows, d)) * 10.0 ** rng.integers(-3, 3, d) + rng.standard_normal(d) * 10.0 ** rng.integers(-2, 3, d))
             .astype(np.float32)) for d in widths]


def _steps(dev, rng, n_steps, pattern="alternating"):
    for step in range(n_steps):
        xs = _batch(rng, dev.N, dev.widths)
        rewards = rng.standard_normal(dev.N).astype(np.float32)
        dones = _done_pattern(pattern, dev.N) if step % 2 == 0 else _done_pattern("none", dev.N)
        dev.update(xs, rewards)
        outs, rew = dev.apply(xs, dev.N, rewards=rewards, dones=dones, reset=True)
        w_obs, w_rew, _ = dev.model.step(dict(enumerate(xs)), rewards, dones)
        for i, o in enumerate(outs):
            assert _bits(o, w_obs[i]), (step, i)
        assert _bits(rew, w_rew), step
        dev.check(step)


@pytest.mark.parametrize("N", ROWS)
def test_update_and_apply_equal_the_restatement(N):
    rng = np.random.default_rng(N)
    for widths in TABLES:
        dev = Device(widths, N)
        _steps(dev, rng, 5)
        for R in (1, 127, 2 * 64):                                # a row count of the apply's own: minibatches, the terminal batch
            xs = _batch(rng, R, widths)
            outs, _ = dev.apply(xs, R)
            want = dev.model.normalize_obs(dict(enumerate(xs)))
            for i, o in enumerate(outs):
                assert _bits(o, want[i]), (widths, R, i)
        dev.check("apply alone")                                  # an apply changes no statistics


@pytest.mark.parametrize("widths,N", [((512,), 257), ((500, 3, 8, 1), 65), ((1, 1, 1, 509), 513), ((3,), 65535)])
def test_total_width_at_the_limit(widths, N):
    dev = Device(widths, N, clip_obs=2.5, epsilon=1e-3)
    _steps(dev, np.random.default_rng(sum(widths) + N), 5)


def test_updates_without_the_returns_block_and_in_place_apply():
    """reset()'s form: the arrays alone, then an apply that zeroes every return; and sample(env=)'s form: outputs over their inputs."""
    capi, L = _lib()
    rng = np.random.default_rng(11)
    dev = Device((10, 3), 300)
    _steps(dev, rng, 2, pattern="none")
    assert np.abs(dev.model.returns).min() > 0
    xs = _batch(rng, 300, dev.widths)
    dev.update(xs)
    outs, _ = dev.apply(xs, 300, reset=True)                      # no done flags: every env
    want = dev.model.reset(dict(enumerate(xs)))
    for i, o in enumerate(outs):
        assert _bits(o, want[i]), i
    dev.check("reset")
    ins = [Guarded(x.nbytes, fill=x) for x in xs]
    rewards = rng.standard_normal(77).astype(np.float32)
    rw = Guarded(rewards.nbytes, fill=rewards)
    capi.check(L.tg_vecnorm_apply(2, _ptrs(ins), _ptrs(ins), dev.w_tab, _ptrs(dev.stats), 300, 10.0, 1e-8, C.c_void_p(rw.ptr), C.c_void_p(rw.ptr), 77,
                                  C.c_void_p(dev.ret_stats.ptr), 10.0, None, None, 0, _stream()))
    torch.cuda.synchronize()
    for i, g in enumerate(ins):
        assert _bits(g.host(np.float32).reshape(xs[i].shape), want[i]) and g.guards_intact()
    assert _bits(rw.host(np.float32), dev.model.normalize_reward(rewards)) and rw.guards_intact()


@pytest.mark.parametrize("gamma", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("pattern", DONES)
def test_returns_recurrence(pattern, gamma):
    rng = np.random.default_rng(len(pattern))
    for N in (1, 300):
        dev = Device((), N, gamma=gamma, clip_reward=1.5)
        for step in range(4):
            rewards = (rng.standard_normal(N) * 3).astype(np.float32)
            dones = _done_pattern(pattern if step != 1 else "none", N)
            dev.update([], rewards)
            _, rew = dev.apply([], 0, rewards=rewards, dones=dones, reset=True)
            _, want, _ = dev.model.step({}, rewards, dones)
            assert _bits(rew, want), (N, step)
            dev.check((N, step))


def test_training_off_applies_without_updating():
    rng = np.random.default_rng(5)
    dev = Device((3,), 300)
    _steps(dev, rng, 3)
    dev.model.training = False
    before = [g.host(np.float64).copy() for g in dev.stats] + [dev.ret_stats.host(np.float64).copy()]
    for step in range(3):
        xs, rewards, dones = _batch(rng, 300, dev.widths), rng.standard_normal(300).astype(np.float32), _done_pattern("alternating", 300)
        outs, rew = dev.apply(xs, 300, rewards=rewards, dones=dones, reset=True)
        w_obs, w_rew, _ = dev.model.step({0: xs[0]}, rewards, dones)
        assert _bits(outs[0], w_obs[0]) and _bits(rew, w_rew)
        dev.check(step)
    after = [g.host(np.float64) for g in dev.stats] + [dev.ret_stats.host(np.float64)]
    assert all(_bits(a, b) for a, b in zip(before, after))


def test_error_returns_take_no_launch():
    capi, L = _lib()
    x, st, out, scratch = Guarded(64 * 4 * 4), Guarded(9 * 8), Guarded(64 * 4 * 4), Guarded(4096)
    ret, rw, rst = Guarded(64 * 8), Guarded(64 * 4), Guarded(24)
    p = C.c_void_p
    xs, sts, outs = _ptrs([x] * 5, 5), _ptrs([st] * 5, 5), _ptrs([out] * 5, 5)
    w = lambda *v: (C.c_int32 * 5)(*v)   # noqa: E731

    def update(n=1, x_tab=xs, widths=w(4), s_tab=sts, N=64, returns=ret.ptr, rewards=rw.ptr, ret_stats=rst.ptr, scr=scratch.ptr):
        return L.tg_vecnorm_update(n, x_tab, widths, s_tab, N, p(returns), p(rewards), 0.99, p(ret_stats), p(scr), _stream())

    def apply(n=1, x_tab=xs, o_tab=outs, widths=w(4), s_tab=sts, R=64, clip=10.0, eps=1e-8, rewards=rw.ptr, rewards_out=rw.ptr, n_rewards=64,
              ret_stats=rst.ptr, returns=ret.ptr, dones=None, n_reset=64):
        return L.tg_vecnorm_apply(n, x_tab, o_tab, widths, s_tab, R, clip, eps, p(rewards), p(rewards_out), n_rewards, p(ret_stats), 10.0, p(returns),
                                  p(dones), n_reset, _stream())

    bad = [update(n=5, widths=w(1, 1, 1, 1, 1)), update(n=-1), update(widths=w(513)), update(n=2, widths=w(500, 13)), update(widths=w(0)),
           update(N=0), update(N=65536), update(N=-3), update(x_tab=None), update(widths=None), update(s_tab=None),
           update(x_tab=_ptrs([None])), update(s_tab=_ptrs([None])), update(scr=None), update(returns=None), update(rewards=None),
           update(ret_stats=None),
           apply(n=5, widths=w(1, 1, 1, 1, 1)), apply(widths=w(513)), apply(o_tab=None), apply(o_tab=_ptrs([None])), apply(x_tab=_ptrs([None])),
           apply(s_tab=None), apply(R=0), apply(R=-1), apply(R=1 << 31), apply(clip=-1.0), apply(eps=-1e-8), apply(clip=float("nan")),
           apply(rewards_out=None), apply(ret_stats=None), apply(n_rewards=-1), apply(n_reset=-1), apply(returns=None, dones=rw.ptr)]
    assert bad == [-1] * len(bad), bad
    assert b"tg_vecnorm_apply" in L.tg_last_error()
    assert update(N=65535, n=0, returns=None, rewards=None, ret_stats=None) == 0          # nothing to do: no launch either
    assert apply(n=0, rewards=None, returns=None) == 0
    torch.cuda.synchronize()
    for g in (x, st, out, scratch, ret, rw, rst):
        assert g.guards_intact() and bool((g.payload() == 0xA5).all())                     # nothing was written
