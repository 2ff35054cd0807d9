"""tactile_gym_amd.action_head and tactile_gym_amd.collect without a GPU: the restatement (tests/action_head_ref.py) against torch's own float32
distributions within the bound its docstring derives, six usual mistakes far outside it, the draws, the exact paths, the classes and the two
loops on a fake env and fake buffers with the C call replaced by device_order, the C ABI entry and the kernel's resources."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import build_units  # noqa: E402
import action_head_ref as ref  # noqa: E402

from tactile_gym_amd import _capi, spaces  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_action_head"]                # at import: the whole file needs the feature
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- test 1: the bound
N1, A1 = 1000, 6
LO1, HI1 = np.full(A1, -1.0, f32), np.full(A1, 1.0, f32)


@pytest.fixture(scope="module")
def case1():
    """The issue's inputs, once: mean in [-1.5, 1.5], log_std in [-3, -1.5]; torch's float32 CPU results and the float64 ones at the same inputs."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(20240613)
    mean = rng.uniform(-1.5, 1.5, (N1, A1)).astype(f32)
    ls = rng.uniform(-3.0, -1.5, (N1, A1)).astype(f32)
    eps = rng.standard_normal((N1, A1)).astype(f32)
    tm, tl, te = torch.from_numpy(mean), torch.from_numpy(ls), torch.from_numpy(eps)
    dist = torch.distributions.Normal(tm, tl.exp())
    x = tm + dist.scale * te                                                  # rsample with the noise given
    g = dist.log_prob(x).sum(dim=1)                                           # DiagGaussianDistribution.log_prob
    a = torch.tanh(x)
    s = g - torch.log(1 - a ** 2 + 1e-6).sum(dim=1)                           # SquashedDiagGaussianDistribution.log_prob
    lo, hi = torch.from_numpy(LO1), torch.from_numpy(HI1)
    env = lo + (0.5 * (a + 1.0) * (hi - lo))                                  # unscale_action
    return dict(mean=mean, ls=ls, eps=eps, x=x.numpy(), g=g.numpy(), a=a.numpy(), s=s.numpy(), env=env.numpy())


def test_torch_float32_stays_within_the_bound_of_exact(case1):
    c = case1
    assert np.abs(c["x"]).max() < 3.0 and (1.0 / (1.0 - c["a"].astype(np.float64) ** 2 + 1e-6)).max() < 110.0      # the issue's regime
    checks = {
        "x": (c["x"], ref.exact_x(c["mean"], c["ls"], c["eps"]), ref.bound_x(c["mean"], c["ls"], c["eps"])),
        "tanh": (c["a"], ref.exact_tanh(c["x"]), ref.bound_tanh(c["x"])),
        "unscale": (c["env"], ref.exact_unscale(c["a"], LO1, HI1), ref.bound_unscale(c["a"], LO1, HI1)),
        "gaussian log_prob": (c["g"], ref.exact_log_prob(c["x"], c["mean"], c["ls"]), ref.bound_gaussian_sum(c["x"], c["mean"], c["ls"], True)),
        "squashed log_prob": (c["s"], ref.exact_log_prob(c["x"], c["mean"], c["ls"], c["a"]),
                              ref.bound_squashed_sum(c["x"], c["mean"], c["ls"], c["a"], True)),
    }
    for name, (got, want, bound) in checks.items():
        err = np.abs(got.astype(np.float64) - want)
        print(f"{name}: max error {err.max():.3g} on magnitudes up to {np.abs(want).max():.3g}, bound there {bound.reshape(-1)[err.argmax()]:.3g}, "
              f"worst error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), name


def test_device_order_stays_within_the_bound_of_exact(case1):
    """The kernel's order (log_std itself where torch takes log(exp(log_std))) at the same inputs, stage by stage at its own outputs."""
    c = case1
    for mode in (ref.GAUSSIAN, ref.SQUASHED):
        d = ref.device_order(mode, c["mean"], c["ls"], LO1, HI1, noise=c["eps"])
        x = d["gaussian"]
        assert (np.abs(x - ref.exact_x(c["mean"], c["ls"], c["eps"])) <= ref.bound_x(c["mean"], c["ls"], c["eps"])).all()
        if mode == ref.GAUSSIAN:
            assert (np.abs(d["log_prob"] - ref.exact_log_prob(x, c["mean"], c["ls"])) <= ref.bound_gaussian_sum(x, c["mean"], c["ls"])).all()
        else:
            a = d["actions"]
            assert (np.abs(a - ref.exact_tanh(x)) <= ref.bound_tanh(x)).all()
            assert (np.abs(d["env"] - ref.exact_unscale(a, LO1, HI1)) <= ref.bound_unscale(a, LO1, HI1)).all()
            assert (np.abs(d["log_prob"] - ref.exact_log_prob(x, c["mean"], c["ls"], a)) <= ref.bound_squashed_sum(x, c["mean"], c["ls"], a)).all()


def _mistakes(c):
    """name -> (wrong value, exact value, bound, factor by which the bound must be broken), each in float64 from the float32 inputs of its stage."""
    x, mean, ls, a = c["x"], c["mean"], c["ls"], c["a"]
    g, k = ref.gaussian_terms(x, mean, ls), ref.correction_terms(a)
    a64 = a.astype(np.float64)
    sq = (N1 // A1) * A1                                                      # rows in square blocks [A, A]: a sum over the other axis has the same shape
    blocks = g[:sq].reshape(-1, A1, A1)
    return {
        "-log sigma left out": ((g + ls.astype(np.float64)).sum(1), g.sum(1), ref.bound_gaussian_sum(x, mean, ls, True), 100.0),
        "sum over the wrong axis": (blocks.sum(1).reshape(-1), blocks.sum(2).reshape(-1), ref.bound_gaussian_sum(x, mean, ls, True)[:sq], 100.0),
        "tanh correction left out": (g.sum(1), g.sum(1) - k.sum(1), ref.bound_squashed_sum(x, mean, ls, a, True), 100.0),
        # The one mistake that 100 x cannot catch, by arithmetic (a deviation from the issue, which asks 100 x of every mistake):
        # 1 - (a + 1e-6)^2 moves w = 1 - a^2 + 1e-6 by (1 + 2 a) 1e-6 <= 3e-6 = 50 U, and any bound has to allow the three roundings behind w,
        # e_w = U (a^2 + |1 - a^2| + w + 1e-6) >= U (1 + w), on the same w with the same condition number 1 / w: the ratio stays below
        # 3e-6 / (U (1 + w)) < 50 in every column, and the other terms of the bound take more off.  It is taken on the correction sum alone
        # against that sum's own share of the bound (the Gaussian sum's share would only hide it); measured 14 x, and 5 is asserted.
        "epsilon inside the square": (np.log(1.0 - (a64 + 1e-6) ** 2).sum(1), k.sum(1), ref.bound_correction_sum(a), 5.0),
        "unscale_action without the 0.5": (LO1 + (a64 + 1.0) * (HI1.astype(np.float64) - LO1), ref.exact_unscale(a, LO1, HI1),
                                           ref.bound_unscale(a, LO1, HI1), 100.0),
        "clip applied to the stored action": (np.clip(ref.exact_x(mean, ls, c["eps"]), LO1, HI1), ref.exact_x(mean, ls, c["eps"]),
                                              ref.bound_x(mean, ls, c["eps"]), 100.0),
    }


@pytest.mark.parametrize("name", ["-log sigma left out", "sum over the wrong axis", "tanh correction left out", "epsilon inside the square",
                                  "unscale_action without the 0.5", "clip applied to the stored action"])
def test_usual_mistakes_break_the_bound(case1, name):
    """Each by more than 100 x, but the epsilon inside the square: measured 14 x its stage's bound where arithmetic keeps any bound's
    ratio below 50 x (see _mistakes; a deviation from the issue's 100 x)."""
    wrong, want, bound, factor = _mistakes(case1)[name]
    ratio = np.abs(wrong - want) / bound
    print(f"{name}: worst error / bound {ratio.max():.4g}, median {np.median(ratio):.4g}")
    assert ratio.max() > factor, name


# ---------------------------------------------------------------------------------------------------------------- test 2: the draws
STREAMS = ((0, 0), (1, 7), (0xDEADBEEFCAFEF00D, 1 << 40))


def test_integers_are_the_generators():
    for seed, counter in STREAMS:
        e = np.array([0, 1, 2, 3, 255, 256, 1 << 20, (1 << 31) + 5, (1 << 40) + 1], dtype=np.uint64)
        got = ref.bits24(seed, counter, e)
        assert got.tolist() == [ref.bits24_int(seed, counter, int(i)) for i in e] and (got >= 0).all() and (got < 1 << 24).all()
    # the uniform mode's integers are tg_sample_actions': u = k 2^-24 with k the 24 bits of element e (csrc/tg_api.hip k_sample_actions)
    u = ref.uniform_draws(3, 5, 64)
    assert u.dtype == f32 and [int(v * 16777216) for v in u] == [ref.bits24_int(3, 5, i) for i in range(64)]
    d = ref.device_order(ref.UNIFORM, None, None, [-0.25, -0.25], [0.25, 0.25], seed=3, counter=5, shape=(32, 2))
    assert np.array_equal(d["env"], (f32(-0.25) + f32(0.5) * u).reshape(32, 2))          # lo + (hi - lo) u, tg_sample_actions' floats


def test_normal_draws_moments_ks_range_and_independence():
    stats = pytest.importorskip("scipy.stats")
    n = 1 << 18
    streams = [ref.normal_draws(seed, counter, n) for seed, counter in STREAMS]
    for (seed, counter), z in zip(STREAMS, streams):
        z64 = z.astype(np.float64)
        m1, m2, m3, m4 = z64.mean(), (z64 ** 2).mean(), (z64 ** 3).mean(), (z64 ** 4).mean()
        p = stats.kstest(z64, stats.norm.cdf).pvalue
        print(f"seed {seed:#x} counter {counter}: moments {m1:.4f} {m2:.4f} {m3:.4f} {m4:.4f}, max |eps| {np.abs(z).max():.3f}, KS p = {p:.3f}")
        # standard errors over n draws: 1 / sqrt(n), sqrt(2 / n), sqrt(15 / n), sqrt(96 / n); five of them each
        assert abs(m1) < 5 / math.sqrt(n) and abs(m2 - 1) < 5 * math.sqrt(2 / n) and abs(m3) < 5 * math.sqrt(15 / n) \
            and abs(m4 - 3) < 5 * math.sqrt(96 / n)
        assert p > 0.01
        assert z.dtype == f32 and np.abs(z).max() <= 5.78 and np.isfinite(z).all()
    assert not np.array_equal(streams[0], streams[1]) and abs(np.corrcoef(streams[0], streams[1])[0, 1]) < 5 / math.sqrt(n)
    assert not np.array_equal(ref.normal_draws(0, 0, 4096), ref.normal_draws(0, 1, 4096))           # another counter
    assert not np.array_equal(ref.normal_draws(0, 0, 4096), ref.normal_draws(1, 0, 4096))           # another seed
    assert np.array_equal(ref.normal_draws(1, 7, 4096), streams[1][:4096])                          # element e depends on (seed, counter, e) only
    # the extreme of the range: k1 = 0 gives u1 = 2^-24, the largest radius
    assert math.sqrt(-2 * math.log(2.0 ** -24)) < 5.78


# ---------------------------------------------------------------------------------------------------------------- test 3: the exact paths
def test_clip_is_np_clip_on_bounds_infinities_and_nan():
    lo, hi = np.array([-0.25, -1.0, 0.0], f32), np.array([0.25, 2.0, 0.0], f32)
    x = np.array([[-0.25, 2.0, 0.0], [0.25, -1.0, 1e-30], [np.inf, -np.inf, -1e-30], [-np.inf, np.inf, np.nan], [0.1, 0.5, 3.0],
                  [np.nextafter(f32(0.25), f32(1)), np.nextafter(f32(-1), f32(-2)), 0.0]], f32)
    got = ref.clip_f32(x, lo, hi)
    assert np.array_equal(got, np.clip(x, lo, hi), equal_nan=True) and got.dtype == f32
    mean = x.copy()
    mean[3, 2] = 0.5
    d = ref.device_order(ref.GAUSSIAN, mean, np.zeros(3, f32), lo, hi, deterministic=True)
    assert np.array_equal(d["env"], np.clip(mean, lo, hi)) and np.array_equal(d["actions"], mean) and d["actions"] is d["gaussian"]


def test_scale_action_inverts_unscale_action():
    rng = np.random.default_rng(5)
    lo, hi = np.array([-0.25, -1.0, 0.5, -3.0], f32), np.array([0.25, 1.0, 2.5, 7.0], f32)
    a = rng.uniform(-1, 1, (500, 4)).astype(f32)
    a[0], a[1] = -1.0, 1.0
    env = ref.unscale_f32(a, lo, hi)
    assert (env >= lo).all() and (env <= hi).all() and np.array_equal(env[0], lo) and np.array_equal(env[1], hi)
    back = ref.scale_f32(env, lo, hi)
    # each direction rounds a few times: the round trip is good to a few float32 roundings of quantities of magnitude <= 1 + |lo| / (hi - lo)
    assert np.abs(back.astype(np.float64) - a).max() <= 8 * ref.U * (1 + np.abs(lo) / (hi - lo)).max()
    assert np.abs(ref.exact_scale(ref.exact_unscale(a, lo, hi), lo, hi) - a).max() < 1e-14
    # the uniform mode: env in [lo, hi), actions = scale_action(env) in [-1, 1]
    d = ref.device_order(ref.UNIFORM, None, None, lo, hi, seed=2, counter=9, shape=(500, 4))
    assert (d["env"] >= lo).all() and (d["env"] <= hi).all() and (np.abs(d["actions"]) <= 1).all() and d["log_prob"] is None
    assert np.array_equal(d["actions"], ref.scale_f32(d["env"], lo, hi))
    assert np.array_equal(d["noise"], ref.uniform_draws(2, 9, 2000).reshape(500, 4))


def test_deterministic_mode_returns_the_mean_and_its_tanh():
    rng = np.random.default_rng(6)
    mean, ls = rng.uniform(-2, 2, (65, 3)).astype(f32), rng.uniform(-25, 4, (65, 3)).astype(f32)
    lo, hi = np.full(3, -0.25, f32), np.full(3, 0.25, f32)
    g = ref.device_order(ref.GAUSSIAN, mean, ls[0], lo, hi, deterministic=True)
    assert np.array_equal(g["actions"], mean) and np.array_equal(g["noise"], np.zeros_like(mean))
    assert np.array_equal(g["log_prob"], ref.device_order(ref.GAUSSIAN, mean, ls[0], lo, hi, noise=np.zeros_like(mean))["log_prob"])
    assert np.abs(g["log_prob"] - (-ls[0].astype(np.float64) - ref.LOG_SQRT_2PI).sum()).max() < 1e-4      # the density at the mean
    s = ref.device_order(ref.SQUASHED, mean, ls, lo, hi, log_std_min=-20, log_std_max=2, deterministic=True)
    assert np.array_equal(s["actions"], np.tanh(mean.astype(np.float64)).astype(f32)) and np.array_equal(s["gaussian"], mean)
    # the clamp: log_std outside [-20, 2] counts as the bound
    clamped = ref.device_order(ref.SQUASHED, mean, np.clip(ls, -20, 2), lo, hi, deterministic=True)
    assert np.array_equal(s["log_prob"], clamped["log_prob"])
    assert not np.array_equal(s["log_prob"], ref.device_order(ref.SQUASHED, mean, ls, lo, hi, deterministic=True)["log_prob"])


# ---------------------------------------------------------------------------------------------------------------- test 4: the module and the loops
torch = pytest.importorskip("torch")
ACT = spaces.Box(low=-0.25, high=0.25, shape=(2,), dtype=np.float32)


def _stubbed(cls_name, *args, **kwargs):
    """A head whose C call is device_order on the CPU tensors' memory."""
    from tactile_gym_amd import action_head
    base = getattr(action_head, cls_name)

    class Stubbed(base):
        def _is_device(self, t):
            return True

        def _c_head(self, mode, mean, log_std, stride, deterministic):
            self.calls.append((mode, stride, deterministic, self.seed, self.counter))
            d = ref.device_order(mode, None if mean is None else mean.numpy(), None if log_std is None else log_std.numpy(), self.low, self.high,
                                 self.log_std_min, self.log_std_max, deterministic, self.seed, self.counter, shape=(self.num_envs, self.action_dim))
            for name, key in (("actions", "actions"), ("env_actions", "env"), ("gaussian_actions", "gaussian"), ("log_prob", "log_prob"),
                              ("noise", "noise")):
                if d[key] is not None:
                    getattr(self, name).numpy()[:] = d[key]

    head = Stubbed(*args, **kwargs)
    head.calls = []
    return head


def test_heads_follow_the_restatement_and_count_their_calls():
    import tactile_gym_amd as tg
    from tactile_gym_amd import action_head
    assert tg.action_head is action_head and tg.DeviceDiagGaussian is action_head.DeviceDiagGaussian
    assert tg.DeviceSquashedDiagGaussian is action_head.DeviceSquashedDiagGaussian
    rng = np.random.default_rng(0)
    mean, ls = torch.from_numpy(rng.uniform(-0.3, 0.3, (5, 2)).astype(f32)), torch.from_numpy(rng.uniform(-3, -1, (5, 2)).astype(f32))
    g = _stubbed("DeviceDiagGaussian", ACT, seed=11)
    assert (g.seed, g.counter, g.num_envs, g.log_std_min, g.log_std_max) == (11, 0, None, -math.inf, math.inf)
    out = g.sample(mean, ls[0])
    assert out[0] is g.actions and out[1] is g.env_actions and out[2] is g.log_prob and g.counter == 1 and g.num_envs == 5
    want = ref.device_order(ref.GAUSSIAN, mean.numpy(), ls[0].numpy(), ACT.low, ACT.high, seed=11, counter=0)
    for t, key in ((g.actions, "actions"), (g.env_actions, "env"), (g.log_prob, "log_prob"), (g.noise, "noise"), (g.gaussian_actions, "gaussian")):
        assert t.dtype == torch.float32 and np.array_equal(t.numpy(), want[key]), key
    assert (g.env_actions.numpy() != g.actions.numpy()).any() and np.abs(g.env_actions.numpy()).max() <= 0.25
    ptrs = [t.data_ptr() for t in out]
    out2 = g.sample(mean, ls, deterministic=True)                              # [N, A] log_std, the same tensors again, the next counter
    assert [t.data_ptr() for t in out2] == ptrs and g.counter == 2 and np.array_equal(g.actions.numpy(), mean.numpy())
    assert g.calls == [(ref.GAUSSIAN, 0, False, 11, 0), (ref.GAUSSIAN, 2, True, 11, 1)]
    s = _stubbed("DeviceSquashedDiagGaussian", ACT, seed=4, num_envs=5, device="cpu")
    assert (s.log_std_min, s.log_std_max, s.num_envs) == (-20.0, 2.0, 5)
    a, e = s.sample_uniform()
    want = ref.device_order(ref.UNIFORM, None, None, ACT.low, ACT.high, seed=4, counter=0, shape=(5, 2))
    assert a is s.actions and e is s.env_actions and np.array_equal(a.numpy(), want["actions"]) and np.array_equal(e.numpy(), want["env"])
    a, e, lp = s.sample(mean, ls)
    want = ref.device_order(ref.SQUASHED, mean.numpy(), ls.numpy(), ACT.low, ACT.high, -20, 2, seed=4, counter=1)
    assert np.array_equal(a.numpy(), want["actions"]) and np.array_equal(e.numpy(), want["env"]) and np.array_equal(lp.numpy(), want["log_prob"])
    assert s.counter == 2 and [c[0] for c in s.calls] == [ref.UNIFORM, ref.SQUASHED]
    # state: seed and counter, nothing else
    assert s.state_dict() == {"seed": 4, "counter": 2}
    other = _stubbed("DeviceSquashedDiagGaussian", ACT, seed=99, num_envs=5, device="cpu")
    other.load_state_dict(s.state_dict())
    s.sample(mean, ls), other.sample(mean, ls)
    assert np.array_equal(s.actions.numpy(), other.actions.numpy()) and other.counter == 3


def test_heads_refuse_what_they_cannot_do():
    from tactile_gym_amd.action_head import DeviceDiagGaussian, DeviceSquashedDiagGaussian
    mean, ls = torch.zeros(5, 2), torch.zeros(2)
    with pytest.raises(ValueError, match="ROCm device"):
        DeviceDiagGaussian(ACT).sample(mean, ls)                               # CPU tensors: there is no CPU path
    g = _stubbed("DeviceDiagGaussian", ACT)
    for bad_mean, bad_ls in ((torch.zeros(5, 3), ls), (torch.zeros(5), ls), (mean, torch.zeros(3)), (mean, torch.zeros(4, 2)), (mean.double(), ls),
                             (mean, ls.double()), (mean, torch.zeros(1, 2))):
        with pytest.raises(ValueError):
            g.sample(bad_mean, bad_ls)
    with pytest.raises(ValueError, match="contiguous"):
        g.sample(torch.zeros(2, 5).t(), ls)                                    # a copy would be a second launch: refused, not made
    with pytest.raises(ValueError, match="contiguous"):
        g.sample(mean, torch.zeros(2, 5).t())
    with pytest.raises(TypeError):
        g.sample(mean.numpy(), ls)
    with pytest.raises(TypeError):
        g.sample(mean, [0.0, 0.0])
    assert g.counter == 0 and g.calls == []                                    # a refused call draws nothing
    g.sample(mean, ls)
    with pytest.raises(ValueError, match="shape"):
        g.sample(torch.zeros(6, 2), ls)                                        # the batch size is fixed by the first call
    box = lambda lo, hi, n=2, dt=np.float32: spaces.Box(low=lo, high=hi, shape=(n,), dtype=dt)   # noqa: E731
    for cls, space in ((DeviceDiagGaussian, box(-1, 1, 17)), (DeviceDiagGaussian, box(-np.inf, np.inf)), (DeviceSquashedDiagGaussian, box(0.5, 0.5)),
                       (DeviceDiagGaussian, spaces.Box(low=-1, high=1, shape=(2, 2), dtype=np.float32)), (DeviceDiagGaussian, object())):
        with pytest.raises(ValueError):
            cls(space)
    assert DeviceDiagGaussian(box(0.5, 0.5)).action_dim == 2                   # a degenerate dimension clips; it cannot be rescaled
    with pytest.raises(ValueError, match="log_std_min"):
        DeviceSquashedDiagGaussian(ACT, log_std_min=3.0)
    with pytest.raises(ValueError, match="seed"):
        DeviceDiagGaussian(ACT, seed=-1)
    with pytest.raises(RuntimeError, match="for_env"):
        DeviceSquashedDiagGaussian(ACT).sample_uniform()
    with pytest.raises(ValueError, match="keys"):
        g.load_state_dict({"seed": 1})
    with pytest.raises(ValueError, match="2\\^64"):
        g.load_state_dict({"seed": 1, "counter": -1})
    assert not hasattr(DeviceDiagGaussian, "sample_uniform")


class FakeEnv:
    """What the two loops touch of an env in obs_mode="torch", on CPU tensors: observation views rewritten in place, auto-reset every 3 steps."""

    def __init__(self, N=4, log=None):
        self.num_envs, self.action_space, self.log = N, ACT, log if log is not None else []
        self._obs = {"oracle": torch.zeros(N, 3)}
        self._rd = (torch.zeros(N), torch.zeros(N, dtype=torch.uint8))
        self._t = 0

    def reset(self):
        self._obs["oracle"].copy_(torch.arange(self.num_envs * 3, dtype=torch.float32).view(-1, 3) * 0.01)
        return dict(self._obs)

    def reward_done_torch(self):
        return self._rd

    def step(self, actions):
        self.log.append(("step", actions.clone()))
        self._t += 1
        self._obs["oracle"].add_(actions.sum(dim=1, keepdim=True))             # in place: a view handed out earlier changes
        self._rd[0].copy_(actions[:, 0] * self._t)
        self._rd[1].copy_((torch.arange(self.num_envs) + self._t) % 3 == 0)
        return dict(self._obs), self._rd[0].numpy().copy(), self._rd[1].numpy().astype(bool), [{}] * self.num_envs


class FakeRollout:
    def __init__(self, T, N, log):
        self.buffer_size, self.n_envs, self.log, self.pos = T, N, log, 0
        self.rewards = torch.zeros(T, N)

    def reset(self):
        self.pos = 0
        self.log.append(("reset",))

    def add(self, obs, action, reward, episode_start, value, log_prob):
        self.log.append(("add", {k: v.clone() for k, v in obs.items()}, action.clone(), reward.clone(), episode_start.clone(), value.clone(),
                         log_prob.clone()))
        self.pos += 1

    def compute_returns_and_advantage(self, last_values, dones):
        self.log.append(("gae", last_values.clone(), dones.clone()))


class FakeReplay:
    def __init__(self, log):
        self.log = log

    def add_from_env(self, actions):
        self.log.append(("add_from_env", actions.clone()))


def _policy(obs):
    o = obs["oracle"]
    return 0.3 * torch.sin(o[:, :2]), torch.tensor([-2.0, -1.0]), o.sum(dim=1)


def _actor(obs):
    o = obs["oracle"]
    return 0.3 * torch.sin(o[:, :2]), -1.0 + 0.1 * torch.cos(o[:, 1:])


def test_collect_rollouts_adds_before_the_step_and_bootstraps_from_the_last_observation():
    from tactile_gym_amd.collect import collect_rollouts
    import tactile_gym_amd as tg
    assert tg.collect.collect_rollouts is collect_rollouts
    log = []
    env, T = FakeEnv(log=log), 5
    buf, head = FakeRollout(T, 4, log), _stubbed("DeviceDiagGaussian", ACT, seed=3)
    obs = env.reset()
    first = {k: v.clone() for k, v in obs.items()}
    starts = torch.ones(4, dtype=torch.uint8)
    last_obs, last_starts = collect_rollouts(env, _policy, buf, head, T, obs, starts)
    assert [e[0] for e in log] == ["reset"] + ["add", "step"] * T + ["gae"]
    twin, twin_head = FakeEnv(), _stubbed("DeviceDiagGaussian", ACT, seed=3)
    o, s = twin.reset(), torch.ones(4, dtype=torch.uint8)
    assert torch.equal(o["oracle"], first["oracle"])
    for t in range(T):
        mean, ls, values = _policy(o)
        a, e, lp = twin_head.sample(mean, ls)
        add, step = log[1 + 2 * t], log[2 + 2 * t]
        assert torch.equal(add[1]["oracle"], o["oracle"]) and torch.equal(add[2], a) and torch.equal(add[3], torch.zeros(4))     # the pre-step obs
        assert torch.equal(add[4], s) and torch.equal(add[5], values) and torch.equal(add[6], lp)
        assert torch.equal(step[1], e) and not torch.equal(e, a)                                 # the env takes the clipped actions
        o, _, _, _ = twin.step(e)
        assert torch.equal(buf.rewards[t], twin._rd[0])
        s = twin._rd[1].clone()
    assert torch.equal(log[-1][1], _policy(o)[2]) and torch.equal(log[-1][2], s)                  # the value of the final observation
    assert torch.equal(last_obs["oracle"], o["oracle"]) and torch.equal(last_starts, s) and last_starts.data_ptr() != env._rd[1].data_ptr()
    assert head.counter == T
    with pytest.raises(ValueError, match="n_steps"):
        collect_rollouts(env, _policy, buf, head, T + 1, last_obs, last_starts)


def test_collect_transitions_switches_from_the_warm_up_and_adds_after_the_step():
    from tactile_gym_amd.collect import collect_transitions
    log = []
    env = FakeEnv(log=log)
    rb, head = FakeReplay(log), _stubbed("DeviceSquashedDiagGaussian", ACT, seed=8, num_envs=4, device="cpu")
    env.reset()
    obs, n = collect_transitions(env, _actor, rb, head, 2, 0, 12)              # last_obs is not needed inside the warm-up
    assert n == 8 and [c[0] for c in head.calls] == [ref.UNIFORM] * 2
    obs, n = collect_transitions(env, _actor, rb, head, 4, n, 12, obs)         # 8 < 12: one more uniform step, then the actor
    assert n == 24 and [c[0] for c in head.calls] == [ref.UNIFORM] * 3 + [ref.SQUASHED] * 3 and head.counter == 6
    assert [c[4] for c in head.calls] == list(range(6))
    assert [e[0] for e in log] == ["step", "add_from_env"] * 6
    twin, twin_head = FakeEnv(), _stubbed("DeviceSquashedDiagGaussian", ACT, seed=8, num_envs=4, device="cpu")
    o = twin.reset()
    for t in range(6):
        if t < 3:
            a, e = twin_head.sample_uniform()
        else:
            a, e, _ = twin_head.sample(*_actor(o))
        assert torch.equal(log[2 * t][1], e) and torch.equal(log[2 * t + 1][1], a), t
        assert (a.abs() <= 1).all() and (e.abs() <= 0.25).all() and torch.equal(e, torch.from_numpy(ref.unscale_f32(a.numpy(), ACT.low, ACT.high)))
        o, _, _, _ = twin.step(e)
    assert torch.equal(obs["oracle"], o["oracle"])
    with pytest.raises(ValueError, match="last_obs"):
        collect_transitions(env, _actor, rb, head, 1, 100, 12)


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entry_is_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    assert re.search(r"\bint tg_action_head\s*\(", header) and "tg_action_head" in _capi.SYMBOLS
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    assert len(BOUND_ENTRY[1]) == 20
    decl = re.search(r"\bint tg_action_head\s*\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == 20
    for name, value in (("GAUSSIAN", 0), ("SQUASHED", 1), ("UNIFORM", 2), ("MAX_ACT", 16)):
        assert re.search(rf"#define TG_HEAD_{name} {value}\b", header) and getattr(_capi, "HEAD_" + name) == value
    assert (ref.GAUSSIAN, ref.SQUASHED, ref.UNIFORM) == (_capi.HEAD_GAUSSIAN, _capi.HEAD_SQUASHED, _capi.HEAD_UNIFORM)
    assert os.path.exists(_capi.LIB_PATH), "library not built"
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tg_action_head\b", nm)
    build_units.assert_exact_product_unit("tg_action_head")


def test_action_head_kernels_use_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = _kernel_scratch(tmp_path)
    head = {k: v for k, v in scratch.items() if "k_action_head" in k}
    assert len(head) == 3, sorted(head)                                        # one instance per mode
    assert all(v == 0 for v in head.values()), head
