"""tactile_gym_amd.vecnorm without a GPU: the kernels' order of operations (tests/vecnorm_ref.py device_order) against SB3's formulas (plain) within
DESIGN.md 4.12's bound, two wrong variants far outside it, known answers, the wrapper's logic on a fake torch-mode env whose two C calls are
replaced by device_order, the C ABI entries and the kernels' resources."""
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
import vecnorm_ref as ref  # noqa: E402

from tactile_gym_amd import _capi, spaces  # noqa: E402

ENTRIES = ("tg_vecnorm_update", "tg_vecnorm_apply")
BOUND = {name: _capi.SYMBOLS[name] for name in ENTRIES}      # at import: the whole file needs the feature
U = 2.0 ** -53
DEPTH = 8                                                    # of the binary tree over a chunk's 256 slots


# ---------------------------------------------------------------------------------------------------------------- the bound
class ErrorBound:
    """a first-order bound on |device_order - exact| of the running mean and variance, carried along the plain recurrence.

    One batch of n rows in C chunks, A = max |x|, bv its variance:
        E_bm = u (DEPTH + 1 + 7 (C - 1)) A                      tree sum and division per chunk; per merge u (A + 3 |delta|), |delta| <= 2 A
        E_bv = u (DEPTH + 10 + 2 (C - 1)) bv + 4 sqrt(bv) E_bm  deviations, squares, tree, division; per merge two additions and the delta^2 term,
                                                                whose input error sums to at most 4 sqrt(bv) E_bm over the merges (Cauchy-Schwarz)
    merged into the running statistics (count, mean, var) with delta = bm - mean, tot = count + n, w = count n / tot:
        E_mean' = (count E_mean + n E_bm) / tot + u (|mean'| + 3 |delta| n / tot)
        E_var'  = (count E_var + n E_bv) / tot + 2 (w / tot) |delta| (E_mean + E_bm) + 6 u var'
    plain makes the same roundings in the running merge and fewer in the batch moments, so |device_order - plain| <= 2 E."""

    def __init__(self, d):
        self.mean, self.var = np.zeros(d), np.zeros(d)

    def update(self, x, before, after):
        """x: the batch; before / after: plain's (mean, var, count) round the update."""
        n = x.shape[0]
        C = (n + ref.CHUNK - 1) // ref.CHUNK
        bm, bv = ref.plain_moments(x)
        A = np.abs(x).max(axis=0)
        e_bm = U * (DEPTH + 1 + 7 * (C - 1)) * A
        e_bv = U * (DEPTH + 10 + 2 * (C - 1)) * bv + 4 * np.sqrt(bv) * e_bm
        mean, var, count = before
        delta, tot = np.abs(bm - mean), count + n
        w = count * n / tot
        self.var = (count * self.var + n * e_bv) / tot + 2 * (w / tot) * delta * (self.mean + e_bm) + 6 * U * after[1]
        self.mean = (count * self.mean + n * e_bm) / tot + U * (np.abs(after[0]) + 3 * delta * n / tot)


def one_pass_moments(x):
    """The wrong variance: E[x^2] - E[x]^2."""
    x = np.asarray(x, dtype=np.float64)
    m = np.mean(x, axis=0)
    return m, np.mean(x * x, axis=0) - m * m


DATA = {"offset": (1e3, 0.1), "standard": (0.0, 1.0)}


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000])
@pytest.mark.parametrize("data", sorted(DATA))
def test_device_order_stays_within_the_bound_of_plain_and_wrong_variants_do_not(data, N):
    mu, sd = DATA[data]
    d = 5
    rng = np.random.default_rng(1000 * N + len(data))
    runs = {"plain": ref.RunningMeanStd((d,), ref.plain_moments), "device": ref.RunningMeanStd((d,), ref.device_moments),
            "one_pass": ref.RunningMeanStd((d,), one_pass_moments), "count0": ref.RunningMeanStd((d,), ref.plain_moments, count=0.0)}
    bound = ErrorBound(d)
    worst = {k: 0.0 for k in runs}
    for _ in range(50):
        x = (mu + sd * rng.standard_normal((N, d))).astype(np.float32)
        p = runs["plain"]
        before = (p.mean, p.var, p.count)
        for r in runs.values():
            r.update(x)
        bound.update(x.astype(np.float64), before, (p.mean, p.var, p.count))
        for k, r in runs.items():
            worst[k] = max(worst[k], float((np.abs(r.mean - p.mean) / (2 * bound.mean)).max()), float((np.abs(r.var - p.var) / (2 * bound.var)).max()))
    print(f"{data} N={N}: error / bound {worst}; bound on mean {2 * bound.mean.max():.3g}, on var {2 * bound.var.max():.3g}")
    assert worst["device"] <= 1.0, worst
    assert worst["count0"] > 100.0, worst
    if data == "offset" and N >= 255:      # below that the float32 squares and their few sums are exact in float64: one pass is not wrong yet
        assert worst["one_pass"] > 100.0, worst


# ---------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("make", [ref.plain, ref.device_order])
def test_first_update_takes_the_batch_mean(make):
    rng = np.random.default_rng(3)
    x = (5.0 + rng.standard_normal((1000, 3))).astype(np.float32)
    vn = make({"oracle": 3}, 1000)
    vn.reset({"oracle": x})
    bm, bv = x.astype(np.float64).mean(0), x.astype(np.float64).var(0)
    rms = vn.obs_rms["oracle"]
    assert rms.count == 1000 + 1e-4
    # the prior (mean 0, var 1, count 1e-4) weighs 1e-7 of the batch: mean = bm (1 - 1e-7), var = bv + 1e-7 (1 - bv + bm^2), to first order
    assert np.abs(rms.mean - bm * (1 - 1e-4 / rms.count)).max() < 1e-12
    assert np.abs(rms.var - (bv + (1e-4 / rms.count) * (1 - bv + bm * bm))).max() < 1e-12


@pytest.mark.parametrize("make", [ref.plain, ref.device_order])
def test_constant_input_drives_var_to_zero_and_the_output_to_zero_or_the_clip(make):
    vn = make({"oracle": 2}, 300, clip_obs=5.0)
    x = np.tile(np.array([[3.0, -2.0]], np.float32), (300, 1))
    for _ in range(20):
        out = vn.reset({"oracle": x})["oracle"]
    rms = vn.obs_rms["oracle"]
    assert (rms.var < 1e-6).all() and (rms.var >= 0).all() and np.abs(rms.mean - [3.0, -2.0]).max() < 1e-6
    # x - mean is the prior's leftover 1e-4 / count of x and var about (1 + x^2) 1e-4 / count: the output tends to 0 like 1 / sqrt(count) ...
    assert np.abs(out).max() < 1e-3
    # ... and anything one unit off the constant lies thousands of standard deviations out: clipped, with its sign
    assert np.array_equal(vn.normalize_obs({"oracle": x[:2] + np.float32(1)})["oracle"], np.full((2, 2), 5.0, np.float32))
    assert np.array_equal(vn.normalize_obs({"oracle": x[:2] - np.float32(1)})["oracle"], np.full((2, 2), -5.0, np.float32))
    zero = make({"oracle": 1}, 4)
    assert np.array_equal(zero.reset({"oracle": np.zeros((4, 1), np.float32)})["oracle"], np.zeros((4, 1), np.float32))     # 0 / sqrt(var + eps)


DONES = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 0], [1, 0, 1], [0, 0, 0]], dtype=bool)      # 5 steps x 3 envs
REWARDS = np.array([[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3]], dtype=np.float32)


@pytest.mark.parametrize("make", [ref.plain, ref.device_order])
def test_returns_recurrence_over_a_done_pattern(make):
    g = 0.5
    vn = make({}, 3, gamma=g)
    vn.reset({})
    # by hand, gamma = 0.5: the value that enters the statistics (before the reset), then the value kept
    seen = [[1, 2, 3], [1.5, 3, 3], [1.75, 2, 4.5], [1.875, 3, 5.25], [1, 3.5, 3]]
    kept = [[1, 2, 0], [1.5, 0, 3], [1.75, 2, 4.5], [0, 3, 0], [1, 3.5, 3]]
    stats = ref.RunningMeanStd((), ref.plain_moments)
    for t in range(5):
        _, rew, _ = vn.step({}, REWARDS[t], DONES[t])
        stats.update(np.array(seen[t], np.float64)[:, None])
        assert np.array_equal(vn.returns, np.array(kept[t], np.float64)), t
        assert abs(vn.ret_rms.mean - stats.mean) < 1e-14 and abs(vn.ret_rms.var - stats.var) < 1e-14 and vn.ret_rms.count == stats.count
        # the reward is normalised with the statistics that include this step's returns
        assert np.array_equal(rew, np.clip(REWARDS[t].astype(np.float64) / np.sqrt(vn.ret_rms.var + 1e-8), -10, 10).astype(np.float32))


def test_returns_are_zeroed_after_the_reward_is_normalised():
    """Zeroing first would feed the statistics 0 instead of the finished env's last return: the variance, and with it the reward, would differ."""
    vn = ref.device_order({}, 2, gamma=1.0)
    vn.reset({})
    vn.step({}, np.array([1, 1], np.float32), np.array([0, 0], bool))
    _, rew, _ = vn.step({}, np.array([1, 5], np.float32), np.array([0, 1], bool))
    after = ref.RunningMeanStd((), ref.device_moments)
    after.update(np.array([[1.0], [1.0]]))
    after.update(np.array([[2.0], [6.0]]))                                   # [2, 0] had the reset come first
    assert vn.ret_rms.var == after.var and np.array_equal(vn.returns, [2.0, 0.0])
    assert np.array_equal(rew, (np.array([1.0, 5.0]) / np.sqrt(after.var + 1e-8)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the wrapper on a fake env
torch = pytest.importorskip("torch")


class FakeEnv:
    """What DeviceVecNormalize touches of a TactileVecEnv in obs_mode="torch", on CPU tensors: auto-reset after `max_steps` steps."""

    def __init__(self, N=6, widths=(("oracle", 3), ("extended_feature", 4)), image=True, obs_mode="torch", max_steps=4, seed=0):
        self.obs_mode, self.num_envs, self.frame_stack, self.channels_first = obs_mode, N, 1, False
        sp = {k: spaces.Box(low=-np.inf, high=np.inf, shape=(d,), dtype=np.float32) for k, d in widths}
        if image:
            sp["tactile"] = spaces.Box(low=0, high=255, shape=(4, 4, 1), dtype=np.uint8)
        self.observation_space = spaces.Dict(sp)
        self.action_space = spaces.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32)
        self._rng = np.random.default_rng(seed)
        self._obs = {k: torch.zeros((N,) + s.shape, dtype=torch.uint8 if k == "tactile" else torch.float32) for k, s in sp.items()}
        self._term = {k: torch.zeros_like(v) for k, v in self._obs.items()}
        self._rd = (torch.zeros(N), torch.zeros(N, dtype=torch.uint8))
        self._age = np.arange(N) % max_steps
        self.max_steps, self.closed = max_steps, False

    def _draw(self, into):
        for k, v in into.items():
            if k != "tactile":
                v.copy_(torch.from_numpy((3.0 + 2.0 * self._rng.standard_normal(tuple(v.shape))).astype(np.float32)))

    def reward_done_torch(self):
        return self._rd

    def _terminal_observation(self):
        return self._term

    def reset(self):
        self._draw(self._obs)
        return dict(self._obs)

    def step_async(self, actions):
        self._actions = actions

    def step_wait(self):
        self._draw(self._obs)
        self._draw(self._term)
        self._age += 1
        done = self._age >= self.max_steps
        self._age[done] = 0
        rew = self._rng.standard_normal(self.num_envs).astype(np.float32)
        self._rd[0].copy_(torch.from_numpy(rew))
        self._rd[1].copy_(torch.from_numpy(done.astype(np.uint8)))
        infos = [{"terminal_observation": {k: v[i].clone() for k, v in self._term.items()}} if done[i] else {} for i in range(self.num_envs)]
        return dict(self._obs), rew.copy(), done.copy(), infos

    def seed(self, seed=None):
        return [seed] * self.num_envs

    def close(self):
        self.closed = True


def _stubbed(*args, **kwargs):
    """A DeviceVecNormalize whose two C calls are device_order on the CPU tensors' memory."""
    from tactile_gym_amd.vecnorm import DeviceVecNormalize

    class Stubbed(DeviceVecNormalize):
        calls = []

        def _rms(self, block, d):
            r = ref.RunningMeanStd((d,), ref.device_moments)
            b = block.numpy()
            r.mean, r.var, r.count = b[:d].copy(), b[d:2 * d].copy(), b[2 * d]
            return r, b

        def _c_update(self, arrays, with_returns):
            self.calls.append("update")
            for k, d, x in zip(self.norm_obs_keys, self._widths, arrays):
                r, b = self._rms(self.obs_rms[k].block, d)
                r.update(x.numpy())
                b[:d], b[d:2 * d], b[2 * d] = r.mean, r.var, r.count
            if with_returns:
                ret = self.returns.numpy()
                ret[:] = ret * self.gamma + self._rd[0].numpy().astype(np.float64)
                r, b = self._rms(self.ret_rms.block, 1)
                r.update(ret[:, None])
                b[0], b[1], b[2] = r.mean[0], r.var[0], r.count

        def _c_apply(self, pairs, rows, rewards=None, rewards_out=None, reset=None):
            self.calls.append("apply")
            for k, d, (x, o) in zip(self.norm_obs_keys, self._widths, pairs):
                b = self.obs_rms[k].block.numpy()
                assert x.numel() == rows * d and o.numel() == rows * d
                y = (x.numpy().reshape(rows, d).astype(np.float64) - b[:d]) / np.sqrt(b[d:2 * d] + self.epsilon)
                o.numpy().reshape(rows, d)[:] = np.clip(y, -self.clip_obs, self.clip_obs).astype(np.float32)
            if rewards is not None:
                y = rewards.numpy().astype(np.float64) / np.sqrt(self.ret_rms.block.numpy()[1] + self.epsilon)
                rewards_out.numpy()[:] = np.clip(y, -self.clip_reward, self.clip_reward).astype(np.float32)
            if reset:
                mask = self._rd[1].numpy().astype(bool) if reset == "done" else np.ones(self.num_envs, bool)
                self.returns.numpy()[mask] = 0.0

    Stubbed.calls = []
    return Stubbed(*args, **kwargs)


def _np(obs):
    return {k: v.numpy().copy() for k, v in obs.items()}


def _assert_stats(vn, model):
    for k, rms in model.obs_rms.items():
        assert np.array_equal(vn.obs_rms[k].mean.numpy(), rms.mean) and np.array_equal(vn.obs_rms[k].var.numpy(), rms.var), k
        assert vn.obs_rms[k].count.item() == rms.count
    assert vn.ret_rms.mean.item() == model.ret_rms.mean and vn.ret_rms.var.item() == model.ret_rms.var and vn.ret_rms.count.item() == model.ret_rms.count
    assert np.array_equal(vn.returns.numpy(), model.returns)


@pytest.mark.parametrize("settings", [dict(), dict(norm_reward=False), dict(norm_obs=False), dict(norm_obs_keys=["extended_feature"], gamma=0.9,
                                                                                                  clip_obs=1.5, clip_reward=0.5, epsilon=1e-4)])
def test_wrapper_follows_the_restatement_on_a_fake_env(settings):
    env, twin = FakeEnv(seed=5), FakeEnv(seed=5)
    vn = _stubbed(env, **settings)
    keys = settings.get("norm_obs_keys", ["oracle", "extended_feature"])
    assert vn.norm_obs_keys == keys and vn.venv is env and vn.unwrapped is env and vn.num_envs == 6 and vn.frame_stack == 1
    model = ref.device_order({k: env.observation_space.spaces[k].shape[0] for k in keys}, 6, **{k: v for k, v in settings.items() if k != "norm_obs_keys"})
    out = vn.reset()
    want = model.reset(_np(twin.reset()))
    for k in out:
        assert np.array_equal(out[k].numpy(), want[k]), k
    assert out["tactile"] is env._obs["tactile"]                                           # image keys: the env's own tensor
    for step in range(12):
        type(vn).calls.clear()
        obs, rew, dones, infos = vn.step(np.zeros((6, 2), np.float32))
        t_obs, t_rew, t_done, t_infos = twin.step_wait()
        w_obs, w_rew, w_term = model.step(_np(t_obs), t_rew, t_done, _np(twin._term))
        assert np.array_equal(dones, t_done) and rew.dtype == np.float32 and np.array_equal(rew, w_rew), step
        assert np.array_equal(vn.get_original_reward(), t_rew)
        for k in obs:
            assert np.array_equal(obs[k].numpy(), w_obs[k]), (step, k)
            assert np.array_equal(vn.get_original_obs()[k].numpy(), t_obs[k].numpy())
        for i in np.nonzero(dones)[0]:
            for k in obs:
                assert np.array_equal(infos[i]["terminal_observation"][k].numpy(), w_term[k][i]), (step, i, k)
        _assert_stats(vn, model)
        r, dn = vn.reward_done_torch()
        assert np.array_equal(r.numpy(), w_rew) and dn is env._rd[1]
        # the launch budget: update (two launches) and apply, one more apply in steps where an env finished
        normalising = model.norm_obs and bool(keys)
        assert type(vn).calls == ["update", "apply"] + (["apply"] if dones.any() and normalising else []), type(vn).calls
    if not settings.get("norm_reward", True):
        assert vn.ret_rms.count.item() == 1e-4 + 12 * 6                                    # tracked in training mode all the same
    vn.close()
    assert env.closed


def test_training_false_freezes_everything():
    env = FakeEnv(seed=2)
    vn = _stubbed(env)
    vn.reset()
    for _ in range(3):
        vn.step(np.zeros((6, 2), np.float32))
    vn.training = False
    frozen = {k: v.copy() for k, v in vn.state_dict().items()}
    type(vn).calls.clear()
    vn.reset()
    for _ in range(5):
        obs, rew, dones, _ = vn.step(np.zeros((6, 2), np.float32))
    assert "update" not in type(vn).calls
    for k, v in vn.state_dict().items():
        if k != "returns":
            assert np.array_equal(v, frozen[k]), k
    assert np.array_equal(vn.returns.numpy(), np.zeros(6))                                 # not accumulated; reset() and the dones zero them
    x = vn.get_original_obs()["oracle"].numpy().astype(np.float64)
    want = np.clip((x - frozen["obs_rms.oracle.mean"]) / np.sqrt(frozen["obs_rms.oracle.var"] + 1e-8), -10, 10).astype(np.float32)
    assert np.array_equal(obs["oracle"].numpy(), want)


def test_key_selection_spaces_and_refusals():
    from tactile_gym_amd.vecnorm import DeviceVecNormalize
    import tactile_gym_amd as tg
    assert tg.DeviceVecNormalize is DeviceVecNormalize and tg.vecnorm.DeviceVecNormalize is DeviceVecNormalize
    vn = _stubbed(FakeEnv(), clip_obs=7.0)
    assert vn.norm_obs_keys == ["oracle", "extended_feature"]                              # every float32 vector key, in the env's order
    assert (vn.training, vn.norm_obs, vn.norm_reward, vn.clip_obs, vn.clip_reward, vn.gamma, vn.epsilon) == (True, True, True, 7.0, 10.0, 0.99, 1e-8)
    sp = vn.observation_space.spaces
    for k, d in (("oracle", 3), ("extended_feature", 4)):
        assert sp[k].shape == (d,) and sp[k].dtype == np.float32 and (sp[k].low == -7.0).all() and (sp[k].high == 7.0).all()
        rms = vn.obs_rms[k]
        assert rms.mean.dtype == torch.float64 and tuple(rms.mean.shape) == (d,) and tuple(rms.var.shape) == (d,) and rms.count.dim() == 0
        assert (rms.mean == 0).all() and (rms.var == 1).all() and rms.count.item() == 1e-4
    assert sp["tactile"] is vn.venv.observation_space.spaces["tactile"] and vn.action_space is vn.venv.action_space
    assert vn.ret_rms.mean.dim() == 0 and vn.ret_rms.var.item() == 1.0 and vn.returns.dtype == torch.float64 and tuple(vn.returns.shape) == (6,)
    with pytest.raises(NotImplementedError, match="tactile"):
        _stubbed(FakeEnv(), norm_obs_keys=["tactile"])
    with pytest.raises(ValueError, match="nothing"):
        _stubbed(FakeEnv(), norm_obs_keys=["nothing"])
    with pytest.raises(ValueError, match="stable_baselines3"):
        _stubbed(FakeEnv(obs_mode="numpy"))
    with pytest.raises(ValueError, match="at most"):
        _stubbed(FakeEnv(widths=(("a", 300), ("b", 213))))
    with pytest.raises(ValueError, match="at most"):
        _stubbed(FakeEnv(widths=tuple((f"k{i}", 2) for i in range(5))))
    assert _stubbed(FakeEnv(widths=(("a", 300), ("b", 212)))).norm_obs_keys == ["a", "b"]
    only_images = _stubbed(FakeEnv(widths=()))                                             # no vector key: reward normalisation only
    assert only_images.norm_obs_keys == [] and only_images.reset()["tactile"] is only_images.venv._obs["tactile"]
    _, rew, _, _ = only_images.step(np.zeros((6, 2), np.float32))
    assert not np.array_equal(rew, only_images.get_original_reward())


def test_state_dict_round_trip_save_load_and_mismatches(tmp_path):
    from tactile_gym_amd.vecnorm import DeviceVecNormalize
    vn = _stubbed(FakeEnv(seed=1), gamma=0.9, clip_obs=3.0, norm_reward=False)
    vn.reset()
    for _ in range(3):
        vn.step(np.zeros((6, 2), np.float32))
    sd = vn.state_dict()
    assert sorted(sd) == sorted([f"obs_rms.{k}.{f}" for k in ("oracle", "extended_feature") for f in ("mean", "var", "count")]
                                + ["ret_rms.mean", "ret_rms.var", "ret_rms.count", "returns"])
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float64 for v in sd.values())
    other = _stubbed(FakeEnv(seed=9))
    other.load_state_dict(sd)
    for k, v in other.state_dict().items():
        assert np.array_equal(v, sd[k]), k
    path = tmp_path / "vn.npz"
    vn.save(path)
    with np.load(path, allow_pickle=False) as z:                                           # plain arrays: no pickle inside
        assert "obs_rms.oracle.mean" in z.files
    loaded = DeviceVecNormalize.load.__func__(type(vn), path, FakeEnv(seed=3))
    assert (loaded.gamma, loaded.clip_obs, loaded.norm_reward, loaded.training, loaded.norm_obs_keys) == (0.9, 3.0, False, True, vn.norm_obs_keys)
    for k, v in loaded.state_dict().items():
        assert np.array_equal(v, sd[k]), k
    with pytest.raises(ValueError, match="keys differ"):
        _stubbed(FakeEnv(widths=(("oracle", 3),))).load_state_dict(sd)
    with pytest.raises(ValueError, match="shape"):
        _stubbed(FakeEnv(widths=(("oracle", 3), ("extended_feature", 5)))).load_state_dict(sd)
    with pytest.raises(ValueError, match="shape"):
        _stubbed(FakeEnv(N=7)).load_state_dict(sd)
    with pytest.raises(ValueError):
        DeviceVecNormalize.load.__func__(type(vn), path, FakeEnv(widths=(("oracle", 3),)))


def test_normalize_and_unnormalize_methods():
    vn = _stubbed(FakeEnv(seed=4))
    vn.reset()
    vn.step(np.zeros((6, 2), np.float32))
    obs = {"oracle": torch.randn(2, 5, 3) * 0.01 + 3.0, "extended_feature": torch.randn(2, 5, 4) * 0.01 + 3.0, "tactile": torch.zeros(10, 4, 4, 1)}
    out = vn.normalize_obs(obs)
    assert out["tactile"] is obs["tactile"] and tuple(out["oracle"].shape) == (2, 5, 3)
    back = vn.unnormalize_obs(out)
    assert torch.allclose(back["oracle"], obs["oracle"], atol=1e-5) and torch.allclose(back["extended_feature"], obs["extended_feature"], atol=1e-5)
    r = torch.tensor([[0.1], [-0.2], [0.3]])
    nr = vn.normalize_reward(r)
    assert tuple(nr.shape) == (3, 1) and torch.allclose(vn.unnormalize_reward(nr), r, atol=1e-6)
    with pytest.raises(ValueError, match="last dimension"):
        vn.normalize_obs(dict(obs, oracle=torch.zeros(10, 4)))
    with pytest.raises(TypeError, match="float32"):
        vn.normalize_obs(dict(obs, oracle=torch.zeros(10, 3, dtype=torch.float64)))


def test_sample_still_refuses_any_other_env():
    from test_replay_cpu import _unallocated
    b = _unallocated(T=4, N=3)
    b.pos = 2
    with pytest.raises(NotImplementedError, match="VecNormalize"):
        b.sample(2, env=object())


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    assert len(_capi.SYMBOLS["tg_vecnorm_update"][1]) == 11 and len(_capi.SYMBOLS["tg_vecnorm_apply"][1]) == 17
    for name, value in (("MAX_ARRAYS", 4), ("MAX_WIDTH", 512), ("MAX_ROWS", 65535)):
        assert re.search(rf"#define TG_VECNORM_{name} {value}\b", header) and getattr(_capi, "VECNORM_" + name) == value
    assert os.path.exists(_capi.LIB_PATH), "library not built"
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bT " + name + r"\b", nm), name
    build_units.assert_exact_product_unit("tg_vecnorm")


def test_vecnorm_kernels_use_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = _kernel_scratch(tmp_path)
    vn = {k: v for k, v in scratch.items() if "k_vecnorm_" in k}
    assert sorted(re.sub(r".*(k_vecnorm_[a-z]+).*", r"\1", k) for k in vn) == ["k_vecnorm_apply", "k_vecnorm_merge", "k_vecnorm_partial"], sorted(vn)
    assert all(v == 0 for v in vn.values()), vn


def test_tree_sum_is_the_documented_order():
    rng = np.random.default_rng(0)
    v = rng.standard_normal((2, 256, 3))
    want = np.zeros((2, 3))
    for c in range(2):
        for j in range(3):
            w = []
            for q in range(4):
                s = list(v[c, 64 * q:64 * q + 64, j])
                for half in (32, 16, 8, 4, 2, 1):
                    s = [s[i] + s[i + half] for i in range(half)]
                w.append(s[0])
            want[c, j] = (w[0] + w[1]) + (w[2] + w[3])
    assert np.array_equal(ref.tree_sum(v), want)
    assert math.isclose(ref.tree_sum(np.ones((1, 256, 1)))[0, 0], 256.0)
