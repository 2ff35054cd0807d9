"""VecNormalize in device memory: stable_baselines3's VecNormalize over a TactileVecEnv made with obs_mode="torch" (csrc/tg_vecnorm.hip:
k_vecnorm_partial, k_vecnorm_merge, k_vecnorm_apply).

    venv = tg.make_vec("edge_follow-v0", num_envs=1024, obs_mode="torch", env_modes={..., "observation_mode": "oracle"})
    vn = tg.DeviceVecNormalize(venv, gamma=0.95)              # SB3's VecNormalize(venv, gamma=0.95)
    obs = vn.reset()                                          # normalised, clipped float32 device tensors of the wrapper's
    obs, rewards, dones, infos = vn.step(actions)             # + 3 launches; rewards: a numpy array of its own
    rb = tg.DeviceReplayBuffer.for_env(vn, 100_000)           # stores the originals, as SB3's replay buffer does
    batch = rb.sample(64, env=vn)                             # normalised with the current statistics: one more launch
    vn.save(path); vn = tg.DeviceVecNormalize.load(path, venv)

The running statistics are float64 device tensors (per key one block mean [d] | var [d] | count, for the discounted return mean | var | count)
and are updated and applied without a trip through the host: a step in training mode enqueues three launches on torch's current stream (the
chunk moments of every normalised column and of the returns, their merge into the statistics, the normalised outputs) and one more over the
terminal observations in steps where an env finished.  Nothing is allocated after construction.  The order of every sum is restated in numpy
by tests/vecnorm_ref.py, bit for bit.  norm_obs_keys=None takes every float32 vector key (PARITY_ASSUMPTIONS.md A45); image keys pass through
as the env's own tensors.  There is no numpy path: stable_baselines3's VecNormalize wraps the numpy obs_mode.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi as capi
from . import spaces
from ._device import launch, ptr

__all__ = ["DeviceVecNormalize", "DeviceRunningMeanStd"]

_SETTINGS = ("training", "norm_obs", "norm_reward", "clip_obs", "clip_reward", "gamma", "epsilon")


class DeviceRunningMeanStd:
    """SB3's RunningMeanStd as views of one float64 device block mean [d] | var [d] | count (d = 1 and 0-dim views for the returns)."""

    def __init__(self, block, shape):
        d = int(np.prod(shape, dtype=np.int64))
        self.block = block
        self.mean, self.var, self.count = block[:d].view(shape), block[d:2 * d].view(shape), block[2 * d]

    def init(self):
        d = (self.block.numel() - 1) // 2
        self.block[:d] = 0.0
        self.block[d:2 * d] = 1.0
        self.block[2 * d] = 1e-4


class DeviceVecNormalize:
    """stable_baselines3's VecNormalize (constructor arguments in SB3's order and with its defaults) over a TactileVecEnv in obs_mode="torch"."""

    def __init__(self, venv, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8,
                 norm_obs_keys=None):
        if getattr(venv, "obs_mode", None) != "torch":
            raise ValueError("DeviceVecNormalize needs an env made with obs_mode='torch'; for the numpy obs_mode use stable_baselines3's own "
                             "VecNormalize, which wraps it as it is")
        sub = getattr(venv.observation_space, "spaces", None)
        if sub is None:
            raise ValueError(f"DeviceVecNormalize needs a Dict observation space, got {venv.observation_space!r}")
        vector = [k for k, s in sub.items() if np.dtype(s.dtype) == np.float32 and len(s.shape) == 1 and s.shape[0] > 0]
        if norm_obs_keys is None:
            keys = vector
        else:
            keys = list(norm_obs_keys)
            for k in keys:
                if k not in sub:
                    raise ValueError(f"norm_obs_keys: {k!r} is not a key of the observation space ({sorted(sub)})")
                if k not in vector:
                    raise NotImplementedError(f"norm_obs_keys: {k!r} is not a float32 vector key; normalising image keys is not built (they pass "
                                              f"through, and SB3's /255 stays where it is)")
            if len(set(keys)) != len(keys):
                raise ValueError(f"norm_obs_keys has a key twice: {keys}")
        widths = [int(sub[k].shape[0]) for k in keys]
        if len(keys) > capi.VECNORM_MAX_ARRAYS or sum(widths) > capi.VECNORM_MAX_WIDTH:
            raise ValueError(f"at most {capi.VECNORM_MAX_ARRAYS} normalised keys of total width {capi.VECNORM_MAX_WIDTH} are built, got {keys} {widths}")
        self.venv = venv
        self.num_envs = N = int(venv.num_envs)
        if not 1 <= N <= capi.VECNORM_MAX_ROWS:
            raise ValueError(f"num_envs must lie in [1, {capi.VECNORM_MAX_ROWS}], got {N}")
        self.action_space = venv.action_space
        self.norm_obs_keys, self._widths = keys, widths
        self.training, self.norm_obs, self.norm_reward = bool(training), bool(norm_obs), bool(norm_reward)
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = float(clip_obs), float(clip_reward), float(gamma), float(epsilon)
        if not (self.clip_obs >= 0 and self.clip_reward >= 0 and self.epsilon >= 0):
            raise ValueError("clip_obs, clip_reward and epsilon must not be negative")
        self.observation_space = spaces.Dict({k: (spaces.Box(low=-self.clip_obs, high=self.clip_obs, shape=s.shape, dtype=np.float32)
                                                  if k in keys and self.norm_obs else s) for k, s in sub.items()})
        self._rd = venv.reward_done_torch()                      # the env's own reward / done buffers: they never move
        self.device = dev = self._rd[0].device
        f64 = dict(dtype=torch.float64, device=dev)
        self.obs_rms = {k: DeviceRunningMeanStd(torch.empty(2 * d + 1, **f64), (d,)) for k, d in zip(keys, widths)}
        self.ret_rms = DeviceRunningMeanStd(torch.empty(3, **f64), ())
        for rms in list(self.obs_rms.values()) + [self.ret_rms]:
            rms.init()
        self.returns = torch.zeros(N, **f64)
        self._scratch = torch.empty(2 * ((N + 255) // 256) * (sum(widths) + 1), **f64)
        self._out = {k: torch.empty((N, d), dtype=torch.float32, device=dev) for k, d in zip(keys, widths)}
        self._term_out = {k: torch.empty((N, d), dtype=torch.float32, device=dev) for k, d in zip(keys, widths)}
        self._rew_out = torch.empty(N, dtype=torch.float32, device=dev)
        self._rew_host = torch.empty(N, dtype=torch.float32, pin_memory=dev.type == "cuda")
        self._old_obs, self._old_reward = None, np.zeros(N, np.float32)
        n = capi.VECNORM_MAX_ARRAYS
        self._tab = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int32 * n)(*widths), (C.c_void_p * n)(*[r.block.data_ptr() for r in self.obs_rms.values()])

    # ------------------------------------------------------------------ the two C entries (tests replace these two methods)
    def _c_update(self, arrays, with_returns):
        """tg_vecnorm_update: `arrays`, one [N, d] float32 tensor per normalised key (or none of them); with_returns: the returns recurrence
        with the env's reward buffer and the update of ret_rms."""
        x_tab, _, w_tab, s_tab = self._tab
        for i, x in enumerate(arrays):
            x_tab[i] = x.data_ptr()
        ret = (self.returns, self._rd[0], self.ret_rms.block) if with_returns else (None, None, None)
        launch("tg_vecnorm_update", self.device, len(arrays), x_tab, w_tab, s_tab, self.num_envs, ptr(ret[0]), ptr(ret[1]), self.gamma,
               ptr(ret[2]), ptr(self._scratch))

    def _c_apply(self, pairs, rows, rewards=None, rewards_out=None, reset=None):
        """tg_vecnorm_apply: `pairs`, one (x, out) of [rows, d] float32 tensors per normalised key (or none); rewards -> rewards_out (any equal
        element count); reset: None, "done" (returns = 0 where the env's done flags are set) or "all"."""
        x_tab, o_tab, w_tab, s_tab = self._tab
        for i, (x, o) in enumerate(pairs):
            x_tab[i], o_tab[i] = x.data_ptr(), o.data_ptr()
        launch("tg_vecnorm_apply", self.device, len(pairs), x_tab, o_tab, w_tab, s_tab, rows, self.clip_obs, self.epsilon, ptr(rewards),
               ptr(rewards_out if rewards is not None else None), rewards.numel() if rewards is not None else 0, ptr(self.ret_rms.block),
               self.clip_reward, ptr(self.returns if reset else None), ptr(self._rd[1] if reset == "done" else None),
               self.num_envs if reset else 0)

    # ------------------------------------------------------------------ VecEnv surface
    def __getattr__(self, name):           # everything else is the env's (frame_stack, channels_first, sample_actions, _cfg ...)
        if name == "venv":
            raise AttributeError(name)
        return getattr(self.venv, name)

    @property
    def unwrapped(self):
        return getattr(self.venv, "unwrapped", self.venv)

    def _vector_inputs(self, obs):
        return [obs[k] for k in self.norm_obs_keys] if self.norm_obs else []

    def _handed_out(self, obs):
        if not (self.norm_obs and self.norm_obs_keys):
            return dict(obs)
        return {k: (self._out[k] if k in self._out else v) for k, v in obs.items()}

    def reset(self):
        obs = self.venv.reset()
        self._old_obs = obs
        xs = self._vector_inputs(obs)
        if self.training and xs:
            self._c_update(xs, False)
        self._c_apply([(x, self._out[k]) for k, x in zip(self.norm_obs_keys, xs)], self.num_envs, reset="all")
        return self._handed_out(obs)

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rewards, dones, infos = self.venv.step_wait()
        self._old_obs, self._old_reward = obs, rewards
        xs = self._vector_inputs(obs)
        if self.training:
            self._c_update(xs, True)
        rew = self._rd[0] if self.norm_reward else None
        self._c_apply([(x, self._out[k]) for k, x in zip(self.norm_obs_keys, xs)], self.num_envs, rewards=rew, rewards_out=self._rew_out, reset="done")
        if xs and dones.any():
            done_ids = [i for i in np.nonzero(dones)[0] if "terminal_observation" in infos[i]]
            if done_ids:
                term = self.venv._terminal_observation()
                self._c_apply([(term[k], self._term_out[k]) for k in self.norm_obs_keys], self.num_envs)
                for i in done_ids:
                    infos[i]["terminal_observation"] = dict(infos[i]["terminal_observation"],
                                                            **{k: self._term_out[k][i].clone() for k in self.norm_obs_keys})
        if self.norm_reward:
            self._rew_host.copy_(self._rew_out)                  # the one small copy (it waits for the stream, as the env's own reward copy did)
            rewards = self._rew_host.numpy().copy()
        return self._handed_out(obs), rewards, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        return self.venv.close()

    def seed(self, seed=None):
        return self.venv.seed(seed)

    def reward_done_torch(self):
        """(normalised reward, done) as device tensors: the wrapper's reward buffer (the env's own with norm_reward=False) and the env's flags."""
        return (self._rew_out if self.norm_reward else self._rd[0]), self._rd[1]

    # ------------------------------------------------------------------ SB3's VecNormalize methods
    def get_original_obs(self):
        """The env's own (unnormalised) observation tensors of the last step / reset."""
        return dict(self._old_obs)

    def get_original_reward(self):
        return self._old_reward.copy()

    def _as_rows(self, x, d, name):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.device:
            raise TypeError(f"{name} must be a float32 tensor on {self.device}, got {getattr(x, 'dtype', type(x).__name__)} "
                            f"{getattr(x, 'device', '')}")
        if x.dim() < 1 or x.shape[-1] != d:
            raise ValueError(f"{name} must have a last dimension of {d}, got shape {tuple(x.shape)}")
        return x.contiguous()

    def normalize_obs(self, obs):
        """`obs` (a dict of tensors of any leading size) with the normalised keys replaced by new normalised tensors: one launch, the current
        statistics, nothing updated."""
        out = dict(obs)
        if not (self.norm_obs and self.norm_obs_keys):
            return out
        xs = [self._as_rows(obs[k], d, f"obs[{k!r}]") for k, d in zip(self.norm_obs_keys, self._widths)]
        rows = {x.numel() // d for x, d in zip(xs, self._widths)}
        if len(rows) != 1:
            raise ValueError(f"the normalised keys differ in their number of rows: {sorted(rows)}")
        rows = rows.pop()
        for k, x in zip(self.norm_obs_keys, xs):
            out[k] = torch.empty_like(x)
        if rows:
            self._c_apply([(x, out[k]) for k, x in zip(self.norm_obs_keys, xs)], rows)
        return out

    def normalize_reward(self, reward):
        if not self.norm_reward:
            return reward
        r = self._as_rows(reward.reshape(-1, 1) if isinstance(reward, torch.Tensor) else reward, 1, "reward")
        out = torch.empty_like(r)
        if r.numel():
            self._c_apply([], 0, rewards=r, rewards_out=out)
        return out.view(reward.shape)

    def _normalize_sample(self, pairs, rewards):
        """DeviceReplayBuffer.sample(env=self): the gathered vector keys ({key: [2 B, d]}) and rewards normalised in place, one launch."""
        xs = [self._as_rows(pairs[k], d, f"observations[{k!r}]") for k, d in zip(self.norm_obs_keys, self._widths)] if self.norm_obs else []
        rows = xs[0].shape[0] if xs else 0
        self._c_apply([(x, x) for x in xs], rows, rewards=rewards if self.norm_reward else None, rewards_out=rewards)

    def unnormalize_obs(self, obs):
        out = dict(obs)
        if self.norm_obs:
            for k in self.norm_obs_keys:
                rms = self.obs_rms[k]
                out[k] = (obs[k].double() * torch.sqrt(rms.var + self.epsilon) + rms.mean).float()
        return out

    def unnormalize_reward(self, reward):
        if not self.norm_reward:
            return reward
        return (reward.double() * torch.sqrt(self.ret_rms.var + self.epsilon)).float()

    # ------------------------------------------------------------------ state
    def state_dict(self):
        """The statistics as host float64 arrays: "obs_rms.<key>.mean | var | count", "ret_rms.mean | var | count", "returns"."""
        sd = {}
        for name, rms in [(f"obs_rms.{k}", r) for k, r in self.obs_rms.items()] + [("ret_rms", self.ret_rms)]:
            for field in ("mean", "var", "count"):
                sd[f"{name}.{field}"] = getattr(rms, field).detach().cpu().numpy().astype(np.float64).copy()
        sd["returns"] = self.returns.detach().cpu().numpy().copy()
        return sd

    def load_state_dict(self, sd):
        mine = self.state_dict()
        if set(sd) != set(mine):
            raise ValueError(f"state_dict keys differ from this env's: {sorted(set(sd) ^ set(mine))}")
        arrays = {}
        for name, ref in mine.items():
            a = np.asarray(sd[name], dtype=np.float64)
            if a.shape != ref.shape:
                raise ValueError(f"state_dict[{name!r}] has shape {a.shape}, this env's is {ref.shape}")
            arrays[name] = a
        for name, rms in [(f"obs_rms.{k}", r) for k, r in self.obs_rms.items()] + [("ret_rms", self.ret_rms)]:
            for field in ("mean", "var", "count"):
                getattr(rms, field).copy_(torch.from_numpy(arrays[f"{name}.{field}"]))
        self.returns.copy_(torch.from_numpy(arrays["returns"]))

    def save(self, path):
        """np.savez of the state_dict, the settings and the normalised keys (no pickle)."""
        extra = {f"settings.{k}": np.float64(getattr(self, k)) for k in _SETTINGS}
        with open(path, "wb") as f:
            np.savez(f, norm_obs_keys=np.array(self.norm_obs_keys, dtype=np.str_), **extra, **self.state_dict())

    @classmethod
    def load(cls, path, venv):
        """The wrapper of `venv` with the settings and statistics of save(path); raises when the env's keys or shapes differ."""
        with np.load(path, allow_pickle=False) as z:
            data = {k: z[k] for k in z.files}
        keys = [str(k) for k in data.pop("norm_obs_keys")]
        kw = {k: data.pop(f"settings.{k}").item() for k in _SETTINGS}
        for k in ("training", "norm_obs", "norm_reward"):
            kw[k] = bool(kw[k])
        self = cls(venv, norm_obs_keys=keys, **kw)
        self.load_state_dict(data)
        return self
