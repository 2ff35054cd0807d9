"""Action heads in device memory: what stable_baselines3 does between the policy network's output and venv.step() with use_sde=False, as one
launch (csrc/tg_action_head.hip: k_action_head).

    head = tg.DeviceDiagGaussian.for_env(venv, seed=0)                  # PPO / RAD_PPO: SB3's DiagGaussianDistribution
    actions, env_actions, log_prob = head.sample(mean, log_std)         # log_std [A]: the policy's state-independent parameter
    buf.add(obs, actions, zeros, starts, values, log_prob)              # the unclipped sample is what the rollout buffer stores
    venv.step(env_actions)                                              # np.clip(actions, low, high) is what the env takes

    head = tg.DeviceSquashedDiagGaussian.for_env(venv, seed=0)          # SAC / RAD_SAC: SB3's SquashedDiagGaussianDistribution
    actions, env_actions = head.sample_uniform()                        # before learning_starts: scale_action(action_space.sample())
    actions, env_actions, log_prob = head.sample(mean, log_std)         # log_std [N, A]: the actor's output, clamped to [-20, 2] here
    venv.step(env_actions); rb.add_from_env(actions)                    # actions in [-1, 1] are stored, unscale_action(actions) is stepped

The three results (and `noise`, `gaussian_actions`) are float32 device tensors of the head's own, allocated once and valid until the next call -
the contract of the env's observation views.  `deterministic=True` is model.predict(deterministic=True): the mean (its tanh).  The draws are
counter based, on the generator of tg_sample_actions: call k of a head depends on (seed, k) only, and state_dict() carries both.  The arithmetic
is restated in tests/action_head_ref.py.  There is no CPU path: CPU tensors raise.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _capi as capi
from ._device import checked_f32, launch, ptr

__all__ = ["DeviceDiagGaussian", "DeviceSquashedDiagGaussian"]


class _DeviceHead:
    _mode = None

    def __init__(self, action_space, seed=0, log_std_min=-math.inf, log_std_max=math.inf, num_envs=None, device=None):
        shape, dtype = getattr(action_space, "shape", None), getattr(action_space, "dtype", None)
        if shape is None or len(shape) != 1 or np.dtype(dtype) != np.float32 or not hasattr(action_space, "low"):
            raise ValueError(f"action_space must be a float32 Box of one dimension, got {action_space!r}")
        A = int(shape[0])
        if not 1 <= A <= capi.HEAD_MAX_ACT:
            raise ValueError(f"the action dimension must lie in [1, {capi.HEAD_MAX_ACT}], got {A}")
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(action_space.low, dtype=np.float32), (A,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(action_space.high, dtype=np.float32), (A,)))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError(f"action_space must be bounded, got low={lo} high={hi}")
        if (lo > hi).any() or (self._mode != capi.HEAD_GAUSSIAN and (lo == hi).any()):
            raise ValueError(f"action_space needs low {'<=' if self._mode == capi.HEAD_GAUSSIAN else '<'} high in every dimension, got "
                             f"low={lo} high={hi}")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        self.log_std_min, self.log_std_max = float(log_std_min), float(log_std_max)
        if not self.log_std_min <= self.log_std_max:
            raise ValueError(f"log_std_min={log_std_min} must not exceed log_std_max={log_std_max}")
        self.action_space, self.action_dim = action_space, A
        self.low, self.high = lo, hi
        self._lo, self._hi = (C.c_float * A)(*lo.tolist()), (C.c_float * A)(*hi.tolist())
        self.seed, self.counter = int(seed), 0
        self.num_envs = self.device = None
        self.actions = self.env_actions = self.gaussian_actions = self.log_prob = self.noise = None
        if num_envs is not None:
            self._allocate(int(num_envs), torch.device("cuda" if device is None else device))

    @classmethod
    def for_env(cls, venv, seed=0, **kwargs):
        """The head of a TactileVecEnv (or a DeviceVecNormalize over one): its action space, num_envs and device."""
        return cls(venv.action_space, seed=seed, num_envs=venv.num_envs, device=torch.device("cuda", venv._cfg.device), **kwargs)

    def _allocate(self, N, device):
        if N < 1:
            raise ValueError(f"num_envs must be positive, got {N}")
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs, self.device = N, device
        f32 = dict(dtype=torch.float32, device=device)
        self.actions, self.env_actions = torch.zeros((N, self.action_dim), **f32), torch.zeros((N, self.action_dim), **f32)
        self.gaussian_actions, self.noise = torch.zeros((N, self.action_dim), **f32), torch.zeros((N, self.action_dim), **f32)
        self.log_prob = torch.zeros(N, **f32)

    # ------------------------------------------------------------------ the C entry (tests replace these two methods)
    def _is_device(self, t):
        return t.is_cuda

    def _c_head(self, mode, mean, log_std, stride, deterministic):
        """tg_action_head at (seed, counter) into the head's own tensors; mean / log_std: None in the uniform mode."""
        own = (None, None) if mode == capi.HEAD_UNIFORM else (self.gaussian_actions, self.log_prob)
        launch("tg_action_head", self.device, ptr(mean), ptr(log_std), stride, self.num_envs, self.action_dim, self._lo, self._hi,
               self.log_std_min, self.log_std_max, mode, 1 if deterministic else 0, self.seed, self.counter, ptr(None), ptr(self.actions),
               ptr(self.env_actions), ptr(own[0]), ptr(own[1]), ptr(self.noise))

    # ------------------------------------------------------------------ sampling
    def _checked(self, x, name, shapes):
        return checked_f32(x, name, shapes, self.device, "the head's device", self._is_device).detach()

    def sample(self, mean, log_std, deterministic=False):
        """(actions, env_actions, log_prob): float32 [N, A], [N, A], [N], the head's own tensors, valid until the next call.  mean: float32
        [N, A]; log_std: float32 [A] or [N, A]; both contiguous (anything else is refused, not copied).  One launch on torch's current stream; the counter moves on by one."""
        A = self.action_dim
        if not isinstance(mean, torch.Tensor):
            raise TypeError(f"mean must be a torch tensor, got {type(mean).__name__}")
        N = self.num_envs if self.num_envs is not None else (int(mean.shape[0]) if mean.dim() == 2 else -1)
        mean = self._checked(mean, "mean", [(N, A)])
        log_std = self._checked(log_std, "log_std", [(A,), (N, A)])
        if log_std.device != mean.device:
            raise ValueError(f"mean and log_std must be on one device, got {mean.device} and {log_std.device}")
        if self.num_envs is None:
            self._allocate(N, mean.device)
        self._c_head(self._mode, mean, log_std, 0 if log_std.dim() == 1 else A, bool(deterministic))
        self.counter += 1
        return self.actions, self.env_actions, self.log_prob

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, sd):
        if set(sd) != {"seed", "counter"}:
            raise ValueError(f"state_dict must have the keys 'seed' and 'counter', got {sorted(sd)}")
        seed, counter = int(sd["seed"]), int(sd["counter"])
        if not (0 <= seed < 1 << 64 and 0 <= counter < 1 << 64):
            raise ValueError(f"seed and counter must lie in [0, 2^64), got {seed} {counter}")
        self.seed, self.counter = seed, counter


class DeviceDiagGaussian(_DeviceHead):
    """stable_baselines3's DiagGaussianDistribution as PPO's collect_rollouts uses it: actions = mean + exp(log_std) eps (stored),
    env_actions = np.clip(actions, low, high) (stepped), log_prob = Normal(mean, exp(log_std)).log_prob(actions).sum(1)."""
    _mode = capi.HEAD_GAUSSIAN

    def __init__(self, action_space, seed=0, num_envs=None, device=None):
        super().__init__(action_space, seed=seed, num_envs=num_envs, device=device)


class DeviceSquashedDiagGaussian(_DeviceHead):
    """stable_baselines3's SquashedDiagGaussianDistribution as SAC's _sample_action uses it: actions = tanh(mean + exp(log_std) eps) in [-1, 1]
    (stored), env_actions = unscale_action(actions) (stepped), log_prob with the tanh correction; log_std is clamped to
    [log_std_min, log_std_max] first, as SAC's actor does."""
    _mode = capi.HEAD_SQUASHED

    def __init__(self, action_space, seed=0, log_std_min=-20.0, log_std_max=2.0, num_envs=None, device=None):
        super().__init__(action_space, seed=seed, log_std_min=log_std_min, log_std_max=log_std_max, num_envs=num_envs, device=device)

    def sample_uniform(self):
        """SAC before learning_starts: (actions, env_actions) with env_actions = action_space.sample() for the whole batch (tg_sample_actions'
        draw at the head's (seed, counter) with the space's bounds) and actions = scale_action(env_actions).  `noise` holds the u in [0, 1)."""
        if self.num_envs is None:
            raise RuntimeError("sample_uniform needs the batch size: make the head with for_env(venv) or num_envs=")
        self._c_head(capi.HEAD_UNIFORM, None, None, 0, False)
        self.counter += 1
        return self.actions, self.env_actions

    def rsample(self, mean, log_std, noise=None):
        """(actions, log_prob): SAC.train's actor.action_log_prob(obs) - sample()'s arithmetic at the head's next (seed, counter), as FRESH
        tensors [B, A] and [B] that carry gradients to mean and log_std (loss_head.squashed_rsample), for any B >= 1: the
        minibatch, not the env batch.  The counter moves on by one.  Under torch.no_grad() (SAC's next actions) nothing is saved.  noise:
        float32 [B, A] used in place of the draws."""
        from .loss_head import squashed_rsample
        if self.device is not None and isinstance(mean, torch.Tensor) and mean.is_cuda and mean.device != self.device:
            raise ValueError(f"mean must be on the head's device {self.device}, got {mean.device}")
        out = squashed_rsample(mean, log_std, self.log_std_min, self.log_std_max, self.seed, self.counter, noise)
        self.counter += 1
        return out
