"""A rollout buffer in device memory: stable_baselines3's RolloutBuffer / DictRolloutBuffer (the on-policy buffer of the reference's PPO /
RAD_PPO) over torch tensors on the ROCm device, filled from obs_mode="torch" observations and read as augmented minibatches without a trip
through the host (csrc/tg_rollout.hip: k_rollout_add, k_rollout_gae, k_rollout_gather; the image keys through augment.py's one fused-gather
entry: csrc/tg_augment.hip, the row-indexed k_random_translate, or for a RandomWarp csrc/tg_affine.hip, the row-indexed k_random_affine).

    buf = tg.DeviceRolloutBuffer.for_env(venv, n_steps, gamma=0.95, gae_lambda=0.9)
    obs, starts = venv.reset(), torch.ones(venv.num_envs, device=buf.device)
    for t in range(n_steps):                                  # SB3's collect_rollouts
        actions, values, log_probs = policy(obs)
        buf.add(obs, actions, zeros, starts, values, log_probs)          # one launch; BEFORE the step: obs are the env's zero-copy views,
        obs, _, _, _ = venv.step(actions)                                # which the step rewrites in place
        rewards, dones = venv.reward_done_torch()
        buf.rewards[t].copy_(rewards)                                    # the step's reward into the slot just written
        starts = dones.clone()
    buf.compute_returns_and_advantage(last_values, starts)              # one launch
    for batch in buf.get(batch_size, augment=augmentations):            # one launch per image key + one
        ...                                                              # batch.observations, .actions, .old_values, .old_log_prob, .advantages, .returns

(With observations that are tensors of their own - clones, numpy arrays - add() can come after the step with its reward, as in SB3.)

Storage is step-major [T, N, ...] (T = buffer_size, N = n_envs), allocated once: one tensor per observation key in its own dtype, float32
`actions` [T, N, A] and float32 [T, N] `rewards`, `episode_starts`, `values`, `log_probs`, `advantages`, `returns`.  SB3's flat sample index
i = n T + t (its swap_and_flatten order) addresses storage row t N + n; nothing is transposed.  Image keys (uint8, three stored dimensions per
sample) come out of get() as float32 with values 0 ... 255, the convention of tactile_gym_amd.augment, or as uint8 on request.  The arithmetic of
compute_returns_and_advantage is restated bit for bit in tests/rollout_ref.py.  There is no CPU path: a CPU device raises.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _capi as capi
from ._device import call, launch, on_device, ptr, stream_of
from .augment import _chw, _gather_images, _unwrap_augment

__all__ = ["DeviceRolloutBuffer", "RolloutBufferSamples", "flat_rows"]

RolloutBufferSamples = collections.namedtuple("RolloutBufferSamples",
                                              ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])

_OBS_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}
_NUMPY_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.bool_): torch.bool}


def flat_rows(indices, T, N):
    """Storage rows (t N + n) of SB3's flat sample indices (i = n T + t): a tensor like `indices`."""
    return (indices % T) * N + indices // T


def _space_shapes(space, name):
    """{key: (shape, torch dtype)} of a Box or a Dict of Boxes (key None for a Box)."""
    sub = space.spaces if hasattr(space, "spaces") else {None: space}
    out = {}
    for k, s in sub.items():
        label = name if k is None else f"{name}[{k!r}]"
        if hasattr(s, "spaces") or getattr(s, "shape", None) is None or getattr(s, "dtype", None) is None:
            raise TypeError(f"{label} must be a Box (nested or non-Box spaces are not built), got {s!r}")
        dt = np.dtype(s.dtype)
        if dt not in _OBS_DTYPES:
            raise TypeError(f"{label} must be uint8 or float32, got {dt}")
        out[k] = (tuple(int(d) for d in s.shape), _OBS_DTYPES[dt])
    if not out:
        raise ValueError(f"{name} has no keys")
    return out


def _positive_int(v, name, tail=""):
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{name} must be a positive integer{tail}, got {v!r}")
    return int(v)


class _DeviceBuffer:
    """What DeviceRolloutBuffer and DeviceReplayBuffer share: the constructor's checks up to the image keys' layout table, the checks of what
    add() and get() / sample() are handed, and the tg_rollout_gather launch.  A subclass sets `buffer_size` (in steps), checks its own
    ROLLOUT_MAX_ARRAYS budget and allocates."""

    def __init__(self, buffer_size, observation_space, action_space, device, n_envs, channels_first):
        _positive_int(buffer_size, "buffer_size")
        self.n_envs = _positive_int(n_envs, "n_envs")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device must be the ROCm device (there is no CPU path), got {self.device}")
        self.observation_space, self.action_space = observation_space, action_space
        self._obs_spec = _space_shapes(observation_space, "observation_space")
        self._dict_obs = None not in self._obs_spec
        act = _space_shapes(action_space, "action_space")
        if None not in act or act[None][1] != torch.float32 or len(act[None][0]) != 1:
            raise TypeError(f"action_space must be a float32 Box of one dimension, got {action_space!r}")
        self.action_dim = act[None][0][0]
        self._image_keys = [k for k, (shape, dt) in self._obs_spec.items() if dt == torch.uint8 and len(shape) == 3]
        if channels_first is not None and not isinstance(channels_first, (bool, np.bool_)):
            raise ValueError(f"channels_first={channels_first!r}: True, False or None")
        self._channels_first = {}
        for k in self._image_keys:
            shape = self._obs_spec[k][0]
            cf = bool(np.argmin(shape) == 0) if channels_first is None else bool(channels_first)
            c, h, w = shape if cf else (shape[2], shape[0], shape[1])
            if h < 2 or w < 2:
                raise ValueError(f"observation_space key {k!r}: image keys need H, W >= 2, got shape {shape} (channels_first={cf})")
            self._channels_first[k] = cf

    def _alloc(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def size(self):
        return self.buffer_size if self.full else self.pos

    def _device_index(self):
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    # ------------------------------------------------------------------ what add() is handed
    def _input(self, x, name, shape, dtypes):
        """`x` checked as a contiguous tensor of `shape` and one of `dtypes`: (tensor, name, whether it came from numpy and still has to be
        uploaded).  _place() does the device half, after every argument of a call has passed this one."""
        if isinstance(x, np.ndarray):
            nd = _NUMPY_DTYPES.get(x.dtype)
            if nd not in dtypes:
                if not (dtypes[0] == torch.float32 and np.issubdtype(x.dtype, np.floating)):
                    raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got numpy {x.dtype}")
                x = x.astype(np.float32)                                # numpy float64 rewards: stored as float32, as SB3 does
            if len(shape) == 1 and tuple(x.shape) == shape + (1,):
                x = x.reshape(shape)
            if tuple(x.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(x.shape)}")
            return torch.from_numpy(np.ascontiguousarray(x)), name, True
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor or a numpy array, got {type(x).__name__}")
        if x.dtype not in dtypes:
            raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
        if tuple(x.shape) != shape:
            if len(shape) == 1 and tuple(x.shape) == shape + (1,) and x.is_contiguous():
                x = x.view(shape)                                   # SB3's values come as [N, 1]
            else:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(x.shape)}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return x, name, False

    def _place(self, checked):
        x, name, from_numpy = checked
        if from_numpy:
            return x.to(self._device_index())
        if not x.is_cuda or x.device != self._device_index():
            raise ValueError(f"{name} must be on the buffer's device ({self.device}; there is no CPU path), got {x.device}")
        return x

    def _obs_inputs(self, obs, name):
        """_input over an observation: every key of a Dict space (the dict's keys checked first), or the one tensor of a Box."""
        N = self.n_envs
        if self._dict_obs:
            if not isinstance(obs, dict) or set(obs) != set(self._obs_spec):
                raise ValueError(f"{name} must be a dict with the keys {sorted(self._obs_spec)}, got "
                                 f"{sorted(obs) if isinstance(obs, dict) else type(obs).__name__}")
            return [self._input(obs[k], f"{name}[{k!r}]", (N,) + shape, (dt,)) for k, (shape, dt) in self._obs_spec.items()]
        shape, dt = self._obs_spec[None]
        return [self._input(obs, name, (N,) + shape, (dt,))]

    # ------------------------------------------------------------------ what get() / sample() are handed, and their plain gather
    @staticmethod
    def _image_options(augment, out_dtype):
        """The module of `augment` (None for None) after the checks of out_dtype and of the two together."""
        module = _unwrap_augment(augment) if augment is not None else None
        if out_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
        if module is not None and out_dtype != torch.float32:
            raise ValueError("out_dtype must be torch.float32 with augment (the augmentation writes float32)")
        return module

    @staticmethod
    def _gather_plain(plain, rows, stream):
        """One k_rollout_gather launch on `stream`: for every (source, destination [B, ...]) of `plain`, destination[b] = the source's storage
        row rows[b] (a row is one destination sample: the source's leading dimensions are the row index)."""
        n, B = len(plain), rows.numel()
        src_tab, dst_tab, bytes_tab = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
        for i, (s, d) in enumerate(plain):
            src_tab[i], dst_tab[i], bytes_tab[i] = s.data_ptr(), d.data_ptr(), d.numel() // B * d.element_size()
        call("tg_rollout_gather", n, src_tab, dst_tab, bytes_tab, ptr(rows), B, stream)


class DeviceRolloutBuffer(_DeviceBuffer):
    """stable_baselines3's RolloutBuffer / DictRolloutBuffer in device memory (constructor arguments in SB3's positional order).  channels_first:
    the layout of the image keys ([C, H, W] or [H, W, C] per sample), needed by get(augment=...); None applies SB3's rule
    (is_image_space_channels_first: the smallest of the three dimensions comes first)."""

    def __init__(self, buffer_size, observation_space, action_space, device="cuda", gae_lambda=1.0, gamma=0.99, n_envs=1, channels_first=None):
        super().__init__(buffer_size, observation_space, action_space, device, n_envs, channels_first)
        self.buffer_size = int(buffer_size)
        self.gae_lambda, self.gamma = float(gae_lambda), float(gamma)
        if len(self._obs_spec) + 5 > capi.ROLLOUT_MAX_ARRAYS:
            raise ValueError(f"observation_space has {len(self._obs_spec)} keys, at most {capi.ROLLOUT_MAX_ARRAYS - 5} are built")
        T, N = self.buffer_size, self.n_envs
        self._obs = {k: self._alloc((T, N) + shape, dt) for k, (shape, dt) in self._obs_spec.items()}
        self.observations = self._obs if self._dict_obs else self._obs[None]
        self.actions = self._alloc((T, N, self.action_dim), torch.float32)
        for name in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, self._alloc((T, N), torch.float32))
        self._add_dst = list(self._obs.values()) + [self.actions, self.rewards, self.episode_starts, self.values, self.log_probs]
        self._add_slot_bytes = [t[0].numel() * t.element_size() for t in self._add_dst]
        n = len(self._add_dst)
        self._tab = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_int32 * n)()
        self.pos, self.full = 0, False

    @classmethod
    def for_env(cls, venv, n_steps, gamma=0.99, gae_lambda=1.0):
        """The buffer of a TactileVecEnv: its spaces, num_envs, device and image layout."""
        return cls(n_steps, venv.observation_space, venv.action_space, device=torch.device("cuda", venv._cfg.device), gae_lambda=gae_lambda,
                   gamma=gamma, n_envs=venv.num_envs, channels_first=bool(venv.channels_first))

    def reset(self):
        """Start a new rollout.  The storage keeps its contents (every slot is rewritten before the buffer is full again)."""
        self.pos, self.full = 0, False

    # ------------------------------------------------------------------ add
    def add(self, obs, action, reward, episode_start, value, log_prob):
        """Write slot `pos` and advance it: one launch on torch's current stream when every argument is a device tensor.  The inputs are only read."""
        if self.full:
            raise RuntimeError(f"add to a full rollout buffer (buffer_size={self.buffer_size}): call reset() first")
        N = self.n_envs
        srcs = self._obs_inputs(obs, "obs")
        srcs.append(self._input(action, "action", (N, self.action_dim), (torch.float32,)))
        srcs.append(self._input(reward, "reward", (N,), (torch.float32,)))
        srcs.append(self._input(episode_start, "episode_start", (N,), (torch.float32, torch.uint8, torch.bool)))
        srcs.append(self._input(value, "value", (N,), (torch.float32,)))
        srcs.append(self._input(log_prob, "log_prob", (N,), (torch.float32,)))
        srcs = [self._place(c) for c in srcs]
        srcs = [t.view(torch.uint8) if t.dtype == torch.bool else t for t in srcs]
        src_tab, dst_tab, bytes_tab, kind_tab = self._tab
        for i, (s, d) in enumerate(zip(srcs, self._add_dst)):
            src_tab[i] = s.data_ptr()
            dst_tab[i] = d.data_ptr() + self.pos * self._add_slot_bytes[i]
            flag = s.dtype == torch.uint8 and d.dtype == torch.float32           # the episode starts as the env's uint8 done flags
            kind_tab[i] = capi.ROLLOUT_FLAG_U8 if flag else capi.ROLLOUT_COPY
            bytes_tab[i] = s.numel() * s.element_size()
        launch("tg_rollout_add", self._device_index(), len(srcs), src_tab, dst_tab, bytes_tab, kind_tab)
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True

    # ------------------------------------------------------------------ GAE
    def compute_returns_and_advantage(self, last_values, dones):
        """SB3's GAE(lambda) over the stored rollout: fills `advantages` and `returns` (one launch).  last_values: float32 [N] (or [N, 1]), the
        value of the observation after the last step; dones: bool, uint8 or float32 [N], whether that step ended the episode."""
        N = self.n_envs
        lv = self._input(last_values, "last_values", (N,), (torch.float32,))
        dn = self._input(dones, "dones", (N,), (torch.uint8, torch.bool, torch.float32))
        lv, dn = self._place(lv), self._place(dn)
        if dn.dtype == torch.bool:
            dn = dn.view(torch.uint8)
        launch("tg_rollout_gae", self._device_index(), ptr(self.rewards), ptr(self.values), ptr(self.episode_starts), ptr(lv), ptr(dn),
               capi.ROLLOUT_DONES["uint8" if dn.dtype == torch.uint8 else "float32"], ptr(self.advantages), ptr(self.returns), self.buffer_size,
               N, self.gamma, self.gae_lambda)

    # ------------------------------------------------------------------ get
    def get(self, batch_size=None, augment=None, indices=None, out_dtype=torch.float32, generator=None):
        """A generator over the minibatches of the full buffer (RolloutBufferSamples of new device tensors).  Without `indices` the order is one
        torch.randperm(T N) on the device (`generator`: a device torch.Generator); with `indices` (int64, SB3's flat sample indices i = n T + t,
        checked once for range) that order is used.  Slices of batch_size are yielded, the last one shorter; None is the whole buffer.  Image keys
        come out float32 (0 ... 255), through `augment` - a RandomTranslate, a RandomWarp or the nn.Sequential holding one - when given, each image key of each
        minibatch being one call of the module (its counter advances, `_params` is set); out_dtype=torch.uint8 without augment keeps them uint8."""
        if not self.full:
            raise RuntimeError(f"get() needs a full rollout buffer: {self.pos} of {self.buffer_size} steps added")
        module = self._image_options(augment, out_dtype)
        T, N = self.buffer_size, self.n_envs
        total = T * N
        batch_size = _positive_int(total if batch_size is None else batch_size, "batch_size", " or None")
        if indices is not None:
            if isinstance(indices, np.ndarray):
                indices = torch.from_numpy(indices)
            if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64 or indices.dim() != 1:
                raise TypeError("indices must be a 1-D int64 tensor")
            if indices.numel() and (int(indices.min()) < 0 or int(indices.max()) >= total):     # the one check (and wait) of this call
                raise ValueError(f"indices must lie in [0, {total}), got [{int(indices.min())}, {int(indices.max())}]")
            indices = indices.to(self._device_index())
        else:
            indices = torch.randperm(total, device=self._device_index(), generator=generator)
        rows = flat_rows(indices, T, N).contiguous()
        return self._batches(rows, batch_size, module, out_dtype)

    def _batches(self, rows, batch_size, module, out_dtype):
        for start in range(0, rows.numel(), batch_size):
            yield self._gather(rows[start:start + batch_size], module, out_dtype)

    def _gather(self, rows, module, out_dtype):
        B = rows.numel()
        dev = self._device_index()
        obs, plain = {}, []                       # plain: (source [T, N, ...], destination [B, ...]) of the one k_rollout_gather launch
        with on_device(dev):
            stream = stream_of(dev)
            for k, (shape, dt) in self._obs_spec.items():
                src = self._obs[k]
                if k in self._image_keys and out_dtype == torch.float32:
                    out = torch.empty((B,) + shape, dtype=torch.float32, device=dev)
                    cf = self._channels_first[k]
                    _gather_images(module, src, out, rows, B, *_chw(shape, cf), cf, stream.value)   # one launch: augment.py
                else:
                    out = torch.empty((B,) + shape, dtype=dt, device=dev)
                    plain.append((src, out))
                obs[k] = out
            fields = []
            for src in (self.actions, self.values, self.log_probs, self.advantages, self.returns):
                out = torch.empty((B,) + tuple(src.shape[2:]), dtype=torch.float32, device=dev)
                plain.append((src, out))
                fields.append(out)
            self._gather_plain(plain, rows, stream)
        return RolloutBufferSamples(obs if self._dict_obs else obs[None], *fields)
