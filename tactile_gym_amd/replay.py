"""A replay buffer in device memory: stable_baselines3's ReplayBuffer / DictReplayBuffer (the off-policy buffer of the reference's SAC / RAD_SAC)
over torch tensors on the ROCm device, filled from obs_mode="torch" observations and sampled as augmented minibatches without a trip through
the host (csrc/tg_replay.hip: k_replay_add, k_replay_draw; the image keys through augment.py's one fused-gather entry: csrc/tg_augment.hip,
the row-indexed k_random_translate, or csrc/tg_affine.hip, the row-indexed k_random_affine; csrc/tg_rollout.hip: k_rollout_gather).

    buf = tg.DeviceReplayBuffer.for_env(venv, buffer_size=100_000, seed=0)
    buf.start(venv.reset())
    for step in range(total):                                 # SB3's collect_rollouts with train_freq = 1
        actions = policy(obs)
        obs, _, _, _ = venv.step(actions)
        buf.add_from_env(actions)                             # one launch AFTER the step: _store_transition, terminal observations included
        batch = buf.sample(64, augment=augmentations)         # one draw launch + one per image key (+ one for vector keys)
        ...                                                   # batch.observations, .actions, .next_observations, .dones, .rewards

    buf.add(obs, next_obs, action, reward, done, infos)       # SB3's own call, with tensors (or numpy arrays) of the caller's

Storage is a step-major ring [T, N, ...] (T = buffer_size // n_envs, N = n_envs), allocated once: float32 `actions` [T, N, A], float32 [T, N]
`rewards`, `dones`, `timeouts`, and per observation key ONE allocation [2, T, N, ...] in the key's dtype whose halves are `observations[k]` and
`next_observations[k]`: the next observation of storage row r is row r + T N of the same base, so one row table serves both halves of a
minibatch.  In the carried form (start / add_next / add_from_env) the next observation is also written ahead into observations[pos + 1] - it
IS the following transition's observation - so nothing has to be kept from before the step.  The draw is counter based (seed, counter, sample)
on tg_sample_actions' generator and restated in tests/replay_ref.py; its distribution is that of SB3's two np.random.randint calls, its numbers
are not (PARITY_ASSUMPTIONS.md A43).  There is no CPU path: a CPU device raises.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _capi as capi
from ._device import call, launch, on_device, ptr, stream_of
from .augment import _chw, _gather_images
from .rollout import _DeviceBuffer, _positive_int
from .vecnorm import DeviceVecNormalize

__all__ = ["DeviceReplayBuffer", "ReplayBufferSamples"]

ReplayBufferSamples = collections.namedtuple("ReplayBufferSamples", ["observations", "actions", "next_observations", "dones", "rewards"])

_M64 = 0xFFFFFFFFFFFFFFFF


class DeviceReplayBuffer(_DeviceBuffer):
    """stable_baselines3's ReplayBuffer / DictReplayBuffer in device memory (constructor arguments in SB3's positional order).  channels_first:
    the layout of the image keys, as in DeviceRolloutBuffer; seed: of sample()'s counter-based draw."""

    def __init__(self, buffer_size, observation_space, action_space, device="cuda", n_envs=1, optimize_memory_usage=False,
                 handle_timeout_termination=True, channels_first=None, seed=0):
        if optimize_memory_usage:
            raise NotImplementedError("optimize_memory_usage=True is not built (SB3's DictReplayBuffer refuses it as well)")
        super().__init__(buffer_size, observation_space, action_space, device, n_envs, channels_first)
        self.buffer_size = max(int(buffer_size) // self.n_envs, 1)          # SB3: the ring's length in steps
        self.optimize_memory_usage = False
        self.handle_timeout_termination = bool(handle_timeout_termination)
        if 2 * len(self._obs_spec) + 4 > capi.ROLLOUT_MAX_ARRAYS:
            raise ValueError(f"observation_space has {len(self._obs_spec)} keys, at most {(capi.ROLLOUT_MAX_ARRAYS - 4) // 2} are built")
        T, N = self.buffer_size, self.n_envs
        if T >= 1 << 31 or N >= 1 << 31:
            raise ValueError(f"buffer_size // n_envs = {T} and n_envs = {N} must be below 2^31")
        self._pair = {k: self._alloc((2, T, N) + shape, dt) for k, (shape, dt) in self._obs_spec.items()}
        self._obs = {k: p[0] for k, p in self._pair.items()}
        self._next = {k: p[1] for k, p in self._pair.items()}
        self.observations = self._obs if self._dict_obs else self._obs[None]
        self.next_observations = self._next if self._dict_obs else self._next[None]
        self.actions = self._alloc((T, N, self.action_dim), torch.float32)
        for name in ("rewards", "dones", "timeouts"):
            setattr(self, name, self._alloc((T, N), torch.float32))
        self._no_timeouts = self._alloc((N,), torch.float32)                 # the source of a slot's timeouts when none are given
        self._row_bytes = {k: p[0, 0, 0].numel() * p.element_size() for k, p in self._pair.items()}
        n = capi.ROLLOUT_MAX_ARRAYS
        self._tab = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_int32 * n)()
        self.seed, self.counter = int(seed), 0
        self.pos, self.full = 0, False
        self._carry = False                # observations[pos] holds the head of a transition that add_next() completes
        self._venv = self._env_tab = None

    @classmethod
    def for_env(cls, venv, buffer_size, seed=0):
        """The buffer of a TactileVecEnv (obs_mode="torch"): its spaces, num_envs, device and image layout; add_from_env() reads the env's own
        device buffers."""
        if getattr(venv, "obs_mode", None) != "torch":
            raise ValueError("for_env needs an env made with obs_mode='torch' (its observations are read in device memory)")
        if isinstance(venv, DeviceVecNormalize):               # the originals are stored, as SB3's replay buffer does: sample(env=) normalises
            venv = venv.venv
        buf = cls(buffer_size, venv.observation_space, venv.action_space, device=torch.device("cuda", venv._cfg.device), n_envs=venv.num_envs,
                  channels_first=bool(venv.channels_first), seed=seed)
        buf._venv = venv
        return buf

    def reset(self):
        """Empty the ring (the storage keeps its contents) and forget a pending carry; the draw counter moves on."""
        self.pos, self.full, self._carry = 0, False, False

    # ------------------------------------------------------------------ add
    def _transition_inputs(self, next_obs, action, reward, done, infos, terminal_obs, timeouts):
        """Every argument of add() / add_next() after `obs`, checked and then placed: (next_obs list, terminal list or None, action, reward,
        done as uint8, timeouts, select or None)."""
        N = self.n_envs
        nxt = self._obs_inputs(next_obs, "next_obs")
        term = self._obs_inputs(terminal_obs, "terminal_obs") if terminal_obs is not None else None
        act = self._input(action, "action", (N, self.action_dim), (torch.float32,))
        rew = self._input(reward, "reward", (N,), (torch.float32,))
        dn = self._input(done, "done", (N,), (torch.uint8, torch.bool, torch.float32))
        if timeouts is not None and infos is not None:
            raise ValueError("timeouts and infos: give one of them")
        if infos is not None:
            if not isinstance(infos, (list, tuple)) or len(infos) != N:
                raise ValueError(f"infos must be a list of {N} dicts, got {type(infos).__name__}")
            timeouts = np.array([bool(info.get("TimeLimit.truncated", False)) for info in infos], dtype=np.float32)
        to = self._input(timeouts, "timeouts", (N,), (torch.float32, torch.uint8, torch.bool)) if timeouts is not None else None
        nxt = [self._place(c) for c in nxt]
        term = [self._place(c) for c in term] if term is not None else None
        act, rew, dn = self._place(act), self._place(rew), self._place(dn)
        to = self._place(to) if to is not None and self.handle_timeout_termination else self._no_timeouts
        if dn.dtype == torch.float32:
            dn = dn != 0                                                     # stored as 0.0 / 1.0 whatever the values: one more launch
        dn = dn.view(torch.uint8) if dn.dtype == torch.bool else dn
        to = to.view(torch.uint8) if to.dtype == torch.bool else to
        return nxt, term, act, rew, dn, to

    def _launch(self, arrays, select):
        """One tg_replay_add over `arrays`: (source, alternative or None, destination tensor of N rows)."""
        src_tab, alt_tab, dst_tab, bytes_tab, kind_tab = self._tab
        N = self.n_envs
        for i, (s, a, d) in enumerate(arrays):
            src_tab[i], alt_tab[i], dst_tab[i] = s.data_ptr(), (a.data_ptr() if a is not None else None), d.data_ptr()
            flag = s.dtype == torch.uint8 and d.dtype == torch.float32       # done / timeout flags as uint8
            kind_tab[i] = capi.ROLLOUT_FLAG_U8 if flag else capi.ROLLOUT_COPY
            bytes_tab[i] = s.numel() * s.element_size() // N
        launch("tg_replay_add", self._device_index(), len(arrays), src_tab, alt_tab, dst_tab, bytes_tab, kind_tab, N, ptr(select))

    def _advance(self):
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full, self.pos = True, 0

    def add(self, obs, next_obs, action, reward, done, infos=None, *, terminal_obs=None, timeouts=None):
        """SB3's add(): write slot `pos` and advance it (a ring: `full` becomes True on the wrap).  done: uint8, bool or float32 [N], stored as
        0.0 / 1.0.  timeouts: a tensor [N], or `infos`, SB3's list of dicts whose "TimeLimit.truncated" is read on the host; neither: zeros.
        With handle_timeout_termination=False zeros are stored whatever is given (SB3 then skips the infos and leaves its timeouts zero).
        terminal_obs: like obs, rows valid where done; next_observations[pos][n] is terminal_obs[n] where done[n], else next_obs[n] (what
        OffPolicyAlgorithm._store_transition does with infos[i]["terminal_observation"]).  One launch on torch's current stream when every
        argument is a device tensor (and done is not float32).  The inputs are only read; a refused call writes nothing."""
        cur = self._obs_inputs(obs, "obs")
        nxt, term, act, rew, dn, to = self._transition_inputs(next_obs, action, reward, done, infos, terminal_obs, timeouts)
        cur = [self._place(c) for c in cur]
        p = self.pos
        arrays = [(s, None, self._obs[k][p]) for s, k in zip(cur, self._obs_spec)]
        arrays += [(s, term[i] if term is not None else None, self._next[k][p]) for i, (s, k) in enumerate(zip(nxt, self._obs_spec))]
        arrays += [(act, None, self.actions[p]), (rew, None, self.rewards[p]), (dn, None, self.dones[p]), (to, None, self.timeouts[p])]
        self._launch(arrays, dn if term is not None else None)
        self._carry = False
        self._advance()

    def start(self, obs):
        """The carried form: write observations[pos], the head of the transition that the next add_next() completes."""
        cur = [self._place(c) for c in self._obs_inputs(obs, "obs")]
        self._launch([(s, None, self._obs[k][self.pos]) for s, k in zip(cur, self._obs_spec)], None)
        self._carry = True

    def add_next(self, next_obs, action, reward, done, *, terminal_obs=None, timeouts=None):
        """Complete the pending transition in one launch: slot pos's next_observations (terminal_obs where done), actions, rewards, dones and
        timeouts, and observations[(pos + 1) % T] = next_obs - the post-reset observation, SB3's _last_obs, the head of the next transition."""
        if not self._carry:
            raise RuntimeError("add_next without a pending observation: call start(obs) first (a full add() ends the carried form)")
        nxt, term, act, rew, dn, to = self._transition_inputs(next_obs, action, reward, done, None, terminal_obs, timeouts)
        p, q = self.pos, (self.pos + 1) % self.buffer_size
        arrays = [(s, term[i] if term is not None else None, self._next[k][p]) for i, (s, k) in enumerate(zip(nxt, self._obs_spec))]
        arrays += [(s, None, self._obs[k][q]) for s, k in zip(nxt, self._obs_spec)]
        arrays += [(act, None, self.actions[p]), (rew, None, self.rewards[p]), (dn, None, self.dones[p]), (to, None, self.timeouts[p])]
        self._launch(arrays, dn if term is not None else None)
        self._advance()

    # ------------------------------------------------------------------ the env's own buffers
    def _build_env_table(self):
        """The sources of add_from_env, once: the library's buffers never move (rebuilt when the selected observation target changes)."""
        venv = self._venv
        obs, rd = venv._observation(), venv.reward_done_torch()
        term = venv._terminal_observation() if venv._cfg.auto_reset else None
        K = len(self._obs_spec)
        n = 2 * K + 4
        src, alt, row_bytes, kinds = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_int32 * n)()
        for i, k in enumerate(self._obs_spec):
            shape, dt = self._obs_spec[k]
            for t in (obs[k],) + ((term[k],) if term is not None else ()):
                if tuple(t.shape) != (self.n_envs,) + shape or t.dtype != dt or not t.is_contiguous():
                    raise ValueError(f"the env's observation {k!r} is {tuple(t.shape)} {t.dtype}, the buffer holds {(self.n_envs,) + shape} {dt}")
            for j in (i, K + i):                                             # next_observations[pos] (terminal where done), observations[pos + 1]
                src[j], alt[j] = obs[k].data_ptr(), (term[k].data_ptr() if term is not None and j < K else None)
                row_bytes[j], kinds[j] = self._row_bytes[k], capi.ROLLOUT_COPY
        # destination bases and slot sizes, in table order
        order = [self._next[k] for k in self._obs_spec] + [self._obs[k] for k in self._obs_spec] + [self.actions, self.rewards, self.dones,
                                                                                                  self.timeouts]
        dst_base = [d.data_ptr() for d in order]
        slot_bytes = [d[0].numel() * d.element_size() for d in order]
        src[2 * K], row_bytes[2 * K], kinds[2 * K] = None, 4 * self.action_dim, capi.ROLLOUT_COPY          # the caller's actions: per call
        src[2 * K + 1], row_bytes[2 * K + 1], kinds[2 * K + 1] = rd[0].data_ptr(), 4, capi.ROLLOUT_COPY
        src[2 * K + 2], row_bytes[2 * K + 2], kinds[2 * K + 2] = rd[1].data_ptr(), 1, capi.ROLLOUT_FLAG_U8
        src[2 * K + 3], row_bytes[2 * K + 3], kinds[2 * K + 3] = self._no_timeouts.data_ptr(), 4, capi.ROLLOUT_COPY   # this env never truncates
        self._env_tab = dict(n=n, K=K, src=src, alt=alt, dst=(C.c_void_p * n)(), row_bytes=row_bytes, kinds=kinds, dst_base=dst_base,
                             slot_bytes=slot_bytes, select=ptr(rd[1] if term is not None else None),
                             target=getattr(venv, "_obs_sel", 0), keep=(obs, term, rd))

    def add_from_env(self, actions):
        """add_next() with every source but the actions taken from the env this buffer was made for (for_env): its observation views, its
        terminal observation views where done, reward_done_torch(); timeouts are zeros (the env never truncates).  Call it after
        venv.step(actions); start(venv.reset()) begins the sequence.  One ctypes call, one launch."""
        if self._venv is None:
            raise RuntimeError("add_from_env needs a buffer made by DeviceReplayBuffer.for_env(venv, ...)")
        if not self._carry:
            raise RuntimeError("add_from_env without a pending observation: call start(venv.reset()) first")
        if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32 or tuple(actions.shape) != (self.n_envs, self.action_dim) \
                or not actions.is_contiguous():
            raise ValueError(f"actions must be a contiguous float32 tensor of shape {(self.n_envs, self.action_dim)}")
        dev = self._device_index()
        if not actions.is_cuda or actions.device != dev:
            raise ValueError(f"actions must be on the buffer's device ({self.device}; there is no CPU path), got {actions.device}")
        if self._env_tab is None or self._env_tab["target"] != getattr(self._venv, "_obs_sel", 0):
            self._build_env_table()
        tab = self._env_tab
        K, p, q = tab["K"], self.pos, (self.pos + 1) % self.buffer_size
        dst, base, slot = tab["dst"], tab["dst_base"], tab["slot_bytes"]
        for j in range(tab["n"]):
            dst[j] = base[j] + (q if K <= j < 2 * K else p) * slot[j]
        tab["src"][2 * K] = actions.data_ptr()
        launch("tg_replay_add", dev, tab["n"], tab["src"], tab["alt"], dst, tab["row_bytes"], tab["kinds"], self.n_envs, tab["select"])
        self._advance()

    # ------------------------------------------------------------------ sample
    def _slot_range(self):
        """(number of slots, first slot) that sample() draws from."""
        T = self.buffer_size
        if not self.full:
            if self.pos == 0:
                raise RuntimeError("sample() from an empty replay buffer")
            return self.pos, 0
        if self._carry:                    # slot pos holds the head of an unfinished transition (SB3's exclusion under optimize_memory_usage)
            if T == 1:
                raise RuntimeError("sample() with a pending carry needs buffer_size // n_envs >= 2: the one slot is being rewritten")
            return T - 1, (self.pos + 1) % T
        return T, 0

    def sample(self, batch_size, env=None, augment=None, out_dtype=torch.float32):
        """ReplayBufferSamples(observations, actions, next_observations, dones, rewards) of new device tensors: dones and rewards [B, 1], dones
        = dones * (1 - timeouts).  Image keys come out float32 (0 ... 255), through `augment` - a RandomTranslate, a RandomWarp or the nn.Sequential
        holding one - when given: observations and next_observations of a key are the two halves of ONE call of the module over 2 B samples (its counter
        advances by one, `_params` covers 2 B samples; the two halves draw independently).  out_dtype=torch.uint8 without augment keeps them
        uint8.  `env` is SB3's VecNormalize argument: a DeviceVecNormalize, whose current statistics normalise the vector keys of observations
        and next_observations and the rewards in one more launch (image keys and `augment` are not touched by it)."""
        if env is not None and not isinstance(env, DeviceVecNormalize):
            raise NotImplementedError(f"sample(env=...): only a tactile_gym_amd DeviceVecNormalize is built, got {type(env).__name__}")
        B = _positive_int(batch_size, "batch_size")
        module = self._image_options(augment, out_dtype)
        M, first = self._slot_range()
        T, N = self.buffer_size, self.n_envs
        dev = self._device_index()
        obs, nxt, plain = {}, {}, []              # plain: (pair [2, T, N, ...], destination [2 B, ...]) of the one k_rollout_gather launch
        whole = {}                                # their destinations by key: what sample(env=) normalises
        with on_device(dev):
            stream = stream_of(dev)
            rows = torch.empty((2 * B,), dtype=torch.int64, device=dev)
            actions = torch.empty((B, self.action_dim), dtype=torch.float32, device=dev)
            rewards, dones = torch.empty((B, 1), dtype=torch.float32, device=dev), torch.empty((B, 1), dtype=torch.float32, device=dev)
            call("tg_replay_draw", B, M, first, T, N, C.c_uint64(self.seed & _M64), C.c_uint64(self.counter & _M64), ptr(self.actions),
                 self.action_dim, ptr(self.rewards), ptr(self.dones), ptr(self.timeouts), T * N, ptr(rows), ptr(actions), ptr(rewards),
                 ptr(dones), stream)
            self.counter += 1
            for k, (shape, dt) in self._obs_spec.items():
                src = self._pair[k]
                if k in self._image_keys and out_dtype == torch.float32:
                    out = torch.empty((2 * B,) + shape, dtype=torch.float32, device=dev)
                    cf = self._channels_first[k]
                    _gather_images(module, src, out, rows, 2 * B, *_chw(shape, cf), cf, stream.value)   # one launch: augment.py
                else:
                    out = torch.empty((2 * B,) + shape, dtype=dt, device=dev)
                    plain.append((src, out))
                    whole[k] = out
                obs[k], nxt[k] = out[:B], out[B:]
            if plain:
                self._gather_plain(plain, rows, stream)
            if env is not None:                                # after the gather: both halves of every vector key and the rewards, in place
                env._normalize_sample(whole, rewards)
        if not self._dict_obs:
            obs, nxt = obs[None], nxt[None]
        return ReplayBufferSamples(obs, actions, nxt, dones, rewards)
