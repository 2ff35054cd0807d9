"""Reference of tactile_gym_amd.replay (csrc/tg_replay.hip): stable_baselines3's ReplayBuffer / DictReplayBuffer semantics restated in numpy.

SB3 (common/buffers.py) keeps [T, N, ...] rings, T = max(buffer_size // n_envs, 1); add() writes slot pos and advances it modulo T, `full`
becoming True on the wrap; sample() draws a slot and an env per sample and returns dones * (1 - timeouts).  OffPolicyAlgorithm._store_transition
replaces the next observation of a finished env by infos[i]["terminal_observation"] before add().

ReplayRef restates that, the carried form (start / add_next: the next observation is written ahead into observations[pos + 1]) and the
counter-based draw of the device (draw_rows, on tests/augment_ref.py's mix64); the device output must equal it bit for bit.
"""
import numpy as np

from augment_ref import GOLDEN, M64, draw_params, mix64, mix64_int, warp_f32


def draw_cells(seed, counter, B, n_slots, first, T, N):
    """(t, n) int64 [B] each: h_b = mix64(mix64(seed + G (counter + 1)) + G (b + 1)); j = ((h_b >> 32) M) >> 32; t = (first + j) % T;
    n = ((h_b & 0xffffffff) N) >> 32."""
    assert 1 <= n_slots <= T and n_slots < 1 << 31 and 1 <= N < 1 << 31 and 0 <= first < T
    head = mix64_int((seed + GOLDEN * (counter + 1)) & M64)
    b = np.arange(B, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(np.uint64(head) + np.uint64(GOLDEN) * (b + np.uint64(1)))
    j = ((h >> np.uint64(32)) * np.uint64(n_slots)) >> np.uint64(32)           # both factors below 2^32: exact in uint64
    n = ((h & np.uint64(0xFFFFFFFF)) * np.uint64(N)) >> np.uint64(32)
    t = (np.int64(first) + j.astype(np.int64)) % np.int64(T)
    return t, n.astype(np.int64)


def draw_rows(seed, counter, B, n_slots, first, T, N):
    """Storage rows t N + n, int64 [B]."""
    t, n = draw_cells(seed, counter, B, n_slots, first, T, N)
    return t * np.int64(N) + n


class ReplayRef:
    """obs_spec: {key: (shape, numpy dtype)}; image keys (uint8, three dimensions) with channels_first[key]."""

    def __init__(self, buffer_size, n_envs, obs_spec, action_dim, seed=0, channels_first=None):
        self.N = int(n_envs)
        self.T = max(int(buffer_size) // self.N, 1)
        self.spec = dict(obs_spec)
        self.channels_first = dict(channels_first or {})
        T, N = self.T, self.N
        self.observations = {k: np.zeros((T, N) + tuple(s), dt) for k, (s, dt) in self.spec.items()}
        self.next_observations = {k: np.zeros((T, N) + tuple(s), dt) for k, (s, dt) in self.spec.items()}
        self.actions = np.zeros((T, N, action_dim), np.float32)
        self.rewards, self.dones, self.timeouts = (np.zeros((T, N), np.float32) for _ in range(3))
        self.pos, self.full, self.carry = 0, False, False
        self.seed, self.counter = int(seed), 0

    def _store(self, next_obs, action, reward, done, terminal_obs, timeouts):
        p = self.pos
        d = np.asarray(done) != 0
        for k in self.spec:
            nxt = np.asarray(next_obs[k]).copy()
            if terminal_obs is not None:
                nxt[d] = np.asarray(terminal_obs[k])[d]
            self.next_observations[k][p] = nxt
        self.actions[p], self.rewards[p], self.dones[p] = action, reward, d.astype(np.float32)
        self.timeouts[p] = 0.0 if timeouts is None else np.asarray(timeouts).astype(np.float32)

    def _advance(self):
        self.pos += 1
        if self.pos == self.T:
            self.full, self.pos = True, 0

    def add(self, obs, next_obs, action, reward, done, terminal_obs=None, timeouts=None):
        for k in self.spec:
            self.observations[k][self.pos] = obs[k]
        self._store(next_obs, action, reward, done, terminal_obs, timeouts)
        self.carry = False
        self._advance()

    def start(self, obs):
        for k in self.spec:
            self.observations[k][self.pos] = obs[k]
        self.carry = True

    def add_next(self, next_obs, action, reward, done, terminal_obs=None, timeouts=None):
        if not self.carry:
            raise RuntimeError("add_next without start")
        self._store(next_obs, action, reward, done, terminal_obs, timeouts)
        for k in self.spec:
            self.observations[k][(self.pos + 1) % self.T] = next_obs[k]       # unselected: the post-reset observation
        self._advance()

    def slot_range(self):
        """(M, first)."""
        if not self.full:
            if self.pos == 0:
                raise RuntimeError("empty")
            return self.pos, 0
        if self.carry:
            if self.T == 1:
                raise RuntimeError("one slot, being rewritten")
            return self.T - 1, (self.pos + 1) % self.T
        return self.T, 0

    def sample(self, B, augment=None, out_uint8=False):
        """augment: None or (translate, p, seed, counter-by-key-order list): one module call per image key, its counter moving on by one each.
        {observations, next_observations, actions, dones, rewards, rows, params: {key: [2 B, 3]}}."""
        M, first = self.slot_range()
        T, N = self.T, self.N
        rows = draw_rows(self.seed, self.counter, B, M, first, T, N)
        self.counter += 1
        both = np.concatenate([rows, rows + T * N])
        obs, nxt, params = {}, {}, {}
        n_calls = 0
        for k, (shape, dt) in self.spec.items():
            pair = np.concatenate([self.observations[k].reshape((T * N,) + tuple(shape)), self.next_observations[k].reshape((T * N,) + tuple(shape))])
            g = pair[both]
            if np.dtype(dt) == np.uint8 and len(shape) == 3 and not out_uint8:
                cf = self.channels_first[k]
                H, W = (shape[1], shape[2]) if cf else (shape[0], shape[1])
                if augment is not None:
                    translate, p, seed, counter = augment
                    prm = draw_params(seed, counter + n_calls, 2 * B, translate, p, H, W)
                    n_calls += 1
                else:
                    prm = np.zeros((2 * B, 3), np.float32)
                params[k] = prm
                g = warp_f32(g, prm, cf)
            obs[k], nxt[k] = g[:B], g[B:]
        flat = lambda a: a.reshape((T * N,) + a.shape[2:])   # noqa: E731
        dones = (flat(self.dones)[rows] * (np.float32(1) - flat(self.timeouts)[rows])).astype(np.float32)
        return dict(observations=obs, next_observations=nxt, actions=flat(self.actions)[rows], dones=dones.reshape(B, 1),
                    rewards=flat(self.rewards)[rows].reshape(B, 1), rows=both, params=params, module_calls=n_calls)
