"""stable_baselines3's VecFrameStack semantics restated in numpy (StackedObservations, channels last), and the rollout the device frame stack is
checked with (tests/test_gpu_frame_stack.py; also run in a child process there).

Per observation key, a stack of n frames along the last axis, oldest first:
- reset: every slot 0 but the newest, which holds the reset observation (reset(mask): the masked envs only);
- step: shift one slot toward the oldest; a done env's terminal observation becomes concat(old stack's newest n - 1 slots, terminal frame) when the
  VecEnv reports one, then its stack is zeroed; the step's observation goes into the newest slot.
"""
import hashlib

import numpy as np


class StackRef:
    def __init__(self, n):
        self.n = n
        self.st = None

    def reset(self, obs, mask=None):
        if self.st is None:
            self.st = {k: np.zeros(v.shape[:-1] + (v.shape[-1] * self.n,), v.dtype) for k, v in obs.items()}
        rows = np.ones(len(next(iter(obs.values()))), bool) if mask is None else np.asarray(mask, bool)
        for k, v in obs.items():
            c = v.shape[-1]
            self.st[k][rows] = 0
            self.st[k][rows, ..., -c:] = v[rows]
        return {k: s.copy() for k, s in self.st.items()}

    def step(self, obs, dones, terminal=None):
        """terminal: {env: {key: frame}} (the VecEnv's info["terminal_observation"]) or None (none reported).  Returns (stacks, terminal stacks)."""
        term = {}
        for k, v in obs.items():
            c = v.shape[-1]
            s = np.roll(self.st[k], -c, axis=-1)
            for i in np.nonzero(dones)[0]:
                if terminal is not None and i in terminal:
                    term.setdefault(int(i), {})[k] = np.concatenate([s[i, ..., :-c], terminal[i][k]], axis=-1)
                s[i] = 0
            s[..., -c:] = v
            self.st[k] = s
        return {k: s.copy() for k, s in self.st.items()}, term


def _host(obs):
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.array(v)) for k, v in obs.items()}


def rollout(env_id, num_envs, frame_stack, steps, env_modes, obs_mode="numpy", auto_reset=True, max_steps=7, image_size=(128, 128), mask_at=3,
            seed=5, **kw):
    """reset, `steps` random-action steps with a reset(mask) of every third env before step `mask_at` (puts the episodes out of phase).
    Returns the event list: ("reset", mask, obs) and ("step", actions, obs, reward, done, {env: terminal obs})."""
    import tactile_gym_amd as tg
    venv = tg.make_vec(env_id, num_envs=num_envs, max_steps=max_steps, image_size=list(image_size), env_modes=env_modes, seed=seed,
                       auto_reset=auto_reset, obs_mode=obs_mode, frame_stack=frame_stack, **kw)
    rng = np.random.default_rng(seed)
    lo, hi = float(np.min(venv.action_space.low)), float(np.max(venv.action_space.high))
    ev = [("reset", None, _host(venv.reset()))]
    for t in range(steps):
        if t == mask_at:
            mask = (np.arange(num_envs) % 3 == 1).astype(np.uint8)
            ev.append(("reset", mask, _host(venv.reset(mask))))
        a = rng.uniform(lo, hi, size=(num_envs, venv.act_dim)).astype(np.float32)
        obs, rew, done, infos = venv.step(a)
        term = {int(i): _host(infos[i]["terminal_observation"]) for i in np.nonzero(done)[0] if "terminal_observation" in infos[i]}
        ev.append(("step", a, _host(obs), np.array(rew), np.array(done), term))
    venv.close()
    return ev


def digest(events):
    h = hashlib.sha256()
    for e in events:
        for part in e[1:]:
            if isinstance(part, dict):
                for k in sorted(part, key=str):
                    v = part[k]
                    if isinstance(v, dict):
                        for kk in sorted(v):
                            h.update(np.ascontiguousarray(v[kk]).tobytes())
                    else:
                        h.update(np.ascontiguousarray(v).tobytes())
            elif part is not None:
                h.update(np.ascontiguousarray(part).tobytes())
    return h.hexdigest()


def expected_from_single(events, n):
    """Apply the restatement to a frame_stack=1 rollout: the events a frame_stack=n rollout of the same env, seed and actions must produce."""
    ref, out = StackRef(n), []
    for e in events:
        if e[0] == "reset":
            out.append(("reset", e[1], ref.reset(e[2], e[1])))
        else:
            _, a, obs, rew, done, term = e
            st, tst = ref.step(obs, done, term if term else None)
            out.append(("step", a, st, rew, done, tst))
    return out
