"""tactile_gym_amd.vec_env without a GPU: what the numpy VecEnv boundary hands out, with the library replaced by a recorder.
The recorder logs every entry's name and integer arguments, and fills every tg_copy_* destination with a value that names the entry, the key
and the terminal flag it came from (column 0 of every env's row: the env's index).  The env is built by the real constructor (obs_mode
"numpy"); the expected C calls and arrays are restated here from the hand-out's description, not from the code under test.  The zero-copy
torch views and the tile download need a device: tests/test_gpu_obs_views.py, tests/test_gpu_boundary.py."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tactile_gym_amd import _capi, vec_env  # noqa: E402

N, H, W, ORACLE_DIM = 3, 4, 4, 10                  # the smallest sizes that keep every axis distinguishable
MODES = ["oracle", "tactile", "visual", "visuotactile", "tactile_and_feature", "visual_and_feature", "visuotactile_and_feature"]
LAYOUTS = [(1, False), (2, False), (1, True), (2, True)]          # (frame_stack, channels_first)
KEYCODE = _capi.OBS_STACK_KEY
ENTRY = {name: i + 1 for i, name in enumerate(["tg_copy_obs_tactile", "tg_copy_obs_visual", "tg_copy_obs_feature", "tg_copy_obs_oracle",
                                               "tg_copy_obs_oracle_terminal", "tg_copy_obs_rows", "tg_copy_obs_stack", "tg_copy_obs_stack_rows"])}
SCENE = {"arm_type": "ur5", "camera": ([0.65, 0.0, 0.05], 0.65, 90.0, -25.0, 75.0, 0.1, 100.0)}


def mark(entry, key, terminal):
    """The value an entry writes: below 256, exact as a byte and as a float."""
    return 16 * ENTRY[entry] + 2 * KEYCODE[key] + int(terminal)


def _addr(a):
    return a.value if isinstance(a, C.c_void_p) else C.cast(a, C.c_void_p).value


class Recorder:
    """The library: every entry is logged as (name, its python-int arguments [, the env ids of a row copy]) and answers 0."""

    def __init__(self, frame_stack, feature_dim):
        self.calls, self.dones, self.fs = [], np.zeros(N, np.uint8), frame_stack
        self.width = {"tactile": H * W, "visual": 3 * H * W, "oracle": ORACLE_DIM, "extended_feature": feature_dim}

    def _fill(self, dst, ids, width, key, value):
        ct = C.c_uint8 if key in ("tactile", "visual") else C.c_float
        a = np.ctypeslib.as_array((ct * (len(ids) * width)).from_address(_addr(dst))).reshape(len(ids), width)
        a[:] = value
        a[:, 0] = ids

    def _ids(self, ptr, n):
        return [int(ptr[j]) for j in range(n)]

    def __getattr__(self, name):
        def entry(*args):
            log = (name, tuple(a for a in args if type(a) is int))
            every = list(range(N))
            if name == "tg_get_reward_done":
                np.ctypeslib.as_array(args[1], (N,))[:] = 0.5 * np.arange(N)
                np.ctypeslib.as_array(args[2], (N,))[:] = self.dones
            elif name == "tg_copy_episode_stats":
                np.ctypeslib.as_array(args[1], (N,))[:] = 10.0 + np.arange(N)
                np.ctypeslib.as_array(args[2], (N,))[:] = 5 + np.arange(N)
            elif name in ("tg_copy_obs_tactile", "tg_copy_obs_visual", "tg_copy_obs_feature"):
                key = {"tg_copy_obs_tactile": "tactile", "tg_copy_obs_visual": "visual", "tg_copy_obs_feature": "extended_feature"}[name]
                self._fill(args[1], every, self.width[key], key, mark(name, key, args[2]))
            elif name in ("tg_copy_obs_oracle", "tg_copy_obs_oracle_terminal"):
                self._fill(args[1], every, ORACLE_DIM, "oracle", mark(name, "oracle", name.endswith("terminal")))
            elif name == "tg_copy_obs_rows":
                key, ids = ("visual" if args[1] else "tactile"), self._ids(args[3], args[4])
                log += (tuple(ids),)
                self._fill(args[5], ids, self.width[key], key, mark(name, key, args[2]))
            elif name == "tg_copy_obs_stack":
                key = {v: k for k, v in KEYCODE.items()}[args[1]]
                self._fill(args[3], every, self.width[key] * self.fs, key, mark(name, key, args[2]))
            elif name == "tg_copy_obs_stack_rows":
                key, ids = {v: k for k, v in KEYCODE.items()}[args[1]], self._ids(args[3], args[4])
                log += (tuple(ids),)
                self._fill(args[5], ids, self.width[key] * self.fs, key, mark(name, key, args[2]))
            elif name.startswith("tg_copy_obs") or name.startswith("tg_get_obs"):
                raise AssertionError(f"{name}: an observation entry this recorder does not know")
            self.calls.append(log)
            return 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls


class Expected:
    """What one key of one hand-out is: the C calls made for it and (shape, dtype, mark, env ids) of the array; mark None: zeros, no call."""

    def __init__(self, mode, frame_stack, channels_first, feature_dim):
        self.fs, self.cf, self.fd = frame_stack, channels_first, feature_dim
        visual = "visual" in mode or "visuo" in mode
        self.keys = [k for k, on in (("oracle", "oracle" in mode), ("tactile", "tactile" in mode), ("visual", visual),
                                     ("extended_feature", "feature" in mode)) if on]

    def stacked(self, key):
        return self.fs > 1 or (key == "visual" and self.cf)

    def shape(self, key, rows):
        n = self.fs if self.stacked(key) else 1
        if key in ("tactile", "visual"):
            c = (3 if key == "visual" else 1) * n
            return ((rows, c, H, W) if self.cf else (rows, H, W, c)), np.uint8
        return (rows, (ORACLE_DIM if key == "oracle" else self.fd) * n), np.float32

    def whole(self, key, terminal):
        t = int(terminal)
        (shape, dtype), ids = self.shape(key, N), list(range(N))
        if shape[-1] == 0:
            return [], (shape, dtype, None, ids)
        if self.stacked(key):
            name, args = "tg_copy_obs_stack", (KEYCODE[key], t)
        elif key == "oracle":
            name, args = ("tg_copy_obs_oracle_terminal" if terminal else "tg_copy_obs_oracle"), ()
        else:
            name, args = {"tactile": "tg_copy_obs_tactile", "visual": "tg_copy_obs_visual", "extended_feature": "tg_copy_obs_feature"}[key], (t,)
        return [(name, args)], (shape, dtype, mark(name, key, terminal), ids)

    def rows(self, key, idx):
        """The terminal observation of the envs `idx`: images and stacks by their row copies, plain vectors from the whole-batch copy."""
        (shape, dtype), ids = self.shape(key, len(idx)), list(idx)
        if shape[-1] == 0:
            return [], (shape, dtype, None, ids)
        if self.stacked(key):
            name = "tg_copy_obs_stack_rows"
            return [(name, (KEYCODE[key], 1, len(ids)), tuple(ids))], (shape, dtype, mark(name, key, True), ids)
        if key in ("tactile", "visual"):
            name = "tg_copy_obs_rows"
            return [(name, (int(key == "visual"), 1, len(ids)), tuple(ids))], (shape, dtype, mark(name, key, True), ids)
        calls, (_, _, m, _) = self.whole(key, True)
        return calls, (shape, dtype, m, ids)

    def batch(self, terminal=False, idx=None):
        calls, specs = [], {}
        for k in self.keys:
            c, specs[k] = self.whole(k, terminal) if idx is None else self.rows(k, idx)
            calls += c
        return calls, specs


def check_array(a, spec, row=None):
    """`a` is the array `spec` describes (row: the one env's row of it, without the batch axis)."""
    shape, dtype, m, ids = spec
    if row is not None:
        shape, ids = shape[1:], [ids[row]]
    assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous, (a.shape, a.dtype, spec)
    flat = a.reshape(len(ids), -1)
    if m is None:
        assert flat.shape[1] == 0
    else:
        assert (flat[:, 0] == ids).all() and (flat[:, 1:] == m).all(), (flat[:, :3], spec)


def check_batch(obs, specs):
    assert list(obs) == list(specs)                                            # the dict's key order
    for k, spec in specs.items():
        check_array(obs[k], spec)


def root(a):
    return a if a.base is None else a.base


def make_env(monkeypatch, mode, frame_stack, channels_first, copy_obs, feature_dim):
    rec = Recorder(frame_stack, feature_dim)
    monkeypatch.setattr(_capi, "lib", lambda: rec)
    monkeypatch.setattr(vec_env.TactileVecEnv, "_set_scene", lambda self, every_step: rec.calls.append(("_set_scene", (int(every_step),))))
    cfg = _capi.TgConfig(num_envs=N, movement_mode=0, auto_reset=1, min_action=-1.0, max_action=1.0)
    sensor = types.SimpleNamespace(struct=_capi.TgSensor(image_h=H, image_w=W))
    env = vec_env.TactileVecEnv(cfg, _capi.TgRobot(ndof=6), sensor, None, observation_mode=mode, obs_mode="numpy", oracle_dim=ORACLE_DIM,
                                feature_dim=feature_dim, copy_obs=copy_obs, scene_spec=SCENE, frame_stack=frame_stack, channels_first=channels_first)
    return env, rec


@pytest.mark.parametrize("copy_obs", [True, False], ids=["copy", "ring"])
@pytest.mark.parametrize("frame_stack,channels_first", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_the_numpy_boundary_hands_out_each_key_from_its_one_source(monkeypatch, mode, frame_stack, channels_first, copy_obs):
    for feature_dim in (0, 3):
        env, rec = make_env(monkeypatch, mode, frame_stack, channels_first, copy_obs, feature_dim)
        exp = Expected(mode, frame_stack, channels_first, feature_dim)
        init = [("tg_create", ())] + [("tg_enable_oracle_obs", ())] * ("oracle" in exp.keys) + [("_set_scene", (1,))] * ("visual" in exp.keys)
        init += [("tg_set_obs_layout", (1,))] * channels_first + [("tg_set_frame_stack", (frame_stack,))] * (frame_stack > 1)
        assert rec.take() == init
        assert list(env.observation_space.spaces) == exp.keys
        for k in exp.keys:
            assert tuple(env.observation_space[k].shape) == exp.shape(k, N)[0][1:] and env.observation_space[k].dtype == exp.shape(k, N)[1]
        fetch, specs = exp.batch()
        actions = np.zeros((N, env.act_dim), np.float32)

        batches = [env.reset()]
        assert rec.take() == [("tg_reset", ()), ("tg_sync", ())] + fetch
        check_batch(batches[0], specs)

        rec.dones[:] = 0                                                       # a step in which no env finishes
        env.step_async(actions)
        assert rec.take() == [("tg_step", (0,))]
        obs, rew, dones, infos = env.step_wait()
        batches.append(obs)
        assert rec.take() == [("tg_get_reward_done", ())] + fetch              # the synchronising call first, then the observation
        check_batch(obs, specs)
        assert rew.dtype == np.float32 and rew.tolist() == [0.0, 0.5, 1.0] and dones.dtype == bool and not dones.any()
        assert len(infos) == N and all(i is vec_env._EMPTY_INFO for i in infos)

        rec.dones[:] = [1, 0, 1]                                               # envs 0 and 2 finish, with auto-reset
        term_calls, term_specs = exp.batch(terminal=True, idx=[0, 2])
        obs, rew, dones, infos = env.step(actions)
        batches.append(obs)
        assert rec.take() == [("tg_step", (0,)), ("tg_get_reward_done", ())] + fetch + [("tg_copy_episode_stats", ())] + term_calls
        check_batch(obs, specs)
        assert dones.tolist() == [True, False, True] and infos[1] is vec_env._EMPTY_INFO
        for j, i in enumerate((0, 2)):
            assert list(infos[i]) == ["episode", "terminal_observation", "TimeLimit.truncated"] and infos[i]["TimeLimit.truncated"] is False
            ep = infos[i]["episode"]
            assert ep["r"] == 10.0 + i and ep["l"] == 5 + i and type(ep["l"]) is int and ep["t"] >= 0
            assert list(infos[i]["terminal_observation"]) == exp.keys
            for k in exp.keys:
                check_array(infos[i]["terminal_observation"][k], term_specs[k], row=j)

        whole_calls, whole_specs = exp.batch(terminal=True)                    # the whole terminal batch, as replay / vecnorm ask for it
        check_batch(env._terminal_observation(), whole_specs)
        assert rec.take() == whole_calls

        rec.dones[:] = 0
        for _ in range(3):
            batches.append(env.step(actions)[0])
        if "tactile" in exp.keys and not exp.stacked("tactile"):               # the plain tactile copy: four rotating buffers, or owned arrays
            roots = [root(b["tactile"]) for b in batches[:5]]
            assert len({id(r) for r in roots[:4]}) == 4
            assert (roots[4] is roots[0]) == (not copy_obs)
            if not copy_obs and not channels_first:
                assert batches[4]["tactile"] is batches[0]["tactile"] and root(env.tactile_numpy(terminal=True)) is not roots[1]
        for k in exp.keys:                                                     # every other array handed out is one of its own
            if k != "tactile" or exp.stacked(k):
                assert len({id(root(b[k])) for b in batches}) == len(batches)
        rec.take()
        env.close()
        assert rec.take() == [("tg_destroy", ())]


def test_the_module_and_a_numpy_env_do_not_import_torch():
    """A fresh interpreter: importing the module, building an env and one reset / step in obs_mode "numpy" leave torch unimported."""
    import subprocess
    code = ("import sys, types, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from tactile_gym_amd import _capi, vec_env\n"
            "class L:\n"
            "    def __getattr__(self, name):\n"
            "        return lambda *a: 0\n"
            "_capi.lib = lambda: L()\n"
            "cfg = _capi.TgConfig(num_envs=2, movement_mode=0, auto_reset=1)\n"
            "sensor = types.SimpleNamespace(struct=_capi.TgSensor(image_h=4, image_w=4))\n"
            "env = vec_env.TactileVecEnv(cfg, _capi.TgRobot(ndof=6), sensor, None, observation_mode='tactile_and_feature', feature_dim=3, channels_first=True)\n"
            "env.reset(); env.step(np.zeros((2, 2), np.float32)); env.close()\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n" % ROOT)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
