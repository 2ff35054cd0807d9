"""CPU tests of the frame stack (frame_stack=n): the numpy restatement of VecFrameStack, the stacked spaces, the Python-level refusals, the new
kernel's resources and the new C ABI symbols.  The device results are checked against the restatement in tests/test_gpu_frame_stack.py."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from frame_stack_ref import StackRef  # noqa: E402

import tactile_gym_amd as tg  # noqa: E402
from tactile_gym_amd import _capi, spaces  # noqa: E402

NEW_SYMBOLS = ["tg_set_frame_stack", "tg_get_frame_stack", "tg_get_obs_stack", "tg_copy_obs_stack", "tg_copy_obs_stack_rows"]


def test_restatement_hand_worked_n3():
    """Two envs, vectors of one element, n = 3; env 0 finishes in step 2 (terminal frame 12, reset observation 100)."""
    ref = StackRef(3)
    st = ref.reset({"v": np.array([[10.0], [20.0]], np.float32)})
    assert st["v"].tolist() == [[0, 0, 10], [0, 0, 20]]
    st, term = ref.step({"v": np.array([[11.0], [21.0]], np.float32)}, np.array([0, 0], bool), None)
    assert st["v"].tolist() == [[0, 10, 11], [0, 20, 21]] and term == {}
    st, term = ref.step({"v": np.array([[100.0], [22.0]], np.float32)}, np.array([1, 0], bool), {0: {"v": np.array([12.0], np.float32)}})
    assert st["v"].tolist() == [[0, 0, 100], [20, 21, 22]]
    assert list(term) == [0] and term[0]["v"].tolist() == [10, 11, 12]
    st, _ = ref.step({"v": np.array([[101.0], [23.0]], np.float32)}, np.array([0, 0], bool), None)
    assert st["v"].tolist() == [[0, 100, 101], [21, 22, 23]]
    # without a terminal observation (auto_reset off): the stack is zeroed, nothing is reported
    st, term = ref.step({"v": np.array([[102.0], [24.0]], np.float32)}, np.array([0, 1], bool), None)
    assert st["v"].tolist() == [[100, 101, 102], [0, 0, 24]] and term == {}
    # masked reset: env 0 only
    st = ref.reset({"v": np.array([[7.0], [99.0]], np.float32)}, np.array([1, 0], bool))
    assert st["v"].tolist() == [[0, 0, 7], [0, 0, 24]]


def test_restatement_images_interleave_slots_per_pixel():
    ref = StackRef(2)
    a = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4, 1)
    st = ref.reset({"tactile": a})
    assert st["tactile"].shape == (2, 3, 4, 2)
    assert (st["tactile"][..., 0] == 0).all() and (st["tactile"][..., 1] == a[..., 0]).all()
    b = a + 100
    st, term = ref.step({"tactile": b}, np.array([1, 0], bool), {0: {"tactile": a[0] + 50}})
    assert (term[0]["tactile"][..., 0] == a[0, ..., 0]).all() and (term[0]["tactile"][..., 1] == a[0, ..., 0] + 50).all()
    assert (st["tactile"][0, ..., 0] == 0).all() and (st["tactile"][1, ..., 0] == a[1, ..., 0]).all()
    assert (st["tactile"][..., 1] == b[..., 0]).all()


def test_restatement_matches_stable_baselines3():
    pytest.importorskip("stable_baselines3")
    gym_spaces = pytest.importorskip("gymnasium.spaces")
    from stable_baselines3.common.vec_env import VecEnv, VecFrameStack

    obs_space = gym_spaces.Dict({"tactile": gym_spaces.Box(0, 255, (4, 4, 1), np.uint8),
                                 "oracle": gym_spaces.Box(-np.inf, np.inf, (3,), np.float32)})
    act_space = gym_spaces.Box(-1, 1, (2,), np.float32)
    record = []

    class Fake(VecEnv):
        def __init__(self):
            self.rng = np.random.default_rng(1)
            self.t = 0
            super().__init__(3, obs_space, act_space)

        def _obs(self):
            return {"tactile": self.rng.integers(0, 255, (3, 4, 4, 1), dtype=np.uint8), "oracle": self.rng.standard_normal((3, 3)).astype(np.float32)}

        def reset(self):
            o = self._obs()
            record.append(("reset", o))
            return o

        def step_async(self, actions):
            pass

        def step_wait(self):
            self.t += 1
            o = self._obs()
            done = np.array([self.t % 3 == 0, self.t % 4 == 0, False])
            infos = [{} for _ in range(3)]
            for i in np.nonzero(done)[0]:
                infos[i]["terminal_observation"] = {k: v[i] + 1 for k, v in self._obs().items()}
            record.append(("step", o, done, {int(i): {k: v.copy() for k, v in infos[i]["terminal_observation"].items()} for i in np.nonzero(done)[0]}))
            return o, np.zeros(3, np.float32), done, infos

        def close(self):
            pass

        def get_attr(self, *a, **k):
            return [None] * 3

        def set_attr(self, *a, **k):
            pass

        def env_method(self, *a, **k):
            return [None] * 3

        def env_is_wrapped(self, *a, **k):
            return [False] * 3

    v = VecFrameStack(Fake(), n_stack=3)
    got = [v.reset()]
    for _ in range(9):
        o, _, _, infos = v.step(np.zeros((3, 2), np.float32))
        got.append((o, infos))
    ref = StackRef(3)
    assert all(np.array_equal(ref.reset(record[0][1])[k], got[0][k]) for k in got[0])
    for (_, o, done, term), (go, ginfos) in zip(record[1:], got[1:]):
        st, tst = ref.step(o, done, term)
        for k in st:
            assert np.array_equal(st[k], go[k])
        for i in tst:
            for k in tst[i]:
                assert np.array_equal(tst[i][k], ginfos[i]["terminal_observation"][k])


def test_stacked_spaces():
    d = spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(128, 128, 1), dtype=np.uint8),
                     "oracle": spaces.Box(low=np.arange(4, dtype=np.float32), high=np.arange(4, dtype=np.float32) + 10, dtype=np.float32)})
    assert spaces.stacked(d, 1) is d
    s = spaces.stacked(d, 3)
    assert s["tactile"].shape == (128, 128, 3) and s["tactile"].dtype == np.uint8
    assert (s["tactile"].low == 0).all() and (s["tactile"].high == 255).all()
    assert s["oracle"].shape == (12,) and s["oracle"].dtype == np.float32
    assert np.array_equal(s["oracle"].low, np.repeat(np.arange(4, dtype=np.float32), 3))
    assert np.array_equal(s["oracle"].high, np.repeat(np.arange(4, dtype=np.float32) + 10, 3))


def test_single_env_classes_refuse_frame_stack():
    from tactile_gym_amd.rl_envs.edge_follow import EdgeFollowEnv
    with pytest.raises(TypeError, match="vec_env_kwargs"):
        EdgeFollowEnv(image_size=[128, 128], frame_stack=2)


@pytest.mark.parametrize("bad", [0, 9, 2.5, True])
def test_frame_stack_range_is_refused(bad):
    """Checked before the device is touched."""
    from tactile_gym_amd.vec_env import TactileVecEnv

    class _Probe(TactileVecEnv):
        def __init__(self):
            TactileVecEnv.__init__(self, None, None, None, None, frame_stack=bad)

    import tactile_gym_amd.vec_env as ve
    old = ve.capi.lib
    ve.capi.lib = lambda: None
    try:
        with pytest.raises(ValueError, match="frame_stack"):
            _Probe()
    finally:
        ve.capi.lib = old


def test_tiles_transfer_and_visual_modes_refused_with_a_stack():
    from tactile_gym_amd.vec_env import TactileVecEnv
    v = TactileVecEnv.__new__(TactileVecEnv)
    v.frame_stack = 2
    with pytest.raises(ValueError, match="frame_stack"):
        TactileVecEnv.set_obs_transfer(v, "tiles")

    class _Cfg:
        num_envs = 1
    import tactile_gym_amd.vec_env as ve
    old = ve.capi.lib
    ve.capi.lib = lambda: None
    try:
        with pytest.raises(NotImplementedError, match="frame_stack"):
            TactileVecEnv(_Cfg(), None, None, None, observation_mode="visuotactile", scene_spec={}, frame_stack=2)
    finally:
        ve.capi.lib = old


def test_every_vec_env_constructor_takes_frame_stack():
    import inspect
    from tactile_gym_amd.rl_envs import edge_follow, object_balance, object_push, object_roll, surface_follow
    from tactile_gym_amd.vec_env import TactileVecEnv
    classes = [edge_follow.EdgeFollowVecEnv, object_balance.ObjectBalanceVecEnv, object_push.ObjectPushVecEnv, object_roll.ObjectRollVecEnv,
               surface_follow.SurfaceFollowAutoVecEnv, surface_follow.SurfaceFollowGoalVecEnv, surface_follow.SurfaceFollowVertVecEnv, TactileVecEnv]
    for cls in classes:
        p = inspect.signature(cls.__init__).parameters
        assert "frame_stack" in p and p["frame_stack"].default == 1, cls.__name__


def test_new_symbols_in_header_ctypes_and_library():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS, name
    lib = os.path.join(ROOT, "tactile_gym_amd", "lib", "libtactile_gym_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    assert _capi.OBS_KEY == {"tactile": 0, "oracle": 1, "extended_feature": 2}
    for key, val in _capi.OBS_KEY.items():
        macro = {"tactile": "TACTILE", "oracle": "ORACLE", "extended_feature": "FEATURE"}[key]
        assert re.search(r"#define TG_OBS_KEY_%s %d\b" % (macro, val), header)


def test_frame_stack_kernel_uses_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = _kernel_scratch(tmp_path)
    ks = {k: v for k, v in scratch.items() if "k_frame_stack" in k}
    assert len(ks) == 7, sorted(scratch)[:20]          # n = 2 .. 8
    assert all(v == 0 for v in ks.values()), ks
