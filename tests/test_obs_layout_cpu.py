"""CPU tests of channels_first (VecTransposeImage on the device) and of the visual frame stacks: the numpy restatement (obs_layout_ref) on
hand-built batches, spaces.transposed, the refusals that need no device, and the new C ABI.  The device results are checked against the
restatement in tests/test_gpu_obs_layout.py."""
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
from obs_layout_ref import (TransposeRef, expected_layout, is_image_space, is_image_space_channels_first, transpose_image,  # noqa: E402
                            transpose_space_shape)

from tactile_gym_amd import _capi, spaces  # noqa: E402

NEW_SYMBOLS = ["tg_set_obs_layout", "tg_get_obs_layout"]


def _rgb(n_envs, h, w, base):
    """[N, H, W, 3]: pixel (e, y, x) is base + 50 e + 10 y + 3 x, plus 0 / 1 / 2 in r / g / b (distinct bytes in these small images)."""
    e, y, x = np.meshgrid(np.arange(n_envs), np.arange(h), np.arange(w), indexing="ij")
    v = base + 50 * e + 10 * y + 3 * x
    return np.stack([v, v + 1, v + 2], axis=-1).astype(np.uint8)


def test_visual_channel_order_is_3s_plus_rgb():
    """Two envs, 2 x 2 rgb images, n = 2: channel 3 s + c of the channels-first stack is colour c of stack slot s (oldest first)."""
    st, tr = StackRef(2), TransposeRef()
    f0, f1 = _rgb(2, 2, 2, 0), _rgb(2, 2, 2, 120)
    o = tr.reset(st.reset({"visual": f0}))["visual"]
    assert o.shape == (2, 6, 2, 2) and o.flags.c_contiguous
    assert (o[:, :3] == 0).all()                                   # the older slot is zero after a reset
    for c in range(3):
        assert np.array_equal(o[:, 3 + c], f0[..., c])
    s, term = st.step({"visual": f1}, np.array([0, 0], bool), None)
    o, _ = tr.step(s, {})
    for c in range(3):
        assert np.array_equal(o["visual"][:, c], f0[..., c]) and np.array_equal(o["visual"][:, 3 + c], f1[..., c])
    assert o["visual"][1, 4, 1, 0] == f1[1, 1, 0, 1]               # env 1, slot 1, green, y 1, x 0


def test_done_zeroes_older_slots_and_builds_the_terminal_stack():
    """n = 3, one env finishes in the second step: its terminal stack is the old stack's newest two slots then the terminal frame; its live
    stack is zero but for the reset frame.  Tactile and visual keys in one batch, channels first."""
    st, tr = StackRef(3), TransposeRef()
    tac = [np.full((2, 2, 2, 1), 10 * k + 1, np.uint8) for k in range(4)]
    vis = [_rgb(2, 2, 2, 30 * k) for k in range(4)]
    tr.reset(st.reset({"tactile": tac[0], "visual": vis[0]}))
    tr.step(*st.step({"tactile": tac[1], "visual": vis[1]}, np.array([0, 0], bool), None)[:1], {})
    term_frames = {0: {"tactile": tac[0][0] + 7, "visual": vis[0][0] + 7}}
    s, t = st.step({"tactile": tac[2], "visual": vis[2]}, np.array([1, 0], bool), term_frames)
    o, tt = tr.step(s, t)
    # live: env 0 reset (zeros, zeros, new frame); env 1 slots (f0, f1, f2)
    assert (o["tactile"][0, :2] == 0).all() and (o["tactile"][0, 2] == tac[2][0, ..., 0]).all()
    assert [int(o["tactile"][1, k, 0, 0]) for k in range(3)] == [1, 11, 21]
    assert (o["visual"][0, :6] == 0).all()
    for c in range(3):
        assert np.array_equal(o["visual"][0, 6 + c], vis[2][0, ..., c])
        assert np.array_equal(o["visual"][1, c], vis[0][1, ..., c]) and np.array_equal(o["visual"][1, 3 + c], vis[1][1, ..., c])
    # terminal (one env, no batch axis): (f0, f1, terminal frame), transposed (2, 0, 1)
    assert list(tt) == [0]
    assert tt[0]["tactile"].shape == (3, 2, 2) and [int(tt[0]["tactile"][k, 1, 1]) for k in range(3)] == [1, 11, 8]
    assert tt[0]["visual"].shape == (9, 2, 2)
    for c in range(3):
        assert np.array_equal(tt[0]["visual"][c], vis[0][0, ..., c]) and np.array_equal(tt[0]["visual"][3 + c], vis[1][0, ..., c])
        assert np.array_equal(tt[0]["visual"][6 + c], vis[0][0, ..., c] + 7)


def test_expected_layout_leaves_vectors_and_n1_tactile_bytes():
    """n = 1, channels first: a tactile batch keeps its bytes ([N, H, W, 1] is [N, 1, H, W]), vectors are untouched, rewards / dones pass."""
    rng = np.random.default_rng(0)
    tac = rng.integers(0, 255, (3, 4, 4, 1), dtype=np.uint8)
    vec = rng.standard_normal((3, 5)).astype(np.float32)
    ev = [("reset", None, {"tactile": tac, "oracle": vec}),
          ("step", None, {"tactile": tac, "oracle": vec}, np.zeros(3, np.float32), np.array([1, 0, 0], bool), {0: {"tactile": tac[0], "oracle": vec[0]}})]
    out = expected_layout(ev, 1, True)
    assert out[0][2]["tactile"].shape == (3, 1, 4, 4) and out[0][2]["tactile"].tobytes() == tac.tobytes()
    assert out[0][2]["oracle"] is vec
    assert out[1][5][0]["tactile"].shape == (1, 4, 4) and out[1][5][0]["tactile"].tobytes() == tac[0].tobytes()
    assert expected_layout(ev, 1, False) is ev


def test_transposed_and_stacked_spaces_match_sb3_shapes():
    d = spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(128, 128, 1), dtype=np.uint8),
                     "visual": spaces.Box(low=0, high=255, shape=(128, 128, 3), dtype=np.uint8),
                     "extended_feature": spaces.Box(low=-np.inf, high=np.inf, shape=(12,), dtype=np.float32)})
    for n in (1, 2, 3, 4, 8):
        s = spaces.transposed(spaces.stacked(d, n))
        assert s["tactile"].shape == (n, 128, 128) and s["visual"].shape == (3 * n, 128, 128)
        for k in ("tactile", "visual"):
            sp = s[k]
            assert sp.dtype == np.uint8 and (sp.low == 0).all() and (sp.high == 255).all()
            assert is_image_space(sp) and is_image_space_channels_first(sp)             # SB3 does not wrap it a second time
            assert sp.shape == transpose_space_shape(spaces.stacked(d, n)[k].shape)
        assert s["extended_feature"].shape == (12 * n,) and s["extended_feature"].dtype == np.float32
    b = spaces.Box(low=0, high=255, shape=(64, 64, 3), dtype=np.uint8)
    assert spaces.transposed(b).shape == (3, 64, 64)
    f = spaces.Box(low=0.0, high=1.0, shape=(64, 64, 3), dtype=np.float32)                  # not an image space: unchanged
    assert spaces.transposed(f) is f


def test_transpose_image_forms():
    a = np.arange(2 * 3 * 4 * 5, dtype=np.uint8).reshape(2, 3, 4, 5)
    assert np.array_equal(transpose_image(a), a.transpose(0, 3, 1, 2)) and transpose_image(a).flags.c_contiguous
    assert np.array_equal(transpose_image(a[1]), a[1].transpose(2, 0, 1))


def test_restatement_matches_stable_baselines3():
    pytest.importorskip("stable_baselines3")
    gym_spaces = pytest.importorskip("gymnasium.spaces")
    from stable_baselines3.common.preprocessing import is_image_space_channels_first as sb3_cf
    from stable_baselines3.common.vec_env import VecEnv, VecFrameStack, VecTransposeImage

    # (16 x 16: the stacks' 9 channels stay the smallest axis, as SB3's channel-axis guess needs)
    obs_space = gym_spaces.Dict({"tactile": gym_spaces.Box(0, 255, (16, 16, 1), np.uint8), "visual": gym_spaces.Box(0, 255, (16, 16, 3), np.uint8),
                                 "oracle": gym_spaces.Box(-np.inf, np.inf, (3,), np.float32)})
    act_space = gym_spaces.Box(-1, 1, (2,), np.float32)
    record = []

    class Fake(VecEnv):
        def __init__(self):
            self.rng = np.random.default_rng(1)
            self.t = 0
            super().__init__(3, obs_space, act_space)

        def _obs(self):
            return {"tactile": self.rng.integers(0, 255, (3, 16, 16, 1), dtype=np.uint8), "visual": self.rng.integers(0, 255, (3, 16, 16, 3), dtype=np.uint8),
                    "oracle": self.rng.standard_normal((3, 3)).astype(np.float32)}

        def reset(self):
            o = self._obs()
            record.append(("reset", None, o))
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
            record.append(("step", None, o, np.zeros(3, np.float32), done,
                           {int(i): {k: v.copy() for k, v in infos[i]["terminal_observation"].items()} for i in np.nonzero(done)[0]}))
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

    for n in (1, 2, 3):
        record.clear()
        inner = Fake()
        v = VecTransposeImage(VecFrameStack(inner, n_stack=n) if n > 1 else inner)
        ours = spaces.transposed(spaces.stacked(spaces.Dict({k: spaces.Box(s.low, s.high, s.shape, s.dtype) for k, s in obs_space.spaces.items()}), n))
        for k in obs_space.spaces:
            assert tuple(v.observation_space[k].shape) == tuple(ours[k].shape), (n, k)
        assert sb3_cf(v.observation_space["visual"]) and sb3_cf(v.observation_space["tactile"])
        got = [("reset", v.reset())]
        for _ in range(9):
            o, _, _, infos = v.step(np.zeros((3, 2), np.float32))
            got.append(("step", o, infos))
        exp = expected_layout(record, n, True)
        for e, g in zip(exp, got):
            for k in e[2]:
                assert np.array_equal(e[2][k], g[1][k]), (n, k)
            if e[0] == "step":
                for i in e[5]:
                    for k in e[5][i]:
                        assert np.array_equal(e[5][i][k], g[2][i]["terminal_observation"][k]), (n, i, k)


def test_single_env_classes_refuse_channels_first():
    from tactile_gym_amd.rl_envs.edge_follow import EdgeFollowEnv
    with pytest.raises(TypeError, match="vec_env_kwargs"):
        EdgeFollowEnv(image_size=[128, 128], channels_first=True)


class _Cfg:
    num_envs = 1


class _NoDevice(Exception):
    pass


def _construct(**kw):
    """TactileVecEnv's constructor up to the device (the library stubbed: its first call raises _NoDevice)."""
    import tactile_gym_amd.vec_env as ve

    class _L:
        def __getattr__(self, name):
            raise _NoDevice(name)
    old = ve.capi.lib
    ve.capi.lib = lambda: _L()
    try:
        ve.TactileVecEnv(_Cfg(), None, None, None, **kw)
    finally:
        ve.capi.lib = old


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_channels_first_must_be_a_bool(bad):
    with pytest.raises(ValueError, match="channels_first"):
        _construct(channels_first=bad)


@pytest.mark.parametrize("mode", ["visual", "visuotactile", "visual_and_feature", "visuotactile_and_feature"])
def test_visual_modes_take_a_frame_stack(mode):
    """frame_stack > 1 with a visual mode whose scene has a camera: the constructor goes on to the device."""
    spec = {"arm_type": "ur5", "camera": ([0.65, 0.0, 0.05], 0.65, 90.0, -25.0, 75.0, 0.1, 100.0)}
    for n, cf in ((3, True), (2, False)):
        with pytest.raises(_NoDevice):
            _construct(observation_mode=mode, scene_spec=spec, frame_stack=n, channels_first=cf)


def test_visual_mode_without_a_scene_camera_is_refused():
    """A scene spec without arm and camera has no image to draw or stack: refused before the device, whatever the stacking options."""
    for n, cf in ((1, False), (2, False), (1, True)):
        with pytest.raises(NotImplementedError, match="scene camera"):
            _construct(observation_mode="visuotactile", scene_spec={"arm_type": "ur5"}, frame_stack=n, channels_first=cf)


def test_tiles_transfer_refusals():
    from tactile_gym_amd.vec_env import TactileVecEnv
    v = TactileVecEnv.__new__(TactileVecEnv)
    v.frame_stack, v.channels_first, v._visual = 1, True, True
    with pytest.raises(ValueError, match="channels_first"):
        TactileVecEnv.set_obs_transfer(v, "tiles")
    v.frame_stack = 2
    with pytest.raises(ValueError, match="frame_stack"):
        TactileVecEnv.set_obs_transfer(v, "tiles")


def test_every_vec_env_constructor_takes_channels_first():
    import inspect
    from tactile_gym_amd.rl_envs import edge_follow, object_balance, object_push, object_roll, surface_follow
    from tactile_gym_amd.vec_env import TactileVecEnv
    classes = [edge_follow.EdgeFollowVecEnv, object_balance.ObjectBalanceVecEnv, object_push.ObjectPushVecEnv, object_roll.ObjectRollVecEnv,
               surface_follow.SurfaceFollowAutoVecEnv, surface_follow.SurfaceFollowGoalVecEnv, surface_follow.SurfaceFollowVertVecEnv, TactileVecEnv]
    for cls in classes:
        p = inspect.signature(cls.__init__).parameters
        assert "channels_first" in p and p["channels_first"].default is False, cls.__name__
        src = inspect.getsource(cls.__init__)
        assert cls is TactileVecEnv or "channels_first=channels_first" in src, cls.__name__


def test_new_symbols_in_header_ctypes_and_library():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.SYMBOLS, name
    assert re.search(r"#define TG_OBS_KEY_VISUAL %d\b" % _capi.OBS_STACK_KEY["visual"], header)
    assert re.search(r"#define TG_ABI_VERSION %d\b" % _capi.ABI_VERSION, header) and _capi.ABI_VERSION == 16
    lib = os.path.join(ROOT, "tactile_gym_amd", "lib", "libtactile_gym_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name


def test_obs_stack_kernels_use_no_scratch(tmp_path):
    """Every instantiation of k_obs_stack (n = 1 .. 8, channels first or last) keeps its registers: no scratch memory."""
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = _kernel_scratch(tmp_path)
    ks = {k: v for k, v in scratch.items() if "k_obs_stack" in k}
    assert len(ks) == 16, sorted(ks)
    assert all(v == 0 for v in ks.values()), ks
