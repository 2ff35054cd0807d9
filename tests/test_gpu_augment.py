"""tactile_gym_amd.augment on the device (csrc/tg_augment.hip: k_random_translate) against tests/augment_ref.py: the output equals the float32
restatement bit for bit and kornia's float64 path within the stated tolerance, for uint8 / float32 inputs in both layouts, on synthetic batches
and on the observations of a device env."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from augment_ref import draw_params, tolerance, warp_f32, warp_kornia  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EDGE = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
            arm_type="ur5", tactile_sensor_name="tactip")
SIZES = [(64, 64), (128, 128), (256, 256), (48, 80)]


def _K():
    import tactile_gym_amd.augment as K
    return K


def _batch(seed, B, C, H, W, dtype, channels_first):
    rng = np.random.default_rng(seed)
    shape = (B, C, H, W) if channels_first else (B, H, W, C)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return rng.random(shape, dtype=np.float32) * np.float32(255)


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(x_np, channels_first=True, **kw):
    x = torch.from_numpy(x_np).cuda()
    out, prm = _K().random_translate(x, channels_first=channels_first, return_params=True, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == x_np.shape
    assert np.array_equal(x.cpu().numpy(), x_np)                                   # the input is only read
    return out.cpu().numpy(), prm.cpu().numpy()


def test_drawn_params_equal_the_numpy_draws():
    x = _batch(0, 4097, 1, 16, 16, np.uint8, True)
    for seed, counter, p, tr in ((0, 0, 0.5, (0.05, 0.05)), (123456789, 77, 0.3, (0.1, 0.25)), (2**63 + 5, 2**40, 0.9, (1.0, 0.0))):
        _, prm = _run(x, seed=seed, counter=counter, p=p, translate=tr)
        assert _bits_equal(prm, draw_params(seed, counter, 4097, tr, p, 16, 16)), (seed, counter)


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_output_bit_exact(dtype, hw, channels_first):
    H, W = hw
    x = _batch(H + W, 64, 2, H, W, dtype, channels_first)
    got, prm = _run(x, channels_first, translate=(0.05, 0.05), p=0.5, seed=7, counter=H)
    assert 0 < prm[:, 0].sum() < 64
    assert _bits_equal(got, warp_f32(x, prm, channels_first))
    assert np.abs(got - warp_kornia(x, prm, channels_first)).max() <= tolerance(x)
    keep = prm[:, 0] == 0
    assert _bits_equal(got[keep], x[keep].astype(np.float32))                     # passed through, not resampled


@pytest.mark.parametrize("B", [1, 4097])
@pytest.mark.parametrize("dtype,channels_first", [(np.uint8, True), (np.float32, False)])
def test_batch_sizes(B, dtype, channels_first):
    x = _batch(B, B, 2, 128, 128, dtype, channels_first)
    got, prm = _run(x, channels_first, translate=(0.05, 0.05), p=0.5, seed=B, counter=1)
    assert _bits_equal(got, warp_f32(x, prm, channels_first))


def test_p0_passes_through_and_p1_applies_everywhere():
    x = _batch(5, 256, 2, 64, 64, np.float32, True)
    got, prm = _run(x, p=0.0, translate=(0.05, 0.05), seed=1)
    assert not prm[:, 0].any() and _bits_equal(got, x)
    got, prm = _run(x, p=1.0, translate=(0.05, 0.05), seed=1)
    assert prm[:, 0].all() and _bits_equal(got, warp_f32(x, prm))


@pytest.mark.parametrize("channels_first", [True, False])
def test_explicit_params_equal_drawn_params(channels_first):
    x = _batch(6, 300, 3, 48, 80, np.uint8, channels_first)
    got, prm = _run(x, channels_first, p=0.5, seed=9, counter=4)
    given = torch.from_numpy(prm).cuda()
    got2, prm2 = _run(x, channels_first, p=0.0, translate=(0.0, 0.0), params=given)   # the draws' arguments are ignored
    assert _bits_equal(got2, got) and _bits_equal(prm2, prm)
    mine = np.array([[1.0, 2.5, -1.75], [1.0, -3.0, 0.0], [0.0, 9.0, 9.0]] * 100, np.float32)    # integer and sub-pixel shifts, a pass
    got3, _ = _run(x, channels_first, params=torch.from_numpy(mine).cuda())
    assert _bits_equal(got3, warp_f32(x, mine, channels_first))


def test_seed_and_counter():
    x = _batch(8, 64, 2, 64, 64, np.uint8, True)
    a, _ = _run(x, seed=3, counter=10)
    b, _ = _run(x, seed=3, counter=10)
    c, _ = _run(x, seed=3, counter=11)
    assert _bits_equal(a, b) and not _bits_equal(a, c)


def test_uint8_and_float32_copies_agree():
    for cf in (True, False):
        x = _batch(9, 64, 3, 64, 64, np.uint8, cf)
        a, pa = _run(x, cf, seed=4, counter=2)
        b, pb = _run(x.astype(np.float32), cf, seed=4, counter=2)
        assert _bits_equal(pa, pb) and _bits_equal(a, b)


def test_many_small_images_grid():
    """B = 65 537 x [1, 16, 16]: more samples than a grid dimension of 65 535 holds."""
    x = _batch(10, 65537, 1, 16, 16, np.uint8, True)
    got, prm = _run(x, translate=(0.2, 0.2), p=0.5, seed=12)
    assert _bits_equal(prm, draw_params(12, 0, 65537, (0.2, 0.2), 0.5, 16, 16))
    assert _bits_equal(got, warp_f32(x, prm))


def test_non_default_stream_is_ordered_after_its_producer():
    x_np = _batch(11, 512, 2, 128, 128, np.uint8, True)
    src = torch.from_numpy(x_np).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        big = torch.rand((4096, 4096), device="cuda")
        for _ in range(4):
            big = big @ big                                   # keep the stream busy before the producer's copy
        x = torch.empty_like(src)
        x.copy_(src)
        out, prm = _K().random_translate(x, seed=5, return_params=True)
    s.synchronize()
    assert _bits_equal(out.cpu().numpy(), warp_f32(x_np, prm.cpu().numpy()))


def test_bad_arguments_raise_on_the_device():
    K = _K()
    x = torch.zeros((2, 1, 16, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        K.random_translate(x.reshape(2, 16, 16))
    with pytest.raises(TypeError):
        K.random_translate(x.half())
    with pytest.raises(ValueError):
        K.random_translate(x, translate=(0.05, 1.5))
    with pytest.raises(Exception, match="H >= 2"):
        K.random_translate(torch.zeros((2, 1, 1, 16), dtype=torch.uint8, device="cuda"))
    assert K.random_translate(x[:0]).shape == (0, 1, 16, 16)


def _env(modes, n, **kw):
    import tactile_gym_amd as tg
    return tg.make_vec("edge_follow-v0", num_envs=n, max_steps=40, image_size=[128, 128], env_modes=modes, seed=4, obs_mode="torch",
                       frame_stack=2, channels_first=True, **kw)


def _steps(v, k, seed=0, reset=True):
    rng = np.random.default_rng(seed)
    obs = v.reset() if reset else None
    for _ in range(k):
        obs, _, _, _ = v.step(rng.uniform(-0.25, 0.25, size=(v.num_envs, v.act_dim)).astype(np.float32))
    return obs


def test_env_tactile_stack_through_the_reference_line():
    K = _K()
    v = _env(EDGE, 256)
    try:
        v.set_obs_guard(True)
        obs = _steps(v, 3)
        t = obs["tactile"]
        assert tuple(t.shape) == (256, 2, 128, 128) and t.dtype == torch.uint8
        before = t.cpu().numpy()
        aug = torch.nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5, seed=21))
        out = aug(t)
        m = aug[0]
        prm = draw_params(21, 0, 256, (0.05, 0.05), 0.5, 128, 128)
        assert np.array_equal(m._params["batch_prob"].cpu().numpy(), prm[:, 0] != 0)
        assert _bits_equal(m._params["translations"].cpu().numpy(), prm[:, 1:])
        assert _bits_equal(out.cpu().numpy(), warp_f32(before, prm))
        assert np.array_equal(t.cpu().numpy(), before)
        out2 = aug(t)                                                              # the next minibatch: counter 1
        assert m.counter == 2 and _bits_equal(out2.cpu().numpy(), warp_f32(before, draw_params(21, 1, 256, (0.05, 0.05), 0.5, 128, 128)))
        _steps(v, 1, reset=False)                                                  # the obs guard finds the observation unchanged
    finally:
        v.close()


def test_env_visuotactile_keys_through_augment_images():
    K = _K()
    v = _env(dict(EDGE, observation_mode="visuotactile"), 16)
    try:
        v.set_obs_guard(True)
        obs = _steps(v, 2, seed=1)
        assert tuple(obs["visual"].shape) == (16, 6, 128, 128)
        is_img = {k: isinstance(val, torch.Tensor) and val.dim() == 4 for k, val in obs.items()}
        host = {k: val.cpu().numpy() if isinstance(val, torch.Tensor) else np.array(val) for k, val in obs.items()}
        m = K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=1.0, seed=8)
        out = K.augment_images(obs, m)
        order = [k for k in obs if is_img[k]]                                      # one call per image key, in the dict's order
        assert sorted(out) == sorted(obs) and "tactile" in order and "visual" in order and m.counter == len(order)
        for c, k in enumerate(order):
            prm = draw_params(8, c, 16, (0.05, 0.05), 1.0, 128, 128)
            assert _bits_equal(out[k].cpu().numpy(), warp_f32(host[k], prm)), k
        for k in obs:
            if is_img[k]:
                assert np.array_equal(obs[k].cpu().numpy(), host[k]), k
            else:
                assert out[k] is obs[k]
        _steps(v, 1, seed=2, reset=False)
    finally:
        v.close()


# ---------------------------------------------------------------------------------------------------------------- every family's stream argument
def _cuda(values, dtype=np.float32, grad=False):
    t = torch.from_numpy(np.asarray(values, dtype=dtype)).cuda()
    return t.requires_grad_() if grad else t


def _family_calls(tg):
    """[(name, call)]: one wrapper of each family that launches through tactile_gym_amd._device at the smallest shape its
    kernel accepts.  A call makes its inputs from fixed values, seeds and counters on the current stream and returns the tensors it produced."""
    from tactile_gym_amd import spaces
    rng = lambda: np.random.default_rng(7)  # noqa: E731
    act = spaces.Box(low=-1.0, high=1.0, shape=(1,), dtype=np.float32)
    obs_space = spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(1, 8, 8), dtype=np.uint8),
                             "oracle": spaces.Box(low=-1.0, high=1.0, shape=(3,), dtype=np.float32)})

    def obs(seed):
        r = np.random.default_rng(seed)
        return {"tactile": _cuda(r.integers(0, 256, (1, 1, 8, 8)), np.uint8), "oracle": _cuda(r.uniform(-1, 1, (1, 3)))}

    def ppo():                                                                   # B = 2, A = 1
        mean, log_std, values = _cuda([[0.1], [-0.2]], grad=True), _cuda([-0.5], grad=True), _cuda([0.3, 0.1], grad=True)
        loss, stats = tg.ppo_loss(mean, log_std, values, _cuda([[0.2], [-0.4]]), _cuda([-0.9, -1.1]), _cuda([1.0, -0.5]), _cuda([0.4, 0.2]))
        loss.backward()
        return [stats, mean.grad, log_std.grad, values.grad]

    def sac_critic():                                                            # B = 1, one critic
        q = _cuda([0.3], grad=True)
        loss, stats = tg.sac_critic_loss([q], [_cuda([0.5])], _cuda([-1.2]), _cuda([0.7]), _cuda([0.0]), 0.99, ent_coef=0.2)
        loss.backward()
        return [stats, q.grad]

    def stem():                                                                  # 1 x 1 x 8 x 8: one output pixel per channel
        r = rng()
        x = _cuda(r.integers(0, 256, (1, 1, 8, 8)), np.uint8)
        w, b = _cuda(r.standard_normal((32, 1, 8, 8)) * 0.1, grad=True), _cuda(r.standard_normal(32) * 0.1, grad=True)
        y = tg.conv_stem(x, w, b)
        y.sum().backward()
        return [y, w.grad, b.grad]

    def tower():                                                                 # B = 1, one 1 -> 1 layer
        x, w, b = _cuda([[0.5]], grad=True), _cuda([[-0.7]], grad=True), _cuda([0.2], grad=True)
        y, = tg.mlp_towers(x, [[(w, b, "tanh")]])
        y.sum().backward()
        return [y, x.grad, w.grad, b.grad]

    def head():                                                                  # N = 1
        h = tg.DeviceDiagGaussian(act, seed=3, num_envs=1, device="cuda")
        h.counter = 5
        return [t.clone() for t in h.sample(_cuda([[0.1]]), _cuda([-0.3]))] + [h.noise.clone()]

    def rollout():                                                               # T = 1, N = 1
        buf = tg.DeviceRolloutBuffer(1, obs_space, act, "cuda", gae_lambda=0.9, gamma=0.95, n_envs=1)
        buf.add(obs(1), _cuda([[0.2]]), _cuda([0.5]), _cuda([1.0]), _cuda([0.3]), _cuda([-0.8]))
        buf.compute_returns_and_advantage(_cuda([0.6]), _cuda([0], np.uint8))
        return list(buf.observations.values()) + [buf.actions, buf.rewards, buf.episode_starts, buf.values, buf.log_probs, buf.advantages,
                                                   buf.returns]

    def replay():                                                                # one slot; sample(1): the draw, the image key, the vector key
        buf = tg.DeviceReplayBuffer(1, obs_space, act, "cuda", n_envs=1, seed=5)
        buf.counter = 9
        buf.add(obs(2), obs(3), _cuda([[0.2]]), _cuda([0.5]), _cuda([1], np.uint8))
        s = buf.sample(1)
        return list(s.observations.values()) + list(s.next_observations.values()) + [s.actions, s.dones, s.rewards]

    return [("ppo_loss", ppo), ("sac_critic_loss", sac_critic), ("conv_stem", stem), ("mlp_towers", tower), ("DeviceDiagGaussian.sample", head),
            ("DeviceRolloutBuffer", rollout), ("DeviceReplayBuffer", replay)]


def _vecnorm_step(tg, venv):
    """reset + one step of a DeviceVecNormalize over `venv` on the current stream: what it handed out and its statistics."""
    vn = tg.DeviceVecNormalize(venv, gamma=0.95)
    vn.reset()
    obs, rewards, _, _ = vn.step(np.array([[0.1, -0.2], [-0.05, 0.25]], np.float32))
    return [obs["oracle"].clone(), torch.from_numpy(rewards), vn.returns.clone(), vn.ret_rms.block.clone(), vn.obs_rms["oracle"].block.clone()]


def test_every_wrapper_family_launches_on_the_current_stream():
    """One wrapper of each family under torch.cuda.stream(side), then side.synchronize() ONLY: every result equals, bit for bit, the same call
    made on the default stream from the same values, seeds and counters.  The default stream is kept busy meanwhile and the results are read
    on the side stream, so a wrapper that launched on another stream than torch's current one is read before it ran."""
    import tactile_gym_amd as tg
    modes = dict(EDGE, observation_mode="oracle")
    envs = [tg.make_vec("edge_follow-v0", num_envs=2, max_steps=6, image_size=[64, 64], env_modes=modes, seed=4, obs_mode="torch") for _ in range(2)]
    try:
        calls = _family_calls(tg)
        want = {name: call() for name, call in calls}
        want["DeviceVecNormalize.step"] = _vecnorm_step(tg, envs[0])
        torch.cuda.synchronize()
        want = {name: [t.detach().cpu().numpy() for t in ts] for name, ts in want.items()}
        busy, out = torch.rand((8192, 8192), device="cuda"), torch.empty((8192, 8192), device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        for _ in range(24):                                                      # the default stream is busy for the whole side section: a launch
            torch.mm(busy, busy, out=out)                                        # that went there by mistake has not run when its result is read
        with torch.cuda.stream(side):
            got = {name: call() for name, call in calls}
            got["DeviceVecNormalize.step"] = _vecnorm_step(tg, envs[1])
            side.synchronize()
            got = {name: [t.detach().cpu().numpy() for t in ts] for name, ts in got.items()}     # read on the side stream as well
        for name, ts in got.items():
            assert len(ts) == len(want[name]) and len(ts) >= 2, name
            for i, (g, w) in enumerate(zip(ts, want[name])):
                assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (name, i, g, w)
                assert np.isfinite(g.astype(np.float64)).all(), (name, i, g)
    finally:
        torch.cuda.synchronize()
        for v in envs:
            v.close()
