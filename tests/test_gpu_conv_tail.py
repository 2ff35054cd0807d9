"""tactile_gym_amd.torch_layers' device tail on the device: conv_relu and linear_relu under autograd against torch's float64 autograd on the
host, what a no_grad forward keeps, the dx launch that a frozen input spares, gradients that reach the stem through conv2's dx,
tg.NatureCNN(device_tail=True) against its own CPU path, and the property the tail exists for: a minibatch row's FEATURES, mean and value have
the bits that the same row produced inside the collection batch, so PPO's first-epoch ratio is exactly 1."""
import gc
import os
import sys
import weakref

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_tail_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

MODES = dict(movement_mode="xy", control_mode="TCP_velocity_control", noise_mode="rand_height", observation_mode="tactile", reward_mode="dense",
             arm_type="ur5", tactile_sensor_name="tactip")
f32 = np.float32


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class _Space:
    def __init__(self, shape):
        self.shape, self.dtype = tuple(shape), np.uint8


# conv2 of the 36 x 36 observation, the stride-3 layer with three channel tiles, a linear layer in both input forms, and two of
# conv_tail_ref.PATH_CASES: Cout = 128 (the forward's four-channel-tile layout) and Cin = 40, K = 360 (short last chunk, partly valid dx tile)
GRAD_CASES = [((32, 8, 8, 64, 4, 4, 2, 3), "conv"), ((4, 10, 13, 96, 3, 2, 3, 5), "conv"), ((64, 3, 3, 64, 3, 3, 1, 5), "linear4"),
              ((64, 3, 3, 64, 3, 3, 1, 5), "linear2"), ((32, 8, 8, 128, 4, 4, 2, 3), "conv"), ((40, 6, 6, 32, 3, 3, 1, 5), "conv")]


@pytest.mark.parametrize("case,form", GRAD_CASES, ids=[ref.case_id(c) + "-" + f for c, f in GRAD_CASES])
def test_gradients_against_float64_autograd(case, form):
    import tactile_gym_amd as tg
    Cin, H, W, Cout, KH, KW, stride, B = case
    rng = np.random.default_rng(1)
    x, w, b, _, dy = ref.random_case(rng, case)
    x = (x - 0.5).astype(f32)                                                 # both signs: about half of the outputs are clamped
    xd = torch.from_numpy(x).cuda().requires_grad_()
    wd, bd = torch.from_numpy(w).cuda().requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
    if form == "conv":
        y = tg.conv_relu(xd, wd, bd, stride)
    elif form == "linear4":
        y = tg.linear_relu(xd, wd.view(Cout, -1), bd).view(B, Cout, 1, 1)
    else:
        y = tg.linear_relu(xd.view(B, -1), wd.view(Cout, -1), bd).view(B, Cout, 1, 1)
    assert y.requires_grad and y.shape == dy.shape
    y.backward(torch.from_numpy(dy).cuda())
    # torch's float64 autograd on the host, masked by ITS y > 0; the device masks by its own float32 y: elements whose exact value lies within
    # the forward bound of zero may be masked differently, and the bounds below are widened by exactly their |g x|, |g| and |g w|
    x64 = torch.from_numpy(x).double().requires_grad_()
    w64, b64 = torch.from_numpy(w).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    y64 = F.relu(F.conv2d(x64, w64, b64, stride=stride))
    y64.backward(torch.from_numpy(dy).double())
    want, fwd_bound = ref.forward(x, w, b, stride)
    y_dev = y.detach().cpu().numpy()
    assert (np.abs(y_dev - want) <= fwd_bound).all() and (y_dev > 0).any() and (y_dev == 0).any()
    flipped = (y_dev > 0) != (want > 0)
    assert not flipped[want > fwd_bound].any()                             # only elements within the bound of zero can differ in the mask
    r = ref.backward(x, w, y_dev, dy, stride)
    got = dict(dw=wd.grad.cpu().numpy(), db=bd.grad.cpu().numpy(), dx=xd.grad.cpu().numpy())
    for k in ("dw", "db", "dx"):
        assert (np.abs(got[k] - r[k]) <= r[k + "_bound"]).all(), k
    rf = ref.backward(x, w, flipped.astype(f32), dy, stride)               # (n + 4) 2^-23 sum |g .| over the flipped elements
    OH, OW = ref.out_hw(H, W, KH, KW, stride)
    M, J = B * OH * OW, Cout * KH * KW
    for k, n, g64 in (("dw", M, w64.grad), ("db", M, b64.grad), ("dx", J, x64.grad)):
        slack = rf[k + "_bound"] / ((n + 4) * 2.0 ** -23)
        assert (np.abs(got[k] - g64.numpy()) <= r[k + "_bound"] + slack).all(), k


def test_linear_relu_gives_the_same_bytes_for_both_input_forms():
    """[B, 64, 3, 3] is the convolution (64, 3, 3); the same data as [B, 576] is split by _split_k into (3, 16, 12).  The chain is defined by k
    alone, so y, dx, dweight and dbias have the same bytes."""
    import tactile_gym_amd as tg
    from tactile_gym_amd import torch_layers
    assert torch_layers._split_k(576) == (3, 16, 12)
    B = 5
    rng = np.random.default_rng(8)
    x, w, b, _, dy = ref.random_case(rng, (64, 3, 3, 64, 3, 3, 1, B))
    x = (x - 0.5).astype(f32)
    out = []
    for shape in ((B, 64, 3, 3), (B, 576)):
        xd = torch.from_numpy(x).cuda().view(shape).requires_grad_()
        wd, bd = torch.from_numpy(w).cuda().view(64, 576).requires_grad_(), torch.from_numpy(b).cuda().requires_grad_()
        y = tg.linear_relu(xd, wd, bd)
        assert y.shape == (B, 64)
        y.backward(torch.from_numpy(dy).cuda().view(B, 64))
        assert xd.grad.shape == shape
        out.append((y.detach(), xd.grad.view(B, 576), wd.grad, bd.grad))
    assert bool((out[0][0] > 0).any()) and bool((out[0][0] == 0).any()) and float(out[0][1].abs().max()) > 0
    for a, c, name in zip(out[0], out[1], ("y", "dx", "dweight", "dbias")):
        assert _same_bytes(a, c), name


def test_a_no_grad_forward_keeps_nothing():
    import tactile_gym_amd as tg
    conv = tg.ConvRelu(32, 64, 4, 2).cuda()

    def held(make_y):
        x = torch.randn(4, 32, 8, 8, device="cuda")
        y = make_y(x)
        rx = weakref.ref(x)
        del x
        gc.collect()
        return y, rx() is not None
    with torch.no_grad():
        y, kept = held(conv)
    assert y.grad_fn is None and not y.requires_grad and not kept         # nothing reachable from the output holds the input
    for p in conv.parameters():
        p.requires_grad_(False)
    y, kept = held(conv)                                                  # grad mode on, everything frozen: nothing to differentiate either
    assert y.grad_fn is None and not kept
    y, kept = held(lambda x: conv(x.requires_grad_()))                    # frozen parameters, but the input wants its gradient
    assert y.grad_fn is not None and kept
    for p in conv.parameters():
        p.requires_grad_(True)
    y, kept = held(conv)
    assert y.grad_fn is not None and kept                                 # and with a gradient wanted the input IS kept


def test_an_input_without_gradient_launches_no_dx_kernel(monkeypatch):
    import tactile_gym_amd as tg
    from tactile_gym_amd import torch_layers
    calls = []
    real = torch_layers.launch

    def spy(entry, dev, *args):
        calls.append((entry, args))
        return real(entry, dev, *args)
    monkeypatch.setattr(torch_layers, "launch", spy)
    conv = tg.ConvRelu(32, 64, 4, 2).cuda()
    x = torch.randn(3, 32, 8, 8, device="cuda")
    conv(x).sum().backward()
    bwd = [a for e, a in calls if e == "tg_conv_relu_bwd"]
    assert len(bwd) == 1 and bwd[0][14].value is None and x.grad is None   # dx_dev = NULL: the library launches no dx kernel
    dw = conv.weight.grad.clone()
    conv.weight.grad = None
    x.requires_grad_()
    conv(x).sum().backward()
    bwd = [a for e, a in calls if e == "tg_conv_relu_bwd"]
    assert len(bwd) == 2 and bwd[1][14].value is not None and x.grad is not None and x.grad.shape == x.shape
    assert _same_bytes(conv.weight.grad, dw)                              # dweight does not depend on whether dx is wanted


def _double_model(m, channels_first):
    """NatureCNN's meaning in float64 on the host, from the module's parameters (as leaves that collect gradients)."""
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in m.state_dict().items()}

    def run(x):
        x = x.cpu().double() / 255.0
        h = F.relu(F.conv2d(x if channels_first else x.permute(0, 3, 1, 2), p["cnn.0.weight"], p["cnn.0.bias"], stride=4))
        h = F.relu(F.conv2d(h, p["cnn.2.weight"], p["cnn.2.bias"], stride=2))
        h = F.relu(F.conv2d(h, p["cnn.4.weight"], p["cnn.4.bias"], stride=1))
        return F.relu(F.linear(h.flatten(1), p["linear.0.weight"], p["linear.0.bias"]))
    return p, run


def test_gradients_reach_the_stem_through_conv2s_dx():
    """Every parameter's gradient of the whole device module against the float64 host model.  The criterion is normwise: the module is four
    layers deep, forward and backward, and each of the eight passes adds at most (n + 4) 2^-23 relative to its sums of absolute terms with
    n <= 1024 here (the linear layer's K at 64 x 64), so 8 (1024 + 4) 2^-23 of the gradient's largest entry bounds the error to first order."""
    import tactile_gym_amd as tg
    torch.manual_seed(2)
    m = tg.NatureCNN(_Space((2, 64, 64)), features_dim=32, device_tail=True).cuda()
    x = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (5, 2, 64, 64), dtype=np.uint8))
    dy = torch.from_numpy(np.random.default_rng(4).standard_normal((5, 32)).astype(f32))
    m(x.cuda()).backward(dy.cuda())
    p64, run = _double_model(m, True)
    run(x).backward(dy.double())
    rel = 8 * (1024 + 4) * 2.0 ** -23
    for name, param in m.named_parameters():
        got, want = param.grad.cpu().double(), p64[name].grad
        assert float(want.abs().max()) > 0, name
        err = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{name}: largest error / largest entry = {err:.3g} (allowed {rel:.3g})")
        assert err <= rel, (name, err)


@pytest.mark.parametrize("channels_first", [True, False])
def test_nature_cnn_device_tail_on_the_device_equals_its_cpu_path(channels_first):
    import tactile_gym_amd as tg

    class Space:
        shape = (2, 64, 64) if channels_first else (64, 64, 2)
    torch.manual_seed(2)
    cpu = tg.NatureCNN(Space(), features_dim=32, channels_first=channels_first, device_tail=True)
    dev = tg.NatureCNN(Space(), features_dim=32, channels_first=channels_first, device_tail=True).cuda()
    dev.load_state_dict(cpu.state_dict())
    x = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (5,) + Space.shape, dtype=np.uint8))
    with torch.no_grad():
        feats_cpu, feats_dev = cpu(x), dev(x.cuda())
        via_sequentials = dev.linear(dev.cnn(x.cuda()))
    assert feats_dev.shape == (5, 32) and torch.allclose(feats_dev.cpu(), feats_cpu, rtol=1e-4, atol=1e-5)
    assert float(feats_dev.abs().max()) > 0 and _same_bytes(via_sequentials, feats_dev)
    torch.manual_seed(4)
    plain = tg.NatureCNN(Space(), features_dim=32, channels_first=channels_first).cuda()      # the torch tail loads the checkpoint, too
    plain.load_state_dict(dev.state_dict(), strict=True)
    with torch.no_grad():
        assert torch.allclose(plain(x.cuda()), feats_dev, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("device_tail", [True, False])
def test_minibatch_rows_reproduce_the_collection_batchs_features_means_and_values(device_tail):
    import tactile_gym_amd as tg
    from tactile_gym_amd.collect import collect_rollouts
    N, T = 8, 2
    venv = tg.make_vec("edge_follow-v0", num_envs=N, max_steps=5, image_size=[128, 128], env_modes=MODES, seed=4, obs_mode="torch", frame_stack=2)
    try:
        space = venv.observation_space.spaces["tactile"]
        torch.manual_seed(5)
        extractor = tg.NatureCNN(space, features_dim=32, device_tail=device_tail).cuda()
        heads = tg.ActorCriticHeads(32, 2, dict(pi=[64, 33], vf=[64, 33]), log_std_init=-1.0).cuda()
        with torch.no_grad():                                                 # SB3's action_net gain of 0.01 would leave every mean near 0
            heads.action_net.weight.mul_(50.0)
        seen = []

        def policy(obs):
            feats = extractor(obs["tactile"])
            mean, log_std, values = heads(feats)
            seen.append((feats.detach().clone(), mean.detach().clone(), values.detach().clone()))
            return mean, log_std, values
        buf = tg.DeviceRolloutBuffer.for_env(venv, T, gamma=0.95, gae_lambda=0.9)
        head = tg.DeviceDiagGaussian.for_env(venv, seed=7)
        obs = venv.reset()
        assert obs["tactile"].dtype == torch.uint8 and obs["tactile"].is_cuda
        collect_rollouts(venv, policy, buf, head, T, obs, torch.ones(N, dtype=torch.uint8, device="cuda"))
        assert buf.full and len(seen) == T + 1 and seen[0][0].shape == (N, 32)
        assert float(seen[0][0].abs().max()) > 0 and not _same_bytes(seen[0][0], seen[1][0])
        collected = list(seen)
        order = torch.tensor([5, 0, 15, 10, 3, 12, 9, 6, 1, 14, 7, 8, 11, 2, 13, 4], dtype=torch.int64, device="cuda")   # i = n T + t
        kw = dict(clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)
        rows, same = 0, True
        with torch.no_grad():
            for k, batch in enumerate(buf.get(batch_size=4, out_dtype=torch.uint8, indices=order)):
                mean, log_std, values = policy(batch.observations)
                feats = seen[-1][0]
                idx = order[4 * k:4 * k + 4].tolist()
                want = [torch.stack([collected[i % T][j][i // T] for i in idx]) for j in range(3)]
                _, stats = tg.ppo_loss(mean, log_std, values, batch.actions, batch.old_log_prob, batch.advantages, batch.returns,
                                       old_values=batch.old_values, **kw)
                ok = (_same_bytes(feats, want[0]) and _same_bytes(mean, want[1]) and _same_bytes(values, want[2])
                      and float(stats[4]) == 0.0 and float(stats[5]) == 0.0)
                if device_tail:                                           # 4 rows in a minibatch, 8 rows at collection: the same bits,
                    assert ok, (k, stats)                                 # approx_kl = clip_fraction = 0: the ratio is exactly 1
                same = same and ok
                rows += 4
        assert rows == N * T
        print(f"device_tail={device_tail}: minibatch rows reproduce the collection bits: {same}")    # with the torch tail: not asserted either way
    finally:
        venv.close()
