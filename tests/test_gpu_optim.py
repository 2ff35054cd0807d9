"""tg.DeviceAdam on the GPU against torch.optim.Adam behind clip_grad_norm_ on the same gradients: the parameters of tg.ActorCriticHeads and a
log_ent_coef-style scalar within twice torch's own distance from the float64 Adam, the state_dict handed to torch and back in the middle of
a run, two param groups clipped together, and tg.train.ppo_train over two minibatches."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LR, B1, B2, EPS, CLIP = 3e-4, 0.9, 0.999, 1e-5, 0.5


def _models(seed=0):
    """(ours, theirs): twice the same parameters - ActorCriticHeads at feature width 8 and a scalar."""
    import tactile_gym_amd as tg
    torch.manual_seed(seed)
    heads = tg.ActorCriticHeads(8, 2, dict(pi=[64, 33], vf=[64, 33]), log_std_init=-1.0).cuda()
    ours = list(heads.parameters()) + [torch.nn.Parameter(torch.zeros(1, device="cuda"))]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    return ours, theirs


def _grads(params, rng, scale):
    return [(rng.standard_normal(tuple(p.shape)) * scale).astype(np.float32) for p in params]


def _give(params, grads):
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).cuda()


def _host(params):
    return [p.detach().cpu().numpy() for p in params]


def _scales(n):
    """Per-step gradient scales that put the norm (about scale sqrt(elements)) on both sides of 0.5."""
    return [1e-4, 1.0, 3e-3, 30.0, 1e-2, 0.3, 1e-3, 5.0][:n]


def test_device_adam_stays_as_close_to_float64_adam_as_torch_does():
    import tactile_gym_amd as tg
    ours, theirs = _models()
    n_elem = sum(p.numel() for p in ours)
    opt = tg.DeviceAdam(ours, lr=LR, eps=EPS)
    adam = torch.optim.Adam(theirs, lr=LR, eps=EPS)
    P = [x.astype(np.float64) for x in _host(ours)]
    M, V = [np.zeros_like(x) for x in P], [np.zeros_like(x) for x in P]
    rng = np.random.default_rng(1)
    coefs = []
    for step, scale in enumerate(_scales(8), start=1):
        grads = _grads(ours, rng, scale)
        _give(ours, grads), _give(theirs, grads)
        kept = [p.grad.clone() for p in ours]
        opt.step(max_grad_norm=CLIP)
        want_norm = torch.nn.utils.clip_grad_norm_(theirs, CLIP)
        adam.step()
        P, M, V, total = ref.step_f64(P, grads, M, V, [step] * len(P), LR, B1, B2, EPS, 0.0, CLIP)
        coefs.append(min(1.0, CLIP / (total + 1e-6)))
        assert all(torch.equal(p.grad, k) for p, k in zip(ours, kept))         # p.grad is left unscaled
        assert opt.total_norm.dtype == torch.float32 and opt.total_norm.is_cuda and opt.total_norm.dim() == 0
        assert abs(float(opt.total_norm) - total) <= float(np.spacing(np.float32(total)))      # within 1 float32 ulp of the float64 norm
        assert abs(float(want_norm) - total) <= 1e-5 * total
    assert min(coefs) < 0.01 and max(coefs) == 1.0 and n_elem > 5000           # clipped hard and not clipped; 15 tensors, one chunk each
    err_ours = max(np.abs(a - b).max() for a, b in zip(_host(ours), P))
    err_torch = max(np.abs(a - b).max() for a, b in zip(_host(theirs), P))
    moved = max(np.abs(a - b).max() for a, b in zip(_host(ours), _host(_models()[0])))
    print(f"max |DeviceAdam - f64| {err_ours:.3g}, max |torch - f64| {err_torch:.3g}, the parameters moved by up to {moved:.3g}")
    assert moved > 5 * LR and err_torch > 0 and err_ours <= 2 * err_torch
    for p in ours:
        st = opt.state[p]
        assert float(st["step"]) == 8 and st["step"].device.type == "cpu" and st["exp_avg"].is_cuda and st["exp_avg_sq"].shape == p.shape


def test_state_dict_goes_to_torch_and_back_in_the_middle_of_a_run():
    import tactile_gym_amd as tg
    ours, theirs = _models(1)
    rng = np.random.default_rng(2)
    steps = [_grads(ours, rng, s) for s in _scales(6)]
    straight = tg.DeviceAdam(theirs, lr=LR, eps=EPS)                            # the run without a hand-over
    for grads in steps:
        _give(theirs, grads)
        straight.step(max_grad_norm=CLIP)
    first = tg.DeviceAdam(ours, lr=LR, eps=EPS)
    for grads in steps[:2]:
        _give(ours, grads)
        first.step(max_grad_norm=CLIP)
    adam = torch.optim.Adam(ours, lr=1.0)
    adam.load_state_dict(copy.deepcopy(first.state_dict()))                    # DeviceAdam -> torch: lr, eps and the state come along
    assert adam.param_groups[0]["lr"] == LR and adam.param_groups[0]["eps"] == EPS
    for grads in steps[2:4]:
        _give(ours, grads)
        torch.nn.utils.clip_grad_norm_(ours, CLIP)
        adam.step()
    second = tg.DeviceAdam(ours, lr=1.0)
    second.load_state_dict(copy.deepcopy(adam.state_dict()))                   # torch -> DeviceAdam
    for p in ours:
        st = second.state[p]
        assert float(st["step"]) == 4 and st["step"].device.type == "cpu" and st["exp_avg"].is_cuda
    for grads in steps[4:]:
        _give(ours, grads)
        second.step(max_grad_norm=CLIP)
    assert all(float(second.state[p]["step"]) == 6 for p in ours)
    # two of the six steps were torch's: the same run up to its rounding, 6 steps of at most lr each
    for a, b in zip(_host(ours), _host(theirs)):
        assert np.abs(a - b).max() <= 1e-3 * 6 * LR


def test_two_param_groups_with_different_lr_are_clipped_together():
    import tactile_gym_amd as tg
    ours, theirs = _models(2)
    k = 4
    opt = tg.DeviceAdam([dict(params=ours[:k]), dict(params=ours[k:], lr=1e-2)], lr=LR, eps=EPS, max_grad_norm=CLIP)
    adam = torch.optim.Adam([dict(params=theirs[:k]), dict(params=theirs[k:], lr=1e-2)], lr=LR, eps=EPS)
    before = _host(ours)
    rng = np.random.default_rng(3)
    z = [np.zeros(tuple(p.shape), np.float32) for p in ours]
    for step, scale in enumerate((1.0, 1e-3), start=1):
        grads = _grads(ours, rng, scale)
        _give(ours, grads), _give(theirs, grads)
        state = (_host(ours), z, z) if step == 1 else (_host(ours), [opt.state[p]["exp_avg"].cpu().numpy() for p in ours],
                                                       [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ours])
        opt.step()                                                             # the constructor's max_grad_norm
        want_norm = torch.nn.utils.clip_grad_norm_(theirs, CLIP)               # ONE norm over both groups
        adam.step()
        P, _, _, total = ref.step_device_order(*state[:1], grads, *state[1:], [step] * len(ours), [LR] * k + [1e-2] * (len(ours) - k), B1, B2, EPS,
                                               0.0, CLIP)
        assert float(opt.total_norm) == float(total) and abs(float(want_norm) - float(total)) <= 1e-5 * float(total)
        for a, b in zip(_host(ours), P):
            assert np.array_equal(a, b)                                        # the restatement's bits, each group at its own lr
    for a, b, c in zip(_host(ours), _host(theirs), before):
        assert np.abs(a - b).max() <= 1e-3 * 2 * 1e-2 and np.abs(a - c).max() > 0
    assert np.abs(_host(ours)[-1] - before[-1]).max() > 5e-3                   # the scalar is in the second group: steps of 1e-2


def test_ppo_train_runs_with_device_adam_and_moves_the_parameters():
    import tactile_gym_amd as tg
    from tactile_gym_amd.rollout import RolloutBufferSamples
    torch.manual_seed(3)
    heads = tg.ActorCriticHeads(8, 2, dict(pi=[64, 33], vf=[64, 33]), log_std_init=-1.0).cuda()
    rows = lambda *shape: torch.randn(*shape, device="cuda")   # noqa: E731
    batches = [RolloutBufferSamples(rows(8, 8), 0.1 * rows(8, 2), rows(8), -1.0 + 0.1 * rows(8), rows(8), rows(8)) for _ in range(2)]

    class Buf:
        def get(self, batch_size, augment=None, out_dtype=None):
            assert batch_size == 8
            return iter(batches)

    opt = tg.DeviceAdam(heads.parameters(), lr=LR, eps=EPS)
    before = [p.detach().clone() for p in heads.parameters()]
    stats = tg.train.ppo_train(heads, opt, Buf(), 1, 8, 0.2, None, 0.0, 0.5, CLIP, None)
    assert stats.shape == (8,) and bool(torch.isfinite(stats).all())
    assert all(not torch.equal(a, b) for a, b in zip(before, heads.parameters()))
    assert all(float(opt.state[p]["step"]) == 2 for p in heads.parameters()) and float(opt.total_norm) > 0
    assert all(bool(torch.isfinite(p).all()) for p in heads.parameters())
