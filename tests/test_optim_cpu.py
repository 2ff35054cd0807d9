"""tactile_gym_amd.optim without a GPU: the restatement (tests/optim_ref.py) and torch's CPU Adam against the float64 Adam, the norm against the
float64 norm, DeviceAdam on CPU tensors with its two C calls replaced by the restatement (the chunk prefix, skipped tensors, the state_dict
hand-over to and from torch.optim.Adam, every refusal, a changed lr), the C ABI entries and the kernels' resources."""
import copy
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import build_units  # noqa: E402
import optim_ref as ref  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_optim_adam"]                 # at import: the whole file needs the feature
torch = pytest.importorskip("torch")
f32 = np.float32
LR, B1, B2 = 3e-4, 0.9, 0.999


# ---------------------------------------------------------------------------------------------------------------- the reference against torch
@pytest.mark.parametrize("n", [7, 4099])
@pytest.mark.parametrize("eps", [1e-5, 1e-8])
def test_reference_is_as_close_to_float64_adam_as_torch_is(eps, n):
    """64 steps, parameters N(0, 1), each step's grad N(0, 1) 10^k with k drawn from -6 .. 2: max |ref - f64| <= 2 max |torch - f64|."""
    rng = np.random.default_rng(1000 + n)
    p0 = rng.standard_normal(n).astype(f32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=LR, eps=eps, foreach=False)
    rp, rm, rv = [p0.copy()], [np.zeros(n, f32)], [np.zeros(n, f32)]
    dp, dm, dv = [p0.astype(np.float64)], [np.zeros(n)], [np.zeros(n)]
    for step in range(1, 65):
        g = (rng.standard_normal(n) * 10.0 ** int(rng.integers(-6, 3))).astype(f32)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        rp, rm, rv, _ = ref.step_device_order(rp, [g], rm, rv, [step], LR, B1, B2, eps)
        dp, dm, dv, _ = ref.step_f64(dp, [g], dm, dv, [step], LR, B1, B2, eps)
    err_ref = np.abs(rp[0] - dp[0]).max()
    err_torch = np.abs(tp.detach().numpy() - dp[0]).max()
    print(f"eps {eps:g}, n {n}: max |ref - f64| {err_ref:.3g}, max |torch - f64| {err_torch:.3g}")
    assert err_torch > 0 and err_ref <= 2 * err_torch


# ---------------------------------------------------------------------------------------------------------------- the norm
@pytest.mark.parametrize("sizes,scale", [((1,), 1.0), ((7, 4099), 1e-3), ((4096, 4097, 3, 64, 12289), 30.0), ((100000, 5), 1e-20), ((65, 1), 1e15)])
def test_total_norm_is_within_one_ulp_of_the_float64_norm(sizes, scale):
    """The double sum over fewer than 2^24 terms carries a relative error far below 2^-24, so rounding its root once to float32 lands on one of
    the two float32 neighbours of the exact norm."""
    rng = np.random.default_rng(sum(sizes))
    grads = [(rng.standard_normal(n) * scale).astype(f32) for n in sizes]
    partials = ref.partial_sums(grads)
    assert partials.dtype == np.float64 and partials.shape == (ref.chunk_prefix(sizes)[-1],)
    total = ref.total_norm(partials)
    exact = ref.norm_f64(grads)
    assert total.dtype == f32 and abs(float(total) - exact) <= float(np.spacing(total))
    assert ref.clip_coef(total, 0.5) == (f32(1) if f32(0.5) / (total + f32(1e-6)) > 1 else f32(0.5) / (total + f32(1e-6)))


def test_clip_coefficient_on_both_sides_of_one_and_not_finite():
    assert ref.clip_coef(f32(0.25), 0.5) == f32(1) and ref.clip_coef(f32(2.0), 0.5) == f32(0.5) / (f32(2.0) + f32(1e-6))
    assert ref.clip_coef(f32(np.inf), 0.5) == 0 and np.isnan(ref.clip_coef(f32(np.nan), 0.5))
    g = [np.array([1.0, np.inf, 2.0], f32), np.ones(5, f32)]
    p, m, v, total = ref.step_device_order([np.zeros(3, f32), np.zeros(5, f32)], g, [np.zeros(3, f32), np.zeros(5, f32)],
                                           [np.zeros(3, f32), np.zeros(5, f32)], [1, 1], LR, B1, B2, 1e-8, max_norm=0.5)
    assert np.isinf(total) and np.isnan(p[0][1]) and np.isfinite(p[0][[0, 2]]).all() and np.isfinite(p[1]).all()     # inf * 0 where the inf stood
    g[1][2] = np.nan
    p, m, v, total = ref.step_device_order([np.zeros(3, f32), np.zeros(5, f32)], g, [np.zeros(3, f32), np.zeros(5, f32)],
                                           [np.zeros(3, f32), np.zeros(5, f32)], [1, 1], LR, B1, B2, 1e-8, max_norm=0.5)
    assert np.isnan(total) and all(np.isnan(x).all() for x in p + m + v)                                             # a NaN norm reaches everything


# ---------------------------------------------------------------------------------------------------------------- DeviceAdam on the host
def _stubbed(params, **kw):
    """A DeviceAdam on CPU tensors whose two C calls are the restatement on the tensors' memory."""
    from tactile_gym_amd.optim import DeviceAdam

    class Stubbed(DeviceAdam):
        def _is_device(self, t):
            return True

        def _c_sumsq(self, dev, grads, counts):
            assert counts == [g.numel() for g in grads]
            self.calls.append(("sumsq", len(grads)))
            part = ref.partial_sums([g.numpy() for g in grads])
            assert part.size <= self._partials.numel()
            self._partials.numpy()[:part.size] = part

        def _c_adam(self, dev, hyper, rows, max_norm, n_partials):
            beta1, beta2, eps, wd = hyper
            self.calls.append(("adam", len(rows), hyper, max_norm, n_partials, [(float(f32(r[4])), float(f32(r[5]))) for r in rows]))
            coef = None
            if max_norm is not None:
                total = ref.total_norm(self._partials.numpy()[:n_partials])
                self.total_norm.numpy()[...] = total
                coef = ref.clip_coef(total, max_norm)
            for p, g, m, v, ss, bc2s in rows:
                out = ref.adam_device_order(p.numpy(), g.numpy(), m.numpy(), v.numpy(), ss, bc2s, beta1, beta2, eps, wd, coef)
                for t, new in zip((p, m, v), out):
                    t.numpy()[...] = new

    opt = Stubbed.__new__(Stubbed)
    opt.calls = []
    opt.__init__(params, **kw)
    return opt


def _params(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(f32))) for s in shapes]


def _set_grads(params, seed, skip=()):
    rng = np.random.default_rng(seed)
    for i, p in enumerate(params):
        g = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(f32))
        p.grad = None if i in skip else g


def test_chunk_prefix():
    from tactile_gym_amd.optim import chunk_prefix
    import tactile_gym_amd as tg
    assert tg.optim.chunk_prefix is chunk_prefix and tg.DeviceAdam is tg.optim.DeviceAdam
    assert (_capi.OPTIM_CHUNK, _capi.OPTIM_MAX_TENSORS) == (ref.CHUNK, ref.MAX_TENSORS) == (4096, 64)
    counts = [1, 4095, 4096, 4097, 8192, 8195, 3]
    assert chunk_prefix(counts) == ref.chunk_prefix(counts) == [0, 1, 2, 3, 5, 7, 10, 11]
    assert chunk_prefix([]) == [0]
    with pytest.raises(ValueError, match="no chunk"):
        chunk_prefix([5, 0])


def test_step_follows_the_restatement_and_skips_tensors_without_a_grad():
    shapes = [(3, 5), (4097,), (), (2, 2)]
    params = _params(shapes)
    opt = _stubbed(params, lr=LR, eps=1e-5, weight_decay=0.01)
    want = dict(p=[p.detach().numpy().copy() for p in params], m=[np.zeros(s, f32) for s in shapes], v=[np.zeros(s, f32) for s in shapes],
                t=[0] * len(shapes))
    assert opt.total_norm is None and opt.state_dict()["state"] == {}
    for it, (skip, max_norm) in enumerate([((), None), ((1,), 0.5), ((1, 3), 100.0), ((), 0.5)]):
        _set_grads(params, 10 + it, skip)
        grads_before = [None if p.grad is None else p.grad.clone() for p in params]
        opt.step(max_grad_norm=max_norm)
        live = [i for i in range(len(shapes)) if i not in skip]
        for i in live:
            want["t"][i] += 1
        P, M, V, total = ref.step_device_order([want["p"][i] for i in live], [params[i].grad.numpy() for i in live], [want["m"][i] for i in live],
                                               [want["v"][i] for i in live], [want["t"][i] for i in live], LR, B1, B2, 1e-5, 0.01, max_norm)
        for k, i in enumerate(live):
            want["p"][i], want["m"][i], want["v"][i] = P[k], M[k], V[k]
        for i, p in enumerate(params):
            st = opt.state[p]
            assert np.array_equal(p.detach().numpy(), want["p"][i]), (it, i)
            assert np.array_equal(st["exp_avg"].numpy(), want["m"][i]) and np.array_equal(st["exp_avg_sq"].numpy(), want["v"][i])
            assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0
            assert float(st["step"]) == want["t"][i]                           # a skipped tensor's step did not advance
            assert p.grad is None or torch.equal(p.grad, grads_before[i])      # p.grad is left unscaled
        if max_norm is not None:
            assert opt.total_norm.dtype == torch.float32 and opt.total_norm.dim() == 0 and float(opt.total_norm) == float(total)
    assert [c[0] for c in opt.calls] == ["adam", "sumsq", "adam", "sumsq", "adam", "sumsq", "adam"]
    assert opt.calls[2][4] == ref.chunk_prefix([15, 1, 4])[-1] and opt.calls[-1][4] == 1 + 2 + 1 + 1
    # bias corrections are per tensor: in the last step tensor 1 is at step 2, tensor 3 at step 3, the others at 4
    assert opt.calls[-1][5] == [tuple(float(x) for x in ref.corrections(LR, B1, B2, t)) for t in (4, 2, 4, 3)]
    opt.zero_grad()
    assert all(p.grad is None for p in params)                                 # torch's zero_grad, set_to_none=True
    before = [p.detach().clone() for p in params]
    n_calls = len(opt.calls)
    opt.step(max_grad_norm=0.5)                                                # no grad anywhere: no launch, nothing moves
    assert len(opt.calls) == n_calls and all(torch.equal(a, b) for a, b in zip(before, params))


def test_constructor_max_grad_norm_and_param_groups_share_the_clip():
    params = _params([(5,), (7,), (3,)])
    opt = _stubbed([dict(params=params[:2]), dict(params=params[2:], lr=1e-2)], lr=LR, max_grad_norm=0.5)
    _set_grads(params, 3)
    p0 = [p.detach().numpy().copy() for p in params]
    opt.step()
    assert [c[0] for c in opt.calls] == ["sumsq", "adam"] and opt.calls[0][1] == 3 and opt.calls[1][1] == 3      # one clip, one launch: the groups differ in lr alone
    z = [np.zeros(p.shape, f32) for p in params]
    P, _, _, total = ref.step_device_order(p0, [p.grad.numpy() for p in params], z, z, [1, 1, 1], [LR, LR, 1e-2], B1, B2, 1e-8, 0.0, 0.5)
    assert all(np.array_equal(p.detach().numpy(), w) for p, w in zip(params, P)) and float(opt.total_norm) == float(total)
    opt.step(max_grad_norm=4.0)                                                # the argument goes before the constructor's value
    assert opt.calls[-1][3] == 4.0
    two = _stubbed([dict(params=params[:2]), dict(params=params[2:], eps=1e-5)], lr=LR)
    two.step()
    assert [c[0] for c in two.calls] == ["adam", "adam"] and [c[2][2] for c in two.calls] == [1e-8, 1e-5]       # another eps: a launch of its own


def test_lr_is_read_on_every_step():
    params = _params([(6,)])
    opt = _stubbed(params, lr=LR)
    for step, lr in enumerate((LR, 1e-4, 5e-3), start=1):
        for group in opt.param_groups:                                         # SB3's update_learning_rate
            group["lr"] = lr
        _set_grads(params, step)
        opt.step()
        assert opt.calls[-1][5] == [tuple(float(x) for x in ref.corrections(lr, B1, B2, step))]


def test_state_dict_goes_to_torch_adam_and_back():
    shapes = [(4, 3), (9,)]
    ours, theirs = _params(shapes, seed=1), _params(shapes, seed=1)
    opt = _stubbed(ours, lr=LR, eps=1e-5)
    for it in range(3):
        _set_grads(ours, 20 + it)
        opt.step()
    adam = torch.optim.Adam(theirs, lr=1.0)                                    # every hyperparameter comes with the state
    adam.load_state_dict(copy.deepcopy(opt.state_dict()))                     # a copy: torch's load keeps the very tensors it is given
    assert adam.param_groups[0]["lr"] == LR and adam.param_groups[0]["eps"] == 1e-5 and not adam.param_groups[0]["amsgrad"]
    for a, b in zip(ours, theirs):
        b.data.copy_(a.data)
        assert float(adam.state[b]["step"]) == 3 and torch.equal(adam.state[b]["exp_avg"], opt.state[a]["exp_avg"])
        assert torch.equal(adam.state[b]["exp_avg_sq"], opt.state[a]["exp_avg_sq"])
    for it in range(3):                                                        # torch goes on from there ...
        _set_grads(theirs, 30 + it)
        adam.step()
    back = _stubbed(ours, lr=1.0)
    back.load_state_dict(copy.deepcopy(adam.state_dict()))                                  # ... and hands back
    for a, b in zip(ours, theirs):
        a.data.copy_(b.data)
        st = back.state[a]
        assert float(st["step"]) == 6 and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
        assert torch.equal(st["exp_avg"], adam.state[b]["exp_avg"]) and torch.equal(st["exp_avg_sq"], adam.state[b]["exp_avg_sq"])
    assert back.param_groups[0]["lr"] == LR and back.param_groups[0]["eps"] == 1e-5
    _set_grads(ours, 40), _set_grads(theirs, 40)
    back.step(), adam.step()
    assert back.calls[-1][5] == [tuple(float(x) for x in ref.corrections(LR, B1, B2, 7))] * 2
    for a, b in zip(ours, theirs):
        assert float(back.state[a]["step"]) == 7
        assert np.abs(a.detach().numpy() - b.detach().numpy()).max() <= 4 * 2.0 ** -24 * np.abs(b.detach().numpy()).max()
    with pytest.raises(ValueError, match="amsgrad"):
        _stubbed(_params(shapes), lr=LR).load_state_dict(torch.optim.Adam(_params(shapes), amsgrad=True).state_dict())


def test_refusals():
    from tactile_gym_amd.optim import DeviceAdam
    ok = lambda: _params([(4, 3)])   # noqa: E731
    with pytest.raises(ValueError, match="float32"):
        _stubbed([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="contiguous"):
        _stubbed([torch.nn.Parameter(torch.zeros(3, 4).t())])
    with pytest.raises(ValueError, match="ROCm device"):
        DeviceAdam(ok())                                                       # CPU tensors: there is no CPU path
    for name, value in (("amsgrad", True), ("maximize", True), ("capturable", True), ("foreach", True), ("fused", True), ("differentiable", True),
                        ("decoupled_weight_decay", True)):
        with pytest.raises(ValueError, match=name):
            _stubbed(ok(), **{name: value})
    with pytest.raises(ValueError, match="device"):                            # parameters on more than one device
        _stubbed(ok() + [torch.nn.Parameter(torch.zeros(3, device="meta"))])
    opt = _stubbed(ok())
    with pytest.raises(ValueError, match="device"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3, device="meta"))]))
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0), dict(max_grad_norm=-0.5),
               dict(max_grad_norm=math.nan), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            _stubbed(ok(), **kw)
    # at the step: sparse, wrongly typed or strided gradients, a bad max_grad_norm - and a refused step advances nothing
    params = _params([(4, 3), (5,)])
    opt = _stubbed(params)
    _set_grads(params, 1)
    opt.step()
    params[1].grad = torch.zeros(5).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    params[1].grad = None                                                      # (torch itself refuses a grad of another dtype)
    params[0].grad = torch.zeros(3, 4).t()
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    _set_grads(params, 2)
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.step(max_grad_norm=-1.0)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    assert [float(opt.state[p]["step"]) for p in params] == [1.0, 1.0] and len(opt.calls) == 1


def test_ppo_train_hands_the_clip_to_device_adam_and_keeps_the_other_path():
    from tactile_gym_amd import train
    from types import SimpleNamespace
    w = _params([(3, 2)])[0]
    batch = SimpleNamespace(observations=torch.ones(4, 3), actions=torch.zeros(4, 2), old_log_prob=torch.zeros(4), advantages=torch.ones(4),
                            returns=torch.zeros(4), old_values=torch.zeros(4))
    buf = SimpleNamespace(get=lambda *a, **k: iter([batch, batch]))
    policy = lambda obs: (obs @ w, torch.zeros(2), (obs @ w).sum(dim=1))   # noqa: E731
    fake_loss = lambda mean, *a, **k: ((mean * mean).sum(), torch.zeros(8))   # noqa: E731
    real, train.ppo_loss = train.ppo_loss, fake_loss
    try:
        opt = _stubbed([w], lr=LR)
        train.ppo_train(policy, opt, buf, 1, 4, 0.2, None, 0.0, 0.5, 0.5, None)
        assert [c[0] for c in opt.calls] == ["sumsq", "adam"] * 2 and opt.calls[1][3] == 0.5 and float(opt.state[w]["step"]) == 2
        opt2 = _stubbed([w], lr=LR)
        train.ppo_train(policy, opt2, buf, 1, 4, 0.2, None, 0.0, 0.5, None, None)
        assert [c[0] for c in opt2.calls] == ["adam"] * 2
        sgd = torch.optim.SGD([w], lr=0.0)
        train.ppo_train(policy, sgd, buf, 1, 4, 0.2, None, 0.0, 0.5, 0.5, None)
        assert float(torch.linalg.vector_norm(w.grad)) <= 0.5 * (1 + 1e-6)     # torch's clip scaled p.grad on the other path
    finally:
        train.ppo_loss = real


# ---------------------------------------------------------------------------------------------------------------- C ABI and resources
def test_c_abi_entries_are_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    for name, n_args, res in (("tg_optim_workspace", 1, "int64_t"), ("tg_optim_sumsq", 6, "int"), ("tg_optim_adam", 18, "int")):
        decl = re.search(rf"\b{res} {name}\s*\(([^;]*)\);", header).group(1)
        assert len(decl.split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
        if res == "int":
            assert decl.split(",")[-1].strip() == "void* hip_stream"           # raw pointers, the stream last
    for name, value in (("CHUNK", 4096), ("MAX_TENSORS", 64)):
        assert re.search(rf"#define TG_OPTIM_{name} {value}\b", header) and getattr(_capi, "OPTIM_" + name) == value
    assert os.path.exists(_capi.LIB_PATH), "library not built"
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("tg_optim_workspace", "tg_optim_sumsq", "tg_optim_adam"):
        assert re.search(rf"\bT {name}\b", nm), name
    build_units.assert_exact_product_unit("tg_loss_head")                      # the unit that includes tg_optim.h: no new unit, no new flag
    L = _capi.lib()
    assert L.tg_optim_workspace(1) == 8 and L.tg_optim_workspace(733) == 8 * 733
    assert L.tg_optim_workspace(0) < 0 and L.tg_last_error().decode().startswith("tg_optim_workspace:")


def test_optim_kernels_use_no_scratch(tmp_path):
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    assert os.path.exists(LIB), "library not built"
    scratch = {k: v for k, v in _kernel_scratch(tmp_path).items() if "k_optim" in k}
    assert len(scratch) == 3, sorted(scratch)                                  # k_optim_sumsq, k_optim_adam<false>, k_optim_adam<true>
    assert all(v == 0 for v in scratch.values()), scratch                      # the table by value is read from the arguments, not copied to the stack
