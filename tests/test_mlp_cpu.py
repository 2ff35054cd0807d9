"""The device MLP towers without a GPU: the float64 restatement (tests/mlp_ref.py) against torch's own float64 autograd, mutants of it against
its bounds, the k tail's operands, tactile_gym_amd.mlp's modules on their CPU path against hand-built torch modules with SB3's names, the checks
that raise, the ABI's declarations, and the kernels' scratch size read from the built library."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import build_units  # noqa: E402
import mlp_ref as ref  # noqa: E402

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402
from test_conv_stem_cpu import LIB, _kernel_scratch  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_mlp_forward"]                 # at import: the whole file needs the feature
f32, f64 = np.float32, np.float64


def _torch_tower(x, tower):
    """(per layer h, leaves) with torch float64 autograd; leaves: x and per layer (w, b) over both row blocks."""
    xt = torch.from_numpy(ref.cat_input(x)).requires_grad_()
    h, hs, leaves = xt, [], []
    for ly in tower:
        w, b = (torch.from_numpy(a).requires_grad_() for a in ref.full_w(ly))
        z = h @ w.T + b
        h = torch.tanh(z) if ly["act"] == "tanh" else torch.relu(z) if ly["act"] == "relu" else z
        hs.append(h)
        leaves.append((w, b))
    return xt, hs, leaves


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape and np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("two", [0, 2])
def test_reference_equals_torch_float64_autograd(two):
    rng = np.random.default_rng(1)
    B, K0 = 7, 9
    x = ref.split_input(ref.random_input(rng, B, K0), 6)
    tower = ref.random_tower(rng, K0, [5, 6, 3], ["tanh", "relu", "none"], two)
    xt, hs, leaves = _torch_tower(x, tower)
    want = ref.tower_forward(x, tower)
    for (h, bound), ht in zip(want, hs):
        _close(h, ht.detach().numpy())
        assert bound.shape == h.shape and (bound > 0).all()
    dy = rng.standard_normal((B, 3 + two))
    hs[-1].backward(torch.from_numpy(dy))
    grads, bounds, dh0, e0 = ref.tower_backward(x, tower, [h.detach().numpy() for h in hs], dy)
    _close(dh0, xt.grad.numpy())
    for (dw, db), (w, b), (bw, bb) in zip(grads, leaves, bounds):
        _close(dw, w.grad.numpy())
        _close(db, b.grad.numpy())
        assert bw.shape == dw.shape and bb.shape == db.shape and (bw >= 0).all()
    assert (e0 > 0).all()


def test_exact_cases_are_float32_numbers_and_the_tail_operands_keep_the_chain():
    rng = np.random.default_rng(2)
    x = ref.split_input(ref.exact_input(rng, 65, 258), 256)
    tower = ref.exact_tower(rng, 258, [256, 256, 256, 2], ["relu", "relu", "none", "relu"], 2)
    ref.assert_exact_forward(x, tower)                                       # four layers at width 256 stay below 2^24
    for h, _ in ref.tower_forward(x, tower):
        assert np.array_equal(h.astype(f32).astype(f64), h)
    xfull, tower, hs, dy = ref.exact_backward_case(rng, 65, 258, [256, 256, 1], ["relu", "relu", "none"])
    ref.assert_exact_backward(ref.split_input(xfull, 256), tower, hs, dy)
    with pytest.raises(AssertionError):                                      # and the check does refuse what is not exact
        ref.assert_exact_forward(x, [ref.layer(np.full((1, 258), 70000.0, f32), np.zeros(1, f32))])
    assert ref.tail_operands_keep_bits()
    assert f32(f64(f32(0.0)) * f64(f32(0.0)) + f64(f32(-0.0))).view(np.uint32) == 0              # fmaf(0, 0, -0.0) = +0.0: why the tail is not (0, 0)
    assert f32(f64(f32(-0.0)) * f64(f32(0.0)) + f64(f32(-0.0))).view(np.uint32) == 0x80000000     # fmaf(-0.0, 0, -0.0) = -0.0


def test_mutants_exceed_the_bounds_by_a_wide_factor():
    rng = np.random.default_rng(3)
    B, K0 = 33, 12
    xfull = ref.random_input(rng, B, K0)
    x = ref.split_input(xfull, 6)
    tower = ref.random_tower(rng, K0, [12, 12, 4], ["tanh", "relu", "tanh"], 4)
    other = ref.random_tower(rng, K0, [12, 12, 4], ["tanh", "relu", "tanh"], 4)
    want = ref.tower_forward(x, tower)
    h_last, bound = want[-1]

    def factor(got, want=h_last, bound=bound):
        return float((np.abs(got - want) / bound).max())

    def mutate(l, **kw):
        t = [dict(ly) for ly in tower]
        t[l].update(kw)
        return ref.tower_forward(x, t)[-1][0]

    zero = lambda a: np.zeros_like(a)   # noqa: E731
    last = tower[-1]
    factors = {
        "bias left out": factor(mutate(1, b=zero(tower[1]["b"]))),
        "activation left out": factor(mutate(0, act="none")),
        "W read transposed (square layer)": factor(mutate(1, w=np.ascontiguousarray(tower[1]["w"].T))),
        "row blocks swapped": factor(mutate(2, w=last["w2"], b=last["b2"], w2=last["w"], b2=last["b"])),
        "column blocks swapped": factor(ref.tower_forward((x[1], x[0]), tower)[-1][0]),
        "towers' outputs swapped": factor(ref.tower_forward(x, other)[-1][0]),
    }
    hs = [h.astype(f32) for h, _ in want]
    dy = rng.standard_normal(h_last.shape).astype(f32)
    grads, bounds, dh0, e0 = ref.tower_backward(x, tower, hs, dy)
    z_as_h = [np.arctanh(np.clip(h.astype(f64), -0.999999, 0.999999)) if ly["act"] == "tanh" else h for h, ly in zip(hs, tower)]
    mg, _, mdh0, _ = ref.tower_backward(x, tower, z_as_h, dy)                 # Tanh' taken as 1 - z^2: act' evaluated at z instead of h
    # ReLU's mask is the same at z and h, so the mutant differs through the Tanh layers alone
    factors["Tanh' taken as 1 - z^2"] = max(float((np.abs(mg[0][0] - grads[0][0]) / bounds[0][0]).max()), factor(mdh0, dh0, e0))
    for name, f in factors.items():
        print(f"{name}: {f:.3g} bounds")
    assert all(f > 1000 for f in factors.values()), factors


def _torch_actor_critic(fd, A, pi, vf, act):
    def seq(widths):
        mods, w0 = [], fd
        for w in widths:
            mods += [nn.Linear(w0, w), act()]
            w0 = w
        return nn.Sequential(*mods), w0

    class Extractor(nn.Module):
        def __init__(self):
            super().__init__()
            self.policy_net, self.dpi = seq(pi)
            self.value_net, self.dvf = seq(vf)

    class Policy(nn.Module):
        def __init__(self):
            super().__init__()
            self.log_std = nn.Parameter(torch.zeros(A))
            self.mlp_extractor = Extractor()
            self.action_net = nn.Linear(self.mlp_extractor.dpi, A)
            self.value_net = nn.Linear(self.mlp_extractor.dvf, 1)

        def forward(self, f):
            return self.action_net(self.mlp_extractor.policy_net(f)), self.log_std, self.value_net(self.mlp_extractor.value_net(f)).flatten()
    return Policy()


def _torch_sac_actor(fd, A, arch, act):
    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            mods, w0 = [], fd
            for w in arch:
                mods += [nn.Linear(w0, w), act()]
                w0 = w
            self.latent_pi = nn.Sequential(*mods)
            self.mu, self.log_std = nn.Linear(w0, A), nn.Linear(w0, A)

        def forward(self, f):
            z = self.latent_pi(f)
            return self.mu(z), self.log_std(z)
    return Actor()


def _torch_critic(fd, A, arch, act, n):
    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(n):
                mods, w0 = [], fd + A
                for w in arch:
                    mods += [nn.Linear(w0, w), act()]
                    w0 = w
                self.add_module(f"qf{i}", nn.Sequential(*mods, nn.Linear(w0, 1)))

        def forward(self, f, a):
            x = torch.cat([f, a], dim=1)
            return tuple(getattr(self, f"qf{i}")(x) for i in range(n))
    return Critic()


def _same_state(ours, plain):
    a, b = ours.state_dict(), plain.state_dict()
    assert set(a) == set(b) and all(a[k].shape == b[k].shape for k in a)
    ours.load_state_dict(plain.state_dict(), strict=True)                    # a checkpoint of the torch modules loads ...
    plain.load_state_dict(ours.state_dict(), strict=True)                    # ... and the other way round


def test_modules_keys_load_both_ways_and_cpu_path_equals_torch():
    import tactile_gym_amd as tg
    from tactile_gym_amd import mlp
    assert tg.mlp is mlp and tg.mlp_towers is mlp.mlp_towers and tg.ActorCriticHeads is mlp.ActorCriticHeads
    assert tg.SacActorHeads is mlp.SacActorHeads and tg.ContinuousCriticHeads is mlp.ContinuousCriticHeads
    torch.manual_seed(4)
    fd, A, B = 20, 3, 9
    f, a = torch.randn(B, fd), torch.randn(B, A)
    heads = tg.ActorCriticHeads(fd, A, [dict(pi=[16, 12], vf=[8])], activation_fn=nn.Tanh, log_std_init=-0.5)
    assert set(heads.state_dict()) == {"log_std", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias",
                                       "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
                                       "mlp_extractor.policy_net.2.bias", "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias"}
    # SB3's initialisation: orthogonal rows (or columns) scaled by the gain, zero biases
    w = heads.mlp_extractor.policy_net[0].weight.detach()
    assert torch.allclose(w @ w.T, 2.0 * torch.eye(16), atol=1e-5) and float(heads.action_net.bias.detach().abs().max()) == 0
    w = heads.action_net.weight.detach()
    assert torch.allclose(w @ w.T, 1e-4 * torch.eye(A), atol=1e-8) and torch.equal(heads.log_std.detach(), torch.full((A,), -0.5))
    w = heads.value_net.weight.detach()
    assert torch.allclose(w @ w.T, torch.eye(1), atol=1e-5)
    plain = _torch_actor_critic(fd, A, [16, 12], [8], nn.Tanh)
    _same_state(heads, plain)
    for got, want in zip(heads(f), plain(f)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=1e-6)
    actor, plain = tg.SacActorHeads(fd, A, [16, 12]), _torch_sac_actor(fd, A, [16, 12], nn.ReLU)
    assert list(actor.state_dict()) == ["latent_pi.0.weight", "latent_pi.0.bias", "latent_pi.2.weight", "latent_pi.2.bias", "mu.weight", "mu.bias",
                                        "log_std.weight", "log_std.bias"]
    _same_state(actor, plain)
    for got, want in zip(actor(f), plain(f)):
        assert got.shape == (B, A) and torch.allclose(got, want, rtol=0, atol=1e-6)
    critic, plain = tg.ContinuousCriticHeads(fd, A, [16, 12], n_critics=3), _torch_critic(fd, A, [16, 12], nn.ReLU, 3)
    assert [k for k in critic.state_dict() if k.startswith("qf1")] == [f"qf1.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    _same_state(critic, plain)
    qs = critic(f, a)
    assert isinstance(qs, tuple) and len(qs) == 3
    for got, want in zip(qs, plain(f, a)):
        assert got.shape == (B, 1) and torch.allclose(got, want, rtol=0, atol=1e-6)
    before = heads(f)[0].detach().clone()
    heads.action_net = nn.Linear(12, A)                                      # a submodule replaced after the first call is the one that runs
    assert not torch.equal(heads(f)[0], before) and torch.allclose(heads(f)[0], heads.action_net(heads.mlp_extractor.policy_net(f)), atol=1e-6)
    sum(q.sum() for q in qs).backward()                                      # the CPU path is differentiable through torch
    assert critic.qf0[0].weight.grad is not None and critic.qf2[4].bias.grad is not None


def test_checks_raise():
    import tactile_gym_amd as tg
    x, w, b = torch.zeros(3, 4), torch.zeros(2, 4), torch.zeros(2)
    tg.mlp_towers(x, [[(w, b, None)]])
    with pytest.raises(TypeError, match="float32"):
        tg.mlp_towers(x.double(), [[(w, b, None)]])
    with pytest.raises(TypeError, match="torch tensor"):
        tg.mlp_towers(x.numpy(), [[(w, b, None)]])
    with pytest.raises(ValueError, match="2-D"):
        tg.mlp_towers(x[0], [[(w, b, None)]])
    with pytest.raises(ValueError, match="contiguous"):
        tg.mlp_towers(torch.zeros(4, 3).T, [[(w, b, None)]])
    with pytest.raises(ValueError, match="share"):
        tg.mlp_towers((x, torch.zeros(2, 1)), [[(torch.zeros(2, 5), b, None)]])
    with pytest.raises(ValueError, match="weight"):
        tg.mlp_towers(x, [[(torch.zeros(2, 5), b, None)]])
    with pytest.raises(ValueError, match="bias"):
        tg.mlp_towers(x, [[(w, torch.zeros(3), None)]])
    with pytest.raises(TypeError, match="weight"):
        tg.mlp_towers(x, [[(w.double(), b, None)]])
    with pytest.raises(ValueError, match="activation"):
        tg.mlp_towers(x, [[(w, b, "gelu")]])
    with pytest.raises(ValueError, match="towers"):
        tg.mlp_towers(x, [[(w, b, None)]] * 5)
    with pytest.raises(ValueError, match="layers"):
        tg.mlp_towers(x, [[(torch.zeros(4, 4), torch.zeros(4), None)] * 5])
    with pytest.raises(ValueError, match="above 256 are not built"):
        tg.mlp_towers(x, [[(torch.zeros(257, 4), torch.zeros(257), None)]])
    with pytest.raises(ValueError, match="above 256 are not built"):
        tg.mlp_towers(x, [[(torch.zeros(200, 4), torch.zeros(200), None, torch.zeros(57, 4), torch.zeros(57))]])
    with pytest.raises(ValueError, match="last layer"):
        tg.mlp_towers(x, [[(w, b, None, w, b), (torch.zeros(1, 2), torch.zeros(1), None)]])
    with pytest.raises(ValueError, match="columns"):
        tg.mlp_towers(torch.zeros(1, 1025), [[(torch.zeros(1, 1025), torch.zeros(1), None)]])
    with pytest.raises(ValueError, match="shared layers"):
        tg.ActorCriticHeads(8, 2, [64, dict(pi=[8], vf=[8])])
    with pytest.raises(ValueError, match="above 256 are not built"):
        tg.ActorCriticHeads(8, 2, dict(pi=[512], vf=[8]))
    with pytest.raises(ValueError, match="hidden layers"):
        tg.SacActorHeads(8, 2, [8, 8, 8, 8])
    with pytest.raises(ValueError, match="activation_fn"):
        tg.ContinuousCriticHeads(8, 2, [8], activation_fn=nn.GELU)
    with pytest.raises(ValueError, match="n_critics"):
        tg.ContinuousCriticHeads(8, 2, [8], n_critics=5)


def test_abi_declarations_and_build_line():
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name, value in (("TG_MLP_MAX_TOWERS", 4), ("TG_MLP_MAX_LAYERS", 4), ("TG_MLP_MAX_WIDTH", 256), ("TG_MLP_MAX_IN", 1024),
                        ("TG_MLP_MAX_ROWS", 2147483616), ("TG_MLP_ACT_NONE", 0), ("TG_MLP_ACT_TANH", 1), ("TG_MLP_ACT_RELU", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
    assert (_capi.MLP_MAX_TOWERS, _capi.MLP_MAX_LAYERS, _capi.MLP_MAX_WIDTH, _capi.MLP_MAX_IN, _capi.MLP_MAX_ROWS) == (4, 4, 256, 1024, 2147483616)
    assert _capi.MLP_ACT == {"none": 0, "tanh": 1, "relu": 2}
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16      # a struct and functions added, no struct changed
    assert "typedef struct tg_mlp_layer {" in header and "typedef struct tg_mlp_tower {" in header
    assert C.sizeof(_capi.TgMlpLayer) == 10 * 8 + 4 * 4 and C.sizeof(_capi.TgMlpTower) == 8 + 2 * 8 + 4 * C.sizeof(_capi.TgMlpLayer)
    fields = re.search(r"typedef struct tg_mlp_layer \{(.*?)\} tg_mlp_layer;", header, re.S).group(1)
    names = re.findall(r"(?:float\*|int32_t)\s+([^;]+);", fields)
    assert [n.strip() for part in names for n in part.split(",")] == [k.rstrip("_") for k, _ in _capi.TgMlpLayer._fields_]
    for name, n_args in (("tg_mlp_forward", 9), ("tg_mlp_backward_workspace", 5), ("tg_mlp_backward", 12)):
        decl = re.search(r"\b(?:int|int64_t) %s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
    L = _capi.lib()
    assert all(hasattr(L, n) for n in ("tg_mlp_forward", "tg_mlp_backward_workspace", "tg_mlp_backward"))
    build_units.assert_exact_product_unit("tg_mlp")
    # the workspace query needs no device: a size for valid shapes, the error's code otherwise
    arr = (_capi.TgMlpTower * 2)()
    for t in range(2):
        arr[t].n_layers = 2
        arr[t].layer[0].in_, arr[t].layer[0].out, arr[t].layer[1].in_, arr[t].layer[1].out = 258, 256, 256, 1
    slab = 2 * (256 * 259 + 257)
    assert L.tg_mlp_backward_workspace(64, 256, 2, arr, 2) == 4 * (2 * slab + 2 * 64 * 258)      # two row tiles' slabs, two towers' dh_0
    assert L.tg_mlp_backward_workspace(32, 256, 2, arr, 1) == 0                                   # one row tile, one tower: in place
    assert L.tg_mlp_backward_workspace(0, 256, 2, arr, 2) == 0
    arr[1].layer[1].in_ = 255
    assert L.tg_mlp_backward_workspace(64, 256, 2, arr, 2) < 0 and L.tg_last_error().decode().startswith("tg_mlp_backward_workspace: tower 1 layer 1")


def test_mlp_kernels_use_no_scratch(tmp_path):
    assert os.path.exists(LIB), "the library is not built: run tactile_gym_amd/csrc/build.sh"
    scratch = _kernel_scratch(tmp_path)
    mlp = {k: v for k, v in scratch.items() if "k_mlp_" in k}
    assert len(mlp) == 3, sorted(mlp)                 # forward, backward and the reduction
    assert all(v == 0 for v in mlp.values()), mlp
