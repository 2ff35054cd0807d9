"""stable_baselines3's policy, value and critic heads on the device MLP towers (csrc/tg_mlp.hip: k_mlp_fwd, k_mlp_bwd, k_mlp_reduce;
DESIGN.md 4.17).

    heads = tg.ActorCriticHeads(features_dim, A, dict(pi=[256, 256], vf=[256, 256]))            # PPO: MlpExtractor, action_net, value_net, log_std
    policy = lambda obs: heads(extractor(obs))                                                    # -> mean [B, A], log_std [A], values [B]
    actor_heads = tg.SacActorHeads(features_dim, A, [256, 256])                                   # SAC: latent_pi, mu, log_std
    critic_heads = tg.ContinuousCriticHeads(features_dim, A, [256, 256])                          # qf0, qf1
    actor = lambda obs: actor_heads(extractor(obs)); critic = lambda obs, act: critic_heads(critic_extractor(obs), act)

A tower is a chain of 1 to 4 layers h_l = act_l(h_{l-1} W_l^T + b_l) (W torch's [out, in], out <= 256, the first in <= 1024); a call runs 1 to
4 towers on one input in ONE launch, and its backward pass in at most two.  Each output element is one float32 fmaf chain over k ascending,
plus the bias, then the activation (Tanh: tanh in double, rounded once): a row's outputs depend on the row alone, so PPO's first-epoch ratio
exp(log_prob_new - log_prob_old) of a minibatch row is computed from the very bits the collection batch produced.  The sums over rows of the
backward pass are taken in a fixed order: the same bits on every run.

Device tensors run the HIP kernels on torch's current stream.  CPU tensors take a plain-torch path of the same meaning (F.linear and torch's
activations) that is not bit-specified: SB3 can save, load and evaluate the modules on the host.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _capi as capi
from ._device import addr, check_f32_like, launch, workspace

__all__ = ["mlp_towers", "ActorCriticHeads", "SacActorHeads", "ContinuousCriticHeads"]

_ACT_OF_MODULE = {nn.Tanh: "tanh", nn.ReLU: "relu", nn.Identity: "none"}


def _act_name(act):
    if act is None:
        return "none"
    if isinstance(act, str) and act.lower() in capi.MLP_ACT:
        return act.lower()
    raise ValueError(f"activation {act!r}: None, 'none', 'tanh' or 'relu' are built")


def _check_x(x):
    """(blocks, K0): the input's one or two column blocks after the checks on them."""
    blocks = list(x) if isinstance(x, (tuple, list)) else [x]
    if not 1 <= len(blocks) <= 2:
        raise ValueError(f"x must be one tensor or a pair of column blocks, got {len(blocks)}")
    for b in blocks:
        if not isinstance(b, torch.Tensor):
            raise TypeError(f"x must be a torch tensor (or a pair), got {type(b).__name__}")
        if b.dtype != torch.float32:
            raise TypeError(f"x must be float32, got {b.dtype}")
        if b.dim() != 2:
            raise ValueError(f"x must be 2-D [B, K], got shape {tuple(b.shape)}")
        if not b.is_contiguous():
            raise ValueError("x must be contiguous")
        if b.device != blocks[0].device or b.shape[0] != blocks[0].shape[0]:
            raise ValueError("the two column blocks of x must share their device and their rows")
    K0 = sum(int(b.shape[1]) for b in blocks)
    if any(b.shape[1] < 1 for b in blocks) or K0 > capi.MLP_MAX_IN:
        raise ValueError(f"x has {K0} columns: 1 to {capi.MLP_MAX_IN} are built")
    if blocks[0].shape[0] > capi.MLP_MAX_ROWS:
        raise ValueError(f"x has {blocks[0].shape[0]} rows: at most {capi.MLP_MAX_ROWS}")
    return blocks, K0


def _check(x, towers):
    """(blocks, spec): the input's column blocks and, per tower, a list of (weight, bias, act, weight2, bias2) with weight2 None except on a
    two-block last layer."""
    blocks, K0 = _check_x(x)
    towers = list(towers)
    if not 1 <= len(towers) <= capi.MLP_MAX_TOWERS:
        raise ValueError(f"{len(towers)} towers: 1 to {capi.MLP_MAX_TOWERS} run in one call")
    spec = []
    for t, tower in enumerate(towers):
        tower = list(tower)
        if not 1 <= len(tower) <= capi.MLP_MAX_LAYERS:
            raise ValueError(f"tower {t} has {len(tower)} layers: 1 to {capi.MLP_MAX_LAYERS} are built")
        layers, width = [], K0
        for l, layer in enumerate(tower):
            layer = tuple(layer)
            if len(layer) not in (3, 5):
                raise ValueError(f"tower {t} layer {l}: (weight, bias, act) or (weight, bias, act, weight2, bias2), got {len(layer)} items")
            w, b, act = layer[:3]
            w2, b2 = layer[3:] if len(layer) == 5 else (None, None)
            if w2 is not None and l != len(tower) - 1:
                raise ValueError(f"tower {t} layer {l}: only a tower's last layer may have a second row block")
            if not isinstance(w, torch.Tensor) or w.dim() != 2:
                raise TypeError(f"tower {t} layer {l}: weight must be a 2-D float32 torch tensor")
            out, out2 = int(w.shape[0]), (int(w2.shape[0]) if isinstance(w2, torch.Tensor) and w2.dim() == 2 else 0)
            if not 1 <= out or out + out2 > capi.MLP_MAX_WIDTH:
                raise ValueError(f"tower {t} layer {l} is {out + out2} wide: widths above {capi.MLP_MAX_WIDTH} are not built")
            check_f32_like(w, f"tower {t} layer {l} weight", (out, width), blocks[0])
            check_f32_like(b, f"tower {t} layer {l} bias", (out,), blocks[0])
            if w2 is not None:
                check_f32_like(w2, f"tower {t} layer {l} weight2", (out2, width), blocks[0])
                check_f32_like(b2, f"tower {t} layer {l} bias2", (out2,), blocks[0])
                if out2 < 1:
                    raise ValueError(f"tower {t} layer {l}: the second row block is empty")
            layers.append((w, b, _act_name(act), w2, b2))
            width = out
        spec.append(layers)
    return blocks, spec


def _descriptors(acts, params, hs, grads=None, dys=None):
    """The tg_mlp_tower array of a call.  acts: per tower the layers' activation names; params / hs / grads: per tower and layer
    (weight, bias, weight2, bias2), (h, h2) and (dweight, dbias, dweight2, dbias2) tensors or None; dys: per tower (dy, dy2)."""
    arr = (capi.TgMlpTower * len(acts))()
    for t, tower in enumerate(acts):
        arr[t].n_layers = len(tower)
        if dys is not None:
            arr[t].dy, arr[t].dy2 = addr(dys[t][0]), addr(dys[t][1])
        for l, act in enumerate(tower):
            ly = arr[t].layer[l]
            w, b, w2, b2 = params[t][l]
            ly.weight, ly.bias, ly.weight2, ly.bias2 = addr(w), addr(b), addr(w2), addr(b2)
            ly.in_, ly.out, ly.out2, ly.act = w.shape[1], w.shape[0], (w2.shape[0] if w2 is not None else 0), capi.MLP_ACT[act]
            ly.h, ly.h2 = addr(hs[t][l][0]), addr(hs[t][l][1])
            if grads is not None:
                ly.dweight, ly.dbias, ly.dweight2, ly.dbias2 = (addr(g) for g in grads[t][l])
    return arr


def _run_forward(x0, x1, acts, params, save_all):
    B, dev = x0.shape[0], x0.device
    hs = []
    for t, tower in enumerate(acts):
        row = []
        for l, _ in enumerate(tower):
            w, _, w2, _ = params[t][l]
            if save_all or l == len(tower) - 1:
                row.append((torch.empty((B, w.shape[0]), dtype=torch.float32, device=dev),
                            torch.empty((B, w2.shape[0]), dtype=torch.float32, device=dev) if w2 is not None else None))
            else:
                row.append((None, None))
        hs.append(row)
    if B == 0:                                                            # nothing to launch (an empty tensor has no address to pass)
        return hs
    arr = _descriptors(acts, params, hs)
    launch("tg_mlp_forward", dev, addr(x0), x0.shape[1], addr(x1), x1.shape[1] if x1 is not None else 0, B, arr, len(acts), int(save_all))
    return hs


def _unflatten(meta, flat):
    """Per tower and layer [weight, bias, weight2, bias2] from the flat parameter list; meta: per tower (acts, two_block)."""
    params, at = [], 0
    for acts, two in meta:
        layers = []
        for l in range(len(acts)):
            n = 4 if two and l == len(acts) - 1 else 2
            layers.append(list(flat[at:at + n]) + [None] * (4 - n))
            at += n
        params.append(layers)
    return params


class _MlpTowers(torch.autograd.Function):
    """apply(meta, n_blocks, grad_mode, *blocks, *flat parameters) -> every tower's last-layer outputs, flat (h, then h2 where the layer has
    two blocks).  meta: per tower (the layers' activation names, whether the last layer has a second row block).  grad_mode: the caller's
    torch.is_grad_enabled() - inside forward it is always off, and needs_input_grad says what the inputs ask for, not whether a graph is
    being built."""

    @staticmethod
    def forward(ctx, meta, n_blocks, grad_mode, *tensors):
        blocks, flat = tensors[:n_blocks], tensors[n_blocks:]
        x0, x1 = blocks[0], (blocks[1] if n_blocks == 2 else None)
        acts = [m[0] for m in meta]
        params = _unflatten(meta, flat)
        needs = bool(grad_mode) and any(ctx.needs_input_grad[3:])
        hs = _run_forward(x0, x1, acts, params, needs)
        outs = []
        for t, (a, two) in enumerate(meta):
            outs.append(hs[t][-1][0])
            if two:
                outs.append(hs[t][-1][1])
        if needs:                                                         # under no_grad, or with everything frozen, nothing is kept
            hidden = [h for t, (a, _) in enumerate(meta) for h, _ in hs[t][:-1]]
            ctx.save_for_backward(*blocks, *flat, *hidden, *outs)
            ctx.mlp = (meta, n_blocks, len(flat), len(hidden))
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        meta, n_blocks, n_flat, n_hidden = ctx.mlp
        saved = ctx.saved_tensors
        blocks, flat = saved[:n_blocks], saved[n_blocks:n_blocks + n_flat]
        hidden, outs = list(saved[n_blocks + n_flat:n_blocks + n_flat + n_hidden]), list(saved[n_blocks + n_flat + n_hidden:])
        x0, x1 = blocks[0], (blocks[1] if n_blocks == 2 else None)
        B, dev = x0.shape[0], x0.device
        acts = [m[0] for m in meta]
        params = _unflatten(meta, flat)
        need = ctx.needs_input_grad[3:]
        alloc = torch.empty if B else torch.zeros                         # B = 0 launches nothing: the gradients are zero
        hs, dys, grads, flat_grads = [], [], [], []
        douts, at = list(douts), n_blocks
        for t, (a, two) in enumerate(meta):
            row = [(hidden.pop(0), None) for _ in a[:-1]]
            row.append((outs.pop(0), outs.pop(0) if two else None))
            hs.append(row)
            dy = [douts.pop(0), douts.pop(0) if two else None]
            for i, g in enumerate(dy):
                if g is not None:
                    if g.dtype != torch.float32:
                        raise TypeError(f"the output's gradient must be float32, got {g.dtype}")
                    dy[i] = g.contiguous()
            dys.append(dy)
            tower_grads = []
            for l in range(len(a)):
                gl = []
                for p in params[t][l]:
                    if p is None:
                        gl.append(None)
                        continue
                    g = alloc(p.shape, dtype=torch.float32, device=dev) if need[at] else None
                    flat_grads.append(g)
                    gl.append(g)
                    at += 1
                tower_grads.append(gl)
            grads.append(tower_grads)
        dx = [alloc(b.shape, dtype=torch.float32, device=dev) if need[i] else None for i, b in enumerate(blocks)]
        if B == 0:
            return (None, None, None, *dx, *flat_grads)
        arr = _descriptors(acts, params, hs, grads, dys)
        Ka, Kb = x0.shape[1], (x1.shape[1] if x1 is not None else 0)
        nbytes = workspace("tg_mlp_backward_workspace", B, Ka, Kb, arr, len(meta))
        work = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        launch("tg_mlp_backward", dev, addr(x0), Ka, addr(x1), Kb, B, arr, len(meta), addr(dx[0]), addr(dx[1]) if n_blocks == 2 else None,
               addr(work), nbytes)
        return (None, None, None, *dx, *flat_grads)


def _act_torch(y, act):
    return torch.tanh(y) if act == "tanh" else F.relu(y) if act == "relu" else y


def mlp_towers(x, towers):
    """Runs every tower on x and returns a list with each tower's output: [B, out] float32, or the pair ([B, out], [B, out2]) where the
    tower's last layer has two row blocks.  x: a contiguous float32 [B, K] tensor, or a pair ([B, Ka], [B, Kb]) of column blocks that stand
    for their concatenation.  towers: 1 to 4 towers, each a list of 1 to 4 layers (weight [out, in], bias [out], act) with act None / 'none',
    'tanh' or 'relu'; a tower's last layer may be (weight, bias, act, weight2, bias2).  Differentiable in x (each block separately), in
    every weight and in every bias.  On the device: one launch forward, at most two backward, on torch's current stream.  On the CPU: plain
    torch, not bit-specified."""
    return _run(*_check(x, towers))


def _run(blocks, spec):
    """mlp_towers behind its checks."""
    if not blocks[0].is_cuda:
        xin = blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)
        result = []
        for layers in spec:
            h = xin
            for w, b, act, w2, b2 in layers[:-1]:
                h = _act_torch(F.linear(h, w, b), act)
            w, b, act, w2, b2 = layers[-1]
            y = _act_torch(F.linear(h, w, b), act)
            result.append(y if w2 is None else (y, _act_torch(F.linear(h, w2, b2), act)))
        return result
    meta = tuple((tuple(layer[2] for layer in layers), layers[-1][3] is not None) for layers in spec)
    flat = []
    for layers in spec:
        for w, b, act, w2, b2 in layers:
            flat += [w, b] if w2 is None else [w, b, w2, b2]
    outs = list(_MlpTowers.apply(meta, len(blocks), torch.is_grad_enabled(), *blocks, *flat))
    return [(outs.pop(0), outs.pop(0)) if two else outs.pop(0) for _, two in meta]


def _act_of(activation_fn):
    if activation_fn not in _ACT_OF_MODULE:
        raise ValueError(f"activation_fn={activation_fn!r}: nn.Tanh, nn.ReLU and nn.Identity are built")
    return _ACT_OF_MODULE[activation_fn]


def _widths(net_arch, what):
    widths = [int(w) for w in net_arch]
    if len(widths) > capi.MLP_MAX_LAYERS - 1:
        raise ValueError(f"{what}={list(net_arch)}: at most {capi.MLP_MAX_LAYERS - 1} hidden layers are built")
    if any(not 1 <= w <= capi.MLP_MAX_WIDTH for w in widths):
        raise ValueError(f"{what}={list(net_arch)}: widths above {capi.MLP_MAX_WIDTH} are not built")
    return widths


def _sequential(in_dim, widths, activation_fn, out_dim=None):
    """SB3's create_mlp: Linear, activation, Linear, activation, ... (+ a last Linear to out_dim): the Linear layers sit at 0, 2, 4, ..."""
    mods, width = [], in_dim
    for w in widths:
        mods += [nn.Linear(width, w), activation_fn()]
        width = w
    if out_dim is not None:
        mods.append(nn.Linear(width, out_dim))
    return nn.Sequential(*mods), width


def _linears(seq, act):
    """(Linear, act) of every Linear of a create_mlp Sequential; a trailing Linear without an activation behind it gets none."""
    mods = list(seq)
    return [(m, act if i + 1 < len(mods) else "none") for i, m in enumerate(mods) if isinstance(m, nn.Linear)]


def _module_call(x, in_dim, towers):
    """mlp_towers for the modules: x is checked, the parameters are the modules' own (float32, contiguous, of the widths they were built
    with; their device is checked against x's).  towers: per tower a list of (Linear, act) or, last, (Linear, act, Linear)."""
    blocks, K0 = _check_x(x)
    if K0 != in_dim:
        raise ValueError(f"the features have {K0} columns, the module was built for {in_dim}")
    spec = []
    for tower in towers:
        layers = []
        for item in tower:
            p = item[0]._parameters                                       # the Linear's own dict: no Module.__getattr__ on the hot path
            w = p["weight"]
            if w.device != blocks[0].device:
                raise ValueError(f"the module's parameters are on {w.device}, the features on {blocks[0].device}")
            if len(item) == 3:
                p2 = item[2]._parameters
                layers.append((w, p["bias"], item[1], p2["weight"], p2["bias"]))
            else:
                layers.append((w, p["bias"], item[1], None, None))
        spec.append(layers)
    return _run(blocks, spec)


class _MlpExtractor(nn.Module):
    """SB3's MlpExtractor without shared layers: policy_net and value_net, create_mlp Sequentials; latent_dim_pi, latent_dim_vf."""

    def __init__(self, features_dim, pi, vf, activation_fn):
        super().__init__()
        self.policy_net, self.latent_dim_pi = _sequential(features_dim, pi, activation_fn)
        self.value_net, self.latent_dim_vf = _sequential(features_dim, vf, activation_fn)


class ActorCriticHeads(nn.Module):
    """What stable_baselines3's ActorCriticPolicy does behind its features extractor for a Box action space: mlp_extractor (policy_net,
    value_net), action_net, value_net and the state-independent log_std, under SB3's parameter names - a checkpoint's entries of those
    names load with strict=True, and the other way round.  forward(features [B, features_dim]) -> (mean [B, A], log_std [A], values [B]):
    the second half of the `policy` of tg.collect.collect_rollouts and tg.train.ppo_train, in ONE launch.
    net_arch: dict(pi=[...], vf=[...]) or SB3's older [dict(pi=..., vf=...)]; at most 3 hidden layers of at most 256 each.  Initialisation is
    SB3's (ortho_init): orthogonal with gain sqrt(2) for the towers, 0.01 for action_net, 1 for value_net, zero biases."""

    def __init__(self, features_dim, action_dim, net_arch, activation_fn=nn.Tanh, log_std_init=0.0, ortho_init=True):
        super().__init__()
        if isinstance(net_arch, (list, tuple)):
            if len(net_arch) != 1 or not isinstance(net_arch[0], dict):
                raise ValueError(f"net_arch={net_arch!r}: shared layers in front of dict(pi=..., vf=...) are not built")
            net_arch = net_arch[0]
        if not isinstance(net_arch, dict) or set(net_arch) - {"pi", "vf"}:
            raise ValueError(f"net_arch={net_arch!r}: dict(pi=[...], vf=[...])")
        self.features_dim, self.action_dim, self.act = int(features_dim), int(action_dim), _act_of(activation_fn)
        if not 1 <= self.features_dim <= capi.MLP_MAX_IN:
            raise ValueError(f"features_dim={features_dim}: 1 to {capi.MLP_MAX_IN} are built")
        if not 1 <= self.action_dim <= capi.MLP_MAX_WIDTH:
            raise ValueError(f"action_dim={action_dim}: widths above {capi.MLP_MAX_WIDTH} are not built")
        self.mlp_extractor = _MlpExtractor(self.features_dim, _widths(net_arch.get("pi", []), "pi"), _widths(net_arch.get("vf", []), "vf"),
                                           activation_fn)
        self.action_net = nn.Linear(self.mlp_extractor.latent_dim_pi, self.action_dim)
        self.value_net = nn.Linear(self.mlp_extractor.latent_dim_vf, 1)
        self.log_std = nn.Parameter(torch.ones(self.action_dim) * float(log_std_init))
        if ortho_init:
            for module, gain in ((self.mlp_extractor, math.sqrt(2.0)), (self.action_net, 0.01), (self.value_net, 1.0)):
                for m in module.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain)
                        m.bias.data.fill_(0.0)

    def forward(self, features):
        towers = [_linears(self.mlp_extractor.policy_net, self.act) + [(self.action_net, "none")],      # made per call: a replaced submodule is the one that runs
                  _linears(self.mlp_extractor.value_net, self.act) + [(self.value_net, "none")]]
        mean, values = _module_call(features, self.features_dim, towers)
        return mean, self.log_std, values.reshape(-1)


class SacActorHeads(nn.Module):
    """stable_baselines3's SAC Actor behind its features extractor: latent_pi, mu and log_std under SB3's names.
    forward(features) -> (mean [B, A], log_std [B, A]), log_std unclamped (DeviceSquashedDiagGaussian clamps it): one tower whose last layer
    has the two row blocks mu and log_std, ONE launch.  Initialisation is nn.Linear's, as in SB3."""

    def __init__(self, features_dim, action_dim, net_arch, activation_fn=nn.ReLU):
        super().__init__()
        self.features_dim, self.action_dim, self.act = int(features_dim), int(action_dim), _act_of(activation_fn)
        if not 1 <= self.features_dim <= capi.MLP_MAX_IN:
            raise ValueError(f"features_dim={features_dim}: 1 to {capi.MLP_MAX_IN} are built")
        if not 1 <= 2 * self.action_dim <= capi.MLP_MAX_WIDTH:
            raise ValueError(f"action_dim={action_dim}: mu and log_std together are wider than {capi.MLP_MAX_WIDTH}, which is not built")
        self.latent_pi, width = _sequential(self.features_dim, _widths(net_arch, "net_arch"), activation_fn)
        self.mu = nn.Linear(width, self.action_dim)
        self.log_std = nn.Linear(width, self.action_dim)

    def forward(self, features):
        tower = _linears(self.latent_pi, self.act) + [(self.mu, "none", self.log_std)]   # made per call: a replaced submodule is the one that runs
        return _module_call(features, self.features_dim, [tower])[0]


class ContinuousCriticHeads(nn.Module):
    """stable_baselines3's ContinuousCritic behind its features extractor: qf0, qf1, ... = create_mlp(features_dim + action_dim, 1, net_arch)
    under SB3's names.  forward(features [B, features_dim], actions [B, A]) -> a tuple of n_critics tensors [B, 1]: n_critics towers on the
    two column blocks (no torch.cat), ONE launch.  Initialisation is nn.Linear's, as in SB3."""

    def __init__(self, features_dim, action_dim, net_arch, activation_fn=nn.ReLU, n_critics=2):
        super().__init__()
        self.features_dim, self.action_dim, self.act, self.n_critics = int(features_dim), int(action_dim), _act_of(activation_fn), int(n_critics)
        if not 1 <= self.n_critics <= capi.MLP_MAX_TOWERS:
            raise ValueError(f"n_critics={n_critics}: 1 to {capi.MLP_MAX_TOWERS} run in one call")
        if self.features_dim < 1 or self.action_dim < 1 or self.features_dim + self.action_dim > capi.MLP_MAX_IN:
            raise ValueError(f"features_dim + action_dim = {self.features_dim + self.action_dim}: 2 to {capi.MLP_MAX_IN} are built")
        widths = _widths(net_arch, "net_arch")
        for i in range(self.n_critics):
            self.add_module(f"qf{i}", _sequential(self.features_dim + self.action_dim, widths, activation_fn, 1)[0])

    def forward(self, features, actions):
        towers = [_linears(getattr(self, f"qf{i}"), self.act) for i in range(self.n_critics)]
        return tuple(_module_call((features, actions), self.features_dim + self.action_dim, towers))
