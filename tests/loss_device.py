"""The device side of the loss kernels' raw-pointer tests (tests/test_gpu_loss_head_abi.py, tests/test_gpu_sac_loss_abi.py,
tests/test_gpu_nonfinite.py): one call of tg_ppo_loss, tg_squashed_rsample, tg_squashed_rsample_bwd, tg_action_head, tg_sac_critic_loss or
tg_sac_actor_loss on buffers between guard bytes, behind its memory checks (guards intact, inputs unchanged, nothing written on an error)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from device_guard import PATTERN, Guarded  # noqa: E402

GAMMA = 0.95
INPUTS = ("mean", "log_std", "values", "actions", "old_log_prob", "advantages", "returns", "old_values")
OUTPUTS = ("stats", "log_prob", "dmean", "dlog_std", "dvalues")
AUTO, ONE, GRID = 0, 1, 2
f32 = np.float32
p = lambda g: C.c_void_p(g.ptr if g is not None else None)   # noqa: E731


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- tg_ppo_loss
def _upload(inp):
    return {k: Guarded(v.nbytes, fill=v) for k, v in inp.items() if v is not None}


def _ppo(inp, dev, kw, path=AUTO, outputs=OUTPUTS, expect_error=False, workspace_bytes=None, **over):
    """One tg_ppo_loss call on the uploaded inputs `dev` -> {output name: host float32 array}.  over: B, A, stride, a missing input (name=None),
    path or a scalar, for the error returns."""
    capi, L = _lib()
    B, A = inp["mean"].shape
    per_row = inp["log_std"].ndim == 2
    sizes = dict(stats=8, log_prob=B, dmean=B * A, dlog_std=B * A if per_row else A, dvalues=B)
    outs = {k: Guarded(4 * sizes[k]) for k in outputs}
    need = int(L.tg_ppo_loss_workspace(B, A))
    assert need == 16 + 8 * ((B + 255) // 256) * (5 + A)
    nbytes = need if workspace_bytes is None else workspace_bytes
    work = Guarded(nbytes)
    clip_vf = kw["clip_range_vf"]
    ptr = {k: p(dev.get(k)) for k in INPUTS}
    if clip_vf is None:
        ptr["old_values"] = p(None)                                           # not read without the clip
    for k in INPUTS:
        if k in over:
            ptr[k] = p(None)
    rc = L.tg_ppo_loss(ptr["mean"], ptr["log_std"], over.get("stride", A if per_row else 0), ptr["values"], ptr["actions"], ptr["old_log_prob"],
                       ptr["advantages"], ptr["returns"], ptr["old_values"], over.get("B", B), over.get("A", A),
                       over.get("clip_range", kw["clip_range"]), -1.0 if clip_vf is None else clip_vf, kw["ent_coef"], kw["vf_coef"],
                       1 if kw["normalize_advantage"] else 0, path, p(outs.get("stats")), p(outs.get("log_prob")), p(outs.get("dmean")),
                       p(outs.get("dlog_std")), p(outs.get("dvalues")), p(None) if over.get("no_workspace") else p(work), nbytes, _stream())
    torch.cuda.synchronize()
    for g in list(dev.values()) + list(outs.values()) + [work]:
        assert g.guards_intact()
    for k, g in dev.items():
        assert _bits(g.host(f32), inp[k].reshape(-1)), k                      # the inputs are unchanged
    if expect_error:
        assert rc != 0 and L.tg_last_error().decode().startswith("tg_ppo_loss:")
        for k, g in outs.items():
            assert bool((g.payload() == PATTERN).all()), k                    # nothing was written
        assert bool((work.payload() == PATTERN).all())
        return None
    capi.check(rc)
    shapes = dict(stats=(8,), log_prob=(B,), dmean=(B, A), dlog_std=(B, A) if per_row else (A,), dvalues=(B,))
    return {k: g.host(f32).reshape(shapes[k]) for k, g in outs.items()}


# ---------------------------------------------------------------------------------------------------------------- tg_action_head, as the heads' tests of the losses use it
def _head(mode, mean, ls, seed, counter, clamp=(-np.inf, np.inf), noise_in=None):
    """tg_action_head -> (actions, log_prob, noise), host float32."""
    capi, L = _lib()
    B, A = mean.shape
    keep = [Guarded(mean.nbytes, fill=mean), Guarded(ls.nbytes, fill=ls)] + ([Guarded(noise_in.nbytes, fill=noise_in)] if noise_in is not None else [])
    outs = [Guarded(4 * B * A), Guarded(4 * B), Guarded(4 * B * A)]
    lo, hi = (C.c_float * A)(*[-1.0] * A), (C.c_float * A)(*[1.0] * A)
    capi.check(L.tg_action_head(p(keep[0]), p(keep[1]), A if ls.ndim == 2 else 0, B, A, lo, hi, clamp[0], clamp[1], mode, 0, seed, counter,
                                p(keep[2]) if noise_in is not None else p(None), p(outs[0]), p(None), p(None), p(outs[1]), p(outs[2]), _stream()))
    torch.cuda.synchronize()
    return outs[0].host(f32).reshape(B, A), outs[1].host(f32), outs[2].host(f32).reshape(B, A)


# ---------------------------------------------------------------------------------------------------------------- tg_squashed_rsample
def _rsample(mean, ls, seed=0, counter=0, noise_in=None, save=True, clamp=(-20.0, 2.0), expect_error=False, null=(), **over):
    capi, L = _lib()
    B, A = mean.shape
    keep = {k: Guarded(v.nbytes, fill=v) for k, v in (("mean", mean), ("ls", ls), ("noise", noise_in)) if v is not None}
    outs = dict(actions=Guarded(4 * B * A), log_prob=Guarded(4 * B))
    if save:
        outs.update(eps=Guarded(4 * B * A), sigma=Guarded(4 * B * A))
    ptr = {k: p(None) if k in null else p(v) for k, v in dict(keep, **outs).items()}
    rc = L.tg_squashed_rsample(ptr["mean"], ptr["ls"], over.get("stride", A if ls.ndim == 2 else 0), over.get("B", B), over.get("A", A), clamp[0],
                               clamp[1], seed, counter, ptr.get("noise", p(None)), ptr["actions"], ptr["log_prob"], ptr.get("eps", p(None)),
                               ptr.get("sigma", p(None)), _stream())
    torch.cuda.synchronize()
    for g in list(keep.values()) + list(outs.values()):
        assert g.guards_intact()
    if expect_error:
        assert rc != 0 and L.tg_last_error().decode().startswith("tg_squashed_rsample:")
        assert all(bool((g.payload() == PATTERN).all()) for g in outs.values())
        return None
    capi.check(rc)
    return {k: g.host(f32).reshape((B,) if k == "log_prob" else (B, A)) for k, g in outs.items()}


def _rsample_bwd(fwd, ls, g_a, g_lp, outputs=("dmean", "dlog_std"), clamp=(-20.0, 2.0), expect_error=False, null=(), **over):
    capi, L = _lib()
    B, A = fwd["actions"].shape
    keep = {k: Guarded(v.nbytes, fill=v) for k, v in (("g_a", g_a), ("g_lp", g_lp), ("actions", fwd["actions"]), ("eps", fwd["eps"]),
                                                      ("sigma", fwd["sigma"]), ("ls", ls)) if v is not None}
    outs = {k: Guarded(4 * B * A) for k in outputs}
    ptr = {k: p(None) if k in null else p(v) for k, v in keep.items()}
    rc = L.tg_squashed_rsample_bwd(ptr.get("g_a", p(None)), ptr.get("g_lp", p(None)), ptr["actions"], ptr["eps"], ptr["sigma"], ptr["ls"],
                                   over.get("stride", A if ls.ndim == 2 else 0), over.get("B", B), over.get("A", A), clamp[0], clamp[1],
                                   p(outs.get("dmean")), p(outs.get("dlog_std")), _stream())
    torch.cuda.synchronize()
    for g in list(keep.values()) + list(outs.values()):
        assert g.guards_intact()
    if expect_error:
        assert rc != 0 and L.tg_last_error().decode().startswith("tg_squashed_rsample_bwd:")
        assert all(bool((g.payload() == PATTERN).all()) for g in outs.values())
        return None
    capi.check(rc)
    return {k: g.host(f32).reshape(B, A) for k, g in outs.items()}


# ---------------------------------------------------------------------------------------------------------------- tg_sac_critic_loss, tg_sac_actor_loss
def _array(guards, null=()):
    """A host array of device pointers; null: positions passed as NULL."""
    return (C.c_void_p * max(1, len(guards)))(*[None if (g is None or k in null) else g.ptr for k, g in enumerate(guards)])


def _flat(inp, src):
    """name -> float32 array for every device input of a call."""
    out = {}
    for k, v in inp.items():
        if isinstance(v, list):
            out.update({f"{k}{i}": q for i, q in enumerate(v)})
        else:
            out[k] = v
    if "log_ent_coef" in src:
        out["log_ent_coef"] = np.array([src["log_ent_coef"]], f32)
    return out


def _finish(L, rc, entry, flat, dev, outs, expect_error):
    torch.cuda.synchronize()
    for g in list(dev.values()) + list(outs.values()):
        assert g.guards_intact()
    for k, g in dev.items():
        assert _bits(g.host(f32), flat[k].reshape(-1)), k                     # the inputs are unchanged
    if expect_error:
        assert rc != 0 and L.tg_last_error().decode().startswith(entry + ":")
        for k, g in outs.items():
            assert bool((g.payload() == PATTERN).all()), k                    # nothing was written
        return True
    return False


def _critic(inp, src, outputs=None, expect_error=False, null=(), **over):
    """One tg_sac_critic_loss call -> dict(stats [8], target [B], dq_cur [n, B]) of the outputs asked (dq_cur rows not asked: absent from
    "dq" names).  outputs: a subset of ("target", "dq_cur0", ...); null: inputs or arrays passed as NULL; over: B, n."""
    capi, L = _lib()
    n, B = len(inp["q_cur"]), inp["rewards"].shape[0]
    names = ("target",) + tuple(f"dq_cur{i}" for i in range(n))
    outputs = names if outputs is None else outputs
    flat = _flat(inp, src)
    dev = {k: Guarded(v.nbytes, fill=v) for k, v in flat.items()}
    outs = {"stats": Guarded(32)}
    outs.update({k: Guarded(4 * B) for k in outputs})
    ptr = {k: p(None) if k in null else p(g) for k, g in dev.items()}
    q_cur = _array([dev[f"q_cur{i}"] for i in range(n)], [i for i in range(n) if f"q_cur{i}" in null])
    q_next = _array([dev[f"q_next{i}"] for i in range(n)], [i for i in range(n) if f"q_next{i}" in null])
    dq = _array([outs.get(f"dq_cur{i}") for i in range(n)])
    rc = L.tg_sac_critic_loss(None if "q_cur" in null else q_cur, None if "q_next" in null else q_next, over.get("n", n), ptr["next_log_prob"],
                              ptr["rewards"], ptr["dones"], over.get("B", B), GAMMA if "gamma" not in over else over["gamma"],
                              ptr.get("log_ent_coef", p(None)), src.get("ent_coef", 0.0), p(None) if "stats" in null else p(outs["stats"]),
                              p(outs.get("target")), dq if any(k.startswith("dq") for k in outputs) else None, _stream())
    if _finish(L, rc, "tg_sac_critic_loss", flat, dev, outs, expect_error):
        return None
    capi.check(rc)
    return {k: g.host(f32) for k, g in outs.items()}


def _actor(inp, src, target_entropy=None, outputs=None, expect_error=False, null=(), **over):
    """One tg_sac_actor_loss call -> dict(stats [8], dlog_prob [B], dq_pi0 .. [B])."""
    capi, L = _lib()
    n, B = len(inp["q_pi"]), inp["log_prob"].shape[0]
    names = ("dlog_prob",) + tuple(f"dq_pi{i}" for i in range(n))
    outputs = names if outputs is None else outputs
    flat = _flat(inp, src)
    dev = {k: Guarded(v.nbytes, fill=v) for k, v in flat.items()}
    outs = {"stats": Guarded(32)}
    outs.update({k: Guarded(4 * B) for k in outputs})
    ptr = {k: p(None) if k in null else p(g) for k, g in dev.items()}
    q_pi = _array([dev[f"q_pi{i}"] for i in range(n)], [i for i in range(n) if f"q_pi{i}" in null])
    dq = _array([outs.get(f"dq_pi{i}") for i in range(n)])
    want = over.get("want", target_entropy is not None)
    rc = L.tg_sac_actor_loss(ptr["log_prob"], None if "q_pi" in null else q_pi, over.get("n", n), over.get("B", B), ptr.get("log_ent_coef", p(None)),
                             src.get("ent_coef", 0.0), 0.0 if target_entropy is None else target_entropy, 1 if want else 0,
                             p(None) if "stats" in null else p(outs["stats"]), p(outs.get("dlog_prob")),
                             dq if any(k.startswith("dq_pi") for k in outputs) else None, _stream())
    if _finish(L, rc, "tg_sac_actor_loss", flat, dev, outs, expect_error):
        return None
    capi.check(rc)
    return {k: g.host(f32) for k, g in outs.items()}
