"""The device Adam's specification (csrc/tg_optim.h) restated in numpy, and the float64 Adam it is judged against.

device order, every float32 operation rounded once, in this order:
    g'   = g * coef                    (only when clipping)
    g''  = g' + wd * p                 (only when wd != 0)
    m    = m + w1 * (g'' - m)          w1 = (float) (1 - beta1)
    v    = v * b2 + w2 * (g'' * g'')   b2 = (float) beta2, w2 = (float) (1 - beta2)
    den  = sqrt(v) / bc2s + eps        bc2s = (float) sqrt(1 - beta2^step)
    p    = p + ss * (m / den)          ss = (float) (-lr / (1 - beta1^step))
The clip: the tensors are cut into chunks of CHUNK elements (a chunk never spans tensors); a chunk's sum of g^2 is taken in double, lane t of
256 adding elements 4 (256 k + t) + j, k = 0 .. 3 outer, j = 0 .. 3 inner, the lanes by the tree v[i] += v[i + off], off = 32 .. 1 inside each
wave of 64 and the four wave sums in wave order; the chunk sums are added in index order from 0; total = (float) sqrt(sum); coef = max_norm /
(total + 1e-6f) in float32, 1 where that exceeds 1 (a NaN stays, as under torch.clamp).
"""
import math

import numpy as np

CHUNK, MAX_TENSORS = 4096, 64
LANES, VEC, PASSES = 256, 4, 4
f32, f64 = np.float32, np.float64


def chunk_prefix(counts):
    """[first chunk of every tensor ..., the total]."""
    prefix = [0]
    for n in counts:
        prefix.append(prefix[-1] + (int(n) + CHUNK - 1) // CHUNK)
    return prefix


def lane_tree(acc):
    """float64 [..., 256] -> [...]: the workgroup's sum (csrc/tg_loss_core.h)."""
    v = np.asarray(acc, f64).reshape(acc.shape[:-1] + (4, 64)).copy()
    off = 32
    while off >= 1:
        nxt = v.copy()
        nxt[..., :64 - off] = v[..., :64 - off] + v[..., off:]
        v = nxt
        off >>= 1
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def partial_sums(grads):
    """float64 [chunks]: every chunk's sum of squares in the kernel's order, the tensors in list order."""
    out = []
    with np.errstate(all="ignore"):
        for g in grads:
            g = np.asarray(g, f32).reshape(-1)
            chunks = (g.size + CHUNK - 1) // CHUNK
            x = np.zeros(chunks * CHUNK, f64)
            x[:g.size] = g.astype(f64) * g.astype(f64)
            x = x.reshape(chunks, PASSES, LANES, VEC)
            acc = np.zeros((chunks, LANES), f64)
            for k in range(PASSES):
                for j in range(VEC):
                    acc = acc + x[:, k, :, j]
            out.append(lane_tree(acc))
    return np.concatenate(out)


def total_norm(partials):
    """(float) sqrt(((0 + partials[0]) + partials[1]) + ...) as a float32 scalar."""
    s = f64(0.0)
    with np.errstate(all="ignore"):
        for x in np.asarray(partials, f64):
            s = s + x
        return f32(np.sqrt(s))


def clip_coef(total, max_norm):
    with np.errstate(all="ignore"):
        q = f32(max_norm) / (f32(total) + f32(1e-6))
    return f32(1.0) if q > f32(1.0) else q


def corrections(lr, beta1, beta2, step):
    """(ss, bc2s) of a tensor at its step count, computed in double and rounded once."""
    return f32(-lr / (1.0 - beta1 ** step)), f32(math.sqrt(1.0 - beta2 ** step))


def adam_device_order(p, g, m, v, ss, bc2s, beta1, beta2, eps, wd=0.0, coef=None):
    """One tensor's step -> (p, m, v), fresh float32 arrays."""
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    w1, w2, b2, eps, wd, ss, bc2s = f32(1.0 - beta1), f32(1.0 - beta2), f32(beta2), f32(eps), f32(wd), f32(ss), f32(bc2s)
    with np.errstate(all="ignore"):
        if coef is not None:
            g = g * f32(coef)
        if wd != 0:
            g = g + wd * p
        m = m + w1 * (g - m)
        v = v * b2 + w2 * (g * g)
        den = np.sqrt(v) / bc2s + eps
        p = p + ss * (m / den)
    assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32
    return p, m, v


def step_device_order(params, grads, ms, vs, steps, lr, beta1, beta2, eps, wd=0.0, max_norm=None):
    """One optimiser step over lists of tensors (steps: each tensor's count AFTER this step; lr: one float or one per tensor) ->
    (params, ms, vs, total) with total the float32 norm, None without a clip."""
    lrs = list(lr) if isinstance(lr, (list, tuple)) else [lr] * len(params)
    total = coef = None
    if max_norm is not None:
        total = total_norm(partial_sums(grads))
        coef = clip_coef(total, max_norm)
    out = [adam_device_order(p, g, m, v, *corrections(lrs[i], beta1, beta2, steps[i]), beta1, beta2, eps, wd, coef)
           for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs))]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], total


def norm_f64(grads):
    return math.sqrt(math.fsum(float(x) * float(x) for g in grads for x in np.asarray(g, f64).reshape(-1)))


def step_f64(params, grads, ms, vs, steps, lr, beta1, beta2, eps, wd=0.0, max_norm=None):
    """torch.optim.Adam after clip_grad_norm_ in float64 throughout -> (params, ms, vs, total)."""
    lrs = list(lr) if isinstance(lr, (list, tuple)) else [lr] * len(params)
    total, coef = None, 1.0
    if max_norm is not None:
        total = norm_f64(grads)
        coef = min(1.0, max_norm / (total + 1e-6))
    P, M, V = [], [], []
    for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        p, g, m, v = (np.asarray(a, f64) for a in (p, g, m, v))
        g = g * coef + wd * p
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        den = np.sqrt(v) / math.sqrt(1.0 - beta2 ** steps[i]) + eps
        p = p - lrs[i] / (1.0 - beta1 ** steps[i]) * (m / den)
        P.append(p), M.append(m), V.append(v)
    return P, M, V, total
