"""Reference of tactile_gym_amd.augment (csrc/tg_augment.hip), in two independent parts.

kornia path: what kornia.augmentation.RandomAffine(degrees=0, translate, scale=(1, 1), p) does to a batch once its parameters are drawn, restated
from kornia's source (warp_affine: normal_transform_pixel normalises the pixel translation with 2 / (W - 1), the matrix is inverted, then
F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False)), in float64 on the CPU; samples that are not applied are passed through.

Restatement: the device arithmetic itself in numpy float32 (every operation one float32 rounding, no fused multiply-add), including the
counter-based draws of tg_sample_actions' generator (SplitMix64's mix64).  The device output must equal it bit for bit.
"""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64_int(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix64(z):
    """SplitMix64's finaliser over a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, counter, n):
    """u_i = (float)(uint32_t)(z >> 40) * 2^-24 for i < n, z = mix64(mix64(seed + G (counter + 1)) + G (i + 1)): float32 [n]."""
    head = mix64_int((seed + GOLDEN * (counter + 1)) & M64)
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = mix64(np.uint64(head) + np.uint64(GOLDEN) * (i + np.uint64(1)))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def draw_params(seed, counter, B, translate, p, H, W):
    """float32 [B, 3] (apply, tx, ty) as the kernel draws them: element 3 b + k."""
    ax, ay = translate
    u = uniforms(seed, counter, 3 * B).reshape(B, 3)
    apply = u[:, 0] < np.float32(p)
    tx = np.float32(ax * W) * (np.float32(2) * u[:, 1] - np.float32(1))
    ty = np.float32(ay * H) * (np.float32(2) * u[:, 2] - np.float32(1))
    return np.stack([apply.astype(np.float32), tx, ty], axis=1).astype(np.float32)


def split_shift(t, n):
    """(o, f): o = floor(-s), f = (float32)(-s - o), s = t n / (n - 1) in float64; -s clamped to [-(n + 2), n + 2] (NaN: -(n + 2))."""
    s = np.float64(t) * n / (n - 1)
    m = -s
    m = -(n + 2.0) if np.isnan(m) else min(max(m, -(n + 2.0)), n + 2.0)
    o = np.floor(m)
    return int(o), np.float32(m - o)


def _shifted(img, oy, ox):
    """img [C, H, W] -> out[c, y, x] = img[c, y + oy, x + ox], 0 outside."""
    C, H, W = img.shape
    out = np.zeros_like(img)
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = img[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def warp_f32(x, params, channels_first=True):
    """The device arithmetic: x uint8 / float32 [B, C, H, W] (or [B, H, W, C]), params [B, 3] -> float32, same layout."""
    x = np.asarray(x)
    xf = x.astype(np.float32)
    if not channels_first:
        xf = xf.transpose(0, 3, 1, 2)
    B, C, H, W = xf.shape
    out = xf.copy()
    one = np.float32(1)
    for b in range(B):
        if params[b, 0] == 0:
            continue
        ox, fx = split_shift(params[b, 1], W)
        oy, fy = split_shift(params[b, 2], H)
        a, bb = _shifted(xf[b], oy, ox), _shifted(xf[b], oy, ox + 1)
        c, d = _shifted(xf[b], oy + 1, ox), _shifted(xf[b], oy + 1, ox + 1)
        h0 = (one - fx) * a + fx * bb
        h1 = (one - fx) * c + fx * d
        out[b] = (one - fy) * h0 + fy * h1
    if not channels_first:
        out = out.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out, dtype=np.float32)


def warp_f32_batched(x, params, channels_first=True):
    """warp_f32 with the loop over samples turned into array operations - per element the same float32 operations in the same order - for
    batches of millions of tiny images, where a Python loop over samples does not end.  tests/test_augment_paths_cpu.py holds it to warp_f32
    bit for bit."""
    xf = np.asarray(x).astype(np.float32)
    if not channels_first:
        xf = xf.transpose(0, 3, 1, 2)
    B, C, H, W = xf.shape
    prm = np.asarray(params, dtype=np.float32)

    def split(t, n):
        with np.errstate(invalid="ignore", over="ignore"):
            m = -(t.astype(np.float64) * n / (n - 1))
            m = np.where(np.isnan(m), -(n + 2.0), np.minimum(np.maximum(m, -(n + 2.0)), n + 2.0))
        o = np.floor(m)
        return o.astype(np.int64), (m - o).astype(np.float32)

    ox, fx = split(prm[:, 1], W)
    oy, fy = split(prm[:, 2], H)
    bi = np.arange(B)[:, None, None]

    def tap(dy, dx):
        yy = np.arange(H)[None, :, None] + (oy + dy)[:, None, None]
        xx = np.arange(W)[None, None, :] + (ox + dx)[:, None, None]
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = xf[bi, :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]                # [B, H, W, C]
        return np.where(ok[..., None], v, np.float32(0)).transpose(0, 3, 1, 2)

    one = np.float32(1)
    fx, fy = fx[:, None, None, None], fy[:, None, None, None]
    h0 = (one - fx) * tap(0, 0) + fx * tap(0, 1)
    h1 = (one - fx) * tap(1, 0) + fx * tap(1, 1)
    out = (one - fy) * h0 + fy * h1
    out = np.where((prm[:, 0] == 0)[:, None, None, None], xf, out)
    assert out.dtype == np.float32
    if not channels_first:
        out = out.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out, dtype=np.float32)


def warp_kornia(x, params, channels_first=True):
    """kornia's path in float64 on the CPU: theta = [[1, 0, -2 tx / (W - 1)], [0, 1, -2 ty / (H - 1)]] through affine_grid / grid_sample
    (bilinear, zeros, align_corners=False); samples whose apply flag is 0 are the input.  float64 numpy, same layout."""
    import torch
    import torch.nn.functional as F
    x64 = np.asarray(x).astype(np.float64)
    if not channels_first:
        x64 = x64.transpose(0, 3, 1, 2)
    B, C, H, W = x64.shape
    t = torch.from_numpy(np.ascontiguousarray(x64))
    prm = np.asarray(params, dtype=np.float64)
    theta = torch.zeros((B, 2, 3), dtype=torch.float64)
    theta[:, 0, 0] = 1.0
    theta[:, 1, 1] = 1.0
    theta[:, 0, 2] = torch.from_numpy(-2.0 * prm[:, 1] / (W - 1))
    theta[:, 1, 2] = torch.from_numpy(-2.0 * prm[:, 2] / (H - 1))
    grid = F.affine_grid(theta, (B, C, H, W), align_corners=False)
    out = F.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    keep = torch.from_numpy(prm[:, 0] == 0)
    out[keep] = t[keep]
    out = out.numpy()
    if not channels_first:
        out = out.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)


def tolerance(x):
    """Bound of |restatement - kornia path| for inputs like x: 1e-3 on [0, 255] data, 4e-6 max|x| on [0, 1] data."""
    m = float(np.abs(np.asarray(x, dtype=np.float64)).max()) if np.asarray(x).size else 0.0
    return 1e-3 if m > 1.0 else 4e-6 * max(m, 1e-30)
