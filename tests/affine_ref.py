"""Reference of tactile_gym_amd.augment's general affine warp (csrc/tg_affine.hip), stage by stage.

draw_params: stage (a), the device's float32 draws restated in numpy (one rounding per operation) - bit for bit.
coeffs_f64:  stage (b) in float64 by matrices and numpy's inverse (the device uses a closed form): the device's float32 coefficients must be
             one rounding away.
warp_f32:    stage (c), the device's float32 warp restated in numpy, vectorised over the batch - bit for bit.
warp_torch:  the geometry checked against torch on the CPU: F.affine_grid(theta = N M^-1 N^-1) + F.grid_sample(bilinear, zeros,
             align_corners=False) in float64, N the (n - 1) normalisation of kornia's warp_affine; samples that are not applied pass through.
             (The pattern of augment_ref.warp_kornia.)
"""
import numpy as np

from augment_ref import uniforms

F32 = np.float32


def draw_params(seed, counter, B, degrees, translate, scale, shear, p, H, W):
    """float32 [B, 8] (apply, tx, ty, angle, scale_x, scale_y, shear_x, shear_y) as the kernel draws them: u_k = element 8 b + k.
    degrees (d0, d1); translate (ax, ay); scale (s0, s1) or (s0, s1, s2, s3); shear (h0, h1, h2, h3): already normalised."""
    d0, d1 = (F32(v) for v in degrees)
    ax, ay = translate
    sc = [F32(v) for v in scale]
    h0, h1, h2, h3 = (F32(v) for v in shear)
    u = uniforms(seed, counter, 8 * B).reshape(B, 8)
    apply = (u[:, 0] < F32(p)).astype(F32)
    tx = F32(ax * W) * (F32(2) * u[:, 1] - F32(1))
    ty = F32(ay * H) * (F32(2) * u[:, 2] - F32(1))
    angle = d0 + (d1 - d0) * u[:, 3]
    sx = sc[0] + (sc[1] - sc[0]) * u[:, 4]
    sy = sc[2] + (sc[3] - sc[2]) * u[:, 5] if len(sc) == 4 else sx
    shx = h0 + (h1 - h0) * u[:, 6]
    shy = h2 + (h3 - h2) * u[:, 7]
    out = np.stack([apply, tx, ty, angle, sx, sy, shx, shy], axis=1)
    assert out.dtype == F32
    return out


def forward_matrix(params, H, W):
    """M [B, 3, 3] in pixel coordinates (x right, y down): M(q) = L Sh (q - c) + c + t, L = R(angle) diag(scale), c the image centre."""
    prm = np.asarray(params, dtype=np.float64)
    B = prm.shape[0]
    tx, ty, ang, scx, scy, shx, shy = (prm[:, k] for k in range(1, 8))
    a = np.deg2rad(ang)
    L = np.zeros((B, 2, 2))
    L[:, 0, 0], L[:, 0, 1] = np.cos(a) * scx, -np.sin(a) * scy
    L[:, 1, 0], L[:, 1, 1] = np.sin(a) * scx, np.cos(a) * scy
    tsx, tsy = np.tan(np.deg2rad(shx)), np.tan(np.deg2rad(shy))
    Sh = np.zeros((B, 2, 2))
    Sh[:, 0, 0], Sh[:, 0, 1] = 1.0, -tsx
    Sh[:, 1, 0], Sh[:, 1, 1] = -tsy, 1.0 + tsx * tsy
    A = L @ Sh
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    M = np.zeros((B, 3, 3))
    M[:, :2, :2] = A
    M[:, :2, 2] = c + prm[:, 1:3] - A @ c
    M[:, 2, 2] = 1.0
    return M


def coeffs_f64(params, H, W):
    """float64 [B, 6] (a00, a01, a02, a10, a11, a12): src = K M^-1 P (j + 1/2, i + 1/2) - 1/2 as a matrix product."""
    Minv = np.linalg.inv(forward_matrix(params, H, W))
    half = np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    unhalf = np.array([[1.0, 0.0, -0.5], [0.0, 1.0, -0.5], [0.0, 0.0, 1.0]])
    P = np.diag([(W - 1.0) / W, (H - 1.0) / H, 1.0])
    K = np.diag([W / (W - 1.0), H / (H - 1.0), 1.0])
    T = unhalf @ K @ Minv @ P @ half
    return np.ascontiguousarray(T[:, :2, :].reshape(-1, 6))


def warp_f32(x, coeffs, apply=None, channels_first=True):
    """The device arithmetic of stage (c): x uint8 / float32 [B, C, H, W] (or [B, H, W, C]), coeffs float32 [B, 6], apply [B] (None: all) ->
    float32, same layout.  Every operation is one float32 rounding, in the kernel's order."""
    xf = np.asarray(x).astype(F32)
    if not channels_first:
        xf = xf.transpose(0, 3, 1, 2)
    B, C, H, W = xf.shape
    co = np.asarray(coeffs)
    assert co.dtype == F32 and co.shape == (B, 6)
    k = [co[:, q][:, None, None] for q in range(6)]
    jf = np.arange(W, dtype=F32)[None, None, :]
    yf = np.arange(H, dtype=F32)[None, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (k[0] * jf + k[1] * yf) + k[2]
        sy = (k[3] * jf + k[4] * yf) + k[5]
        ok = (sx > F32(-1)) & (sx < F32(W)) & (sy > F32(-1)) & (sy < F32(H))      # false for NaN
    assert sx.dtype == F32 and sy.dtype == F32
    sx, sy = np.where(ok, sx, F32(0)), np.where(ok, sy, F32(0))
    flx, fly = np.floor(sx), np.floor(sy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    fx, fy = (sx - flx)[:, None], (sy - fly)[:, None]
    flat = xf.reshape(B, C, H * W)

    def tap(dy, dx):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        idx = (np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1)).reshape(B, 1, H * W)
        v = np.take_along_axis(flat, idx, axis=2).reshape(B, C, H, W)
        return np.where(inside[:, None], v, F32(0))

    one = F32(1)
    h0 = (one - fx) * tap(0, 0) + fx * tap(0, 1)
    h1 = (one - fx) * tap(1, 0) + fx * tap(1, 1)
    out = (one - fy) * h0 + fy * h1
    out = np.where(ok[:, None], out, F32(0))
    if apply is not None:
        out = np.where((np.asarray(apply) == 0)[:, None, None, None], xf, out)
    assert out.dtype == F32
    if not channels_first:
        out = out.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)


def warp_torch(x, params, channels_first=True):
    """torch's path in float64 on the CPU: theta = N M^-1 N^-1 through affine_grid / grid_sample (bilinear, zeros, align_corners=False);
    samples whose apply flag is 0 are the input.  float64 numpy, same layout."""
    import torch
    import torch.nn.functional as F
    x64 = np.asarray(x).astype(np.float64)
    if not channels_first:
        x64 = x64.transpose(0, 3, 1, 2)
    B, C, H, W = x64.shape
    prm = np.asarray(params, dtype=np.float64)
    N = np.array([[2.0 / (W - 1), 0.0, -1.0], [0.0, 2.0 / (H - 1), -1.0], [0.0, 0.0, 1.0]])
    theta = N @ np.linalg.inv(forward_matrix(prm, H, W)) @ np.linalg.inv(N)
    t = torch.from_numpy(np.ascontiguousarray(x64))
    grid = F.affine_grid(torch.from_numpy(np.ascontiguousarray(theta[:, :2, :])), (B, C, H, W), align_corners=False)
    out = F.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    keep = torch.from_numpy(prm[:, 0] == 0)
    out[keep] = t[keep]
    out = out.numpy()
    if not channels_first:
        out = out.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)
