"""Case table of the scene camera kernel (csrc/tg_scene.hip: k_scene), plain numpy, deterministic from seeds: small scenes, each aimed at one
branch of the kernel at the smallest shape where the branch exists.  tests/test_scene_cases_cpu.py shows by a census (a numpy restatement
of the kernel's box rule and thresholds) that every case reaches the branch it is named for;
tests/test_gpu_scene_matrix.py draws every case on the device (tg_selftest_scene) and asks for the oracle's bytes.

Coordinates are eye space: the view is the identity, so xf holds the frames themselves (eye <- frame, [R row-major | t]) and light_eye is
the light.  The camera looks along -z, w = -z; window x = W/2 + k x / w, y = H/2 - k y / w with k = (H / 2) / tan(fov / 2).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

FOV, NEAR, FAR = 60.0, 0.1, 10.0
LIGHT = (np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])).astype(np.float32)
BACKGROUND = (178, 178, 204)
SIZES = [(64, 64), (128, 128), (256, 256), (128, 256), (256, 128), (48, 80)]     # (H, W)
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
f32 = np.float32


def focal(H, fov=FOV):
    return f32((1.0 / math.tan(0.5 * fov * (math.pi / 180.0))) * 0.5 * H)


def unproject(px, py, w, H, W, fov=FOV):
    """Eye-space point that lands on window position (px, py) at eye depth w."""
    k = float(focal(H, fov))
    px, py, w = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(w, np.float64))
    return np.stack([(px - 0.5 * W) * w / k, (0.5 * H - py) * w / k, -w], -1)


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def xform(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(np.float32)


def to_frame(p_eye, xf):
    """Frame coordinates (float32) of eye-space points under the eye <- frame transform xf [12]."""
    R, t = xf[:9].astype(np.float64).reshape(3, 3), xf[9:].astype(np.float64)
    return ((np.asarray(p_eye, np.float64) - t) @ np.linalg.inv(R).T).astype(np.float32)


class Builder:
    """Collects triangles given in eye space (as env 0 sees them) into an indexed set in frame coordinates."""

    def __init__(self, xf0):
        self.xf0, self.v, self.f, self.c = xf0, [], [], []

    def add(self, tri_eye, frame, rgb):
        t = np.asarray(tri_eye, np.float64).reshape(-1, 3, 3)
        self.v.append(to_frame(t.reshape(-1, 3), self.xf0[frame]).reshape(-1, 3, 3))
        self.f.append(np.full(len(t), frame, np.uint8))
        self.c.append(np.broadcast_to(np.asarray(rgb, np.uint8), (len(t), 3)).copy())

    def add_local(self, tri_local, frame, rgb):
        t = np.asarray(tri_local, np.float32).reshape(-1, 3, 3)
        self.v.append(t); self.f.append(np.full(len(t), frame, np.uint8))
        self.c.append(np.broadcast_to(np.asarray(rgb, np.uint8), (len(t), 3)).copy())

    def arrays(self):
        v = np.concatenate(self.v).reshape(-1, 3).astype(np.float32)
        return v, np.arange(len(v), dtype=np.int32).reshape(-1, 3), np.concatenate(self.f), np.concatenate(self.c)


def make_case(name, H, W, verts, tris, tri_frame, tri_rgb, xf, hf=None, spheres=None, fov=FOV, near=NEAR, far=FAR, **notes):
    xf = np.ascontiguousarray(xf, np.float32)
    return SimpleNamespace(name=name, H=H, W=W, verts=np.ascontiguousarray(verts, np.float32).reshape(-1, 3),
                           tris=np.ascontiguousarray(tris, np.int32).reshape(-1, 3), tri_frame=np.ascontiguousarray(tri_frame, np.uint8),
                           tri_rgb=np.ascontiguousarray(tri_rgb, np.uint8).reshape(-1, 3), xf=xf, n=xf.shape[0], n_frames=xf.shape[1], hf=hf,
                           spheres=None if spheres is None else np.ascontiguousarray(spheres, np.float32), fov=fov, near=near, far=far,
                           light=LIGHT, background=BACKGROUND, notes=notes)


def rgbs(rng, n):
    return rng.integers(30, 256, (n, 3)).astype(np.uint8)


def right_tri(x0, y0, bw, bh, w, H, W):
    """Right triangle whose pixel box is exactly [x0, x0 + bw) x [y0, y0 + bh) (corners a quarter pixel inside the box rule's thresholds)."""
    return unproject([x0 + 0.25, x0 + bw - 0.25, x0 + 0.25], [y0 + 0.25, y0 + 0.25, y0 + bh - 0.25], w, H, W)


def _frames_xf(rng, n_frames, n, jitter=0.004, scales=None):
    """[n][n_frames][12]: frame 0 the identity in every env (the product's world frame), the others rigid (x scale), moved a little per env."""
    xf = np.zeros((n, n_frames, 12), np.float32)
    base = [(np.eye(3), np.zeros(3))] + [(rot(0, rng.normal(0, 0.4)) @ rot(1, rng.normal(0, 0.4)) @ rot(2, rng.normal(0, 1.0)), rng.normal(0, 0.05, 3))
                                         for _ in range(n_frames - 1)]
    for e in range(n):
        for f, (R, t) in enumerate(base):
            s = 1.0 if scales is None else scales.get(f, 1.0)
            d = np.zeros(3) if f == 0 or e == 0 else rng.normal(0, jitter, 3)
            Re = R if f == 0 or e == 0 else R @ rot(2, rng.normal(0, 0.01))
            xf[e, f] = xform(Re * s, t + d)
    return xf


def _dust_tris(rng, H, W, n_small, n_mid, region):
    """Eye-space sub-pixel triangles and a sprinkle of triangles a few pixels across, spread over region = (x0, y0, x1, y1) in pixels."""
    out = []
    for n, lo, hi, w0, w1 in ((n_small, 0.8, 1.6, 0.5, 1.0), (n_mid, 4.5, 6.5, 2.0, 3.0)):     # the dust in front: its float32 depths are coarse
        cx, cy = rng.uniform(region[0], region[2], n), rng.uniform(region[1], region[3], n)
        w = rng.uniform(w0, w1, n)
        off = rng.uniform(-0.5, 0.5, (n, 3, 2)) * rng.uniform(lo, hi, (n, 1, 1))
        dw = rng.uniform(-0.002, 0.002, (n, 3))
        out.append(unproject(cx[:, None] + off[..., 0], cy[:, None] + off[..., 1], w[:, None] + dw, H, W))
    return out


def dust(H, W, seed=1):
    """Dense dust inside the first tile (enough survivors there to flush both wave queues), thin dust over the whole image and a margin
    around it.  (Dense everywhere would tell no more, and a sub-pixel triangle's float32 edge functions get noisier with the square of the
    image side, which tests/scene_f64.py has to leave out.)"""
    rng = np.random.default_rng(seed)
    tw, th = min(W, 128), min(H, 128)
    dense = _dust_tris(rng, H, W, 1700, 1750, (0, 0, tw, th))        # about 1150 survivors in each wave queue: the census wants > 1008
    thin = _dust_tris(rng, H, W, *((500, 250) if (W > tw or H > th) else (150, 80)), (-0.1 * W, -0.1 * H, 1.1 * W, 1.1 * H))
    small, mid = np.concatenate([dense[0], thin[0]]), np.concatenate([dense[1], thin[1]])
    xf = _frames_xf(rng, 5, 2)
    b = Builder(xf[0])
    for part in (small, mid):
        px = 0.5 * W + float(focal(H)) * part[:, 0, 0] / -part[:, 0, 2]
        fr = 1 + np.clip((4 * px / tw).astype(int) % 4, 0, 3)
        fr[::10] = 0
        for f in range(5):
            b.add(part[fr == f], f, rgbs(rng, int((fr == f).sum())))
    return make_case("dust", H, W, *b.arrays(), xf)


def areas(H=256, W=256, seed=2):
    rng = np.random.default_rng(seed)
    boxes = [(10, 10, 2, 2), (20, 10, 5, 1), (30, 10, 8, 8), (45, 10, 13, 5), (10, 30, 64, 64), (10, 180, 65, 64), (150, 150, 1, 1), (160, 150, 2, 1),
             # straddling the tile border at x = 128: 8 + 8 columns (64 | 64), 9 + 7 (72 | 56), 64 + 64 x 64 rows (4096 | 4096), 65 + 65 (4160 | 4160)
             (120, 100, 16, 8), (119, 112, 16, 8), (64, 4, 128, 64), (63, 70, 130, 64),
             # ... at y = 128, and all four tiles
             (200, 120, 8, 16), (212, 119, 8, 16), (180, 63, 64, 130), (124, 124, 8, 8), (90, 90, 76, 76)]
    xf = _frames_xf(rng, 3, 2, jitter=0.0)
    b = Builder(xf[0])
    for i, (x0, y0, bw, bh) in enumerate(boxes):
        b.add(right_tri(x0, y0, bw, bh, 1.0 + 0.05 * i, H, W), i % 3, rgbs(rng, 1))
    return make_case("areas", H, W, *b.arrays(), xf, boxes=boxes)


def _widths(name, H, W, widths, rows_of):
    """One triangle per clipped box width k, clipped by the right image edge, stacked down a strip of many image heights; env e shows the
    e-th window of the strip (the frame is shifted by 150 rows per env at depth 1)."""
    rng = np.random.default_rng(7)
    k_f = float(focal(H))
    D = 150.0 / k_f
    slots, e, y = [], 0, 0
    for k in widths:
        h = rows_of(k)
        if y + h > H:
            e, y = e + 1, 0
        slots.append((k, h, e, y))
        y += h
    n = e + 1
    xf = np.zeros((n, 2, 12), np.float32)
    for i in range(n):
        xf[i, 0], xf[i, 1] = IDENT, xform(np.eye(3), (0.0, i * D, 0.0))
    tri, col = [], rgbs(rng, len(slots))
    for (k, h, e, y) in slots:
        w = 1.0 + 0.01 * k / 128.0
        p = unproject([W - k + 0.25, W - k + 0.25, W + 3000.0], [y + 0.25, y + h - 0.25, y + 0.5 * h], w, H, W)
        p[:, 1] -= e * D
        tri.append(p)
    b = Builder(xf[0])
    b.add_local(np.asarray(tri, np.float32), 1, col)
    return make_case(name, H, W, *b.arrays(), xf, slots=slots)


def widths_wave(H=128, W=128):
    return _widths("widths_wave", H, W, range(1, 129), lambda k: min(128, max(2, -(-200 // k))))


def widths_group(H=128, W=128):
    return _widths("widths_group", H, W, range(33, 129), lambda k: min(128, -(-4097 // k) + 1))


def huge_overflow(H=128, W=128, count=96):
    rng = np.random.default_rng(3)
    depth = 1.0 + 0.02 * rng.permutation(count)
    b = Builder(np.stack([IDENT]))
    for i in range(count):
        y = 0.6 * i
        b.add(unproject([2.25, 120.75, 120.75], [y + 0.25, y + 70.0, y + 72.75], depth[i], H, W), 0, rgbs(rng, 1))
    return make_case("huge_overflow", H, W, *b.arrays(), np.stack([IDENT])[None])


def big_overflow(H=128, W=128, count=2200):
    rng = np.random.default_rng(4)
    b = Builder(np.stack([IDENT, IDENT]))
    x0, y0 = rng.integers(0, W - 9, count), rng.integers(0, H - 8, count)
    for i in range(count):
        b.add(right_tri(x0[i], y0[i], 9, 8, 1.0 + 2.0 * rng.random(), H, W), i & 1, rgbs(rng, 1))
    return make_case("big_overflow", H, W, *b.arrays(), np.stack([IDENT, IDENT])[None])


def sphere_rows(rng, n, ns, H, W):
    """[n][ns][8] translucent spheres inside the picture."""
    sp = np.zeros((n, ns, 8), np.float32)
    for e in range(n):
        for s in range(ns):
            w = rng.uniform(0.6, 2.0)
            sp[e, s, :3] = unproject(rng.uniform(0.1 * W, 0.9 * W), rng.uniform(0.1 * H, 0.9 * H), w, H, W)
            sp[e, s, 3] = rng.uniform(0.02, 0.08) * w
            sp[e, s, 4:7] = rng.uniform(0, 255, 3)
            sp[e, s, 7] = rng.choice([0.5, 0.75, 1.0])
    return sp


MANY_CLUSTERS = 6960


def many_chunks(clusters=MANY_CLUSTERS, name="many_chunks", H=128, W=128):
    """A line of `clusters` clusters of 8 tiny triangles, 3 cm apart along x: build_scene_chunks ends a chunk after 8 triangles when the next
    one would quadruple its extent, so every cluster is a chunk of its own.  Plus 200 triangles with boxes of 72 pixels and 16 spheres."""
    rng = np.random.default_rng(5)
    xf = np.stack([IDENT, IDENT, xform(np.eye(3), (0.0, 0.05, -2.0))])[None]
    b = Builder(xf[0])
    x0, y0 = rng.integers(0, W - 9, 200), rng.integers(0, H - 8, 200)
    for i in range(200):
        b.add(right_tri(x0[i], y0[i], 9, 8, 1.0 + 2.0 * rng.random(), H, W), 1, rgbs(rng, 1))
    cx = (np.arange(clusters) - clusters // 2)[:, None] * 0.03 + np.arange(8)[None, :] * 1e-4
    t = np.zeros((clusters, 8, 3, 3), np.float32)
    t[..., 0] = cx[..., None]
    t[:, :, 1, 0] += 8e-4
    t[:, :, 2, 1] = 8e-4
    b.add_local(t.reshape(-1, 3, 3), 2, rgbs(rng, clusters * 8))
    return make_case(name, H, W, *b.arrays(), xf, spheres=sphere_rows(rng, 1, 16, H, W))


def view_frame(target, dist, yaw_deg, pitch_deg):
    """eye <- world of Bullet's computeViewMatrixFromYawPitchRoll (roll 0, z up), as a frame."""
    y, p = math.radians(yaw_deg), math.radians(pitch_deg)
    E = rot(2, y) @ rot(0, p)
    eye = np.asarray(target, np.float64) + E @ np.array([0.0, -float(dist), 0.0])
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, E @ np.array([0.0, 0.0, 1.0]))
    s /= np.linalg.norm(s)
    V = np.stack([s, np.cross(s, f), -f])
    return xform(V, -V @ eye)


def planes(H, W, seed=6):
    """Dust, and among it triangles that cross the near plane (one or two corners at w < near, w < 0 included), cross the far plane, lie wholly
    before near / beyond far, have a corner at w == near exactly; and the 200 m ground plane of tests/test_oracle_scene.py under its camera."""
    rng = np.random.default_rng(seed)
    small, mid = _dust_tris(rng, H, W, 500, 200, (-0.1 * W, -0.1 * H, 1.1 * W, 1.1 * H))
    xf = np.stack([np.stack([IDENT, view_frame([0.35, 0.0, -0.25], 0.75, 90.0, -35.0), xform(rot(2, 0.3), (0.01 * e, 0.0, 0.0))]) for e in range(2)])
    b = Builder(xf[0])
    b.add(small, 2, rgbs(rng, len(small))); b.add(mid[::2], 2, rgbs(rng, len(mid[::2]))); b.add(mid[1::2], 0, rgbs(rng, len(mid[1::2])))
    P = lambda px, py, w: unproject(px, py, w, H, W)[None] if w > 0 else np.array([[(px - 0.5 * W) / W, (0.5 * H - py) / H, -w]])
    special = [[P(0.2 * W, 0.8 * H, 0.05), P(0.5 * W, 0.3 * H, 1.0), P(0.7 * W, 0.7 * H, 1.5)],          # one corner before near
               [P(0.6 * W, 0.2 * H, -0.5), P(0.8 * W, 0.4 * H, 1.0), P(0.9 * W, 0.1 * H, 2.0)],          # one corner behind the eye
               [P(0.1 * W, 0.1 * H, 0.05), P(0.3 * W, 0.2 * H, -0.3), P(0.2 * W, 0.5 * H, 1.2)],         # two corners before near
               [P(0.3 * W, 0.6 * H, 9.0), P(0.6 * W, 0.9 * H, 11.0), P(0.4 * W, 0.95 * H, 12.0)],        # crossing far
               [P(0.5 * W, 0.5 * H, 0.05), P(0.6 * W, 0.5 * H, 0.09), P(0.5 * W, 0.6 * H, 0.07)],        # wholly before near
               [P(0.5 * W, 0.5 * H, 10.5), P(0.9 * W, 0.5 * H, 11.0), P(0.5 * W, 0.9 * H, 12.0)]]        # wholly beyond far
    for i, s in enumerate(special):
        b.add(np.concatenate(s), (0, 2)[i & 1], rgbs(rng, 1))
    k = float(focal(H))
    on_near = np.array([[(0.35 * W - 0.5 * W) * 0.1 / k, 0.0, 0.0], [0.05, 0.1, -0.8], [0.2, -0.1, -0.9]], np.float32)
    on_near[0, 2] = -np.float32(NEAR)                                                                     # w == near exactly (frame 0: identity)
    b.add_local(on_near[None], 0, (250, 120, 10))
    g = np.array([[100.0, -100.0, -0.625], [100.0, 100.0, -0.625], [-100.0, 100.0, -0.625], [-100.0, -100.0, -0.625]], np.float32)
    b.add_local(g[[0, 1, 2, 0, 2, 3]].reshape(2, 3, 3), 1, (255, 255, 255))
    return make_case("planes", H, W, *b.arrays(), xf)


def degenerate(H, W, seed=8, permuted=False):
    """Repeated and collinear corners (det == 0, nn == 0), two identical triangles of different colours (a tie on depth: the larger rgb
    wins), among ordinary triangles; `permuted`: the same triangles in another order."""
    rng = np.random.default_rng(seed)
    n = 150
    cx, cy, w = rng.uniform(0, W, n), rng.uniform(0, H, n), rng.uniform(0.8, 2.0, n)
    off = rng.uniform(-0.08, 0.08, (n, 3, 2)) * min(H, W)
    body = unproject(cx[:, None] + off[..., 0], cy[:, None] + off[..., 1], w[:, None] + rng.uniform(-0.1, 0.1, (n, 3)), H, W)
    xf = _frames_xf(rng, 3, 2)
    b = Builder(xf[0])
    b.add(body[:100], 1, rgbs(rng, 100)); b.add(body[100:], 0, rgbs(rng, 50))
    a, c, d = unproject([0.2 * W, 0.7 * W, 0.4 * W], [0.2 * H, 0.3 * H, 0.8 * H], [0.6, 0.65, 0.7], H, W)
    b.add(np.array([[a, a, c], [a, c, c], [a, a, a], [a, 0.5 * (a + c), c], [c, a, 0.25 * a + 0.75 * c]]), 1, rgbs(rng, 5))
    tie = np.array([a, c, d])
    b.add(tie[None], 2, (200, 40, 90)); b.add(tie[None], 2, (90, 220, 10)); b.add(tie[None][:, ::-1], 2, (90, 100, 250))
    v, t, f, col = b.arrays()
    ties = [len(t) - 3, len(t) - 2, len(t) - 1]               # the three coincident triangles; the last is wound the other way
    if permuted:
        p = np.random.default_rng(99).permutation(len(t))
        t, f, col = t[p], f[p], col[p]
        ties = [int(np.nonzero(p == i)[0][0]) for i in ties]
    return make_case("degenerate_perm" if permuted else "degenerate", H, W, v, t, f, col, xf, stated_ties=ties)


def _blob(rng, centre_px, w, radius_px, H, W, count=60):
    ang = rng.uniform(0, 2 * math.pi, count)
    rr = radius_px * np.sqrt(rng.random(count))
    cx, cy = centre_px[0] + rr * np.cos(ang), centre_px[1] + rr * np.sin(ang)
    off = rng.uniform(-3.0, 3.0, (count, 3, 2))
    return unproject(cx[:, None] + off[..., 0], cy[:, None] + off[..., 1], w + rng.uniform(-0.05, 0.05, (count, 3)), H, W)


def frames(H, W, seed=9):
    """16 frames, rotated and translated, frames 5 and 9 uniformly scaled by 0.3 and 3; one blob of triangles per frame, blobs straddle every
    interior tile border; frame 0 (the identity) is not empty."""
    rng = np.random.default_rng(seed)
    xf = _frames_xf(rng, 16, 3, jitter=0.02, scales={5: 0.3, 9: 3.0})
    mx, my = (128 if W > 128 else W // 2), (128 if H > 128 else H // 2)
    spots = [(mx, my), (mx, 0.3 * my), (mx, H - 0.3 * my), (0.3 * mx, my), (W - 0.3 * mx, my), (mx, 0.7 * my), (0.6 * mx, my), (mx + 0.5 * (W - mx), my)]
    spots += [(rng.uniform(0, W), rng.uniform(0, H)) for _ in range(8)]
    b = Builder(xf[0])
    for f in range(16):
        b.add(_blob(rng, spots[f], rng.uniform(0.7, 2.0), 14.0, H, W), f, rgbs(rng, 60))
    return make_case("frames", H, W, *b.arrays(), xf)


def heightfield(H, W, rows, cols, sel, mesh, seed=10):
    """A rows x cols heightfield per env in the last frame (tilted towards the eye), hf_sel NULL or naming thirds 0, 1, 2 mixed over the envs,
    alone or over a mesh."""
    rng = np.random.default_rng(seed + 31 * rows + cols)
    n = 4
    xf = np.stack([np.stack([IDENT, xform(rot(0, -0.9) @ rot(2, 0.4 + 0.1 * e), (0.02 * e, -0.05, -1.0))]) for e in range(n)])
    b = Builder(xf[0])
    if mesh:
        b.add(_blob(rng, (0.5 * W, 0.5 * H), 1.0, 0.3 * min(H, W), H, W, 80), 0, rgbs(rng, 80))
        b.add(_blob(rng, (0.4 * W, 0.6 * H), 0.9, 0.2 * min(H, W), H, W, 40), 1, rgbs(rng, 40))
        arrays = b.arrays()
    else:
        arrays = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros(0, np.uint8), np.zeros((0, 3), np.uint8))
    scale = 0.7 / (max(rows, cols) - 1)
    thirds = 3 if sel else 1
    # a smooth swell plus roughness in proportion to the grid spacing: a fine grid stays a surface, not a pile of overlapping slivers
    jj, ii = np.divmod(np.arange(rows * cols), rows)
    swell = 0.04 * np.sin(3.1 * ii / (rows - 1) + np.arange(thirds * n).reshape(thirds, n, 1)) * np.cos(2.3 * jj / (cols - 1))
    heights = swell + rng.uniform(-1.0, 1.0, (thirds, n, rows * cols)) * min(0.06, 0.3 * scale) + np.arange(thirds)[:, None, None] * 0.05
    zoff = rng.uniform(-0.02, 0.02, (thirds, n)).astype(np.float32)
    hf = SimpleNamespace(rows=rows, cols=cols, scale=scale, rgb=(20, 60, 255), heights=heights if sel else heights[0], zoff=zoff if sel else zoff[0],
                         sel=np.array([0, 1, 2, 1], np.uint8) if sel else None)
    return make_case(f"hf_{rows}x{cols}_{'sel' if sel else 'nosel'}_{'mesh' if mesh else 'alone'}", H, W, *arrays, xf, hf=hf)


def hf_mesh(case, env):
    """The env's heightfield as the kernel tessellates it (float32, the kernel's expressions): verts [rows * cols][3] indexed j * rows + i,
    tris [2 (rows-1)(cols-1)][3]."""
    hf = case.hf
    third = 0 if hf.sel is None else int(hf.sel[env] & 3)
    Hh = (hf.heights[third, env] if hf.sel is not None else hf.heights[env]).astype(np.float32)
    zo = f32(hf.zoff[third, env] if hf.sel is not None else hf.zoff[env])
    cx, cy, s = f32(0.5) * f32(hf.rows - 1), f32(0.5) * f32(hf.cols - 1), f32(hf.scale)
    j, i = np.divmod(np.arange(hf.rows * hf.cols), hf.rows)
    v = np.stack([(i.astype(np.float32) - cx) * s, (j.astype(np.float32) - cy) * s, Hh - zo], 1).astype(np.float32)
    cell = np.arange((hf.rows - 1) * (hf.cols - 1))
    ci, cj = cell % (hf.rows - 1), cell // (hf.rows - 1)
    at = lambda a, c: c * hf.rows + a
    t = np.stack([np.stack([at(ci, cj), at(ci, cj + 1), at(ci + 1, cj)], 1), np.stack([at(ci + 1, cj), at(ci, cj + 1), at(ci + 1, cj + 1)], 1)], 1)
    return v, t.reshape(-1, 3).astype(np.int32)


def spheres(H, W, count=16, seed=11):
    """An opaque wall over the left part of the picture and translucent spheres: in front of and behind the wall, crossing near, beyond far, the
    eye inside one, a sub-pixel radius, alpha 0 slots, two overlapping spheres in both list orders (env 0 / env 1); env 2: random ones."""
    rng = np.random.default_rng(seed)
    wall = unproject([-5, 0.6 * W, -5, 0.6 * W, 0.6 * W, -5], [-5, -5, H + 5, -5, H + 5, H + 5], 1.5, H, W).reshape(2, 3, 3)
    xf = np.stack([np.stack([IDENT, IDENT])] * 3)
    b = Builder(xf[0])
    b.add(wall, 0, (60, 160, 90))
    b.add(_blob(rng, (0.7 * W, 0.5 * H), 1.2, 0.2 * min(H, W), H, W, 30), 1, rgbs(rng, 30))
    if count == 0:
        return make_case("spheres0", H, W, *b.arrays(), xf)
    U = lambda px, py, w: unproject(px * W, py * H, w, H, W)
    rows = [(U(0.2, 0.3, 1.0), 0.08, (255, 0, 0), 0.5), (U(0.3, 0.7, 2.0), 0.2, (0, 255, 0), 0.5), (U(0.6, 0.4, 1.5), 0.15, (0, 0, 255), 0.75),
            (U(0.8, 0.8, 0.12), 0.05, (255, 255, 0), 0.5), (U(0.5, 0.5, 10.8), 0.5, (255, 0, 255), 0.5), (np.array([0.01, 0.02, -0.05]), 0.5, (9, 9, 9), 1.0),
            (U(0.85, 0.2, 1.0), 0.0005, (255, 255, 255), 1.0), (U(0.4, 0.5, 1.0), 0.1, (200, 100, 0), 0.0),
            (U(0.75, 0.55, 0.9), 0.09, (250, 30, 30), 0.5), (U(0.8, 0.6, 1.0), 0.09, (30, 30, 250), 0.5)]
    sp = np.zeros((3, count, 8), np.float32)
    for e in range(2):
        order = list(range(len(rows)))
        if e == 1:
            order[8], order[9] = 9, 8
        for s, r in enumerate(order[:count]):
            c, rad, col, a = rows[r]
            sp[e, s, :3], sp[e, s, 3], sp[e, s, 4:7], sp[e, s, 7] = c, rad, col, a
    sp[2] = sphere_rows(rng, 1, count, H, W)[0]
    return make_case(f"spheres{count}", H, W, *b.arrays(), xf, spheres=sp)


def sphere_iw32(case, env, s):
    """mb_blend_spheres' own float32 expressions for sphere s of env, operation by operation: (the ray meets the sphere and near <= w <= far
    [H][W], the float32 bits of 1 / w [..., H, W]).  The radius may be an array [N, 1, 1] (sphere_tangent searches it)."""
    return _sphere_iw32(case.H, case.W, case.fov, case.near, case.far, case.spheres[env, s, :3], case.spheres[env, s, 3])


def _sphere_iw32(H, W, fov, near, far, centre, r, rows=None, cols=None):
    k, hw, hh, one = focal(H, fov), f32(0.5) * f32(W), f32(0.5) * f32(H), f32(1.0)
    py, px = np.meshgrid(np.arange(H, dtype=np.float32) if rows is None else rows.astype(np.float32),
                         np.arange(W, dtype=np.float32) if cols is None else cols.astype(np.float32), indexing="ij")
    dx, dy = ((px + f32(0.5)) - hw) / k, (hh - (py + f32(0.5))) / k
    A = (dx * dx + dy * dy) + one
    cx, cy, cz, r = f32(centre[0]), f32(centre[1]), f32(centre[2]), np.asarray(r, np.float32)
    B = (dx * cx + dy * cy) - cz
    Cc = ((cx * cx + cy * cy) + cz * cz) - r * r
    disc = B * B - A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (B - np.sqrt(disc)) / A
        iw = one / w
    assert iw.dtype == np.float32
    return (disc >= 0) & (w >= f32(near)) & (w <= f32(far)), iw.view(np.uint32)


def sphere_tangent(H=128, W=128):
    """A wall over the whole picture at w = 1.5 and one opaque-looking (alpha 1) sphere poking through it, its radius chosen - one float32
    step at a time from 0.11 - so that at some pixel centre the sphere's float32 1 / w has exactly the bits of the wall's: the sphere test
    is `1 / w strictly above the opaque key's`, so that pixel keeps the wall's colour, and a test with >= would blend it."""
    wall = unproject([-9, W + 9, -9, W + 9, W + 9, -9], [-9, -9, H + 9, -9, H + 9, H + 9], 1.5, H, W).reshape(2, 3, 3)
    xf = np.stack([IDENT])[None]
    b = Builder(xf[0])
    b.add(wall, 0, (60, 160, 90))
    bare = make_case("sphere_tangent_wall", H, W, *b.arrays(), xf)
    keys = (oracle(bare)[1][0].reshape(H, W) >> np.uint64(32)).astype(np.uint32)
    centre = unproject(0.5 * W + 0.3, 0.5 * H - 0.2, 1.6, H, W).astype(np.float32)
    rows, cols = np.arange(H // 2 - 8, H // 2 + 8), np.arange(W // 2 - 8, W // 2 + 8)
    radius = None
    for start in range(0, 400000, 20000):
        r = (f32(0.11).view(np.uint32) + np.arange(start, start + 20000, dtype=np.uint32)).view(np.float32)[:, None, None]
        ok, bits = _sphere_iw32(H, W, FOV, NEAR, FAR, centre, r, rows, cols)
        hit = (ok & (bits == keys[np.ix_(rows, cols)][None])).any(axis=(1, 2))
        if hit.any():
            radius = float(r[np.argmax(hit), 0, 0])
            break
    assert radius is not None, "no radius puts the sphere's 1 / w on the wall's bits"
    sp = np.zeros((1, 1, 8), np.float32)
    sp[0, 0, :3], sp[0, 0, 3], sp[0, 0, 4:7], sp[0, 0, 7] = centre, radius, (250, 20, 240), 1.0
    return make_case("sphere_tangent", H, W, *b.arrays(), xf, spheres=sp)


def tiny(n):
    """16 x 16, a few triangles in a moving frame and one sphere, 7 distinct transforms, env i taking transform i % 7: the env counts."""
    rng = np.random.default_rng(12)
    H = W = 16
    seven = np.stack([np.stack([IDENT, xform(rot(2, 0.3 * k), (0.02 * k, -0.01 * k, 0.0))]) for k in range(7)])
    b = Builder(seven[0])
    b.add(_blob(rng, (8, 8), 1.0, 5.0, H, W, 12), 1, rgbs(rng, 12))
    b.add(right_tri(1, 1, 12, 9, 2.0, H, W), 0, (90, 200, 40))
    sp7 = sphere_rows(rng, 7, 1, H, W)
    idx = np.arange(n) % 7
    return make_case(f"tiny{n}", H, W, *b.arrays(), seven[idx], spheres=sp7[idx]), idx


HF_SHAPES = [(2, 2), (3, 5), (5, 3), (64, 64)]
_AT_EVERY_SIZE = {"dust": dust, "planes": planes, "degenerate": degenerate, "degenerate_perm": lambda H, W: degenerate(H, W, permuted=True),
                  "spheres16": spheres, "spheres1": lambda H, W: spheres(H, W, 1), "spheres0": lambda H, W: spheres(H, W, 0),
                  "hf_3x5_sel_mesh": lambda H, W: heightfield(H, W, 3, 5, True, True), "hf_64x64_nosel_alone": lambda H, W: heightfield(H, W, 64, 64, False, False)}
_FIXED = {"areas": (areas, [(256, 256)]), "frames": (frames, [(256, 256), (128, 256), (256, 128)]), "widths_wave": (widths_wave, [(128, 128)]),
          "widths_group": (widths_group, [(128, 128)]), "huge_overflow": (huge_overflow, [(128, 128)]), "big_overflow": (big_overflow, [(128, 128)]),
          "many_chunks": ((lambda H, W: many_chunks(H=H, W=W)), [(128, 128)]), "sphere_tangent": (sphere_tangent, [(128, 128)])}
for _r, _c in HF_SHAPES:
    for _sel in (False, True):
        for _mesh in (False, True):
            _n = f"hf_{_r}x{_c}_{'sel' if _sel else 'nosel'}_{'mesh' if _mesh else 'alone'}"
            if _n not in _AT_EVERY_SIZE:
                _FIXED[_n] = ((lambda H, W, r=_r, c=_c, s=_sel, m=_mesh: heightfield(H, W, r, c, s, m)), [(128, 128)])

KEYS = [(name, H, W) for name in _AT_EVERY_SIZE for (H, W) in SIZES] + [(name, H, W) for name, (_, sizes) in _FIXED.items() for (H, W) in sizes]
IDS = [f"{n}-{h}x{w}" for n, h, w in KEYS]


@functools.lru_cache(maxsize=None)
def get(name, H, W):
    c = _AT_EVERY_SIZE[name](H, W) if name in _AT_EVERY_SIZE else _FIXED[name][0](H, W)
    c.name = name
    return c


def full_tris(case, env):
    """(verts, tris, tri_frame, tri_rgb) of everything env draws: the shared set plus its heightfield as triangles of the last frame."""
    if case.hf is None:
        return case.verts, case.tris, case.tri_frame, case.tri_rgb
    hv, ht = hf_mesh(case, env)
    return (np.concatenate([case.verts, hv]), np.concatenate([case.tris, ht + len(case.verts)]).astype(np.int32),
            np.concatenate([case.tri_frame, np.full(len(ht), case.n_frames - 1, np.uint8)]),
            np.concatenate([case.tri_rgb, np.tile(np.array(case.hf.rgb, np.uint8), (len(ht), 1))]))


_ORACLE = {}


def oracle(case):
    """(images uint8 [n][H][W][3], z keys uint64 [n][H * W]) of mb_render_scene + mb_blend_spheres; rendered once per case."""
    key = (case.name, case.H, case.W, case.n)
    if key not in _ORACLE:
        import ctypes as C
        from oracle import minibullet as mb
        fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        imgs, keys = np.zeros((case.n, case.H, case.W, 3), np.uint8), np.zeros((case.n, case.H * case.W), np.uint64)
        bg, le = np.array(case.background, np.uint8), np.ascontiguousarray(case.light, np.float32)
        cache = {}
        for e in range(case.n):
            sig = (case.xf[e].tobytes(), None if case.spheres is None else case.spheres[e].tobytes(), e if case.hf is not None else -1)
            if sig in cache:
                imgs[e], keys[e] = imgs[cache[sig]], keys[cache[sig]]
                continue
            cache[sig] = e
            v, t, f, c = (np.ascontiguousarray(a) for a in full_tris(case, e))
            xf = np.ascontiguousarray(case.xf[e])
            mb.lib().mb_render_scene(v.ctypes.data_as(fp), t.ctypes.data_as(C.POINTER(C.c_int32)), f.ctypes.data_as(u8), c.ctypes.data_as(u8), len(t),
                                     xf.ctypes.data_as(fp), le.ctypes.data_as(fp), case.fov, case.near, case.far, case.W, case.H, bg.ctypes.data_as(u8),
                                     keys[e].ctypes.data_as(C.POINTER(C.c_uint64)), imgs[e].ctypes.data_as(u8))
            if case.spheres is not None:
                sp = np.ascontiguousarray(case.spheres[e])
                mb.lib().mb_blend_spheres(sp.ctypes.data_as(fp), sp.shape[0], le.ctypes.data_as(fp), case.fov, case.near, case.far, case.W, case.H,
                                          keys[e].ctypes.data_as(C.POINTER(C.c_uint64)), imgs[e].ctypes.data_as(u8))
        imgs.setflags(write=False); keys.setflags(write=False)
        _ORACLE[key] = (imgs, keys)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------- the path census
def project32(case, env, verts=None, tris=None, tri_frame=None):
    """The kernel's set-up of every triangle in float32, operation by operation (setup_verts): w [nt][3], alive (not wholly before near /
    beyond far), all_near (every corner at w >= near), box (x0, x1, y0, y1) clipped to the image - the whole image when a corner is before near."""
    verts = case.verts if verts is None else verts
    tris = case.tris if tris is None else tris
    tri_frame = case.tri_frame if tri_frame is None else tri_frame
    M = case.xf[env][tri_frame][:, None, :]                                  # [nt][1][12]
    v = verts[tris]                                                          # [nt][3][3]
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    ex = ((M[..., 0] * vx + M[..., 1] * vy) + M[..., 2] * vz) + M[..., 9]
    ey = ((M[..., 3] * vx + M[..., 4] * vy) + M[..., 5] * vz) + M[..., 10]
    ez = ((M[..., 6] * vx + M[..., 7] * vy) + M[..., 8] * vz) + M[..., 11]
    k, hw, hh, near, far = focal(case.H, case.fov), f32(0.5) * f32(case.W), f32(0.5) * f32(case.H), f32(case.near), f32(case.far)
    w = -ez
    X, Y = k * ex + hw * w, hh * w - k * ey
    alive = ~((w < near).all(1) | (w > far).all(1))
    all_near = (w >= near).all(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = f32(1.0) / w
        sx, sy = X * r, Y * r
    fw, fh = f32(case.W) + f32(1.0), f32(case.H) + f32(1.0)
    cl = lambda a, hi: np.minimum(np.maximum(a, f32(-1.0)), hi)
    with np.errstate(invalid="ignore"):
        minx, maxx, miny, maxy = cl(sx.min(1), fw), cl(sx.max(1), fw), cl(sy.min(1), fh), cl(sy.max(1), fh)
        x0 = np.maximum(0, np.ceil(minx - f32(0.515625)).astype(np.int64)); x1 = np.minimum(case.W - 1, np.floor(maxx - f32(0.484375)).astype(np.int64))
        y0 = np.maximum(0, np.ceil(miny - f32(0.515625)).astype(np.int64)); y1 = np.minimum(case.H - 1, np.floor(maxy - f32(0.484375)).astype(np.int64))
    x0, x1 = np.where(all_near, x0, 0), np.where(all_near, x1, case.W - 1)
    y0, y1 = np.where(all_near, y0, 0), np.where(all_near, y1, case.H - 1)
    alive = alive & (x0 <= x1) & (y0 <= y1)
    return SimpleNamespace(w=w, alive=alive, all_near=all_near, box=(x0, x1, y0, y1))


def tiles_of(case):
    tw, th = min(case.W, 128), min(case.H, 128)
    return [(tx, ty, tx + tw - 1, ty + th - 1) for ty in range(0, case.H, th) for tx in range(0, case.W, tw)]


def census(case, env, consts, tile):
    """Per triangle of the shared set, in one tile: in_tile, the tile-clipped box width and area, the wave queue (small: full box <= small_area)
    and the fill path by the clipped area: 0 the lane itself, 1 a wavefront (> big_area), 2 the workgroup (> huge_area)."""
    p = project32(case, env)
    x0, x1, y0, y1 = p.box
    in_tile = p.alive & ~((x0 > tile[2]) | (x1 < tile[0]) | (y0 > tile[3]) | (y1 < tile[1]))
    cx0, cx1, cy0, cy1 = np.maximum(x0, tile[0]), np.minimum(x1, tile[2]), np.maximum(y0, tile[1]), np.minimum(y1, tile[3])
    bw = cx1 - cx0 + 1
    area = bw * (cy1 - cy0 + 1)
    small = p.all_near & ((x1 - x0 + 1) * (y1 - y0 + 1) <= consts.small_area)
    path = (area > consts.big_area).astype(int) + (area > consts.huge_area).astype(int)
    return SimpleNamespace(in_tile=in_tile, bw=bw, area=area, small=small, path=path)


def chunk_visible(case, env, sphere, frame, tile):
    """The kernel's chunk cull restated (float64): does the chunk's sphere, scaled by the frame, touch the tile's frustum?"""
    M = case.xf[env][frame].astype(np.float64)
    c = sphere[:, :3].astype(np.float64)
    x = (M[:, 0:3] * c).sum(1) + M[:, 9]; y = (M[:, 3:6] * c).sum(1) + M[:, 10]; w = -((M[:, 6:9] * c).sum(1) + M[:, 11])
    r = sphere[:, 3] * np.sqrt(M[:, 0] ** 2 + M[:, 3] ** 2 + M[:, 6] ** 2) * 1.001 + 1e-6
    k, hw, hh = float(focal(case.H, case.fov)), 0.5 * case.W, 0.5 * case.H
    L, T, R_, B = hw - tile[0], hh - tile[1], (tile[2] + 1) - hw, (tile[3] + 1) - hh
    vis = (w + r >= case.near) & (w - r <= case.far)
    vis &= (k * x + L * w >= -r * math.hypot(k, L)) & (R_ * w - k * x >= -r * math.hypot(k, R_))
    vis &= (T * w - k * y >= -r * math.hypot(k, T)) & (k * y + B * w >= -r * math.hypot(k, B))
    return vis


def sphere_trace(case, env, s):
    """Sphere s of env against every pixel ray, float64 (the rule of mb_blend_spheres): (the ray meets the sphere [H][W], eye depth w of the
    near intersection [H][W], radius in pixels at the centre's depth)."""
    k = float(focal(case.H, case.fov))
    px, py = np.meshgrid(np.arange(case.W) + 0.5, np.arange(case.H) + 0.5)
    dx, dy = (px - 0.5 * case.W) / k, (0.5 * case.H - py) / k
    cx, cy, cz, r = (float(v) for v in case.spheres[env, s, :4])
    A, B, Cq = dx * dx + dy * dy + 1.0, dx * cx + dy * cy - cz, cx * cx + cy * cy + cz * cz - r * r
    disc = B * B - A * Cq
    w = (B - np.sqrt(np.maximum(disc, 0.0))) / A
    return disc >= 0, w, k * r / max(-cz, 1e-9)
