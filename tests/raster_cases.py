"""Deterministic inputs for the raster tests (tests/test_raster_f64_cpu.py, tests/test_gpu_raster_matrix.py): stimuli built at the raster's
dispatch boundaries and at the edges of its arithmetic and of its conservative culls.

Most meshes are built directly in GL eye space (x right, y up, w = -z forward; the transform is the identity) and seen by a synthetic sensor
with a 90 degree field of view: its projection constant kx = W/2 is exact in float32, so a vertex at w = 2^-5 with a dyadic x lands exactly
on a pixel centre and an edge between two such vertices has e = 0 exactly at the centres it passes through.  The synthetic sensor exists at
every image size (64^2 ... 256^2, 128 x 256, 256 x 128): its untouched depth is a dome at eye depth 0.036 - 0.046, with a pasted ring in the
corners.
"""
import ctypes as C

import numpy as np

NEAR, FAR = 0.01, 1.0
W_PIX = 2.0 ** -5       # eye depth at which dyadic coordinates project exactly (kx = W/2, iw = 32)


class Sensor:
    """What tg_sensor points at, for the synthetic sensor or a committed reference image set (SensorDesc)."""

    def __init__(self, W, H, fov, nodef_dep, nodef_gray, border_mask, name):
        from tactile_gym_amd import _capi as capi
        self.W, self.H, self.fov, self.name = W, H, fov, name
        self.near, self.far = NEAR, FAR
        self.nodef_dep = np.ascontiguousarray(nodef_dep, np.float32)
        self.nodef_gray = np.ascontiguousarray(nodef_gray, np.float32)
        self.border_mask = np.ascontiguousarray(border_mask, np.uint8)
        s = capi.TgSensor()
        s.image_h, s.image_w = H, W
        s.fov_deg, s.near_plane, s.far_plane = fov, NEAR, FAR
        s.turn_off_border = 0
        s.nodef_dep = self.nodef_dep.ctypes.data_as(C.POINTER(C.c_float))
        s.nodef_gray = self.nodef_gray.ctypes.data_as(C.POINTER(C.c_float))
        s.border_mask = self.border_mask.ctypes.data_as(C.POINTER(C.c_uint8))
        self.struct = s

    def depth_of_w(self, w):
        return (FAR / (FAR - NEAR)) - NEAR * FAR / ((FAR - NEAR) * w)


def _synthetic_nodef(W, H):
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (u + 0.5) / W * 2 - 1, (v + 0.5) / H * 2 - 1
    r2 = u * u + v * v
    w = 0.036 + 0.005 * r2
    return ((FAR / (FAR - NEAR)) - NEAR * FAR / ((FAR - NEAR) * w)).astype(np.float32), r2


def synthetic_sensor(W, H, border=True):
    dep, r2 = _synthetic_nodef(W, H)
    border = (r2 > 1.6).astype(np.uint8) if border else np.zeros((H, W), np.uint8)
    gray = np.where(border == 1, 40.0 + 60.0 * r2 + 0.37, 0.0)
    return Sensor(W, H, 90.0, dep, gray, border, f"synthetic{W}x{H}" + ("" if border.any() else "_noborder"))


def hf_sensor(case, H, W):
    """The sensor a heightfield case is seen by: its reference image set where one exists (square sizes), else the synthetic sensor;
    "synthetic": the synthetic sensor without its pasted ring, whose deepest untouched pixels - the image corners - then count."""
    if case.sensor_name == "synthetic":
        return synthetic_sensor(W, H, border=False)
    return fixture_sensor(case.sensor_name, H) if H == W else synthetic_sensor(W, H)


def fixture_sensor(name, size):
    import warnings
    from tactile_gym_amd.robot_model import SensorDesc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = SensorDesc(name, "standard", (size, size))
    s = Sensor(size, size, d.cam["fov"], d.nodef_dep, d.nodef_gray, d.border_mask, f"{name}{size}")
    assert d.cam["near"] == NEAR and d.cam["far"] == FAR
    return s


IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)


def _rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    if ax == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if ax == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def xform(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(np.float32)


def eye_xy(fx, fy, w, W=128, H=128):
    """Eye-space x, y of window point (fx, fy) at eye depth w for the synthetic sensor (kx = W/2, ky = H/2)."""
    return (fx - W / 2) / (W / 2) * w, (H / 2 - fy) / (H / 2) * w


class Case:
    def __init__(self, name, verts, tris, xfs, closed=False):
        self.name, self.closed = name, closed
        self.verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        self.tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        self.xfs = np.ascontiguousarray(xfs, np.float32).reshape(-1, 12)
        self.kind = "mesh"


class HfCase:
    def __init__(self, name, heights, zoff, scale, xfs, sensor_name):
        self.name, self.scale, self.sensor_name = name, scale, sensor_name
        self.heights = np.ascontiguousarray(heights, np.float64)          # [n][rows][cols]
        self.zoff = np.ascontiguousarray(zoff, np.float32)
        self.xfs = np.ascontiguousarray(xfs, np.float32).reshape(-1, 12)
        self.rows, self.cols = self.heights.shape[1:]
        self.kind = "hf"

    def mesh(self, i):
        from oracle.ref_env import heightfield_mesh
        return heightfield_mesh(self.heights[i], self.scale, float(self.zoff[i]))


def _soup(rng, n, size_px=(4, 40), w=(0.028, 0.045), span=1.0):
    """n random triangles of the given window size at eye depths w, over the middle `span` of a 128-wide view (scale-free: kx = W/2)."""
    c = rng.uniform(-0.9 * span, 0.9 * span, size=(n, 1, 2))
    r = rng.uniform(size_px[0], size_px[1], size=(n, 1, 1)) / 64.0
    ang = rng.uniform(0, 2 * np.pi, size=(n, 3)) + np.array([0, 2.1, 4.2])
    ndc = c + r * np.stack([np.cos(ang), np.sin(ang)], -1)
    ww = rng.uniform(*w, size=(n, 3))
    v = np.stack([ndc[..., 0] * ww, ndc[..., 1] * ww, -ww], -1)
    return v.reshape(-1, 3), np.arange(3 * n).reshape(n, 3)


def _jitter_xfs(rng, n, tilt=0.05, shift=0.002):
    xfs = [IDENT]
    for _ in range(n - 1):
        R = _rot(0, rng.normal(0, tilt)) @ _rot(1, rng.normal(0, tilt))
        xfs.append(xform(R, rng.normal(0, shift, 3) * np.array([1, 1, 0.3])))
    return np.stack(xfs)


def _box(c, h):
    """Closed box, outward winding (counter-clockwise seen from outside), 12 triangles."""
    c, h = np.asarray(c, np.float64), np.asarray(h, np.float64)
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * h + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = []
    for a, b, cc, d in quads:
        t += [(a, b, cc), (a, cc, d)]
    return v, np.array(t)


def _cat(parts):
    vs, ts, off = [], [], 0
    for v, t in parts:
        vs.append(np.asarray(v, np.float64).reshape(-1, 3))
        ts.append(np.asarray(t) + off)
        off += vs[-1].shape[0]
    return np.concatenate(vs), np.concatenate(ts)


def mesh_cases():
    rng = np.random.default_rng(20261015)
    cases = []
    # dispatch boundaries: 32 / 33 (block kernel), 256 / 257 (k_render_small / scatter), and a soup that takes a forced k_render_tactile
    # more than one record round (2 x 1500 records > 1024)
    for n in (32, 33, 256, 257, 1500):
        v, t = _soup(rng, n, size_px=(4, 40) if n < 1000 else (3, 12))
        cases.append(Case(f"soup{n}", v, t, _jitter_xfs(rng, 3)))
    # vertices on pixel centres, edges through pixel centres (e = 0 exactly), shared edges, a T-junction, degenerate triangles (s == 0:
    # collinear, repeated vertex), coplanar overlapping triangles (depth ties); at w = 2^-5, where the projection is exact
    W = 128
    def P(px, py, w=W_PIX):
        x, y = eye_xy(px + 0.5, py + 0.5, w, W, W)
        return (x, y, -w)
    v = [P(20, 20), P(60, 20), P(20, 60), P(60, 60),                 # two triangles sharing the diagonal 1-2
         P(70, 20), P(110, 20), P(90, 40), P(80, 30), P(100, 30),    # a fan about vertex 6: overlapping triangles with edges on pixel centres
         P(30, 70), P(50, 90), P(70, 110),                           # collinear (s == 0)
         P(90, 90), P(90, 90), P(100, 100),                          # repeated vertex
         P(20, 100), P(50, 100), P(20, 120), P(25, 95), P(55, 105), P(30, 124)]   # two overlapping coplanar triangles
    t = [(0, 1, 2), (1, 3, 2), (4, 5, 6), (4, 7, 6), (5, 6, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17), (18, 19, 20)]
    # the T-junction proper: a big triangle (21, 22, 23) whose edge 21-22 carries vertex 24 of two smaller ones
    v += [P(64, 70), P(124, 70), P(94, 124), P(94, 70), P(94, 50)]
    t += [(21, 22, 23), (21, 25, 24), (24, 25, 22)]
    tilt = [xform(np.eye(3), (0, 0, 0)), xform(np.eye(3), (0, 0, -0.002)), xform(_rot(1, 0.02), (0, 0, 0))]
    cases.append(Case("pixel_centres", v, t, np.stack(tilt)))
    # slivers, and faces nearly parallel to the view rays (the plane through the eye is edge-on: s ~ 0)
    v, t = [], []
    for k in range(8):
        a = np.array(P(10 + 14 * k, 8)); b = np.array(P(12 + 14 * k, 120)); c = b + np.array([1e-6 * (k + 1), 0, 0])
        v += [a, b, c]; t.append((3 * k, 3 * k + 1, 3 * k + 2))
    for k, eps in enumerate((0.0, 1e-5, 1e-4, 1e-3)):
        # a face containing the ray through pixel column 30 + 20 k, tilted by eps out of it
        x0, _ = eye_xy(30.5 + 20 * k, 0, 1.0)
        base = len(v)
        v += [(x0 * 0.03, 0.02, -0.03), (x0 * 0.045 + eps * 0.045, -0.02, -0.045), (x0 * 0.03 - eps * 0.03, -0.02, -0.03)]
        t.append((base, base + 1, base + 2))
    cases.append(Case("slivers_grazing", v, t, np.stack([IDENT, xform(_rot(0, 0.01), (0, 0, 0))])))
    # the near plane: 1, 2 and 3 vertices behind it, vertices exactly at w = near
    v, t = [], []
    for k, ws in enumerate([(0.005, 0.03, 0.03), (0.005, 0.004, 0.03), (0.005, 0.006, 0.008), (NEAR, 0.03, 0.03), (NEAR, NEAR, 0.03),
                            (NEAR, 0.005, 0.03), (0.0, 0.03, 0.02), (-0.01, 0.03, 0.025)]):
        cx, cy = -0.6 + 0.4 * (k % 4), -0.4 + 0.8 * (k // 4)
        ndc = [(cx - 0.3, cy - 0.25), (cx + 0.3, cy - 0.2), (cx, cy + 0.3)]
        for (nx, ny), w in zip(ndc, ws):
            v.append((nx * max(w, 0.01), ny * max(w, 0.01), -w))
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    cases.append(Case("near_plane", v, t, np.stack([IDENT, xform(np.eye(3), (0, 0, 0.001))])))
    # depths at far and at zcull (the largest untouched depth: these triangles can never win and must change nothing), next to one that wins
    v, t = [], []
    for k, w in enumerate((FAR, 0.99 * FAR, 0.046, 0.04605, 0.0455)):
        cx = -0.7 + 0.35 * k
        v += [((cx - 0.15) * w, -0.5 * w, -w), ((cx + 0.15) * w, -0.5 * w, -w), (cx * w, 0.5 * w, -w)]
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    cases.append(Case("far_zcull", v, t, np.stack([IDENT, xform(np.eye(3), (0, 0, -0.0004))])))
    # a plane swept in depth across the dome: |diff| runs through 1e-4, 1.96e-4 (first grey level) and 0.05 (saturation)
    v = [(-0.06, -0.06, -0.0455), (0.06, -0.06, -0.0455), (0.06, 0.06, -0.020), (-0.06, 0.06, -0.020)]
    sweep = [xform(np.eye(3), (0, 0, dz)) for dz in (0.0, -0.001, -0.004, 0.0003)]
    cases.append(Case("depth_sweep", v, [(0, 1, 2), (0, 2, 3)], np.stack(sweep)))
    # planes facing the camera 2.2e-4 below the deepest untouched depth of some 16 x 16 blocks of the 128^2 synthetic image: grey level 1
    # there, inside the block kernel's depth-plane cull margin (a block is skipped when the plane lies less than 1.5e-4 below it)
    dep, r2 = _synthetic_nodef(128, 128)
    bmax = sorted({float(dep[by:by + 16, bx:bx + 16][r2[by:by + 16, bx:bx + 16] <= 1.6].max())
                   for by in range(0, 128, 16) for bx in range(0, 128, 16) if (r2[by:by + 16, bx:bx + 16] <= 1.6).any()})
    C0, C1 = FAR / (FAR - NEAR), -NEAR * FAR / (FAR - NEAR)
    planes = [xform(np.eye(3), (0, 0, -C1 / ((b - 2.2e-4) - C0))) for b in bmax[::4]]
    v = [(-0.1, -0.1, 0.0), (0.1, -0.1, 0.0), (0.1, 0.1, 0.0), (-0.1, 0.1, 0.0)]
    cases.append(Case("grey_threshold_planes", v, [(0, 1, 2), (0, 2, 3)], np.stack(planes)))
    # > 256 triangles, each over 96 pixels of one 128 x 128 tile (and of one 64 x 64 tile): the scatter kernel's big-triangle queue overflows
    n = 300
    c = rng.uniform(-0.85, -0.25, size=(n, 1, 2))
    ang = rng.uniform(0, 2 * np.pi, size=(n, 1)) + np.array([0, 2.1, 4.2])
    ndc = c + (14.0 / 64) * np.stack([np.cos(ang), np.sin(ang)], -1)
    ww = rng.uniform(0.03, 0.045, size=(n, 3))
    v = np.stack([ndc[..., 0] * ww, ndc[..., 1] * ww, -ww], -1).reshape(-1, 3)
    cases.append(Case("scatter_overflow", v, np.arange(3 * n).reshape(n, 3), np.stack([IDENT, xform(np.eye(3), (0.003, -0.002, 0))])))
    # closed outward meshes at grazing angles: two interpenetrating boxes; a box cut by the near plane (drawn with the cull on and off)
    v, t = _cat([_box((0.0, 0.0, -0.05), (0.012, 0.01, 0.011)), _box((0.006, 0.004, -0.045), (0.008, 0.012, 0.009))])
    g = [IDENT, xform(_rot(1, np.pi / 4 - 1e-4) @ _rot(0, 0.3), (0, 0, 0)), xform(_rot(0, np.arctan(0.01 / 0.05) + 1e-5), (0, 0, 0)),
         xform(_rot(2, 0.4) @ _rot(1, 0.2), (0.002, 0, 0.006))]
    cases.append(Case("boxes_interpenetrating", v, t, np.stack(g), closed=True))
    v, t = _box((0.0, 0.0, -0.02), (0.015, 0.012, 0.0145))
    g = [IDENT, xform(_rot(1, 0.3), (0, 0, 0)), xform(_rot(0, 0.5) @ _rot(1, -0.2), (0.004, 0, 0.001))]
    cases.append(Case("box_near_cut", v, t, np.stack(g), closed=True))
    return cases


def _heights(rng, rows, cols, amp=0.004):
    i, j = np.mgrid[0:rows, 0:cols].astype(np.float64)
    h = np.zeros((rows, cols))
    for _ in range(4):
        kx, ky, ph = rng.uniform(0.05, 0.5), rng.uniform(0.05, 0.5), rng.uniform(0, 2 * np.pi)
        h += amp / 4 * np.sin(kx * i + ky * j + ph)
    return h


def heightfield_cases():
    """Camera looking down -z of the heightfield frame at height hc above the plane z = 0 (w = hc - z)."""
    rng = np.random.default_rng(1015)
    cases = []

    def down(hc, x=0.0, y=0.0, R=np.eye(3)):
        # eye = R (p - (x, y, hc)): the camera at (x, y, hc) looking along -z, rotated by R^T
        R = np.asarray(R, np.float64)
        return xform(R, -R @ np.array([x, y, hc]))

    for name, rows, cols, scale, sensor, xfs in [
        # rows != cols, the product's scale; the camera over the middle and over the grid's border and corner
        ("hf_48x80", 48, 80, 0.006, "tactip", [down(0.040), down(0.041, x=0.14), down(0.040, x=-0.141, y=0.237)]),
        # a fine grid: a TacTip view of many cells (more than 256 records survive in a tile)
        ("hf_fine", 64, 64, 0.0015, "tactip", [down(0.039), down(0.0405, x=0.01, y=-0.005)]),
        # DIGIT (narrow view: the cell-mask kernel), and a strongly tilted camera
        ("hf_digit", 64, 64, 0.006, "digit", [down(0.0185), down(0.019, y=0.02, R=_rot(0, 0.9)), down(0.018, R=_rot(1, -1.2) @ _rot(2, 0.7))]),
        # the surface at the depth of the deepest untouched pixels (the corners): contact where the frustum window's box is tight, so a
        # window without its widening loses the cells there
        ("hf_frustum_corner", 64, 64, 0.006, "synthetic", [down(0.0457), down(0.0456, x=0.003, R=_rot(2, 0.5)), down(0.0457, y=-0.004, R=_rot(2, 0.8))]),
        ("hf_tilted", 40, 72, 0.004, "tactip", [down(0.018, R=_rot(0, 1.1)), down(0.0075, x=0.05, R=_rot(1, 1.4) @ _rot(0, 0.3))]),
    ]:
        n = len(xfs)
        hs = np.stack([_heights(rng, rows, cols, amp=0.0003 if sensor == "synthetic" else 0.004) for _ in range(n)])
        zoff = np.array([0.5 * (h.min() + h.max()) for h in hs], np.float32)
        cases.append(HfCase(name, hs, zoff, scale, np.stack(xfs), sensor))
    return cases


def oracle_images(case, sensor, i0=0, i1=None):
    """uint8 images of the CPU oracle (oracle/minibullet.c) for envs i0..i1 of the case."""
    from oracle import minibullet as mb
    out = []
    i1 = case.xfs.shape[0] if i1 is None else i1
    for i in range(i0, i1):
        v, t = (case.verts, case.tris) if case.kind == "mesh" else case.mesh(i)
        cur = sensor.nodef_dep.copy()
        mb.render_depth(v, t, case.xfs[i], sensor.fov, NEAR, FAR, sensor.W, sensor.H, cur)
        out.append(mb.t_s_camera(cur, sensor.nodef_dep, sensor.nodef_gray, sensor.border_mask))
    return np.stack(out)
