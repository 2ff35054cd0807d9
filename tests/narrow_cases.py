"""The case matrix of the direct narrowphase tests (tests/test_narrow_cases_cpu.py, tests/test_gpu_narrowphase_matrix.py): placements of a
convex hull A against a box or a second hull B for the wave-mapped GJK / EPA of csrc/tg_narrowphase.hpp and its C restatement
oracle/narrowphase.c, at the geometry the workloads' generic placements never reach.

A Case is (name, cls, hull A [n][3] in B's frame, half extents or hull B, scale, expected).  `expected` is (signed distance, unit normal or
None) where the class has a closed form, else None: the reference is then oracle/gjk_epa.py (reference()).

Classes, by the rule their answer obeys:
  generic / faceparallel / deep / contain / far / small / subset / dup / edgeparallel / scaled / hulls / hullbox8   the independent numpy GJK / EPA
  boxbox / point / segment   a closed form
  touching    cores that touch to within GJK's own threshold (|distance| <= 1e-14 scale-1 metres: gjk() returns "touching" at x.x <= 1e-28):
              "no normal" or a distance of rounding size, never a depth (PARITY A38a)
  symmetric   overlaps whose origin falls exactly on a lower-dimensional simplex: the restatement's known limit (PARITY A38b)

One wavefront draws one case, so the matrix stays at a few thousand placements; everything is deterministic in the seeds below."""
import ctypes as C
import dataclasses
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tactile_gym_amd", "assets")
BOXES = {"cube": (0.04, 0.04, 0.04), "brick": (0.04, 0.03, 0.02), "plate": (0.06, 0.02, 0.005)}
GAPS = (8e-3, 1e-3, 1e-6, 1e-9, 1e-12, -1e-12, -1e-9, -1e-6, -1e-3, -4e-3, -8e-3)     # along the pressing direction, metres at scale 1
TINY_GAPS = (1e-15, -1e-15)              # inside gjk()'s touching threshold: class "touching"
SCALES = (1e-3, 250.0)
SUBSET_N = (1, 2, 3, 4, 5, 8, 63, 64, 65, 128, 129)                                   # around one lane slot (64) and two
PADDED_N = (1151, 1152)                  # at the kSlots cap of tg_narrowphase.hpp
HULL_B_N = (1, 4, 8, 63, 64, 65, 133, 255, 256)                                       # ... and round the kSlotsB cap
DUP_PAIRS = ((10, 11), (63, 64), (5, 69), (64, 128))                                  # neighbouring lanes; one lane, two slots
MAX_N_HULL, MAX_N_B = 1152, 256
CLASSES = ("generic", "faceparallel", "deep", "contain", "far", "small", "point", "segment", "subset", "dup", "boxbox", "edgeparallel", "scaled",
           "hulls", "hullbox8", "touching", "symmetric")
dp = C.POINTER(C.c_double)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    cls: str
    hull: np.ndarray                     # [n][3] float64, in B's frame
    half: tuple = None                   # the box's half extents, or
    hull_b: np.ndarray = None            # ... B's hull [n_b][3] in its own frame
    scale: float = 1.0                   # of hull and box together: every bound is this times the scale-1 bound
    expected: tuple = None               # (sd, normal or None)
    pair: str = ""                       # hullbox8: the name both members of a pair share


@functools.lru_cache(maxsize=None)
def shape(name):
    """The committed hulls, centred on their vertex mean."""
    path, key = {"tactip": ("robots/ur5_right_angle_tactip.npz", "tip_hull_verts"), "digitac": ("robots/mg400_right_angle_digitac.npz", "tip_hull_verts"),
                 "dish": ("objects/spinning_plate.npz", "hull"), "spool": ("objects/plate_buffer.npz", "hull")}[name]
    h = np.ascontiguousarray(np.load(os.path.join(ASSETS, path))[key], dtype=np.float64)
    h = h - h.mean(0)
    h.setflags(write=False)
    return h


def corners(half, centre=(0.0, 0.0, 0.0)):
    s = np.array([[(i >> 2 & 1) * 2 - 1, (i >> 1 & 1) * 2 - 1, (i & 1) * 2 - 1] for i in range(8)], dtype=np.float64)
    return s * np.asarray(half, float) + np.asarray(centre, float)


def rot(ax, ang):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def rot_about(axis, ang):
    """About a coordinate axis, with exact 0 / 1 entries on it: the coordinates along it stay as they are, ties included.  "q": a quarter
    turn with exact entries throughout."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    c, s = (0.0, 1.0) if isinstance(ang, str) else (np.cos(ang), np.sin(ang))
    R = np.zeros((3, 3))
    R[axis, axis] = 1.0
    R[u, u] = R[v, v] = c
    R[u, v], R[v, u] = -s, s
    return R


def random_rot(rng):
    return rot(rng.normal(size=3), rng.uniform(0, np.pi))


def press(h, half, axis, sign, gap, lateral, exact=False):
    """Translate h so that its extreme vertices along -sign e_axis stand `gap` off the box face sign e_axis, the first of them at `lateral`
    (fractions of the face's half extents) on the face.  exact: the extreme coordinate IS the face's, to the bit."""
    g = np.array(h, dtype=np.float64)
    k = g[:, axis] * sign
    first = int(np.argmin(k))
    tied = k == k[first]
    g[:, axis] += sign * (half[axis] + gap) - g[first, axis]
    if exact:
        g[tied, axis] = sign * half[axis]
    for j, u in enumerate(((axis + 1) % 3, (axis + 2) % 3)):
        g[:, u] += lateral[j] * half[u] - g[first, u]
    return g


def pressed(h, half, axis, sign):
    """The closed form of a placement of press() within 1e-6 of the face on either side, its first extreme vertex well inside the face's
    outline: the signed distance is that vertex's from the face's plane, the normal the face's.  (At such distances x / |x| of any GJK is
    rounding noise, the reference's too, and the reference's GJK stalls up to 1e-10 m off where hull vertices lie 1e-10 m apart in height.)"""
    gap = (h[:, axis] * sign).min() - half[axis]
    if not 0.0 < abs(gap) <= 1.001e-6:
        return None
    n = np.zeros(3); n[axis] = sign
    return float(gap), n


def point_box(p, half):
    q = np.maximum(np.abs(p) - half, 0.0)
    d = float(np.linalg.norm(q))
    return d, np.sign(p) * q / d


def segment_box(p0, p1, half):
    """Distance of a segment from the box where they are apart: the squared distance is a convex piecewise quadratic of the parameter; between
    the parameters at which a coordinate crosses a face the quadratic is minimised in closed form."""
    half = np.asarray(half, float)
    v = p1 - p0
    ts = {0.0, 1.0}
    for a in range(3):
        if v[a] != 0.0:
            ts |= {t for t in ((half[a] - p0[a]) / v[a], (-half[a] - p0[a]) / v[a]) if 0.0 < t < 1.0}
    ts = sorted(ts)
    best = None
    for t0, t1 in zip(ts[:-1], ts[1:]):
        m = p0 + 0.5 * (t0 + t1) * v
        act = np.abs(m) > half
        sg = np.sign(m)
        a2, b1 = float((v[act] ** 2).sum()), float((v[act] * (p0[act] - sg[act] * half[act])).sum())
        t = min(max(-b1 / a2, t0), t1) if a2 > 0.0 else t0
        d, n = point_box(p0 + t * v, half) if (np.abs(p0 + t * v) > half).any() else (0.0, None)
        if best is None or d < best[0]:
            best = (d, n)
    return best


def subset(h, n, rng):
    return np.ascontiguousarray(h[np.sort(rng.choice(h.shape[0], n, replace=False))])


def padded(h, n, rng):
    """h with duplicates of its own vertices mixed in, up to n."""
    g = np.concatenate([h, h[rng.integers(0, h.shape[0], n - h.shape[0])]])
    return np.ascontiguousarray(g[rng.permutation(n)])


def with_dup(h, i, j, direction):
    """h with its extreme vertex along `direction` at the indices i and j and nowhere else (the vertex j held is gone)."""
    g = np.array(h)
    w = int(np.argmax(g @ direction))
    v = g[w].copy()
    g[w] = g[i]
    g[i] = g[j] = v
    return g


def c_oracle(hull, half=None, hull_b=None):
    """oracle/narrowphase.c on one case -> [11] = found, sd, normal, witness on A, witness on B (zeros past `found` where it is 0)."""
    from oracle import minibullet as mb
    hull = np.ascontiguousarray(hull, dtype=np.float64)
    sd = C.c_double(); n = (C.c_double * 3)(); pa = (C.c_double * 3)(); pb = (C.c_double * 3)()
    if hull_b is None:
        e = np.ascontiguousarray(half, dtype=np.float64)
        ok = mb.lib().mb_gjk_epa_hull_box(hull.ctypes.data_as(dp), hull.shape[0], e.ctypes.data_as(dp), C.byref(sd), n, pa, pb)
    else:
        b = np.ascontiguousarray(hull_b, dtype=np.float64)
        ok = mb.lib().mb_gjk_epa_hull_hull(hull.ctypes.data_as(dp), hull.shape[0], b.ctypes.data_as(dp), b.shape[0], C.byref(sd), n, pa, pb)
    return np.array([1.0, sd.value] + list(n) + list(pa) + list(pb)) if ok else np.zeros(11)


def reference(case):
    """The independent numpy / scipy GJK / EPA -> (signed distance, normal from B to A)."""
    from oracle import gjk_epa as g
    A = g.hull_support(case.hull)
    B = g.box_support([0, 0, 0], np.eye(3), case.half) if case.hull_b is None else g.hull_support(case.hull_b)
    d, qa, qb, _ = g.gjk(A, B)
    if d > 0:
        return d, (qa - qb) / d
    dep, nn = g.epa(A, B)
    return -dep, -nn


def _newton_touch(h, half, hull_b=None):
    """Shift h three times along the oracle's normal by the oracle's distance: the cores end up touching to within rounding."""
    for _ in range(3):
        o = c_oracle(h, half, hull_b)
        if o[0] != 1.0:
            break
        h = h - o[1] * o[2:5]
    return h


@functools.lru_cache(maxsize=1)
def cases():
    out = []

    def add(name, cls, hull, half=None, hull_b=None, scale=1.0, expected=None, pair="", face=None, box=None):
        if face is not None:                                                             # a placement of press() on this face of half / box
            expected = pressed(hull, half if box is None else box, *face)
            expected = expected and (expected[0] * scale, expected[1])
        hull = np.ascontiguousarray(hull, dtype=np.float64) * scale
        assert 1 <= hull.shape[0] <= MAX_N_HULL and np.isfinite(hull).all(), name
        if hull_b is not None:
            hull_b = np.ascontiguousarray(hull_b, dtype=np.float64) * scale
            assert 1 <= hull_b.shape[0] <= MAX_N_B, name
            hull_b.setflags(write=False)
        else:
            half = tuple(float(x) * scale for x in half)
        hull.setflags(write=False)
        out.append(Case(f"{cls}-{len(out)}-{name}", cls, hull, half, hull_b, scale, expected, pair))

    tips = ("tactip", "digitac")
    rng = np.random.default_rng(20260)
    lat = lambda s=0.5: rng.uniform(-s, s, 2)   # noqa: E731
    face = lambda i: (i % 3, 1.0 if (i // 3) % 2 else -1.0)   # noqa: E731

    # generic attitudes: every committed hull and an 8-corner hull, pressed on a face at every gap; then round faces, edges and corners
    small_box = corners((0.01, 0.015, 0.02))
    for sn in tips + ("dish", "spool", "box8"):
        h0 = small_box if sn == "box8" else shape(sn)
        for bn in (BOXES if sn in tips else ("cube", "plate")):
            for i, gap in enumerate(GAPS):
                ax, sg = face(i + len(out))
                add(f"{sn}-{bn}-gap{gap:g}", "generic", press(h0 @ random_rot(rng).T, BOXES[bn], ax, sg, gap, lat()), BOXES[bn], face=(ax, sg))
    for sn in tips:
        for t in range(30):
            half = np.array(BOXES["brick"])
            p = rng.uniform(-1, 1, size=3)
            p = p / np.abs(p).max()
            add(f"{sn}-brick-round{t}", "generic", shape(sn) @ random_rot(rng).T + p * (half + 0.012 + rng.uniform(-0.004, 0.008)), BOXES["brick"])

    # face-parallel: a turn about the pressing axis only (0, a quarter turn, two generic angles), each of the six faces; the dish's rim (64
    # vertices tie along z), the spool (4 tie along x) and an 8-corner hull (4 tie everywhere) make every support query a tie
    angles = (0.0, "q", 0.7, 2.9)
    for sn in tips + ("dish", "spool", "box8"):
        h0 = small_box if sn == "box8" else shape(sn)
        for bn in (BOXES if sn in tips else ("cube", "brick")):
            for f in range(6):
                ax, sg = face(f)
                for i, gap in enumerate(GAPS):
                    if sn not in tips and (i + f) % 2:
                        continue
                    ang = angles[(i + f) % 4]
                    add(f"{sn}-{bn}-face{f}-turn{ang}-gap{gap:g}", "faceparallel", press(h0 @ rot_about(ax, ang).T, BOXES[bn], ax, sg, gap, lat(0.3)), BOXES[bn], face=(ax, sg))

    # deep: the hull's centre anywhere inside the box; containment both ways
    for sn in tips + ("spool",):
        for bn in BOXES:
            for t in range(16):
                R = random_rot(rng) if t % 4 else rot_about(t % 3, angles[(t // 4) % 4])
                add(f"{sn}-{bn}-{t}", "deep", shape(sn) @ R.T + rng.uniform(-1, 1, 3) * BOXES[bn], BOXES[bn])
    for t in range(24):
        bn = list(BOXES)[t % 3]
        hb = np.array(BOXES[bn])
        inner = 0.2 * hb.min() * rng.uniform(0.5, 1.0, 3)
        add(f"box8-in-{bn}-{t}", "contain", corners(inner) @ random_rot(rng).T + rng.uniform(-0.5, 0.5, 3) * hb, BOXES[bn])
        add(f"{bn}-in-box8-{t}", "contain", corners(rng.uniform(0.11, 0.14, 3)) @ random_rot(rng).T + rng.uniform(-0.2, 0.2, 3) * hb, BOXES[bn])
        if t % 3 == 0:
            add(f"{bn}-in-tactip-x10-{t}", "contain", 10.0 * shape("tactip") @ random_rot(rng).T + rng.uniform(-0.2, 0.2, 3) * hb, BOXES[bn])

    # far: 1 to 25 box sizes away
    for t in range(36):
        bn = list(BOXES)[t % 3]
        h0 = (shape("tactip"), shape("digitac"), small_box, np.zeros((1, 3)))[t % 4]
        u = rng.normal(size=3)
        add(f"{bn}-{t}", "far", h0 @ random_rot(rng).T + u / np.linalg.norm(u) * max(BOXES[bn]) * 2 * rng.uniform(1, 25), BOXES[bn])

    # points and segments (closed forms where they are outside), triangles and tetrahedra
    for t in range(66):
        bn = list(BOXES)[t % 3]
        half = np.array(BOXES[bn])
        ax, sg = face(t)
        gap = GAPS[t % 5] if t < 33 else abs(rng.normal()) * 0.02                       # GAPS[:5]: the positive ones
        p = press(np.zeros((1, 3)), half, ax, sg, gap, lat(1.6))
        add(f"{bn}-{t}", "point", p, BOXES[bn], expected=point_box(p[0], half))
        seg = rng.normal(size=(2, 3)) * 0.02
        if t % 3 == 0:
            seg[1, ax] = seg[0, ax]                                                       # parallel to the face
        seg = press(seg, half, ax, sg, gap, lat(1.2))
        d, n = segment_box(seg[0], seg[1], half)
        add(f"{bn}-{t}", "segment", seg, BOXES[bn], expected=(d, n))
    for t in range(60):
        bn = list(BOXES)[t % 3]
        ax, sg = face(t)
        k = (1, 2, 3, 4)[t % 4]
        h = rng.normal(size=(k, 3)) * 0.015
        if t < 44:
            add(f"n{k}-{bn}-gap{GAPS[t % 11]:g}", "small", press(h, BOXES[bn], ax, sg, GAPS[t % 11], lat()), BOXES[bn], face=(ax, sg))
        else:                                                                             # inside, off every symmetry
            add(f"n{k}-{bn}-inside{t}", "small", 0.2 * h + rng.uniform(-0.7, 0.7, 3) * BOXES[bn], BOXES[bn])

    # subsets of a tip hull round the lane-slot boundaries
    for n in SUBSET_N:
        for t in range(8):
            sn, bn = tips[t % 2], list(BOXES)[t % 3]
            ax, sg = face(t + n)
            h = subset(shape(sn), n, rng)
            R = random_rot(rng) if t % 2 else rot_about(ax, angles[t // 2])
            add(f"n{n}-{sn}-{bn}-gap{GAPS[(t + n) % 11]:g}", "subset", press(h @ R.T, BOXES[bn], ax, sg, GAPS[(t + n) % 11], lat()), BOXES[bn], face=(ax, sg))

    # duplicate vertices: the hull padded to the slot cap, and the supporting vertex itself twice, at chosen indices
    for n in PADDED_N:
        for t in range(16):
            bn = list(BOXES)[t % 3]
            ax, sg = face(t)
            h = padded(shape("tactip"), n, rng)
            R = random_rot(rng) if t % 2 else rot_about(ax, angles[(t // 2) % 4])
            add(f"padded{n}-{bn}-gap{GAPS[t % 11]:g}", "dup", press(h @ R.T, BOXES[bn], ax, sg, GAPS[t % 11], lat()), BOXES[bn], face=(ax, sg))
    for i, j in DUP_PAIRS:
        for t in range(12):
            bn = list(BOXES)[t % 3]
            ax, sg = face(t)
            R = random_rot(rng) if t % 2 else rot_about(ax, angles[(t // 2) % 4])
            h = subset(shape("digitac"), 129, rng) @ R.T
            e = np.zeros(3); e[ax] = -sg
            add(f"pair{i}-{j}-{bn}-gap{GAPS[t % 11]:g}", "dup", press(with_dup(h, i, j, e), BOXES[bn], ax, sg, GAPS[t % 11], lat()), BOXES[bn], face=(ax, sg))

    # ... and the same on a hull with ties of its own: the dish, whose rim holds 64 vertices in one plane, stood on its rim plane's normal along
    # x (an exact quarter turn) and pressed face-parallel on the faces +-x.  GJK's first query, along (1, 0, 0) exactly, then meets the 64 tied
    # vertices and their duplicates: the lowest index wins, and which vertex that is shows in the witness points
    dish_x = shape("dish") @ rot_about(1, "q").T
    for n in PADDED_N:
        for t in range(6):
            bn = list(BOXES)[t % 3]
            sg = 1.0 if t % 2 else -1.0
            h = padded(dish_x, n, rng) @ rot_about(0, angles[t % 4]).T
            add(f"dishpad{n}-{bn}-gap{GAPS[(3 * t) % 11]:g}", "dup", press(h, BOXES[bn], 0, sg, GAPS[(3 * t) % 11], lat(0.3)), BOXES[bn], face=(0, sg))
    for t, (i, j) in enumerate(DUP_PAIRS + DUP_PAIRS):
        bn = list(BOXES)[t % 3]
        sg = 1.0 if t < 4 else -1.0
        h = with_dup(dish_x @ rot_about(0, angles[t % 4]).T, i, j, np.array([1.0, 0.0, 0.0]))
        add(f"dishpair{i}-{j}-{bn}-gap{GAPS[(2 * t + 1) % 11]:g}", "dup", press(h, BOXES[bn], 0, sg, GAPS[(2 * t + 1) % 11], lat(0.3)), BOXES[bn], face=(0, sg))

    # box against box, axis-aligned: separated along one axis with a lateral offset; overlapping with a unique least overlap
    for bn, half in BOXES.items():
        half = np.array(half)
        for f in range(6):
            ax, sg = face(f)
            for gap in GAPS[:5]:
                ha = rng.uniform(0.005, 0.03, 3)
                h = press(corners(ha), half, ax, sg, gap, lat(0.8))
                n = np.zeros(3); n[ax] = sg
                add(f"{bn}-face{f}-gap{gap:g}", "boxbox", h, tuple(half), expected=((h[:, ax] * sg).min() - half[ax], n))
        t = 0
        while t < 20:
            ha, c = rng.uniform(0.005, 0.03, 3), rng.uniform(-1, 1, 3) * half
            h = corners(ha, c)
            over = np.minimum(half - h.min(0), h.max(0) + half)                           # per axis: the shorter way out
            o = np.sort(over)
            if o[0] <= 0 or o[1] - o[0] < 1e-3:
                continue
            ax = int(np.argmin(over))
            n = np.zeros(3); n[ax] = 1.0 if half[ax] - h[:, ax].min() < h[:, ax].max() + half[ax] else -1.0
            add(f"{bn}-overlap{t}", "boxbox", h, tuple(half), expected=(-o[0], n))
            t += 1

    # an edge of an 8-corner hull parallel to a box edge: turned about one axis only, next to the box edge along that axis
    for t in range(30):
        bn = list(BOXES)[t % 3]
        half = np.array(BOXES[bn])
        ax = t % 3
        c = np.zeros(3)
        u, v = (ax + 1) % 3, (ax + 2) % 3
        c[u], c[v] = (half[u] + rng.uniform(-0.004, 0.02)) * (1 if t & 1 else -1), (half[v] + rng.uniform(-0.004, 0.02)) * (1 if t & 2 else -1)
        c[ax] = rng.uniform(-0.5, 0.5) * half[ax]
        add(f"{bn}-axis{ax}-{t}", "edgeparallel", corners(rng.uniform(0.008, 0.02, 3)) @ rot_about(ax, rng.uniform(0.1, 1.4)).T + c, BOXES[bn])

    # hull and box scaled together (gaps down to 1e-9 of scale 1: scaled by 1e-3 that is 1e-12, still outside gjk()'s touching threshold)
    for sc in SCALES:
        for t in range(40):
            sn, bn = tips[t % 2], list(BOXES)[t % 3]
            ax, sg = face(t)
            gap = (8e-3, 1e-3, 1e-6, 1e-9, -1e-9, -1e-6, -1e-3, -4e-3)[t % 8]
            if t < 30:
                R = random_rot(rng) if t % 2 else rot_about(ax, angles[(t // 2) % 4])
                h = press(shape(sn) @ R.T, BOXES[bn], ax, sg, gap, lat())
            else:
                h = shape(sn) @ random_rot(rng).T + rng.uniform(-1, 1, 3) * BOXES[bn]
            add(f"x{sc:g}-{sn}-{bn}-{t}", "scaled", h, BOXES[bn], scale=sc, face=(ax, sg) if t < 30 else None)

    # two hulls: B = the spool and subsets of it and of the dish round its slot boundaries; A = the dish, a tip, a small subset
    for nb in HULL_B_N:
        src = shape("spool") if nb <= 133 else shape("dish")
        for t in range(12):
            B = src if nb == src.shape[0] else subset(src, nb, rng)
            A = (shape("dish"), shape("tactip"), subset(shape("digitac"), 65, rng), padded(shape("tactip"), 1152, rng))[t % 4]
            R = random_rot(rng) if t % 3 else rot_about(2, angles[(t // 3) % 4])
            u = rng.normal(size=3); u /= np.linalg.norm(u)
            if t % 3 == 0:
                u = np.array([0.0, 0.0, 1.0 if t % 2 else -1.0])
            Ar = A @ R.T
            reach = (B @ u).max() - (Ar @ u).min()                                         # A - B reaches the origin's plane along u at this offset
            off = u * (reach + ((8e-3, 1e-3, 1e-6, 2e-8, -2e-8, -1e-6, -1e-3, -4e-3)[t] if t < 8 else -rng.uniform(0.0, 1.0) * reach))
            add(f"nb{nb}-na{A.shape[0]}-{t}", "hulls", Ar + off, hull_b=B)

    # the same hull against the box and against the box's 8 corners as a hull: one answer
    for t in range(60):
        bn = list(BOXES)[t % 3]
        ax, sg = face(t)
        h0 = (shape("tactip"), shape("digitac"), subset(shape("tactip"), 64, rng), small_box, shape("spool"))[t % 5]
        R = random_rot(rng) if t % 2 else rot_about(ax, angles[(t // 2) % 4])
        h = press(h0 @ R.T, BOXES[bn], ax, sg, GAPS[t % 11], lat()) if t < 44 else h0 @ R.T + rng.uniform(-0.8, 0.8, 3) * BOXES[bn]
        add(f"{bn}-{t}-box", "hullbox8", h, BOXES[bn], pair=f"p{t}", face=(ax, sg) if t < 44 else None)
        add(f"{bn}-{t}-hull", "hullbox8", h, hull_b=corners(BOXES[bn]), pair=f"p{t}", face=(ax, sg) if t < 44 else None, box=BOXES[bn])

    # touching: the extreme vertices exactly in a face's plane; the tiny gaps; random attitudes walked onto the surface by Newton steps
    for sn in tips + ("dish", "box8"):
        h0 = small_box if sn == "box8" else shape(sn)
        for bn in BOXES:
            for f in range(6):
                ax, sg = face(f)
                for k, ang in enumerate(angles[:3] if sn in tips else angles[:2]):
                    add(f"plane-{sn}-{bn}-face{f}-turn{ang}", "touching", press(h0 @ rot_about(ax, ang).T, BOXES[bn], ax, sg, 0.0, lat(0.3) * (k > 0), exact=True), BOXES[bn])
                add(f"tiny-{sn}-{bn}-face{f}", "touching", press(h0 @ rot_about(ax, angles[f % 4]).T, BOXES[bn], ax, sg, TINY_GAPS[f % 2], lat(0.3)), BOXES[bn])
    for t in range(300):
        sn, bn = tips[t % 2], list(BOXES)[t % 3]
        half = np.array(BOXES[bn])
        p = rng.uniform(-1, 1, size=3)
        p = p / np.abs(p).max()
        h = shape(sn) @ random_rot(rng).T + p * (half + 0.012 + rng.uniform(-0.003, 0.006))
        add(f"newton-{sn}-{bn}-{t}", "touching", _newton_touch(h, BOXES[bn]), BOXES[bn])

    # symmetric overlaps: the origin of the difference falls exactly on a vertex, an edge or a face of GJK's simplex
    add("cube0.01-concentric", "symmetric", corners((0.01, 0.01, 0.01)), BOXES["cube"])
    add("point-on-x", "symmetric", np.array([[0.01, 0.0, 0.0]]), BOXES["cube"])
    add("segment-through-centre", "symmetric", np.array([[-0.01, 0.0, 0.0], [0.02, 0.0, 0.0]]), BOXES["cube"])
    add("point-at-centre", "symmetric", np.zeros((1, 3)), BOXES["brick"])
    add("brick-in-plate-concentric", "symmetric", corners((0.01, 0.005, 0.002)), BOXES["plate"])
    add("point-on-y", "symmetric", np.array([[0.0, -0.015, 0.0]]), BOXES["brick"])
    assert {c.cls for c in out} == set(CLASSES)
    return tuple(out)


def of_class(cls):
    return [(i, c) for i, c in enumerate(cases()) if c.cls == cls]


@functools.lru_cache(maxsize=1)
def oracle_results():
    """[n_cases][11] of oracle/narrowphase.c over the whole matrix, computed once and shared (read-only)."""
    r = np.stack([c_oracle(c.hull, c.half, c.hull_b) for c in cases()])
    r.setflags(write=False)
    return r


def batches(indexed):
    """Cases that one launch of tg_selftest_narrowphase(_hulls) can take together: the same n_hull and the same box or hull B.
    -> [(indices, hulls [k][n][3], half or None, hull_b or None)]"""
    groups = {}
    for i, c in indexed:
        key = (c.hull.shape[0], c.half, None if c.hull_b is None else c.hull_b.tobytes())
        groups.setdefault(key, []).append((i, c))
    return [([i for i, _ in g], np.ascontiguousarray(np.stack([c.hull for _, c in g])), g[0][1].half, g[0][1].hull_b) for g in groups.values()]


@functools.lru_cache(maxsize=1)
def references():
    """(sd [n_cases], normal [n_cases][3]) of every case but the touching and symmetric ones (NaN there): the closed form where the class has
    one, else the numpy / scipy GJK / EPA.  Computed once and shared (read-only)."""
    cs = cases()
    sd, nrm = np.full(len(cs), np.nan), np.full((len(cs), 3), np.nan)
    for i, c in enumerate(cs):
        if c.cls in ("touching", "symmetric"):
            continue
        sd[i], n = c.expected if c.expected is not None else reference(c)
        if n is not None:
            nrm[i] = n
    sd.setflags(write=False); nrm.setflags(write=False)
    return sd, nrm


# ---- the persistent manifold under scripts of operations (tg_selftest_manifold against mb_manifold_add / mb_manifold_refresh)
OP_WORDS, MANI_WORDS = 36, 65            # include/tactile_gym_hip_test.h
ADD, REFRESH, NOP = 0.0, 1.0, 2.0
BRK = 2.0 ** -13                         # the known-answer scripts' breaking threshold and grid: every sum and product in them is exact
EYE = np.eye(3).reshape(9)


def op_add(la, depth, n=(0.0, 0.0, 1.0), breaking=BRK, oa=(0, 0, 0), Ra=EYE, ob=(0, 0, 0), Rb=EYE, pa=None):
    """An add of the point whose world position on A is pa (default: la, for bodies at the origin), B's point `depth` below it along n."""
    pa = np.asarray(la if pa is None else pa, float)
    n = np.asarray(n, float)
    return np.concatenate([[ADD, breaking], oa, Ra, ob, Rb, pa, pa - depth * n, n, [depth]]).astype(np.float64)


def op_refresh(oa=(0, 0, 0), Ra=EYE, ob=(0, 0, 0), Rb=EYE, breaking=BRK):
    return np.concatenate([[REFRESH, breaking], oa, Ra, ob, Rb, np.zeros(10)]).astype(np.float64)


def replay(script):
    """[n_ops][36] through the C oracle -> [n_ops][65] in the device's layout: la, lb, nrm, pa, pb [4][3] each, depth [4], count."""
    from oracle import minibullet as mb
    L = mb.lib()
    L.mb_manifold_add.argtypes = [C.POINTER(mb.MBManifold), C.c_double, dp, dp, dp, dp, dp, dp, dp, C.c_double]
    L.mb_manifold_refresh.argtypes = [C.POINTER(mb.MBManifold), C.c_double, dp, dp, dp, dp]
    L.mb_manifold_add.restype = L.mb_manifold_refresh.restype = None
    m = mb.MBManifold()
    out = np.zeros((len(script), MANI_WORDS))
    for k, op in enumerate(script):
        a = [np.ascontiguousarray(op[s]) for s in (slice(2, 5), slice(5, 14), slice(14, 17), slice(17, 26), slice(26, 29), slice(29, 32), slice(32, 35))]
        if op[0] == ADD:
            L.mb_manifold_add(C.byref(m), op[1], *[x.ctypes.data_as(dp) for x in a], C.c_double(op[35]))
        elif op[0] == REFRESH:
            L.mb_manifold_refresh(C.byref(m), op[1], *[x.ctypes.data_as(dp) for x in a[:4]])
        for j, f in enumerate((m.la, m.lb, m.nrm, m.pa, m.pb)):
            out[k, 12 * j:12 * j + 12] = np.array([list(r) for r in f]).reshape(12)
        out[k, 60:64] = list(m.depth)
        out[k, 64] = m.n
    return out


def live(states):
    """The words a comparison looks at: everything of the slots below the count, and the count (a dead slot keeps what it last held on
    either side, which nothing reads)."""
    mask = np.zeros(states.shape, bool)
    n = states[..., 64].astype(int)
    for s in range(4):
        on = (n > s)[..., None]
        for j in range(5):
            mask[..., 12 * j + 3 * s:12 * j + 3 * s + 3] = on
        mask[..., 60 + s] = on[..., 0]
    mask[..., 64] = True
    return mask


def _square(depths):
    g = 2.0 ** -7                                                                        # 7.8 mm, a multiple of BRK
    return [op_add((x, y, 0.0), d) for (x, y), d in zip(((0, 0), (g, 0), (g, g), (0, g)), depths)]


@functools.lru_cache(maxsize=1)
def known_scripts():
    """name -> [n_ops][36].  What each must do is asserted in tests/test_narrow_cases_cpu.py on the oracle's states."""
    g, up = 2.0 ** -7, np.nextafter(BRK, 1.0)
    d4 = (-1 * BRK / 8, -2 * BRK / 8, -3 * BRK / 8, -4 * BRK / 8)
    s = {}
    s["replace_within_threshold"] = _square(d4) + [op_add((g + BRK / 2, 0.0, 0.0), -7 * BRK / 8)]
    s["depth_at_threshold"] = [op_add((0, 0, 0), BRK), op_add((g, 0, 0), up), op_add((0, g, 0), BRK), op_add((g, g, 0), 1.0)]
    s["fifth_new_is_deepest"] = _square(d4) + [op_add((4 * g, g / 2, 0.0), -BRK)]
    for k in range(4):
        d = [-BRK / 8] * 4
        d[k] = -BRK / 2
        s[f"fifth_slot{k}_is_deepest"] = _square(d) + [op_add(((-3 * g, g / 2), (4 * g, g / 2), (4 * g, g / 2), (-3 * g, g / 2))[k] + (0.0,), -BRK / 4)]
    s["fifth_deepest_tie"] = _square((-BRK / 8, -BRK / 2, -BRK / 2, -BRK / 8)) + [op_add((4 * g, g / 2, 0.0), -BRK / 4)]
    s["fifth_area_tie"] = _square(d4) + [op_add((-3 * g, 5 * g, 0.0), -BRK)]
    line = [op_add((k * g, 0.0, 0.0), 0.0) for k in range(4)]
    s["refresh_empty"] = [op_refresh(), op_refresh(oa=(g, 0, 0))]
    s["refresh_keeps_at_threshold"] = line + [op_refresh(oa=(0, 0, BRK)), op_refresh(oa=(BRK, 0, 0)), op_refresh(oa=(0, -BRK, 0))]
    s["refresh_drops_past_threshold"] = line + [op_refresh(oa=(0, 0, up)), op_refresh()] + line + [op_refresh(oa=(BRK + 2.0 ** -30, 0, 0))]
    # A lifted by twice the threshold: the one point whose normal looks up has separated, the others (normals down) only sank in
    flip = lambda k: [op_add((j * g, 0.0, 0.0), 0.0, n=(0.0, 0.0, 1.0 if j == k else -1.0)) for j in range(4)]   # noqa: E731
    s["refresh_drops_middle"] = flip(1) + [op_refresh(oa=(0, 0, 2 * BRK))]
    s["refresh_drops_last"] = flip(3) + [op_refresh(oa=(0, 0, 2 * BRK))]
    s["refresh_drops_first_of_two"] = flip(0)[:2] + [op_refresh(oa=(0, 0, 2 * BRK))]
    return {k: np.stack(v) for k, v in s.items()}


N_RANDOM_SCRIPTS, N_RANDOM_OPS = 300, 24


@functools.lru_cache(maxsize=1)
def random_scripts():
    """[300][24][36]: two bodies in small rigid motions, points near the plane between them; adds (some next to a cached point, some too far off
    the surface), refreshes after moves that now and then carry a point past the threshold."""
    rng = np.random.default_rng(4711)
    out = np.zeros((N_RANDOM_SCRIPTS, N_RANDOM_OPS, OP_WORDS))
    brk = 1e-4
    for s in range(N_RANDOM_SCRIPTS):
        oa, ob = rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.05
        Ra, Rb = random_rot(rng), random_rot(rng)
        nl = np.array([0.0, 0.0, 1.0])                                                   # the contact plane's normal in A's frame
        pts = []
        for k in range(N_RANDOM_OPS):
            if rng.random() < 0.62:
                if pts and rng.random() < 0.3:
                    la = pts[rng.integers(len(pts))] + rng.normal(size=3) * 0.4 * brk    # next to a cached point, mostly within the threshold
                else:
                    la = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.normal() * 2e-5])
                pts.append(la)
                depth = rng.uniform(-3e-4, 1.15e-4)
                out[s, k] = op_add(la, depth, n=Ra @ nl, breaking=brk, oa=oa, Ra=Ra.reshape(9), ob=ob, Rb=Rb.reshape(9), pa=oa + Ra @ la)
            else:
                big = rng.random() < 0.35
                oa = oa + Ra @ (rng.normal(size=3) * (8e-5 if big else 1.5e-5))
                Ra = rot(rng.normal(size=3), rng.normal() * (4e-3 if big else 5e-4)) @ Ra
                ob = ob + rng.normal(size=3) * 1e-5
                out[s, k] = op_refresh(oa, Ra.reshape(9), ob, Rb.reshape(9), breaking=brk)
    out.setflags(write=False)
    return out


def rule_shares(scripts, states):
    """From the oracle's states: the share of scripts in which an add replaced a cached point within the threshold, an add met a full
    manifold and put a cached point out by the area rule, a refresh dropped a point that was not the last (the last one took its slot)."""
    hit = np.zeros((len(scripts), 3), bool)
    for s, (script, st) in enumerate(zip(scripts, states)):
        prev = np.zeros(MANI_WORDS)
        for op, cur in zip(script, st):
            n0, n1 = int(prev[64]), int(cur[64])
            la0, la1 = prev[:12].reshape(4, 3), cur[:12].reshape(4, 3)
            if op[0] == ADD and n0 == n1 and not np.array_equal(prev, cur):
                slot = [i for i in range(n1) if not np.array_equal(prev[[*range(3 * i, 3 * i + 3), 60 + i]], cur[[*range(3 * i, 3 * i + 3), 60 + i]])]
                near = len(slot) == 1 and ((la0[slot[0]] - la1[slot[0]]) ** 2).sum() < op[1] ** 2
                hit[s, 0 if near else 1] = True
                assert near or n0 == 4
            elif op[0] == REFRESH and n1 < n0:
                kept = [i for i in range(n0) if any(np.array_equal(la0[i], la1[j]) for j in range(n1))]
                order = [j for i in kept for j in range(n1) if np.array_equal(la0[i], la1[j])]
                hit[s, 2] |= order != sorted(order)
            prev = cur
    return dict(zip(("replace", "fifth", "swap"), hit.mean(0)))
