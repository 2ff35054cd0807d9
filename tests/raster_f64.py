"""An independent double-precision tactile raster: getCameraImage's depth channel + t_s_camera, with a mask of the pixels f32 may decide
otherwise.

Written from PyBullet's camera model and DESIGN.md section 5's geometry, not from oracle/minibullet.c:
  * eye space is GL's (x right, y up, -z forward), w = -z_eye;  computeProjectionMatrixFOV(fov, aspect=1, near, far) and a W x H viewport
    put the eye point (x, y, -w) at window x = W/2 (1 + x / (w tan(fov/2))), y = H/2 (1 - y / (w tan(fov/2))) (rows counted from the top)
    and window depth (the depth buffer value) d = far/(far-near) - near far / ((far-near) w);
  * a triangle is clipped to w >= near (the result is a convex polygon of 3 or 4 vertices);
  * pixel (px, py) samples its centre (px + 0.5, py + 0.5); a polygon covers it when the centre is inside or on its boundary, and the
    depth there is that of the ray through the centre hitting the triangle's plane (1/w is affine in window coordinates: the same thing);
  * the depth image is the minimum over covering polygons, initialised with the untouched sensor's depth nodef_dep;
  * t_s_camera (tactile_sensor.py:261-294): diff = z - nodef, zero if |diff| <= 1e-4, u8(min(|diff|, 0.05) / 0.05 * 255), border pixels
    u8(nodef_gray).

Every quantity is computed in float64 from the float32 inputs (vertices, transform).  The product computes in float32, so a pixel is
reported AMBIGUOUS when the f32 computation may legitimately give another byte.  Rather than a fixed margin per criterion, each pixel gets
an interval [z_lo, z_hi] of depths the f32 raster can produce and is ambiguous when t_s_camera maps the two ends to different bytes.  That
covers, in one rule, the four ways f32 can differ:
  * coverage: the centre lies within EDGE_MARGIN_PX = 1e-3 px, or within the f32 error bound of the edge function, of an
    edge of a polygon that could win the depth test (then z_lo takes that polygon's depth and z_hi does not);
  * depth ties: two candidate depths within the depth error bound (at least DEPTH_FLOOR = 2e-7; the interval spans both);
  * the 1e-4 zero threshold: |diff| within the depth bound of 1e-4 (the interval straddles it);
  * grey truncation: 5100 |diff| within 5100 x the depth bound of an integer (about 1e-3 of a grey level for a 2e-7 bound).

The f32 error bounds (U = 2^-24, the unit roundoff; first order, times ERR_SAFETY = 2 for what first order leaves out):
  * eye coordinates ((M0 vx + M1 vy) + M2 vz) + M9: 4 U sum |terms| per component;
  * window position hw + kx (cx / w): kx (dcx / w + |cx| dw / w^2) + 4 U (|kx cx / w| + hw), plus the clip parameter's error
    (dwA + dwB) / |wB - wA| times the clipped edge's window length for vertices made by the near clip;
  * vertex depth C0 + C1 / w: |C1| dw / w^2 + 3 U (|C0| + |C1 / w|) + the rounding of C0, C1 to float32;
  * interpolated depth ((e0 d0 + e1 d1) + e2 d2) / s: the largest vertex depth error + |grad d| x the largest window error of a vertex
    (moving a vertex moves the affine depth by at most that) + sum r_i (max d - min d) / |s| (the edge functions' rounding r_i =
    3 U (|a| + |b|) for e = a - b moves the barycentric weights, hence the depth within the polygon's depth range).
A polygon whose |s| is within its error bound (degenerate in f32) is an uncertain candidate everywhere in its box.
"""
import numpy as np

U = 2.0 ** -24
ERR_SAFETY = 2.0
EDGE_MARGIN_PX = 1e-3
DEPTH_FLOOR = 2e-7
ZERO_EPS = 1e-4
MAX_PEN = 0.05


def camera_constants(fov_deg, near, far, W, H):
    ys = 1.0 / np.tan(np.radians(fov_deg) / 2.0)
    return dict(kx=ys * W / 2.0, ky=ys * H / 2.0, hw=W / 2.0, hh=H / 2.0, C0=far / (far - near), C1=-near * far / (far - near), near=near,
                W=W, H=H)


def t_s_camera_f64(z, nodef_dep, nodef_gray, border_mask, turn_off_border=False):
    """u8 image of depths z (f64) - tactile_sensor.py:261-294 in exact arithmetic."""
    diff = np.abs(z - nodef_dep.astype(np.float64))
    diff = np.where(diff <= ZERO_EPS, 0.0, diff)
    img = np.floor(np.minimum(diff, MAX_PEN) / MAX_PEN * 255.0).astype(np.uint8)
    if not turn_off_border:
        img = np.where(border_mask == 1, nodef_gray.astype(np.float32).astype(np.uint8), img)
    return img


def _clip_near(c, dc, near):
    """Clip the eye-space triangle c [3][3] (x, y, z; w = -z) with per-vertex absolute errors dc [3][3] to w >= near.  Returns a list of
    (x, y, w, dx_eye, dy_eye, dw, dt_rel) per polygon vertex; dt_rel: the clip parameter's error (0 for original vertices)."""
    out = []
    for k in range(3):
        a, b = c[k], c[(k + 1) % 3]
        da, db = dc[k], dc[(k + 1) % 3]
        wa, wb = -a[2], -b[2]
        if wa >= near:
            out.append((a[0], a[1], wa, da[0], da[1], da[2], 0.0, 0.0))
        if (wa >= near) != (wb >= near):
            t = (near - wa) / (wb - wa)
            dt = (da[2] + db[2]) / abs(wb - wa) + 3 * U * abs(t)
            x = a[0] + t * (b[0] - a[0])
            y = a[1] + t * (b[1] - a[1])
            dx = da[0] + abs(t) * (da[0] + db[0]) + 3 * U * (abs(a[0]) + abs(t * (b[0] - a[0])))
            dy = da[1] + abs(t) * (da[1] + db[1]) + 3 * U * (abs(a[1]) + abs(t * (b[1] - a[1])))
            out.append((x, y, near, dx, dy, 0.0, dt * abs(b[0] - a[0]), dt * abs(b[1] - a[1])))
    return out


def render_f64(verts, tris, M, fov_deg, near, far, nodef_dep, nodef_gray, border_mask, turn_off_border=False):
    """Tactile image (u8 [H, W]) of the mesh (verts f32 [n][3], tris [m][3]) placed by M (12 f32: row-major rotation, translation; object ->
    GL eye space) and the mask of ambiguous pixels (bool [H, W])."""
    H, W = nodef_dep.shape
    K = camera_constants(fov_deg, near, far, W, H)
    kx, ky, hw, hh, C0, C1 = K["kx"], K["ky"], K["hw"], K["hh"], K["C0"], K["C1"]
    dconst = abs(C0 - float(np.float32(C0))) + 2 * U * abs(C0)
    M = np.asarray(M, dtype=np.float32).astype(np.float64).reshape(12)
    R, tr = M[:9].reshape(3, 3), M[9:]
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    eye = v @ R.T + tr
    deye = 4 * U * (np.abs(v) @ np.abs(R).T + np.abs(tr))
    nd = nodef_dep.astype(np.float64)
    z_sure = nd.copy()                       # min over polygons that surely cover the centre (and the untouched depth)
    z_lo = np.full((H, W), np.inf)           # min over polygons that may cover it, each at the low end of its depth bound
    dz_sure = np.zeros((H, W))               # depth error bound of the winner of z_sure
    fy_all, fx_all = np.mgrid[0:H, 0:W].astype(np.float64) + 0.5
    for tri in tris:
        c, dc = eye[tri], deye[tri]
        poly = _clip_near(c, dc, near)
        if len(poly) < 3:
            continue
        P = np.array([(hw + kx * (x / w), hh - ky * (y / w)) for (x, y, w, *_) in poly])
        dP = np.array([(kx * (dx / w + abs(x) * dw / w ** 2) + 4 * U * (abs(kx * x / w) + hw) + kx * ex / w,
                        ky * (dy / w + abs(y) * dw / w ** 2) + 4 * U * (abs(ky * y / w) + hh) + ky * ey / w)
                       for (x, y, w, dx, dy, dw, ex, ey) in poly]) * ERR_SAFETY
        # a vertex on the near plane makes two clip vertices a hair apart: merge window vertices closer than their error (the edge between
        # them has no direction to speak of; the pixels near the point stay within the margins of the neighbouring edges)
        keep = [0]
        for k in range(1, len(poly)):
            if np.hypot(*(P[k] - P[keep[-1]])) > dP[k].max() + dP[keep[-1]].max() + EDGE_MARGIN_PX:
                keep.append(k)
        if len(keep) > 3 and np.hypot(*(P[keep[-1]] - P[0])) <= dP[keep[-1]].max() + dP[0].max() + EDGE_MARGIN_PX:
            keep.pop()
        collapsed = len(keep) < 3       # within error of a point or a segment: a sliver at most, treated as degenerate below
        if not collapsed:
            poly, P, dP = [poly[k] for k in keep], P[keep], dP[keep]
        wv = np.array([p[2] for p in poly])
        dwv = np.array([p[5] for p in poly])
        dv = C0 + C1 / wv
        ddv = (abs(C1) * dwv / wv ** 2 + 3 * U * (abs(C0) + np.abs(C1 / wv)) + dconst) * ERR_SAFETY
        n = len(poly)
        # signed area (twice) and its error: degenerate in f32 when |s| is within it
        s = sum(P[k, 0] * P[(k + 1) % n, 1] - P[(k + 1) % n, 0] * P[k, 1] for k in range(n))
        ext = np.ptp(P, axis=0)
        ds_bound = ERR_SAFETY * (8 * U * (ext[0] + 1) * (ext[1] + 1) + 2 * (dP[:, 0].max() * (ext[1] + 1) + dP[:, 1].max() * (ext[0] + 1)))
        degenerate = collapsed or abs(s) <= ds_bound
        mrg = dP.max() + EDGE_MARGIN_PX + 1.0
        x0, x1 = int(max(0, np.floor(P[:, 0].min() - mrg))), int(min(W - 1, np.ceil(P[:, 0].max() + mrg)))
        y0, y1 = int(max(0, np.floor(P[:, 1].min() - mrg))), int(min(H - 1, np.ceil(P[:, 1].max() + mrg)))
        if x0 > x1 or y0 > y1:
            continue
        fx, fy = fx_all[y0:y1 + 1, x0:x1 + 1], fy_all[y0:y1 + 1, x0:x1 + 1]
        # depth at the centre: the ray (X w, Y w, -w) through it meets the triangle's plane
        nrm = np.cross(c[1] - c[0], c[2] - c[0])
        X, Y = (fx - hw) / kx, (hh - fy) / ky
        den = nrm[0] * X + nrm[1] * Y - nrm[2]
        num = float(nrm @ c[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            iw = den / num if num != 0.0 else np.full(fx.shape, np.nan)
            d = C0 + C1 * iw
        dmin, dmax = dv.min(), dv.max()
        d = np.where(np.isfinite(d), np.clip(d, dmin, dmax), dmin)
        sg = 1.0 if s > 0 else -1.0
        inside = np.ones(fx.shape, bool)
        near_edge = np.zeros(fx.shape, bool)
        sum_rnd = np.zeros(fx.shape)
        for k in range(n):
            (ax, ay), (bx, by) = P[k], P[(k + 1) % n]
            a_, b_ = (ax - fx) * (by - fy), (bx - fx) * (ay - fy)
            e = a_ - b_                                   # sg * e > 0 inside
            rnd = ERR_SAFETY * 3 * U * (np.abs(a_) + np.abs(b_))
            de = rnd + dP[k, 0] * np.abs(by - fy) + dP[(k + 1) % n, 1] * np.abs(ax - fx) \
                + dP[(k + 1) % n, 0] * np.abs(ay - fy) + dP[k, 1] * np.abs(bx - fx)
            L = np.hypot(bx - ax, by - ay)
            if L > 0:     # distance from the centre to the edge segment
                tt = np.clip(((fx - ax) * (bx - ax) + (fy - ay) * (by - ay)) / L ** 2, 0.0, 1.0)
                dist = np.hypot(fx - (ax + tt * (bx - ax)), fy - (ay + tt * (by - ay)))
                margin = np.maximum(EDGE_MARGIN_PX, de / L)
            else:
                dist = np.hypot(fx - ax, fy - ay)
                margin = np.full(fx.shape, EDGE_MARGIN_PX)
            near_edge |= (dist <= margin) | (np.abs(e) <= de)
            inside &= sg * e >= 0
            sum_rnd += rnd
        if degenerate:    # f32 may give it a sliver of area along its edges, at any depth in its range
            sure = np.zeros(fx.shape, bool)
            maybe = near_edge
            dd = np.full(fx.shape, ddv.max() + (dmax - dmin))
        else:
            sure = inside & ~near_edge
            maybe = near_edge
            # the vertices' window errors move the (affine) depth by at most |grad d| x the largest of them; the edge functions' rounding
            # moves the barycentric weights, hence the depth within the polygon's depth range
            (x0_, y0_), (x1_, y1_), (x2_, y2_) = P[0], P[1], P[2]
            s3 = (x1_ - x0_) * (y2_ - y0_) - (x2_ - x0_) * (y1_ - y0_)
            gx = ((dv[1] - dv[0]) * (y2_ - y0_) - (dv[2] - dv[0]) * (y1_ - y0_)) / s3 if s3 != 0.0 else np.inf
            gy = ((x1_ - x0_) * (dv[2] - dv[0]) - (x2_ - x0_) * (dv[1] - dv[0])) / s3 if s3 != 0.0 else np.inf
            dd = ddv.max() + np.hypot(gx, gy) * dP.max() + sum_rnd * (dmax - dmin) / abs(s)
        dd = np.maximum(dd, DEPTH_FLOOR)
        zs, zl, dzs = z_sure[y0:y1 + 1, x0:x1 + 1], z_lo[y0:y1 + 1, x0:x1 + 1], dz_sure[y0:y1 + 1, x0:x1 + 1]
        win = sure & (d < zs)
        dzs[win] = dd[win]
        zs[win] = d[win]
        # every candidate at the low end of its bound: sure ones too (a tie within the bound may go either way)
        cand = sure | maybe
        np.minimum(zl, np.where(cand, d - dd, np.inf), out=zl)
        # a sure candidate within its bound above the winner still bounds z from below; the winner's upper end is z_sure + dz
    hi = np.minimum(z_sure + np.maximum(dz_sure, DEPTH_FLOOR), nd)     # z = min(nodef, ...): never above the untouched depth
    lo = np.minimum(z_sure - np.maximum(dz_sure, DEPTH_FLOOR), z_lo)
    lo = np.minimum(lo, nd)
    best = z_sure
    img = t_s_camera_f64(best, nodef_dep, nodef_gray, border_mask, turn_off_border)
    a = t_s_camera_f64(lo, nodef_dep, nodef_gray, border_mask, turn_off_border)
    b = t_s_camera_f64(hi, nodef_dep, nodef_gray, border_mask, turn_off_border)
    amb = a != b
    return img, amb
