"""A float64 numpy raster of the scene camera's rule (oracle/minibullet.c mb_render_scene + mb_blend_spheres; csrc/tg_scene.hip): homogeneous
edge functions on pixel centres, closest wins (on an exact tie the larger rgb), flat shade 0.6 + 0.35 max(0, n . l) two-sided, translucent
spheres blended in list order.  Every real quantity is float64 (from the float32 inputs); the roundings to a grey level that the rule itself
names - (uint)(c * intensity + 0.5), (uint8)(alpha src + (1 - alpha) dst + 0.5) - are kept.

Next to the image it returns the pixels where float32 and float64 may legitimately decide differently (`unsure`): an edge function within a
relative 1e-5 of zero while the other two are not clearly negative; a depth within 1e-5 of the near / far plane; the winner's depth within
1e-5 of the runner-up's; for a sphere, its discriminant, its depth against a plane or against the opaque surface within the same margin.
"Relative 1e-5" of an edge function is taken relative to its own three terms |a| x + |b| y + |c|.  That alone does not cover float32: a, b, c
are themselves differences of products (Y1 w2 - Y2 w1 ...) that cancel for a small triangle - by (image side / triangle size)^2 - so the
oracle's edge function carries the rounding of those products however far it is from zero on its own scale.  Measured with the literal rule
alone: 1 - 30 pixels per image of sub-pixel triangles differ (dust, frames, the 64 x 64 heightfield).  So to the 1e-5 is added ROUND = two
float32 roundings (2 x 2^-23) of the absolute sum of the products the quantity is made of - the precision of the number format, nothing
fitted: with it no pixel differs, with less (0) some do.  The same for 1 / w = (E0 + E1 + E2) / det.
An exact tie in float64 is decided like the oracle's (larger rgb) only between triangles with the same corners in the same order; a case
that ties otherwise names those triangles in notes["stated_ties"] and the test treats their pixels explicitly."""
import numpy as np

import scene_cases as sc

TOL = 1e-5
ROUND = 2 * 2.0 ** -23


def render(case, env, drop=()):
    """(image float64 [H][W][3] of whole grey levels, unsure bool [H][W]); drop: triangles of the shared set left undrawn."""
    H, W = case.H, case.W
    verts, tris, frame, rgb = sc.full_tris(case, env)
    k = float(sc.focal(H, case.fov))
    hw, hh, near, far = 0.5 * W, 0.5 * H, float(np.float32(case.near)), float(np.float32(case.far))
    inv_near, inv_far = float(np.float32(1.0) / np.float32(case.near)), float(np.float32(1.0) / np.float32(case.far))
    light = case.light.astype(np.float64)
    best = np.zeros((H, W)); btol = np.zeros((H, W)); key = np.zeros((H, W), np.int64); unsure = np.zeros((H, W), bool)
    col = np.zeros((H, W, 3)); col[:] = case.background
    if len(tris):
        M = case.xf[env].astype(np.float64)[frame]                              # [nt][12]
        v = verts.astype(np.float64)[tris]                                      # [nt][3][3]
        e = np.einsum("tij,tkj->tki", M[:, :9].reshape(-1, 3, 3), v) + M[:, None, 9:]
        w = -e[..., 2]
        X, Y = k * e[..., 0] + hw * w, hh * w - k * e[..., 1]
        keep = ~((w < near).all(1) | (w > far).all(1))
        all_near = (w >= near).all(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            sx, sy = X / w, Y / w
        x0 = np.where(all_near, np.floor(np.nan_to_num(sx.min(1)) - 0.5 - 1e-3), 0).clip(0, W).astype(int)
        x1 = np.where(all_near, np.ceil(np.nan_to_num(sx.max(1)) - 0.5 + 1e-3), W - 1).clip(-1, W - 1).astype(int)
        y0 = np.where(all_near, np.floor(np.nan_to_num(sy.min(1)) - 0.5 - 1e-3), 0).clip(0, H).astype(int)
        y1 = np.where(all_near, np.ceil(np.nan_to_num(sy.max(1)) - 0.5 + 1e-3), H - 1).clip(-1, H - 1).astype(int)
        keep &= (x0 <= x1) & (y0 <= y1)
        keep[list(drop)] = False
        for t in np.nonzero(keep)[0]:
            Xt, Yt, wt, et = X[t], Y[t], w[t], e[t]
            a = np.array([Yt[1] * wt[2] - Yt[2] * wt[1], Yt[2] * wt[0] - Yt[0] * wt[2], Yt[0] * wt[1] - Yt[1] * wt[0]])
            b = np.array([wt[1] * Xt[2] - wt[2] * Xt[1], wt[2] * Xt[0] - wt[0] * Xt[2], wt[0] * Xt[1] - wt[1] * Xt[0]])
            c = np.array([Xt[1] * Yt[2] - Xt[2] * Yt[1], Xt[2] * Yt[0] - Xt[0] * Yt[2], Xt[0] * Yt[1] - Xt[1] * Yt[0]])
            det = c @ wt
            mag = np.abs(c * wt).sum()
            if mag == 0.0:                                  # three coincident corners: nothing to draw, nothing to doubt
                continue
            flat = abs(det) <= 1e-6 * mag                   # collinear corners: float32 sees det == 0 or noise; only its line is in doubt
            fx, fy = np.arange(x0[t], x1[t] + 1) + 0.5, np.arange(y0[t], y1[t] + 1) + 0.5
            E = a[:, None, None] * fx[None, None, :] + b[:, None, None] * fy[None, :, None] + c[:, None, None]
            # the size of an edge function: the sum of the absolute values of the products it is made of (its float32 error is relative to that)
            A_ = np.abs(np.array([Yt[1] * wt[2], Yt[2] * wt[0], Yt[0] * wt[1]])) + np.abs(np.array([Yt[2] * wt[1], Yt[0] * wt[2], Yt[1] * wt[0]]))
            B_ = np.abs(np.array([wt[1] * Xt[2], wt[2] * Xt[0], wt[0] * Xt[1]])) + np.abs(np.array([wt[2] * Xt[1], wt[0] * Xt[2], wt[1] * Xt[0]]))
            C_ = np.abs(np.array([Xt[1] * Yt[2], Xt[2] * Yt[0], Xt[0] * Yt[1]])) + np.abs(np.array([Xt[2] * Yt[1], Xt[0] * Yt[2], Xt[1] * Yt[0]]))
            S = A_[:, None, None] * fx[None, None, :] + B_[:, None, None] * fy[None, :, None] + C_[:, None, None]
            sg = 1.0 if det > 0 else -1.0
            Es = sg * E
            tol = np.maximum(TOL * (np.abs(a)[:, None, None] * fx[None, None, :] + np.abs(b)[:, None, None] * fy[None, :, None] + np.abs(c)[:, None, None]), ROUND * S)
            maybe = (np.abs(Es) <= tol).any(0) & (Es >= -tol).all(0)
            sl = (slice(y0[t], y1[t] + 1), slice(x0[t], x1[t] + 1))
            if flat:
                unsure[sl] |= maybe
                continue
            inside = (Es >= 0).all(0)
            iw = E.sum(0) / det
            itol = TOL * np.abs(iw) + ROUND * (S.sum(0) / abs(det) + np.abs(iw) * (C_ @ np.abs(wt)) / abs(det))
            unsure[sl] |= maybe & (iw >= inv_far - itol) & (iw <= inv_near + itol)
            unsure[sl] |= inside & ((np.abs(iw - inv_far) <= itol) | (np.abs(iw - inv_near) <= itol))
            hit = inside & (iw >= inv_far) & (iw <= inv_near)
            if not hit.any():
                continue
            u, vv = et[1] - et[0], et[2] - et[0]
            n = np.cross(u, vv)
            nn = np.linalg.norm(n)
            ndl = 0.0
            if nn > 0:
                ndl = (n @ light) / nn
                if n @ et[0] > 0:
                    ndl = -ndl
                ndl = max(ndl, 0.0)
            shade = np.floor(rgb[t].astype(np.float64) * (0.6 + 0.35 * ndl) + 0.5)
            kk = (int(shade[0]) << 16) | (int(shade[1]) << 8) | int(shade[2])
            B, T, K, Cc, U = best[sl], btol[sl], key[sl], col[sl], unsure[sl]
            U |= hit & (B > 0) & (iw != B) & (np.abs(iw - B) <= itol + T)        # within the margin of the depth it meets: either may win
            win = hit & ((iw > B) | ((iw == B) & (kk > K)))
            B[win] = iw[win]; T[win] = itol[win]; K[win] = kk; Cc[win] = shade
    if case.spheres is not None:
        px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
        dx, dy = (px - hw) / k, (hh - py) / k
        A = dx * dx + dy * dy + 1.0
        for S in case.spheres[env].astype(np.float64):
            cx, cy, cz, r, alpha = S[0], S[1], S[2], S[3], S[7]
            if not alpha > 0:
                continue
            Bq = dx * cx + dy * cy - cz
            Cq = cx * cx + cy * cy + cz * cz - r * r
            disc = Bq * Bq - A * Cq
            scale = Bq * Bq + np.abs(A * Cq)
            with np.errstate(invalid="ignore", divide="ignore"):
                ws = (Bq - np.sqrt(np.maximum(disc, 0.0))) / A
                iw = 1.0 / ws
                ok = (disc >= 0) & (ws >= near) & (ws <= far) & (iw > best)
                rim = np.abs(disc) <= TOL * scale          # the rim: the float32 discriminant cancels (B^2 - A C), its sign is noise there
                edge = (disc >= 0) & ((np.abs(ws - near) <= TOL * near) | (np.abs(ws - far) <= TOL * far) | ((best > 0) & (np.abs(iw - best) <= TOL * best + btol)))
                unsure |= (rim | edge) & (ws >= near * (1 - 1e-3)) & (ws <= far * (1 + 1e-3))
                nrm = np.stack([(ws * dx - cx) / r, (ws * dy - cy) / r, (-ws - cz) / r], -1)
            inten = 0.6 + 0.35 * np.maximum(np.nan_to_num(nrm @ light), 0.0)
            src = np.floor(S[4:7][None, None, :] * inten[..., None] + 0.5)
            col = np.where(ok[..., None], np.floor(alpha * src + (1.0 - alpha) * col + 0.5), col)
    return col, unsure
