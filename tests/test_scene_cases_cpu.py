"""CPU checks of the scene camera's case table (tests/scene_cases.py), no device needed:
- build_scene_chunks (through tg_selftest_scene_plan, the product's own object) keeps every triangle, once, with its corners and attribute;
- the census: a numpy restatement of the kernel's box rule and area thresholds, with the constants the plan entry reports, shows that each
  case reaches the branch of k_scene it is named for - if a constant changes, this fails instead of the coverage quietly disappearing;
- the oracle (mb_render_scene + mb_blend_spheres) against a float64 raster of the same rule (tests/scene_f64.py) on every case: outside the
  pixels where float32 may legitimately decide otherwise (at most 2 % of an image) every channel agrees within one grey level."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import scene_cases as sc
import scene_f64

FIELDS = ("n_chunks", "n_cverts", "tile_w", "tile_h", "big_cap", "lds_bytes", "accepted", "small_area", "big_area", "huge_area", "huge_cap",
          "big_cap_max", "chunk", "max_chunks", "max_spheres", "max_frames")


def plan(verts, tris, tri_frame, tri_rgb, H, W, tables=True):
    from tactile_gym_amd import _capi as capi
    verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32)
    tri_frame, tri_rgb = np.ascontiguousarray(tri_frame, np.uint8), np.ascontiguousarray(tri_rgb, np.uint8)
    nt = len(tris)
    p = capi.TgScenePlan()
    sphere, table, cverts = np.zeros((nt, 4), np.float32), np.zeros((nt, 5), np.int32), np.zeros((3 * nt, 3), np.float32)
    tris_out, local, attr = np.zeros((nt, 3), np.int32), np.zeros(nt, np.uint32), np.zeros(nt, np.uint32)
    fp, ip, u8, u32 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    ptr = (lambda a, t: a.ctypes.data_as(t)) if tables else (lambda a, t: None)
    r = capi.test_lib().tg_selftest_scene_plan(len(verts), verts.ctypes.data_as(fp), nt, tris.ctypes.data_as(ip), tri_frame.ctypes.data_as(u8),
                                               tri_rgb.ctypes.data_as(u8), W, H, C.byref(p), ptr(sphere, fp), ptr(table, ip), ptr(cverts, fp),
                                               ptr(tris_out, ip), ptr(local, u32), ptr(attr, u32))
    assert r == 0, capi.test_lib().tg_selftest_last_error()
    out = SimpleNamespace(**{k: getattr(p, k) for k in FIELDS})
    out.sphere, out.table, out.cverts, out.tris, out.local, out.attr = sphere[:p.n_chunks], table[:p.n_chunks], cverts[:p.n_cverts], tris_out, local, attr
    return out


_PLANS = {}


def case_plan(case):
    key = (case.name, case.H, case.W)
    if key not in _PLANS:
        _PLANS[key] = plan(case.verts, case.tris, case.tri_frame, case.tri_rgb, case.H, case.W)
    return _PLANS[key]


def check_chunks(verts, tris, tri_frame, tri_rgb, p):
    nt = len(tris)
    start, count, frame, vstart, vcount = (p.table[:, k].astype(np.int64) for k in range(5))
    assert count.sum() == nt and vcount.sum() == p.n_cverts                                   # counts add up
    assert (count >= 1).all() and (count <= p.chunk).all() and (vcount >= 1).all() and (vcount <= p.chunk).all() if nt else p.n_chunks == 0
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(count)[:-1]])) and np.array_equal(vstart, np.concatenate([[0], np.cumsum(vcount)[:-1]]))
    owner = np.repeat(np.arange(p.n_chunks), count)                                           # the chunk of every output triangle
    assert np.array_equal(p.attr >> 24, frame[owner])                                         # one frame per chunk
    loc = np.stack([(p.local >> (8 * j)) & 255 for j in range(3)], 1).astype(np.int64)
    assert (p.local >> 24 == 0).all() and (loc < vcount[owner][:, None]).all()
    assert np.array_equal(p.tris, vstart[owner][:, None] + loc)                               # tri_local and tris name the same vertices
    # every input triangle exactly once, its corner coordinates and its attribute unchanged
    attr_in = (tri_frame.astype(np.uint32) << 24) | (tri_rgb[:, 0].astype(np.uint32) << 16) | (tri_rgb[:, 1].astype(np.uint32) << 8) | tri_rgb[:, 2]
    rows_in = np.concatenate([verts[tris].reshape(nt, 9).view(np.uint32), attr_in[:, None]], 1)
    rows_out = np.concatenate([p.cverts[p.tris].reshape(nt, 9).view(np.uint32), p.attr[:, None]], 1)
    order = lambda r: r[np.lexsort(r.T[::-1])]
    assert np.array_equal(order(rows_in), order(rows_out))
    # every vertex inside its chunk's sphere
    vowner = np.repeat(np.arange(p.n_chunks), vcount)
    d = np.linalg.norm(p.cverts.astype(np.float64) - p.sphere[vowner, :3].astype(np.float64), axis=1)
    assert (d <= p.sphere[vowner, 3].astype(np.float64) * (1 + 1e-6) + 1e-30).all()


@pytest.mark.parametrize("key", sc.KEYS, ids=sc.IDS)
def test_chunk_invariants(key):
    case = sc.get(*key)
    if len(case.tris) == 0:
        p = case_plan(case)
        assert p.n_chunks == 0 and p.accepted == 1
        return
    check_chunks(case.verts, case.tris, case.tri_frame, case.tri_rgb, case_plan(case))


def test_chunk_invariants_product_scene():
    from tactile_gym_amd.robot_model import compose_scene
    v, t, f, c = compose_scene("ur5", "standard", "tactip", 6)
    p = plan(v, t, f, c, 128, 128)
    assert p.accepted == 1 and p.n_chunks > 100
    check_chunks(v, t, f, c, p)


def consts():
    return case_plan(sc.get("areas", 256, 256))


def test_constants():
    k = consts()
    assert (k.small_area, k.big_area, k.huge_area, k.huge_cap, k.big_cap_max, k.chunk, k.max_chunks, k.max_spheres, k.max_frames) == \
        (4, 64, 4096, 64, 2048, 64, 8192, 16, 16)
    assert (k.tile_w, k.tile_h, k.big_cap) == (128, 128, 2048)
    small = case_plan(sc.get("dust", 48, 80))
    assert (small.tile_w, small.tile_h) == (80, 48)


def _all(case):
    k = consts()
    return [(e, tile, sc.census(case, e, k, tile)) for e in range(case.n) for tile in sc.tiles_of(case)]


@pytest.mark.parametrize("size", sc.SIZES, ids=[f"{h}x{w}" for h, w in sc.SIZES])
def test_census_dust(size):
    """Both wave queues flush and leave a tail whatever order the chunks are taken in: a workgroup has 16 wavefronts, so more than 16 x 63
    survivors in a tile put 64 into one wavefront's queue, and a total that is no multiple of 64 leaves some wavefront a tail."""
    case = sc.get("dust", *size)
    p = case_plan(case)
    assert p.n_chunks >= 40 and len(np.unique(case.tri_frame)) >= 4
    for small in (True, False):
        tot = [int((c.in_tile & (c.small == small)).sum()) for _, _, c in _all(case)]
        assert any(t > 16 * 63 and t % 64 != 0 for t in tot), (small, tot)
    sizes = np.concatenate([c.area[c.in_tile] for _, _, c in _all(case)])
    assert (sizes == 1).any() and ((sizes >= 6) & (sizes <= 9)).any() and sizes.max() <= consts().big_area


def test_census_areas():
    case, k = sc.get("areas", 256, 256), consts()
    cs = [c for e, _, c in _all(case) if e == 0]
    seen = set(np.concatenate([c.area[c.in_tile] for c in cs]).tolist())
    assert {k.small_area, k.small_area + 1, k.big_area, k.big_area + 1, k.huge_area, k.huge_area + 64} <= seen, sorted(seen)
    paths = np.stack([np.where(c.in_tile, c.path, -1) for c in cs])                 # [tile][tri]
    in_tiles = (paths >= 0).sum(0)
    assert (in_tiles == 2).sum() >= 6 and (in_tiles == 4).sum() >= 2                # boxes over a tile border, and over the corner
    assert any(len(set(col[col >= 0])) > 1 for col in paths.T)                     # one triangle, two paths in two tiles
    for want in (k.big_area, k.huge_area):                                          # a straddler whose clipped area is exactly the threshold in both tiles
        assert any((np.stack([c.area for c in cs])[:, t][paths[:, t] >= 0] == want).sum() == 2 for t in range(paths.shape[1]))


def test_census_widths():
    for name, path, lo in (("widths_wave", 1, 1), ("widths_group", 2, 33)):
        case = sc.get(name, 128, 128)
        got = set()
        for _, _, c in _all(case):
            got |= set(c.bw[c.in_tile & (c.path == path)].tolist())
        assert got >= set(range(lo, 129)), sorted(set(range(lo, 129)) - got)
        own = [int(c.in_tile.sum()) for _, _, c in _all(case)]
        assert sum(own) == len(case.tris), own                                      # every triangle shows in exactly one env


def test_census_overflows():
    k = consts()
    (_, _, c), = _all(sc.get("huge_overflow", 128, 128))
    assert int((c.in_tile & (c.path == 2)).sum()) >= 80 > k.huge_cap
    case = sc.get("big_overflow", 128, 128)
    (_, _, c), = _all(case)
    assert case_plan(case).big_cap == k.big_cap_max and int((c.in_tile & (c.path == 1)).sum()) > k.big_cap_max


def test_census_many_chunks():
    case = sc.get("many_chunks", 128, 128)
    p = case_plan(case)
    assert p.accepted == 1 and 64 <= p.big_cap < 128, (p.n_chunks, p.big_cap)
    (_, _, c), = _all(case)
    assert int((c.in_tile & (c.path == 1)).sum()) > p.big_cap
    assert case.spheres.shape[1] == consts().max_spheres and (case.spheres[..., 7] > 0).all()
    assert p.big_cap * 4 < 16 * 8 * 4                                               # the 16 spheres (128 floats) spill past the big queue's LDS
    for clusters, over in ((sc.MANY_CLUSTERS + 300, False), (8300, True)):
        big = sc.many_chunks(clusters)
        q = plan(big.verts, big.tris, big.tri_frame, big.tri_rgb, 128, 128, tables=False)
        assert q.accepted == 0 and (q.n_chunks > q.max_chunks) == over and (over or q.big_cap < 64), (q.n_chunks, q.big_cap)


@pytest.mark.parametrize("size", sc.SIZES, ids=[f"{h}x{w}" for h, w in sc.SIZES])
def test_census_planes(size):
    case = sc.get("planes", *size)
    near, far = np.float32(case.near), np.float32(case.far)
    p = sc.project32(case, 0)
    before = (p.w < near).sum(1)
    assert (p.alive & (before == 1)).any() and (p.alive & (before == 2)).any() and (p.alive & ~p.all_near & (p.w < 0).any(1)).any()
    assert (p.alive & (p.w > far).any(1) & (p.w < far).any(1)).any()                # crossing far
    assert (before == 3).any() and (p.w > far).all(1).any()                         # wholly before near / beyond far
    assert (p.all_near & (p.w == near).any(1)).any()                                # a corner at w == near exactly: still all_near
    assert (np.abs(case.verts) == 100.0).any()                                      # the 200 m ground plane
    assert case_plan(case).n_chunks >= 10


def test_census_frames():
    for size in ((256, 256), (128, 256), (256, 128)):
        case = sc.get("frames", *size)
        p = case_plan(case)
        assert case.n_frames == 16 and set(case.tri_frame.tolist()) == set(range(16))
        norms = np.linalg.norm(case.xf[0][:, [0, 3, 6]].astype(np.float64), axis=1)
        assert abs(norms[5] - 0.3) < 1e-6 and abs(norms[9] - 3.0) < 1e-5 and np.allclose(np.delete(norms, [5, 9]), 1.0, atol=1e-6)
        for e in range(case.n):
            vis = np.stack([sc.chunk_visible(case, e, p.sphere, p.table[:, 2], tile) for tile in sc.tiles_of(case)])
            assert vis.any(1).all() and (~vis).any(1).all()                         # visible and culled chunks in every tile
            assert (vis.sum(0) >= 2).any()                                          # a chunk over a tile border
        # no triangle of a culled chunk reaches a pixel of the tile: the census' own boxes
        k = consts()
        owner = np.repeat(np.arange(p.n_chunks), p.table[:, 1])
        moved = SimpleNamespace(**{**case.__dict__, "verts": p.cverts, "tris": p.tris, "tri_frame": (p.attr >> 24).astype(np.uint8)})
        for e in range(case.n):
            for tile in sc.tiles_of(case):
                c = sc.census(moved, e, k, tile)
                vis = sc.chunk_visible(case, e, p.sphere, p.table[:, 2], tile)
                assert not (c.in_tile & ~vis[owner]).any()


def test_census_degenerate_heightfield_spheres():
    case = sc.get("degenerate", 128, 128)
    v = case.verts[case.tris]
    assert ((v[:, 0] == v[:, 1]).all(1)).any() and ((v[:, 0] == v[:, 1]).all(1) & (v[:, 1] == v[:, 2]).all(1)).any()
    same = (v[:-1].reshape(-1, 9) == v[1:].reshape(-1, 9)).all(1) & (case.tri_rgb[:-1] != case.tri_rgb[1:]).any(1)
    assert same.any()                                                               # two identical triangles of different colours
    perm = sc.get("degenerate_perm", 128, 128)
    assert not np.array_equal(perm.tris, case.tris) and np.array_equal(np.sort(perm.tris[:, 0]), np.sort(case.tris[:, 0]))
    names = {k[0] for k in sc.KEYS}
    for r, c in sc.HF_SHAPES:
        for s in ("sel", "nosel"):
            for m in ("mesh", "alone"):
                assert f"hf_{r}x{c}_{s}_{m}" in names
    hf = sc.get("hf_3x5_sel_mesh", 128, 128).hf
    assert set(hf.sel.tolist()) == {0, 1, 2} and hf.rows != hf.cols
    sp = sc.get("spheres16", 128, 128).spheres
    assert sp.shape[1] == 16 and (sp[0, :, 7] == 0).any() and np.array_equal(sp[0, 8], sp[1, 9]) and np.array_equal(sp[0, 9], sp[1, 8])
    for size in sc.SIZES:                                   # the sphere edge cases, against the projection
        case = sc.get("spheres16", *size)
        wall = np.zeros((case.H, case.W), bool); wall[:, :int(0.6 * case.W) - 1] = True          # the opaque wall at w = 1.5
        tr = [sc.sphere_trace(case, 0, s) for s in range(10)]
        vis = [m & (w >= case.near) & (w <= case.far) for m, w, _ in tr]
        assert (vis[0] & wall & (tr[0][1] < 1.5)).sum() >= 4                                       # in front of the wall
        assert (tr[1][0] & wall).sum() >= 4 and (tr[1][1][tr[1][0] & wall] > 1.5).all()           # behind it: hidden there
        m, w, _ = tr[3]; assert (m & (w < case.near)).any() and (m & (w >= case.near)).any()      # crossing near
        m, w, _ = tr[4]; assert m.any() and (w[m] > case.far).all()                               # beyond far
        assert np.linalg.norm(case.spheres[0, 5, :3]) < case.spheres[0, 5, 3] and not vis[5].any()   # the eye inside: the near intersection is behind
        assert tr[6][2] < 0.5                                                                      # a radius below half a pixel
        assert case.spheres[0, 7, 7] == 0 and tr[7][0].any()                                       # an alpha 0 slot that would show
        assert (vis[8] & vis[9]).sum() >= 4                                                        # two overlapping spheres
    assert sc.get("spheres0", 128, 128).spheres is None and sc.get("spheres1", 128, 128).spheres.shape[1] == 1
    assert any((sc.get(n, h, w).tri_frame == 0).any() for n, h, w in sc.KEYS)


def test_census_sphere_tangent():
    """At some pixel centre the sphere's float32 1 / w (mb_blend_spheres' expressions, restated) has exactly the bits of the wall's z key, on a
    fragment that passes every other test: only `strictly above` keeps the wall's colour there.  The restatement is the oracle's: the pixels
    it calls in front are exactly the pixels the oracle blended."""
    case = sc.get("sphere_tangent", 128, 128)
    imgs, keys = sc.oracle(case)
    ok, bits = sc.sphere_iw32(case, 0, 0)
    wall = (keys[0].reshape(case.H, case.W) >> np.uint64(32)).astype(np.uint32)
    assert (wall > 0).all() and case.spheres[0, 0, 7] == 1.0
    equal, front = ok & (bits == wall), ok & (bits > wall)
    assert equal.sum() >= 1 and front.sum() >= 8 and (ok & (bits < wall)).sum() >= 8
    blended = (imgs[0] != imgs[0][0, 0]).any(axis=2)
    assert np.array_equal(blended, front) and not blended[equal].any()


SHARE_CAP = 0.02


def compare_with_f64(case):
    """[(env, left-out share, largest difference outside the left-out pixels, bad pixel mask)] per distinct image of the case.
    Stated ties (degenerate: three coincident triangles, one wound the other way - float32 gives it depth bits of its own, so which of the
    two windings wins a pixel is the oracle's rounding): where the float64 images with only one winding drawn differ, the oracle must show
    one of the two; those pixels are stated, not counted as left out."""
    imgs, _ = sc.oracle(case)
    out, seen = [], set()
    ties = case.notes.get("stated_ties")
    for e in range(case.n):
        if imgs[e].tobytes() in seen:
            continue
        seen.add(imgs[e].tobytes())
        got = imgs[e].astype(np.float64)
        if ties:
            (ra, ua), (rb, ub) = scene_f64.render(case, e, drop=ties[2:]), scene_f64.render(case, e, drop=ties[:2])
            stated = (ra != rb).any(axis=2)
            assert stated.mean() > 0.02                                             # the tie is really in the picture
            diff = np.minimum(np.abs(got - ra).max(axis=2), np.abs(got - rb).max(axis=2))
            diff[~stated] = np.abs(got - ra).max(axis=2)[~stated]
            unsure = (ua | ub) & ~stated
            first = (np.abs(got - ra).max(axis=2) <= 1)[stated & ~(ua | ub)]
            assert 0 < first.sum()                                                  # (both windings win somewhere or one everywhere: either is the rule)
        else:
            ref, unsure = scene_f64.render(case, e)
            diff = np.abs(got - ref).max(axis=2)
        out.append((e, float(unsure.mean()), float(diff[~unsure].max()), (diff > 1.0) & ~unsure))
    return out


@pytest.mark.parametrize("key", sc.KEYS, ids=sc.IDS)
def test_oracle_against_f64(key):
    case = sc.get(*key)
    for e, share, worst, bad in compare_with_f64(case):
        print(f"f64 {case.name} {case.H}x{case.W} env {e}: left out {100 * share:.3f} %, largest difference {worst:.0f}")
        assert not bad.any(), (f"{case.name} {case.H}x{case.W} env {e}: {int(bad.sum())} pixels differ by more than one grey level, first (row, col) "
                               f"{np.argwhere(bad)[:4].tolist()}")
        assert share <= SHARE_CAP, f"{case.name} {case.H}x{case.W} env {e}: {100 * share:.2f} % of the image left out"
