"""The scene camera kernel (csrc/tg_scene.hip: k_scene) called directly through the test library (tg_selftest_scene: the product's own
build_scene_chunks, scene_prepare, launch_scene_static, launch_scene) on the case table of tests/scene_cases.py: every case, at every image
size it is listed for, byte-identical to the CPU oracle (mb_render_scene + mb_blend_spheres), with the static pass and without; the env
mask with save_prev; the env counts 1, 37 and 65535 (the most grid.y holds; 65536 is refused); and the refusals.
tests/test_scene_cases_cpu.py shows that each case reaches the branch it is named for.
"""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def draw(case, use_static=0, mask=None, prev=None, n=None, xf=None, spheres=None, n_frames=None, side=None, fill=SENTINEL):
    """(rc, images [n][H][W][3], prev); images start as `fill` (an array: as given)."""
    from tactile_gym_amd import _capi as capi
    fp, ip, u8, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
    xf = np.ascontiguousarray(case.xf if xf is None else xf, np.float32)
    n = xf.shape[0] if n is None else n
    H, W = (case.H, case.W) if side is None else side
    s = capi.TgSceneTest()
    s.image_h, s.image_w, s.n_verts, s.n_tris = H, W, len(case.verts), len(case.tris)
    keep = [np.ascontiguousarray(case.verts), np.ascontiguousarray(case.tris), np.ascontiguousarray(case.tri_frame), np.ascontiguousarray(case.tri_rgb)]
    if len(case.tris):
        s.verts, s.tris, s.tri_frame, s.tri_rgb = keep[0].ctypes.data_as(fp), keep[1].ctypes.data_as(ip), keep[2].ctypes.data_as(u8), keep[3].ctypes.data_as(u8)
    s.n_frames, s.use_static = (xf.shape[1] if n_frames is None else n_frames), use_static
    s.fov_deg, s.near_plane, s.far_plane = case.fov, case.near, case.far
    for k in range(3):
        s.light_eye[k], s.background[k] = float(case.light[k]), int(case.background[k])
    if case.hf is not None:
        hf = case.hf
        keep += [np.ascontiguousarray(hf.heights, np.float64), np.ascontiguousarray(hf.zoff, np.float32)]
        s.hf_heights, s.hf_zoff, s.hf_rows, s.hf_cols, s.hf_scale = keep[-2].ctypes.data_as(dp), keep[-1].ctypes.data_as(fp), hf.rows, hf.cols, hf.scale
        if hf.sel is not None:
            keep.append(np.ascontiguousarray(hf.sel, np.uint8))
            s.hf_sel = keep[-1].ctypes.data_as(u8)
        for k in range(3):
            s.hf_rgb[k] = hf.rgb[k]
    spheres = case.spheres if spheres is None else spheres
    if spheres is not None:
        keep.append(np.ascontiguousarray(spheres, np.float32))
        s.spheres, s.n_spheres = keep[-1].ctypes.data_as(fp), spheres.shape[1]
    out = np.full((n, H, W, 3), fill, np.uint8) if np.isscalar(fill) else np.ascontiguousarray(fill).copy()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    r = capi.test_lib().tg_selftest_scene(C.byref(s), n, xf.ctypes.data_as(fp), None if m is None else m.ctypes.data_as(u8), out.ctypes.data_as(u8),
                                          None if prev is None else prev.ctypes.data_as(u8))
    return r, out, prev


def report(case, tag, out, ref):
    for i in range(out.shape[0]):
        bad = (out[i] != ref[i]).any(axis=2)
        assert not bad.any(), (f"{case.name} {case.H}x{case.W} {tag} env {i}: {int(bad.sum())} pixels differ from the oracle, first (row, col) "
                               f"{np.argwhere(bad)[:4].tolist()}: kernel {out[i][bad][:4].tolist()}, oracle {ref[i][bad][:4].tolist()}")


@pytest.mark.parametrize("key", sc.KEYS, ids=sc.IDS)
def test_every_case_matches_the_oracle(key):
    case = sc.get(*key)
    ref, _ = sc.oracle(case)
    r, out, _ = draw(case)
    assert r == 0
    report(case, "per env", out, ref)
    if (case.tri_frame == 0).any():                           # the static pass draws frame 0 once instead: the same bytes
        r, out1, _ = draw(case, use_static=1)
        assert r == 0
        report(case, "static", out1, ref)
        assert np.array_equal(out, out1)


def test_static_pass_is_exercised():
    assert sum(1 for k in sc.KEYS if (sc.get(*k).tri_frame == 0).any()) >= 30


@pytest.mark.parametrize("size", sc.SIZES, ids=[f"{h}x{w}" for h, w in sc.SIZES])
def test_triangle_order_does_not_matter(size):
    a, b = sc.get("degenerate", *size), sc.get("degenerate_perm", *size)
    ra, oa, _ = draw(a, use_static=1)
    rb, ob, _ = draw(b)
    assert ra == 0 and rb == 0 and np.array_equal(oa, ob)
    report(a, "static", oa, sc.oracle(a)[0])


@pytest.mark.parametrize("name,size", [("frames", (128, 256)), ("hf_3x5_sel_mesh", (48, 80)), ("spheres16", (256, 128))])
def test_mask_and_save_prev(name, size):
    """n = 5, mask 1 0 1 1 0: masked-out envs keep the sentinel in out and in prev; drawn envs get prev = what out held, out = the oracle."""
    base = sc.get(name, *size)
    n, idx = 5, np.arange(5) % base.n
    case = sc.make_case(base.name + "_mask", base.H, base.W, base.verts, base.tris, base.tri_frame, base.tri_rgb, base.xf[idx], hf=base.hf,
                        spheres=None if base.spheres is None else base.spheres[idx])
    if base.hf is not None:
        hf = base.hf
        case.hf = type(hf)(**{**hf.__dict__, "heights": hf.heights[..., idx, :], "zoff": hf.zoff[..., idx], "sel": None if hf.sel is None else hf.sel[idx]})
    ref, _ = sc.oracle(case)
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    held = np.random.default_rng(0).integers(0, 256, (n, case.H, case.W, 3)).astype(np.uint8)
    held[mask == 0] = SENTINEL
    prev = np.full_like(held, SENTINEL)
    for static in (0, 1):
        p = prev.copy()
        r, out, p = draw(case, use_static=static, mask=mask, prev=p, fill=held)
        assert r == 0
        for i in range(n):
            if mask[i]:
                assert np.array_equal(p[i], held[i]), f"env {i}: prev is not the image out held"
                report(case, f"masked static {static}", out[i:i + 1], ref[i:i + 1])
            else:
                assert (out[i] == SENTINEL).all() and (p[i] == SENTINEL).all(), f"masked-out env {i} was written"


@pytest.mark.parametrize("n", [1, 37, 65535])
def test_env_counts(n):
    case, idx = sc.tiny(n)
    seven, _ = sc.tiny(7)
    ref, _ = sc.oracle(seven)
    assert len({ref[i].tobytes() for i in range(7)}) == 7
    for static in (0, 1):
        r, out, _ = draw(case, use_static=static)
        assert r == 0
        bad = (out.reshape(n, -1) != ref.reshape(7, -1)[idx]).any(axis=1)
        assert not bad.any(), f"{int(bad.sum())} of {n} envs differ from the oracle, first {np.nonzero(bad)[0][:8].tolist()}"
    if n == 65535:
        big, _ = sc.tiny(65536)
        r, out, _ = draw(big)
        assert r == -1 and (out == SENTINEL).all()


def test_refusals():
    """Each returns -1 and writes nothing: the many_chunks scene with a few more chunks (big_cap < 64), with more than 8192 chunks, 17
    spheres, 17 frames, a side above 128 that is no multiple of 128, a bad projection, an index out of range."""
    for clusters in (sc.MANY_CLUSTERS + 300, 8300):
        r, out, _ = draw(sc.many_chunks(clusters))
        assert r == -1 and (out == SENTINEL).all(), clusters
    case = sc.get("spheres16", 128, 128)
    r, out, _ = draw(case, spheres=np.concatenate([case.spheres, case.spheres[:, :1]], 1))
    assert r == -1 and (out == SENTINEL).all()
    r, out, _ = draw(case, xf=np.tile(case.xf[:, :1], (1, 17, 1)))
    assert r == -1 and (out == SENTINEL).all()
    for side in ((192, 128), (128, 130)):
        r, out, _ = draw(case, side=side)
        assert r == -1 and (out == SENTINEL).all(), side
    tris = case.tris.copy(); tris[3, 1] = len(case.verts)
    fr = case.tri_frame.copy(); fr[0] = case.n_frames
    for what, kw in (("near = 0", dict(near=0.0)), ("far < near", dict(far=0.05)), ("fov = 180", dict(fov=180.0)), ("vertex index", dict(tris=tris)),
                     ("tri_frame", dict(tri_frame=fr))):
        a = dict(verts=case.verts, tris=case.tris, tri_frame=case.tri_frame, tri_rgb=case.tri_rgb)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        r, out, _ = draw(sc.make_case("bad", 128, 128, a["verts"], a["tris"], a["tri_frame"], a["tri_rgb"], case.xf, spheres=case.spheres, **kw))
        assert r == -1 and (out == SENTINEL).all(), what
    r, out, _ = draw(case)                                     # and the entry still draws after the refusals
    assert r == 0 and np.array_equal(out, sc.oracle(case)[0])
