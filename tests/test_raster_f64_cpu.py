"""The CPU oracle's tactile raster (oracle/minibullet.c) against an independent float64 raster (tests/raster_f64.py) on the raster case set
(tests/raster_cases.py) and on the sensors' untouched images; launch_render's kernel choice for the product's stimuli, and the refusals of
kernels that cannot draw an input.  No GPU: the choice and the refusals are host code of the test library.

The oracle and the kernels share one single-precision specification and are compared with each other bit for bit by the
GPU suites; an error in that specification (a projection constant, the pixel centre, the depth formula, t_s_camera's thresholds) would pass
those.  Here every pixel the f32 arithmetic cannot legitimately decide otherwise must equal the float64 raster's byte, and the pixels that
can (raster_f64's ambiguity mask) must stay few, so the check cannot pass by calling everything ambiguous.
"""
import ctypes as C
import os

import numpy as np
import pytest

import raster_cases as rc
import raster_f64 as rf

MAX_AMBIGUOUS = 0.02         # per image
# cases built to put pixel centres on edges (e = 0 exactly, shared edges, T-junctions) and to graze faces: every such pixel is ambiguous
MAX_AMBIGUOUS_ON_EDGES = {"pixel_centres": 0.04, "slivers_grazing": 0.04}

_MESH = {c.name: c for c in rc.mesh_cases()}
_HF = {c.name: c for c in rc.heightfield_cases()}


def _check(name, sensor, verts, tris, xf):
    from oracle import minibullet as mb
    cur = sensor.nodef_dep.copy()
    mb.render_depth(verts, tris, xf, sensor.fov, rc.NEAR, rc.FAR, sensor.W, sensor.H, cur)
    ref = mb.t_s_camera(cur, sensor.nodef_dep, sensor.nodef_gray, sensor.border_mask)
    img, amb = rf.render_f64(verts, tris, xf, sensor.fov, rc.NEAR, rc.FAR, sensor.nodef_dep, sensor.nodef_gray, sensor.border_mask)
    bad = (img != ref) & ~amb
    assert not bad.any(), (f"{name} on {sensor.name}: {int(bad.sum())} unambiguous pixels differ, e.g. (row, col) "
                           f"{np.argwhere(bad)[:5].tolist()}: oracle {ref[bad][:5]}, f64 {img[bad][:5]}")
    frac = float(amb.mean())
    assert frac <= MAX_AMBIGUOUS_ON_EDGES.get(name, MAX_AMBIGUOUS), f"{name} on {sensor.name}: {100 * frac:.2f} % of the pixels ambiguous"
    return int((ref[sensor.border_mask == 0] > 0).sum())


@pytest.mark.parametrize("sensor", ["synthetic128", "synthetic128x256", "tactip128"])
@pytest.mark.parametrize("case", sorted(_MESH))
def test_oracle_matches_f64_raster_meshes(case, sensor):
    s = rc.fixture_sensor("tactip", 128) if sensor == "tactip128" else (rc.synthetic_sensor(128, 128) if sensor == "synthetic128"
                                                                        else rc.synthetic_sensor(256, 128))
    c = _MESH[case]
    touched = sum(_check(case, s, c.verts, c.tris, xf) for xf in c.xfs)
    if case != "far_zcull":      # (whose triangles lie behind the untouched skin by construction)
        assert touched > 0, f"{case}: nothing in contact - the case tests nothing"


@pytest.mark.parametrize("case", sorted(_HF))
def test_oracle_matches_f64_raster_heightfields(case):
    c = _HF[case]
    s = rc.hf_sensor(c, 128, 128)
    touched = 0
    for i in range(c.xfs.shape[0]):
        v, t = c.mesh(i)
        touched += _check(case, s, v, t, c.xfs[i])
    assert touched > 0


@pytest.mark.parametrize("name", ["tactip", "digit", "digitac"])
@pytest.mark.parametrize("size", [64, 128, 256])
def test_untouched_sensor_images(name, size):
    """Nothing in view: the border pasted from the reference image, zero elsewhere - on both rasters, with no ambiguous pixel."""
    from oracle import minibullet as mb
    s = rc.fixture_sensor(name, size)
    cur = s.nodef_dep.copy()
    mb.render_depth(np.zeros((1, 3), np.float32), np.zeros((0, 3), np.int32), rc.IDENT, s.fov, rc.NEAR, rc.FAR, size, size, cur)
    ref = mb.t_s_camera(cur, s.nodef_dep, s.nodef_gray, s.border_mask)
    img, amb = rf.render_f64(np.zeros((1, 3), np.float32), np.zeros((0, 3), np.int32), rc.IDENT, s.fov, rc.NEAR, rc.FAR, s.nodef_dep,
                             s.nodef_gray, s.border_mask)
    assert not amb.any()
    assert np.array_equal(img, ref)
    assert np.array_equal(ref, np.where(s.border_mask == 1, s.nodef_gray.astype(np.uint8), 0))


def test_f64_raster_sees_a_half_pixel_shift():
    """The f64 raster is not the oracle's restatement: a spec error of half a pixel (centres at integers) is caught by it."""
    from oracle import minibullet as mb
    s = rc.synthetic_sensor(128, 128)
    c = _MESH["soup33"]
    cur = s.nodef_dep.copy()
    mb.render_depth(c.verts, c.tris, c.xfs[0], s.fov, rc.NEAR, rc.FAR, 128, 128, cur)
    ref = mb.t_s_camera(cur, s.nodef_dep, s.nodef_gray, s.border_mask)
    # the same scene moved right by half a pixel: what a raster that samples at (px, py) instead of (px + 0.5, py + 0.5) would draw
    v = c.verts.astype(np.float64)
    v[:, 0] += 0.5 / 64.0 * (-v[:, 2])
    img, amb = rf.render_f64(v.astype(np.float32), c.tris, c.xfs[0], s.fov, rc.NEAR, rc.FAR, s.nodef_dep, s.nodef_gray, s.border_mask)
    assert ((img != ref) & ~amb).sum() > 100


# ------------------------------------------------------------------------------------------------- launch_render's choice, without a device
def _kernel_of(sensor, mesh=None, hf=None, kernel=0, sqr=1, fills=0, cull=0):
    from tactile_gym_amd import _capi as capi
    out = C.c_int32(-7)
    if hf is None:
        rc_ = capi.test_lib().tg_selftest_render_kernel(C.byref(sensor.struct), C.byref(mesh.struct), 0, 0, 0.0, kernel, sqr, fills, cull,
                                                       C.byref(out))
    else:
        rows, cols, scale = hf
        rc_ = capi.test_lib().tg_selftest_render_kernel(C.byref(sensor.struct), None, rows, cols, scale, kernel, 0, 0, 0, C.byref(out))
    assert rc_ == 0, capi.test_lib().tg_selftest_last_error()
    return out.value


def _asset_mesh(name):
    from tactile_gym_amd.robot_model import ASSETS, MeshDesc
    d = "stimuli" if name.endswith("_edge") else "objects"
    z = np.load(os.path.join(ASSETS, d, f"{name}.npz"))
    return MeshDesc(z["verts"], z["tris"])


def test_product_dispatch_table():
    """The kernel every environment's stimulus is drawn with (tg_create's flags: skip_quad_reject on every shared mesh, fills_view for
    object_balance's bodies)."""
    from tactile_gym_amd import _capi as capi
    for size in (64, 128, 256):
        s = rc.fixture_sensor("tactip", size)
        for name in ("long_edge", "short_edge", "cube"):
            assert _kernel_of(s, _asset_mesh(name)) == (capi.RK_TACTILE_64 if size == 64 else capi.RK_BLOCKS), (name, size)
        for name in ("pole", "round_plate"):       # object_balance's pole and ball_on_plate: fills the view
            assert _kernel_of(s, _asset_mesh(name), fills=1) == (capi.RK_TACTILE_64 if size == 64 else capi.RK_SMALL), (name, size)
        for name, fills in (("sphere", 0), ("plate_buffer", 1)):   # the marble (object_roll), the spinning plate
            assert _kernel_of(s, _asset_mesh(name), fills=fills) == (capi.RK_SCATTER_64 if size == 64 else capi.RK_SCATTER_128), (name, size)
    for name in ("digit", "digitac", "tactip"):     # surface_follow: 64 x 64 grid, 6 mm
        for size in (128, 256):
            want = capi.RK_HF_BANDS if name == "tactip" else capi.RK_HF_CELLS
            assert _kernel_of(rc.fixture_sensor(name, size), hf=(64, 64, 0.006)) == want, (name, size)
        assert _kernel_of(rc.fixture_sensor(name, 64), hf=(64, 64, 0.006)) == capi.RK_TACTILE_64
    # the direct entry without the product's flag keeps the per-quad reject kernel reachable
    m33 = rc.mesh_cases()[1]
    from tactile_gym_amd.robot_model import MeshDesc
    assert _kernel_of(rc.synthetic_sensor(128, 128), MeshDesc(m33.verts, m33.tris), sqr=0) == capi.RK_SMALL_QREJ


def test_forced_kernels_refused_when_they_cannot_draw():
    from tactile_gym_amd import _capi as capi
    from tactile_gym_amd.robot_model import MeshDesc
    cases = {c.name: MeshDesc(c.verts, c.tris) for c in rc.mesh_cases()}
    s64, s128, s256x128 = rc.synthetic_sensor(64, 64), rc.synthetic_sensor(128, 128), rc.synthetic_sensor(256, 128)
    hf = (64, 64, 0.006)
    refused = [(s128, cases["soup33"], None, capi.RK_BLOCKS), (s128, cases["soup257"], None, capi.RK_SMALL),
               (s128, cases["soup257"], None, capi.RK_SMALL_QREJ), (s64, cases["soup32"], None, capi.RK_BLOCKS),
               (s64, cases["soup32"], None, capi.RK_SCATTER_128), (s64, cases["soup32"], None, capi.RK_TACTILE_128),
               (s64, cases["soup32"], None, capi.RK_SMALL), (s128, cases["soup32"], None, capi.RK_HF_BANDS),
               (s128, cases["soup32"], None, capi.RK_HF_CELLS), (s128, None, hf, capi.RK_BLOCKS), (s128, None, hf, capi.RK_SCATTER_128),
               (s128, None, hf, capi.RK_SCATTER_64), (s128, None, hf, capi.RK_SMALL), (s64, None, hf, capi.RK_HF_BANDS)]
    for s, mesh, h, k in refused:
        assert _kernel_of(s, mesh, h, kernel=k) == -1, (s.name, k)
    accepted = [(s128, cases["soup32"], None, capi.RK_BLOCKS), (s256x128, cases["soup256"], None, capi.RK_SMALL),
                (s128, cases["soup1500"], None, capi.RK_TACTILE_64), (s256x128, None, hf, capi.RK_HF_CELLS),
                (s64, cases["soup33"], None, capi.RK_SCATTER_64)]
    for s, mesh, h, k in accepted:
        assert _kernel_of(s, mesh, h, kernel=k) == k, (s.name, k)
    # a back-face cull asked for a mesh that is not closed: refused (the cull would not be licensed)
    out = C.c_int32()
    assert capi.test_lib().tg_selftest_render_kernel(C.byref(s128.struct), C.byref(cases["soup32"].struct), 0, 0, 0.0, 0, 1, 0, 1,
                                                     C.byref(out)) == -1
    assert _kernel_of(s128, cases["boxes_interpenetrating"], cull=1) == capi.RK_BLOCKS


def test_direct_render_refuses_more_envs_than_grid_y_holds():
    """tg_render_tactile / tg_render_tactile_heightfield: n = 65536 is refused before anything touches a device (grid.y <= 65535)."""
    from tactile_gym_amd import _capi as capi
    s = rc.synthetic_sensor(64, 64)
    from tactile_gym_amd.robot_model import MeshDesc
    m = MeshDesc(_MESH["soup32"].verts, _MESH["soup32"].tris)
    xf = np.zeros((1, 12), np.float32)
    out = np.zeros(1, np.uint8)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    assert capi.lib().tg_render_tactile(C.byref(s.struct), C.byref(m.struct), 65536, xf.ctypes.data_as(fp), out.ctypes.data_as(u8)) == -1
    h, z = np.zeros(4), np.zeros(1, np.float32)
    assert capi.lib().tg_render_tactile_heightfield(C.byref(s.struct), 2, 2, 0.006, 65536, h.ctypes.data_as(C.POINTER(C.c_double)),
                                                    z.ctypes.data_as(fp), xf.ctypes.data_as(fp), out.ctypes.data_as(u8)) == -1
