"""Every raster kernel launch_render can launch, forced through the test library (tg_selftest_render), on the raster case set
(tests/raster_cases.py) at every image size it can draw: each image byte-identical to the CPU oracle, so every kernel that can draw an input
gives the same bytes; the kernel launched is the one asked for.  Plus, per kernel, the env mask and the fused auto-reset's terminal layer,
and the env counts 1, ragged, and 65535 (the most grid.y holds; 65536 is refused).
"""
import ctypes as C

import numpy as np
import pytest

import raster_cases as rc

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (128, 128), (256, 256), (128, 256), (256, 128)]     # (H, W)
SENTINEL = 0xA5


def _kernels():
    from tactile_gym_amd import _capi as capi
    mesh = [capi.RK_BLOCKS, capi.RK_SMALL_QREJ, capi.RK_SMALL, capi.RK_TACTILE_128, capi.RK_TACTILE_64, capi.RK_SCATTER_128, capi.RK_SCATTER_64]
    hf = [capi.RK_HF_BANDS, capi.RK_HF_CELLS, capi.RK_TACTILE_128, capi.RK_TACTILE_64]
    return mesh, hf


def _sensor(H, W, hf_case=None):
    return rc.synthetic_sensor(W, H) if hf_case is None else rc.hf_sensor(hf_case, H, W)


def _mesh_desc(case):
    from tactile_gym_amd.robot_model import MeshDesc
    return MeshDesc(case.verts, case.tris)


def render(sensor, case, kernel, xfs=None, mask=None, term_xfs=None, term_mask=None, cull=0, n=None):
    """(rc, launched kernel, images [n][H][W], terminal images or None); images start as SENTINEL."""
    from tactile_gym_amd import _capi as capi
    xfs = np.ascontiguousarray(case.xfs if xfs is None else xfs, np.float32)
    n = xfs.shape[0] if n is None else n
    out = np.full((n, sensor.H, sensor.W), SENTINEL, np.uint8)
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    launched = C.c_int32(-7)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    tx = tm = to = None
    if term_xfs is not None:
        tx, tm = np.ascontiguousarray(term_xfs, np.float32), np.ascontiguousarray(term_mask, np.uint8)
        to = np.full_like(out, SENTINEL)
    args = [m.ctypes.data_as(u8) if m is not None else None, tx.ctypes.data_as(fp) if tx is not None else None,
            tm.ctypes.data_as(u8) if tm is not None else None, to.ctypes.data_as(u8) if to is not None else None]
    L = capi.test_lib()
    if case.kind == "mesh":
        mesh = _mesh_desc(case)
        r = L.tg_selftest_render(C.byref(sensor.struct), C.byref(mesh.struct), 0, 0, 0.0, None, None, n, xfs.ctypes.data_as(fp), kernel, 1, 0,
                                 cull, *args, out.ctypes.data_as(u8), C.byref(launched))
    else:
        h = np.ascontiguousarray(case.heights[:n], np.float64)
        z = np.ascontiguousarray(case.zoff[:n], np.float32)
        r = L.tg_selftest_render(C.byref(sensor.struct), None, case.rows, case.cols, case.scale, h.ctypes.data_as(C.POINTER(C.c_double)),
                                 z.ctypes.data_as(fp), n, xfs.ctypes.data_as(fp), kernel, 0, 0, 0, *args, out.ctypes.data_as(u8),
                                 C.byref(launched))
    return r, launched.value, out, to


def _can_draw(sensor, case, kernel, cull=0):
    from tactile_gym_amd import _capi as capi
    got = C.c_int32(-7)
    if case.kind == "mesh":
        mesh = _mesh_desc(case)
        r = capi.test_lib().tg_selftest_render_kernel(C.byref(sensor.struct), C.byref(mesh.struct), 0, 0, 0.0, kernel, 1, 0, cull, C.byref(got))
    else:
        r = capi.test_lib().tg_selftest_render_kernel(C.byref(sensor.struct), None, case.rows, case.cols, case.scale, kernel, 0, 0, 0, C.byref(got))
    assert r == 0
    assert got.value in (kernel, -1)
    return got.value == kernel


def _oracle(sensor, case, xfs):
    """Oracle images of the case's stimulus under transforms xfs (env i: the case's env i % n_case for heightfields)."""
    from oracle import minibullet as mb
    out = []
    for i, xf in enumerate(xfs):
        v, t = (case.verts, case.tris) if case.kind == "mesh" else case.mesh(i % case.xfs.shape[0])
        cur = sensor.nodef_dep.copy()
        mb.render_depth(v, t, xf, sensor.fov, rc.NEAR, rc.FAR, sensor.W, sensor.H, cur)
        out.append(mb.t_s_camera(cur, sensor.nodef_dep, sensor.nodef_gray, sensor.border_mask))
    return np.stack(out)


_CASES = {c.name: c for c in rc.mesh_cases() + rc.heightfield_cases()}


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_every_kernel_matches_the_oracle(name, size):
    H, W = size
    case = _CASES[name]
    sensor = _sensor(H, W, case if case.kind == "hf" else None)
    mesh_k, hf_k = _kernels()
    ref = _oracle(sensor, case, case.xfs)
    drawn = []
    for cull in ((0, 1) if case.kind == "mesh" and case.closed else (0,)):
        for k in (mesh_k if case.kind == "mesh" else hf_k):
            if not _can_draw(sensor, case, k, cull):
                r, launched, _, _ = render(sensor, case, k, cull=cull)
                assert r == -1 and launched == -1, f"kernel {k} cannot draw {name} at {H}x{W} but was launched"
                continue
            r, launched, out, _ = render(sensor, case, k, cull=cull)
            assert r == 0, f"kernel {k}: rc {r}"
            assert launched == k
            for i in range(out.shape[0]):
                bad = out[i] != ref[i]
                assert not bad.any(), (f"{name} {H}x{W} kernel {k} cull {cull} env {i}: {int(bad.sum())} pixels differ from the oracle, first "
                                       f"(row, col) {np.argwhere(bad)[:4].tolist()}: kernel {out[i][bad][:4]}, oracle {ref[i][bad][:4]}")
            drawn.append(k)
    # which kernels can draw what: every 64-multiple image has the 64 x 64 kernels, every 128-multiple one the rest
    want = {k for k in (mesh_k if case.kind == "mesh" else hf_k) if (H % 128 == 0 and W % 128 == 0) or k in (7, 9)}
    from tactile_gym_amd import _capi as capi
    if case.kind == "mesh" and case.tris.shape[0] > 32:
        want.discard(capi.RK_BLOCKS)
    if case.kind == "mesh" and case.tris.shape[0] > 256:
        want -= {capi.RK_SMALL, capi.RK_SMALL_QREJ}
    assert set(drawn) == want, (sorted(set(drawn)), sorted(want))


def _mask_case(kernel):
    from tactile_gym_amd import _capi as capi
    return _CASES["hf_48x80"] if kernel in (capi.RK_HF_BANDS, capi.RK_HF_CELLS) else _CASES["soup32"]


@pytest.mark.parametrize("kernel", range(1, 10))
def test_mask_and_terminal_layer(kernel):
    """Envs whose mask byte is 0 keep their image; envs flagged in term_mask (and mask) get the terminal image too, the others keep the
    terminal buffer; every drawn image equals the oracle."""
    case = _mask_case(kernel)
    H = W = 128
    sensor = _sensor(H, W, case if case.kind == "hf" else None)
    n = 5
    base = case.xfs
    xfs = np.stack([base[i % len(base)] for i in range(n)])
    txfs = np.stack([base[(i + 1) % len(base)] for i in range(n)])
    if case.kind == "hf":    # the terminal image of env i shows env i's heightfield: draw it from another camera height
        txfs = txfs.copy()
        txfs[:, 11] += 0.001
        case = rc.HfCase(case.name, np.stack([case.heights[i % len(base)] for i in range(n)]),
                         np.array([case.zoff[i % len(base)] for i in range(n)], np.float32), case.scale, xfs, case.sensor_name)
    mask = np.array([1, 0, 1, 1, 0], np.uint8)
    tmask = np.array([1, 1, 0, 1, 0], np.uint8)
    r, launched, out, term = render(sensor, case, kernel, xfs=xfs, mask=mask, term_xfs=txfs, term_mask=tmask)
    assert r == 0 and launched == kernel
    ref, tref = _oracle(sensor, case, xfs), _oracle(sensor, case, txfs)
    for i in range(n):
        if mask[i]:
            assert np.array_equal(out[i], ref[i]), f"kernel {kernel} env {i}: {(out[i] != ref[i]).sum()} pixels differ"
        else:
            assert (out[i] == SENTINEL).all(), f"kernel {kernel}: masked-out env {i} was written"
        if mask[i] and tmask[i]:
            assert np.array_equal(term[i], tref[i]), f"kernel {kernel} env {i}: terminal image, {(term[i] != tref[i]).sum()} pixels differ"
        else:
            assert (term[i] == SENTINEL).all(), f"kernel {kernel}: terminal image of env {i} written"
    assert (tref[mask.astype(bool) & tmask.astype(bool)] != ref[mask.astype(bool) & tmask.astype(bool)]).any()   # the two layers differ


@pytest.mark.parametrize("n", [1, 37, 65535])
def test_env_counts(n):
    """n = 1, a ragged count and the most grid.y holds, at 64 x 64 with the kernel the product chooses; every env against the oracle of
    its transform (7 distinct ones, env i takes i % 7).  n = 65536 is refused by the test entry and by tg_render_tactile."""
    from tactile_gym_amd import _capi as capi, hip_ops
    case = _CASES["soup257"]
    sensor = rc.synthetic_sensor(64, 64)
    rng = np.random.default_rng(n)
    distinct = np.stack([case.xfs[0]] + [rc.xform(rc._rot(0, a) @ rc._rot(1, b), (0.002 * a, -0.001 * b, 0.0))
                                         for a, b in rng.normal(0, 0.05, size=(6, 2))])
    ref = _oracle(sensor, case, distinct)
    idx = np.arange(n) % 7
    r, launched, out, _ = render(sensor, case, capi.RK_AUTO, xfs=distinct[idx])
    assert r == 0 and launched == capi.RK_SCATTER_64
    bad = (out.reshape(n, -1) != ref.reshape(7, -1)[idx]).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {n} envs differ from the oracle, first {np.nonzero(bad)[0][:8].tolist()}"
    if n == 65535:
        xf = np.zeros((65536, 12), np.float32)
        r, launched, _, _ = render(sensor, case, capi.RK_AUTO, xfs=xf)
        assert r == -1 and launched == -1
        with pytest.raises(Exception):
            hip_ops.render_tactile(sensor, _mesh_desc(case), xf)
