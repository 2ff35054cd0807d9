"""k_render_blocks' step 4 (csrc/tg_raster.hip, TG_BLK_DEAL): every reached block is drawn whole by ONE wavefront, and the reached blocks are
dealt to the workgroup's four wavefronts by load - ranked by the number of records that reach them, handed out in snake order, rotated by the
env index.  A block that no wavefront takes, or that two take with different records, shows as a block that differs from the CPU oracle
(oracle/minibullet.c), so every check here is the byte-for-byte comparison of whole images, through the test library's tg_selftest_render
forced to the block kernel (tg_selftest_render_twice for the launch after a launch).

Meshes are built in eye space for the synthetic sensor of tests/raster_cases.py (90 degree view: a block of the 128 x 128 image is 0.25 wide in
normalised device coordinates, whatever the image size), at eye depths in front of its dome (w < 0.036), so that what is built is drawn:
    few1 .. few5    k small triangles, each inside its own 16 x 16 block of the 128 x 128 image: exactly k reached blocks, so 4 - k wavefronts
                    have nothing to draw; 5 envs, so that the rotation by env takes every value and comes round
    fan             32 triangles from the two sides of one block out beyond the image in 32 directions, their far vertex behind the near plane:
                    each is clipped to a quadrilateral, 64 records (rec_cap) that all reach that block, while the blocks around the rim are
                    reached by one or two - nearly every block reached, very unequal loads, one distinct count after another
    ties            32 small triangles in 32 different blocks: every load is 1, the ranks are the block indices
    soup32          raster_cases' random soup, at 128 x 128, 256 x 256 and 128 x 256 with 1, 3 and 65 envs, the last with an env mask and the
                    terminal layer
    moved           two launches on one buffer: the triangles of few5, then the same moved by two blocks - blocks the first launch drew and
                    the second no longer reaches are restored beside newly reached ones, and save_prev receives the first launch's images
"""
import ctypes as C

import numpy as np
import pytest

import raster_cases as rc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
W_NEAR_SIDE = 0.030        # eye depth of the small triangles: in front of the dome (0.036 ... 0.046) everywhere


def _tri_in_block(bx, by, w=W_NEAR_SIDE):
    """A triangle inside block (bx, by) of the 128 x 128 image, 8 pixels across, away from the block's sides."""
    px = [(16 * bx + 4.0, 16 * by + 4.0), (16 * bx + 12.0, 16 * by + 5.0), (16 * bx + 7.0, 16 * by + 12.0)]
    return [rc.eye_xy(x, y, w) + (-w,) for x, y in px]


def _blocks_case(name, blocks, n_envs=5):
    v = [p for bx, by in blocks for p in _tri_in_block(bx, by)]
    t = np.arange(len(v)).reshape(-1, 3)
    # about half a pixel of shift per env (a pixel of the 128-wide image is 2 w / 128 = 4.7e-4 at this depth; the triangles keep 4 pixels
    # from their block's sides): every env its own image, the same blocks
    xfs = [rc.xform(np.eye(3), (2.8e-4 * i, -2.0e-4 * i, 0.0)) for i in range(n_envs)]
    return rc.Case(name, v, t, np.stack(xfs))


FEW_BLOCKS = [(3, 2), (4, 5), (1, 6), (6, 1), (5, 4)]     # inside the dome's unpasted part, no two in one row or column of blocks


def _fan_case():
    v, t = [], []
    w = W_NEAR_SIDE
    cx, cy = 16 * 3 + 8.0, 16 * 4 + 8.0                       # the middle of block (3, 4)
    for k in range(32):
        a = 2 * np.pi * k / 32
        dx, dy = np.cos(a), np.sin(a)
        # two vertices 7 pixels to either side of the block's middle, across the direction; the third far out along it, behind the near plane
        # (w = 0.005 < near = 0.01): the near-plane clip leaves a quadrilateral, two records
        A = rc.eye_xy(cx - 7 * dy, cy + 7 * dx, w) + (-w,)
        B = rc.eye_xy(cx + 7 * dy, cy - 7 * dx, w) + (-w,)
        far = rc.eye_xy(cx + 400 * dx, cy + 400 * dy, 0.005) + (-0.005,)
        v += [A, B, far]
        t.append((3 * k, 3 * k + 1, 3 * k + 2))
    xfs = [rc.IDENT, rc.xform(np.eye(3), (2.0e-4, 1.0e-4, 0.0)), rc.xform(rc._rot(2, 0.05), (0.0, 0.0, 0.001))]
    return rc.Case("fan", v, t, np.stack(xfs))


def _ties_case():
    blocks = [(bx, by) for by in range(1, 7) for bx in range(1, 7) if (bx + by) % 2 == 0][:16] + \
             [(bx, by) for by in range(1, 7) for bx in range(1, 7) if (bx + by) % 2 == 1][:16]
    return _blocks_case("ties", blocks)


def _render(sensor, case, xfs, mask=None, term_xfs=None, term_mask=None, xfs2=None, mask2=None):
    """(images, terminal images or None, save_prev of the second launch or None) of k_render_blocks; every buffer starts as SENTINEL."""
    from tactile_gym_amd import _capi as capi
    from tactile_gym_amd.robot_model import MeshDesc
    fp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    xfs = np.ascontiguousarray(xfs, np.float32)
    n = xfs.shape[0]
    out = np.full((n, sensor.H, sensor.W), SENTINEL, np.uint8)

    def ptr(a, ty):
        return None if a is None else a.ctypes.data_as(ty)

    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    tx = None if term_xfs is None else np.ascontiguousarray(term_xfs, np.float32)
    tm = None if term_mask is None else np.ascontiguousarray(term_mask, np.uint8)
    to = None if term_xfs is None else np.full_like(out, SENTINEL)
    x2 = None if xfs2 is None else np.ascontiguousarray(xfs2, np.float32)
    m2 = None if mask2 is None else np.ascontiguousarray(mask2, np.uint8)
    prev = None if xfs2 is None else np.full_like(out, SENTINEL)
    mesh = MeshDesc(case.verts, case.tris)
    launched = C.c_int32(-7)
    L = capi.test_lib()
    r = L.tg_selftest_render_twice(C.byref(sensor.struct), C.byref(mesh.struct), 0, 0, 0.0, None, None, n, ptr(xfs, fp), capi.RK_BLOCKS, 1, 0, 0,
                                   ptr(m, u8), ptr(tx, fp), ptr(tm, u8), ptr(to, u8), ptr(out, u8), C.byref(launched), ptr(x2, fp), ptr(m2, u8),
                                   ptr(prev, u8))
    assert r == 0, L.tg_selftest_last_error()
    assert launched.value == capi.RK_BLOCKS
    return out, to, prev


_ORACLE = {}


def _oracle(sensor, case, xfs):
    """Oracle images of the case's mesh under xfs; each (sensor, case, transform) is drawn once and shared."""
    from oracle import minibullet as mb
    out = []
    for xf in np.asarray(xfs, np.float32).reshape(-1, 12):
        key = (sensor.name, case.name, xf.tobytes())
        if key not in _ORACLE:
            cur = sensor.nodef_dep.copy()
            mb.render_depth(case.verts, case.tris, xf, sensor.fov, rc.NEAR, rc.FAR, sensor.W, sensor.H, cur)
            img = mb.t_s_camera(cur, sensor.nodef_dep, sensor.nodef_gray, sensor.border_mask)
            img.setflags(write=False)
            _ORACLE[key] = img
        out.append(_ORACLE[key])
    return np.stack(out)


def _same(got, ref, what):
    for i in range(ref.shape[0]):
        bad = got[i] != ref[i]
        if bad.any():
            rows, cols = np.nonzero(bad)
            blocks = sorted({(int(r) // 16, int(c) // 16) for r, c in zip(rows, cols)})
            raise AssertionError(f"{what} env {i}: {int(bad.sum())} pixels differ from the oracle, in blocks (row, col) {blocks[:12]}")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_few_reached_blocks(k):
    """Exactly k reached blocks in 5 envs: wavefronts with nothing to draw, every rotation of the dealing."""
    sensor = rc.synthetic_sensor(128, 128)
    case = _blocks_case(f"few{k}", FEW_BLOCKS[:k])
    ref = _oracle(sensor, case, case.xfs)
    for i in range(ref.shape[0]):       # what was built is what is drawn: k blocks hold pressed pixels
        changed = {(r // 16, c // 16) for r, c in zip(*np.nonzero((ref[i] != 0) & (sensor.border_mask != 1)))}
        assert len(changed) == k, changed
    out, _, _ = _render(sensor, case, case.xfs)
    _same(out, ref, f"few{k}")


@pytest.mark.parametrize("size", [(128, 128), (256, 256), (128, 256)], ids=["128x128", "256x256", "128x256"])
@pytest.mark.parametrize("name", ["fan", "ties"])
def test_unequal_and_equal_loads(name, size):
    """fan: 64 records on one block, one or two on the rim's; ties: 32 blocks of load 1."""
    H, W = size
    sensor = rc.synthetic_sensor(W, H)
    case = _fan_case() if name == "fan" else _ties_case()
    ref = _oracle(sensor, case, case.xfs)
    if name == "fan" and size == (128, 128):    # nearly every block is drawn on (the pasted corners cannot be)
        changed = {(r // 16, c // 16) for r, c in zip(*np.nonzero((ref[0] != 0) & (sensor.border_mask != 1)))}
        assert len(changed) >= 48, len(changed)
    out, _, _ = _render(sensor, case, case.xfs)
    _same(out, ref, f"{name} {H}x{W}")


@pytest.mark.parametrize("size", [(128, 128), (256, 256), (128, 256)], ids=["128x128", "256x256", "128x256"])
def test_sizes_env_counts_mask_and_terminal_layer(size):
    """The random soup at 1, 3 and 65 envs; the 65 with an env mask and the terminal layer."""
    H, W = size
    sensor = rc.synthetic_sensor(W, H)
    case = {c.name: c for c in rc.mesh_cases()}["soup32"]
    base = case.xfs
    for n in (1, 3):
        out, _, _ = _render(sensor, case, base[:n])
        _same(out, _oracle(sensor, case, base[:n]), f"soup32 {H}x{W} n={n}")
    n = 65
    idx, tidx = np.arange(n) % len(base), (np.arange(n) + 1) % len(base)
    mask = (np.arange(n) % 5 != 1).astype(np.uint8)
    tmask = (np.arange(n) % 3 != 2).astype(np.uint8)
    out, term, _ = _render(sensor, case, base[idx], mask=mask, term_xfs=base[tidx], term_mask=tmask)
    ref = _oracle(sensor, case, base)
    drawn, both = mask.astype(bool), (mask & tmask).astype(bool)
    _same(out[drawn], ref[idx][drawn], f"soup32 {H}x{W} n=65 masked")
    assert (out[~drawn] == SENTINEL).all(), "a masked-out env was written"
    _same(term[both], ref[tidx][both], f"soup32 {H}x{W} n=65 terminal layer")
    assert (term[~both] == SENTINEL).all(), "the terminal image of an env without one was written"


def test_second_launch_restores_left_blocks_and_saves_the_old_images():
    """The triangles of few5, then moved two blocks to the right and one down on the same buffer: the second launch restores the blocks the
    first drew and it does not reach, draws the newly reached ones, and leaves the first launch's images in save_prev.  Env 2 is masked out
    of the second launch: it keeps its image and its save_prev."""
    sensor = rc.synthetic_sensor(128, 128)
    case = _blocks_case("few5", FEW_BLOCKS)
    step = 2.0 * W_NEAR_SIDE / 128 * 16                               # one block in eye space at the triangles' depth
    xfs2 = np.stack([rc.xform(np.eye(3), (xf[9] + (2 * step if i != 4 else 0.0), xf[10] - (step if i != 4 else 0.0), 0.0))
                     for i, xf in enumerate(case.xfs)])                # (env 4 stays where it was: the same blocks again)
    mask2 = np.array([1, 1, 0, 1, 1], np.uint8)
    ref1, ref2 = _oracle(sensor, case, case.xfs), _oracle(sensor, case, xfs2)
    assert (ref1[0] != ref2[0]).any() and (ref1[4] == ref2[4]).all()
    out, _, prev = _render(sensor, case, case.xfs, xfs2=xfs2, mask2=mask2)
    drawn = mask2.astype(bool)
    _same(out[drawn], ref2[drawn], "second launch")
    _same(out[~drawn], ref1[~drawn], "env masked out of the second launch")
    _same(prev[drawn], ref1[drawn], "save_prev")
    assert (prev[~drawn] == SENTINEL).all(), "save_prev of a masked-out env was written"
