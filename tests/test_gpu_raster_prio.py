"""k_render_blocks with its front end at raised issue priority (csrc/tg_raster.hip, TG_BLK_PRIO): s_setprio is a hint to the SIMD's arbiter
and cannot change a pixel, so every check is the byte-for-byte comparison with the CPU oracle (oracle/minibullet.c), through the test
library's tg_selftest_render / tg_selftest_render_twice forced to the block kernel, as tests/test_gpu_raster_deal.py does.

What the priority changes is who runs when workgroups of very different loads share a CU, so ONE launch holds workgroups of every load.  The
mesh is shared by a launch's envs; the loads are spread by per-env transforms of the 64-record fan of test_gpu_raster_deal:
    full        the fan in full view: nearly every block reached, 64 records on one of them
    partly      shifted by three and a half blocks: part of it off the image
    behind      pushed behind the sensor's dome: records, but no block is reached
    sliver      shifted until one or two blocks still show it (searched on the CPU with the oracle; the test fails if none is found)
    off         shifted off the image altogether: nothing to set up, nothing reached
Shapes: 128 x 128, 256 x 256 (four regions per env, each with a load of its own) and 128 x 256; 1, 5 and 65 envs; an env mask whose
masked-out envs - the first and the last of the batch among them - must keep every byte (guard images round the drawn ones), the terminal
layer, and a second launch on the same buffers with the loads permuted across the envs (restore path, save_prev)."""
import numpy as np
import pytest

import raster_cases as rc
from test_gpu_raster_deal import SENTINEL, W_NEAR_SIDE, _fan_case, _oracle, _render, _same

pytestmark = pytest.mark.gpu

PIX = 2.0 * W_NEAR_SIDE / 128          # one pixel of the 128-wide view in eye space at the fan's depth
KINDS = ("full", "partly", "behind", "sliver", "off")


def _changed_blocks(img, sensor):
    """The 16 x 16 blocks of an oracle image that hold a pressed pixel outside the pasted ring."""
    return {(r // 16, c // 16) for r, c in zip(*np.nonzero((img != 0) & (sensor.border_mask != 1)))}


_FOUND = {}


def _load_xfs(sensor):
    """{kind: transform} for the fan on this sensor; the sliver is searched with the oracle: the first shift along x that leaves one or two
    blocks changed."""
    if sensor.name in _FOUND:
        return _FOUND[sensor.name]
    case = _fan_case()
    eye = np.eye(3)
    xfs = {"full": rc.IDENT, "partly": rc.xform(eye, (56 * PIX, 0.0, 0.0)), "behind": rc.xform(eye, (0.0, 0.0, -0.05)),
           "off": rc.xform(eye, (0.0, 40.0, 0.0))}
    sliver = None
    for dx in np.arange(70.0, 84.0, 0.25):                     # (pixels of shift at the fan's depth: 56 leave half of it, 80 nothing)
        xf = rc.xform(eye, (dx * PIX, 0.0, 0.0))
        if 1 <= len(_changed_blocks(_oracle(sensor, case, xf[None])[0], sensor)) <= 2:
            sliver = xf
            break
    assert sliver is not None, "no shift leaves one or two blocks of the fan in the image"
    xfs["sliver"] = sliver
    ref = {k: _oracle(sensor, case, v[None])[0] for k, v in xfs.items()}
    n_blocks = (sensor.W // 16) * (sensor.H // 16)
    full, partly = len(_changed_blocks(ref["full"], sensor)), len(_changed_blocks(ref["partly"], sensor))
    assert full >= 0.7 * n_blocks * (128 * 128) / (sensor.W * sensor.H) or full >= 48, full       # what was built is what is drawn
    assert 0 < partly and _changed_blocks(ref["partly"], sensor) != _changed_blocks(ref["full"], sensor)
    assert not _changed_blocks(ref["behind"], sensor) and not _changed_blocks(ref["off"], sensor)
    _FOUND[sensor.name] = xfs
    return xfs


def _batch(sensor, n, shift=0):
    """n transforms that go round the five loads (env i: kind (i + shift) % 5), every env also moved by a fraction of a pixel of its own."""
    xfs = _load_xfs(sensor)
    out = []
    for i in range(n):
        xf = xfs[KINDS[(i + shift) % 5]].copy()
        xf[9] += 0.13 * PIX * (i // 5)
        out.append(xf)
    return np.stack(out)


@pytest.mark.parametrize("size", [(128, 128), (256, 256), (128, 256)], ids=["128x128", "256x256", "128x256"])
@pytest.mark.parametrize("n", [1, 5, 65])
def test_every_load_in_one_launch(size, n):
    H, W = size
    sensor = rc.synthetic_sensor(W, H)
    case = _fan_case()
    xfs = _batch(sensor, n)
    out, _, _ = _render(sensor, case, xfs)
    _same(out, _oracle(sensor, case, xfs), f"loads {H}x{W} n={n}")


@pytest.mark.parametrize("size", [(128, 128), (256, 256), (128, 256)], ids=["128x128", "256x256", "128x256"])
def test_env_mask_guard_images_and_terminal_layer(size):
    H, W = size
    sensor = rc.synthetic_sensor(W, H)
    case = _fan_case()
    n = 65
    xfs, txfs = _batch(sensor, n), _batch(sensor, n, shift=2)
    mask = (np.arange(n) % 7 != 3).astype(np.uint8)
    mask[0] = mask[n - 1] = 0                                  # guard images: the first and the last env of the batch are not drawn
    tmask = (np.arange(n) % 3 != 1).astype(np.uint8)
    out, term, _ = _render(sensor, case, xfs, mask=mask, term_xfs=txfs, term_mask=tmask)
    drawn, both = mask.astype(bool), (mask & tmask).astype(bool)
    _same(out[drawn], _oracle(sensor, case, xfs)[drawn], f"masked {H}x{W}")
    assert (out[~drawn] == SENTINEL).all(), "a masked-out env was written"
    _same(term[both], _oracle(sensor, case, txfs)[both], f"terminal layer {H}x{W}")
    assert (term[~both] == SENTINEL).all(), "the terminal image of an env without one was written"


@pytest.mark.parametrize("size", [(128, 128), (256, 256)], ids=["128x128", "256x256"])
def test_second_launch_with_the_loads_permuted(size):
    """Every env changes its load between the launches: blocks the first launch drew are restored where the second reaches less, drawn where
    it reaches more, and save_prev holds the first launch's images.  The first and the last env are masked out of the second launch."""
    H, W = size
    sensor = rc.synthetic_sensor(W, H)
    case = _fan_case()
    n = 10
    xfs1, xfs2 = _batch(sensor, n), _batch(sensor, n, shift=3)
    mask2 = np.ones(n, np.uint8)
    mask2[0] = mask2[n - 1] = 0
    out, _, prev = _render(sensor, case, xfs1, xfs2=xfs2, mask2=mask2)
    ref1, ref2 = _oracle(sensor, case, xfs1), _oracle(sensor, case, xfs2)
    drawn = mask2.astype(bool)
    _same(out[drawn], ref2[drawn], "second launch")
    _same(out[~drawn], ref1[~drawn], "env masked out of the second launch")
    _same(prev[drawn], ref1[drawn], "save_prev")
    assert (prev[~drawn] == SENTINEL).all(), "save_prev of a masked-out env was written"
