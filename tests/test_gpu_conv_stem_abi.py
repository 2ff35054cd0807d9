"""tg_conv_stem, tg_conv_stem_bwd_workspace and tg_conv_stem_bwd (csrc/tg_conv_stem.hip) called directly on raw pointers, every buffer between
guard bytes inside a larger allocation: the shapes of tests/conv_stem_ref.py (one output, non-square images in both layouts, every channel
count up to the limit, 65 images, the 961-position M tail of 128 x 128, more than one column chunk), uint8 and float32 input.

On the grid cases float32 arithmetic is exact in every order, so the float64 restatement IS the required bits; on random weights the results
lie within the derived bounds (conv_stem_ref's docstring).  An image's output must not depend on the batch around it; two backward calls must
give the same bits; the error returns take no launch and write nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conv_stem_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN, Guarded  # noqa: E402

f32 = np.float32


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _p(g):
    return C.c_void_p(g.ptr if g is not None else None)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dims(x, channels_first):
    B = x.shape[0]
    Cn, H, W = x.shape[1:] if channels_first else (x.shape[3], x.shape[1], x.shape[2])
    return B, Cn, H, W


def _forward(x, w, b, scale, channels_first):
    """One tg_conv_stem call between guards -> host float32 [B, 32, OH, OW]; the inputs must come back unchanged."""
    capi, L = _lib()
    B, Cn, H, W = _dims(x, channels_first)
    OH, OW = ref.out_hw(H, W)
    gx, gw, gb = Guarded(x.nbytes, fill=x), Guarded(w.nbytes, fill=w), Guarded(b.nbytes, fill=b)
    gy = Guarded(4 * B * 32 * OH * OW)
    capi.check(L.tg_conv_stem(_p(gx), int(x.dtype == f32), int(channels_first), B, Cn, H, W, _p(gw), _p(gb), float(scale), _p(gy), _stream()))
    torch.cuda.synchronize()
    for g in (gx, gw, gb, gy):
        assert g.guards_intact()
    assert _bits(gx.host(x.dtype).reshape(x.shape), x) and _bits(gw.host(f32).reshape(w.shape), w) and _bits(gb.host(f32), b)
    return gy.host(f32).reshape(B, 32, OH, OW)


def _backward(x, y, dy, scale, channels_first, shrink=0, twice=False):
    """One tg_conv_stem_bwd call (two with twice=True, into fresh outputs) with a workspace of exactly the queried size less `shrink` bytes
    -> (dweight, dbias) host float32, or the return code when shrink > 0."""
    capi, L = _lib()
    B, Cn, H, W = _dims(x, channels_first)
    nbytes = L.tg_conv_stem_bwd_workspace(B, Cn, H, W)
    assert nbytes > 0
    gx, gy, gdy = Guarded(x.nbytes, fill=x), Guarded(y.nbytes, fill=y), Guarded(dy.nbytes, fill=dy)
    gws = Guarded(nbytes - shrink)
    results = []
    for _ in range(2 if twice else 1):
        gdw, gdb = Guarded(4 * 32 * Cn * 64), Guarded(4 * 32)
        rc = L.tg_conv_stem_bwd(_p(gx), int(x.dtype == f32), int(channels_first), B, Cn, H, W, _p(gy), _p(gdy), float(scale), _p(gdw), _p(gdb),
                                _p(gws), nbytes - shrink, _stream())
        torch.cuda.synchronize()
        for g in (gx, gy, gdy, gws, gdw, gdb):
            assert g.guards_intact()
        if shrink:
            assert rc != 0 and L.tg_last_error().decode().startswith("tg_conv_stem_bwd:")
            assert bool((gdw.payload() == PATTERN).all()) and bool((gdb.payload() == PATTERN).all()) and bool((gws.payload() == PATTERN).all())
            return rc
        capi.check(rc)
        assert _bits(gx.host(x.dtype).reshape(x.shape), x) and _bits(gy.host(f32).reshape(y.shape), y) and _bits(gdy.host(f32).reshape(dy.shape), dy)
        results.append((gdw.host(f32).reshape(32, Cn, 8, 8).copy(), gdb.host(f32).copy()))
    if twice:
        assert _bits(results[0][0], results[1][0]) and _bits(results[0][1], results[1][1])
    return results[0]


def _within(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: largest error / bound = {ratio:.3g}")
    assert (err <= bound).all(), (what, ratio)


def _id(case):
    H, W, Cn, B, cf, fl = case
    return f"{H}x{W}-c{Cn}-b{B}-{'chw' if cf else 'hwc'}-{'f32' if fl else 'u8'}"


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=_id)
def test_forward_grid_bits_and_random_bound(case):
    H, W, Cn, B, cf, fl = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x, w, b, scale = ref.grid_forward_case(rng, B, Cn, H, W, cf, fl)
    want, _ = ref.forward(x, w, b, scale, cf)
    if want.size >= 64:
        assert (want > 0).any() and (want == 0).any()                      # the clamp is exercised
    assert _bits(_forward(x, w, b, scale, cf), want.astype(f32))
    x, w, b, scale = ref.random_forward_case(rng, B, Cn, H, W, cf, fl)
    want, bound = ref.forward(x, w, b, scale, cf)
    _within(_forward(x, w, b, scale, cf), want, bound, "y")


@pytest.mark.parametrize("shape", [(36, 36, 3, False), (128, 128, 1, True), (40, 52, 2, True)])
def test_an_image_alone_equals_the_image_in_a_batch_of_65(shape):
    H, W, Cn, cf = shape
    rng = np.random.default_rng(7)
    x, w, b, scale = ref.random_forward_case(rng, 65, Cn, H, W, cf, False)
    for at in (0, 31, 64):
        x[at] = x[5]
    batch = _forward(x, w, b, scale, cf)
    alone = _forward(x[5:6].copy(), w, b, scale, cf)
    for at in (0, 5, 31, 64):
        assert _bits(batch[at], alone[0]), at


@pytest.mark.parametrize("case", ref.BWD_CASES, ids=_id)
def test_backward_grid_bits_random_bound_and_repeat(case):
    H, W, Cn, B, cf, fl = case
    rng = np.random.default_rng(hash(case) % 2**32)
    x, y, dy, scale = ref.grid_backward_case(rng, B, Cn, H, W, cf, fl, gmax=ref.gmax_of(case))
    assert (y == 0).any() and (dy[y == 0] != 0).any()                      # the mask matters
    dw_want, db_want, _, _ = ref.backward(x, y, dy, scale, cf)
    dw, db = _backward(x, y, dy, scale, cf)
    assert _bits(db, db_want.astype(f32))
    assert _bits(dw, dw_want.astype(f32))
    x, y, dy, scale = ref.random_backward_case(rng, B, Cn, H, W, cf, fl)
    dw_want, db_want, dw_bound, db_bound = ref.backward(x, y, dy, scale, cf)
    dw, db = _backward(x, y, dy, scale, cf, twice=True)
    _within(db, db_want, db_bound, "dbias")
    _within(dw, dw_want, dw_bound, "dweight")


def test_a_workspace_one_byte_short_is_an_error():
    rng = np.random.default_rng(3)
    x, y, dy, scale = ref.grid_backward_case(rng, 3, 1, 40, 52, True, False)
    assert _backward(x, y, dy, scale, True, shrink=1) != 0


def test_forward_of_a_backward_grid_case_feeds_the_backward():
    """The kernel's own forward output as the backward's y: the pair as the autograd function uses it."""
    rng = np.random.default_rng(11)
    x, w, b, scale = ref.grid_forward_case(rng, 3, 3, 40, 52, False, False)
    y = _forward(x, w, b, scale, False)
    dy = rng.integers(-4, 5, y.shape).astype(f32)
    dw_want, db_want, _, _ = ref.backward(x, y, dy, scale, False)
    dw, db = _backward(x, y, dy, scale, False)
    assert _bits(dw, dw_want.astype(f32)) and _bits(db, db_want.astype(f32))


def test_error_returns_write_nothing_and_name_the_function():
    capi, L = _lib()
    x = np.zeros((1, 1, 8, 8), np.uint8)
    gx, gw, gb, gy = Guarded(64, fill=x), Guarded(4 * 32 * 64), Guarded(4 * 32), Guarded(4 * 32)
    gdw, gdb, gws = Guarded(4 * 32 * 64), Guarded(4 * 32), Guarded(1 << 16)
    outs = (gy, gdw, gdb, gws)

    def fwd(xp=gx, B=1, Cn=1, H=8, W=8, wp=gw, bp=gb, yp=gy):
        return L.tg_conv_stem(_p(xp), 0, 1, B, Cn, H, W, _p(wp), _p(bp), 1.0, _p(yp), _stream()), "tg_conv_stem:"

    def bwd(xp=gx, B=1, Cn=1, H=8, W=8, yp=gy, dyp=gy, dwp=gdw, dbp=gdb, wsp=gws, nbytes=1 << 16):
        return (L.tg_conv_stem_bwd(_p(xp), 0, 1, B, Cn, H, W, _p(yp), _p(dyp), 1.0, _p(dwp), _p(dbp), _p(wsp), nbytes, _stream()),
                "tg_conv_stem_bwd:")

    calls = [lambda: fwd(xp=None), lambda: fwd(wp=None), lambda: fwd(bp=None), lambda: fwd(yp=None), lambda: fwd(Cn=0), lambda: fwd(Cn=13),
             lambda: fwd(H=7), lambda: fwd(W=7), lambda: fwd(B=-1),
             lambda: bwd(xp=None), lambda: bwd(yp=None), lambda: bwd(dyp=None), lambda: bwd(dwp=None), lambda: bwd(dbp=None),
             lambda: bwd(wsp=None), lambda: bwd(Cn=0), lambda: bwd(Cn=13), lambda: bwd(H=7), lambda: bwd(W=7), lambda: bwd(B=-1),
             lambda: bwd(nbytes=0)]
    for k, call in enumerate(calls):
        rc, who = call()
        torch.cuda.synchronize()
        assert rc != 0 and L.tg_last_error().decode().startswith(who), (k, rc, L.tg_last_error())
        for g in outs:
            assert g.guards_intact() and bool((g.payload() == PATTERN).all()), k
    for bad in ((-1, 1, 8, 8), (1, 0, 8, 8), (1, 13, 8, 8), (1, 1, 7, 8), (1, 1, 8, 7)):
        assert L.tg_conv_stem_bwd_workspace(*bad) < 0 and L.tg_last_error().decode().startswith("tg_conv_stem_bwd_workspace:")
    # B = 0 does nothing
    capi.check(L.tg_conv_stem(_p(gx), 0, 1, 0, 1, 8, 8, _p(gw), _p(gb), 1.0, _p(gy), _stream()))
    capi.check(L.tg_conv_stem_bwd(_p(gx), 0, 1, 0, 1, 8, 8, _p(gy), _p(gy), 1.0, _p(gdw), _p(gdb), _p(gws), 1 << 16, _stream()))
    torch.cuda.synchronize()
    for g in outs:
        assert g.guards_intact() and bool((g.payload() == PATTERN).all())


WRAPPING = [c for c in ref.BWD_CASES if ref.geometry(c[3], c[0], c[1])["regions"] > 256 or ref.geometry(c[3], c[0], c[1])["n_chunks"] > 1]


@pytest.mark.parametrize("case", WRAPPING, ids=_id)
def test_forward_of_a_wrapping_backward_grid_case_feeds_the_backward(case):
    """As above on the cases whose workgroups walk more than one region, or whose images have more than one column chunk."""
    H, W, Cn, B, cf, fl = case
    assert len(WRAPPING) == 5
    rng = np.random.default_rng(11)
    x, w, b, scale = ref.grid_forward_case(rng, B, Cn, H, W, cf, fl)
    y = _forward(x, w, b, scale, cf)
    want, _ = ref.forward(x, w, b, scale, cf)
    assert _bits(y, want.astype(f32))
    gmax = ref.gmax_of(case)
    assert y.size // 32 * gmax * 255 < 2 ** 24                             # grid_backward_case's condition, on this dy
    dy = rng.integers(-gmax, gmax + 1, y.shape).astype(f32)
    dw_want, db_want, _, _ = ref.backward(x, y, dy, scale, cf)
    dw, db = _backward(x, y, dy, scale, cf)
    assert _bits(dw, dw_want.astype(f32)) and _bits(db, db_want.astype(f32))


@pytest.mark.parametrize("channels_first", [True, False], ids=["chw", "hwc"])
@pytest.mark.parametrize("hw", [(37, 39), (40, 52)], ids=["37x39", "40x52"])
def test_forward_a_nan_pixel_is_nan_where_its_windows_are_and_changes_nothing_else(hw, channels_first):
    """float32 input, one NaN pixel inside the window of position 0 of its region.  (40, 52) has 9 x 12 = 108 positions a region, no multiple of
    32: the lanes past the region's last position compute on position 0, so they hold the NaN - and store nothing.  (37, 39) has 8 x 8 = 64."""
    (H, W), Cn, B = hw, 2, 3
    g = ref.geometry(B, H, W)
    assert g["regions"] == B and (g["OH"] * g["OW"]) % 32 == (0 if hw == (37, 39) else 12)
    rng = np.random.default_rng(13)
    x, w, b, scale = ref.random_forward_case(rng, B, Cn, H, W, channels_first, True)
    clean = _forward(x, w, b, scale, channels_first)
    py, px = 5, 6                                                          # inside the windows of positions (0, 0), (0, 1), (1, 0), (1, 1)
    if channels_first:
        x[1, 1, py, px] = np.nan
    else:
        x[1, py, px, 1] = np.nan
    got = _forward(x, w, b, scale, channels_first)
    hit = np.zeros(clean.shape, bool)
    hit[1, :, :2, :2] = True
    assert np.isnan(got[hit]).all()                                        # all 32 channels: ReLU hands the NaN on, as torch.relu does
    assert not np.isnan(got[~hit]).any() and _bits(got[~hit], clean[~hit])  # everything else, in every image, has the clean run's bits
