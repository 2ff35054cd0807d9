"""k_random_affine (csrc/tg_affine.hip) through the C entries on raw pointers: tg_random_affine / tg_random_affine_rows called through ctypes on
offsets INSIDE larger flat byte buffers (that is where the misaligned pointers come from; nothing is read or written outside an allocation),
with guard bytes round the output, params_out and coeffs_out.

Stage (c) is driven exactly: the coefficients are given (coeffs_in), so the output must equal tests/affine_ref.py's float32 restatement bit for
bit on every path that affine_plan names - asked of tg_selftest_affine_plan with the real addresses - for both dtypes and both layouts."""
import collections
import ctypes as C
import os
import re
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from affine_ref import coeffs_f64, warp_f32  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import Guarded  # noqa: E402

F32 = np.float32
PER_ELEMENT, GATHER, STAGED = 0, 1, 2
NO_RANGES = (0.0, 0.0) + (0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)     # ax, ay; d0, d1, s0, s1, s2, s3, h0, h1, h2, h3

Case = collections.namedtuple("Case", "name path dtype channels_first C H W B in_off out_off")


def _capi():
    from tactile_gym_amd import _capi
    return _capi


def _cases():
    out = []
    for dtype in (np.uint8, np.float32):
        e = np.dtype(dtype).itemsize
        for cf in (True, False):
            def case(path, Cn, H, W, B=17, in_off=0, out_off=0):
                name = f"{('elem', 'gather', 'staged')[path]}-{np.dtype(dtype).name}-{'cf' if cf else 'cl'}-{Cn}x{H}x{W}-B{B}-i{in_off}-o{out_off}"
                out.append(Case(name, path, dtype, cf, Cn, H, W, B, in_off, out_off))
            case(STAGED, 1, 16, 16)
            # four chunks a plane, channels last one plane of eight: 16 and 32 KiB of uint8 are staged, 64 and 128 KiB of float32 gathered
            case(STAGED if dtype == np.uint8 else GATHER, 2, 128, 128, B=5)
            case(STAGED, 3, 32, 32)
            case(STAGED, 6, 16, 24, B=1)
            # a ragged last chunk: 4608 = 4096 + 512; channels last in float32 the plane is 36 KiB, above the staged path's limit
            case(GATHER if dtype == np.float32 and not cf else STAGED, 2, 72, 64)
            if dtype == np.float32:
                case(STAGED if cf else GATHER, 2, 64, 128, B=5)                               # 32 KiB planes (channels last: 64 KiB, gathered): the limit
            elif cf:
                case(GATHER, 3, 18, 18)                                           # 324 bytes: a multiple of 4, not of 16
            else:
                case(GATHER, 1, 18, 18)
            case(GATHER, 2, 16, 16, in_off=e)                                     # a misaligned input
            case(GATHER if dtype == np.uint8 else STAGED, 1, 6, 6, B=5)           # 36 elements: quads run over the row ends; 36 B / 144 B
            case(PER_ELEMENT, 1, 17, 23)                                          # 391 elements: no multiple of 4
            case(PER_ELEMENT, 3, 17, 23, B=5)
            case(PER_ELEMENT, 2, 16, 16, out_off=4)                               # a misaligned output
            case(PER_ELEMENT, 6, 17, 23, B=1, in_off=e, out_off=8)
    # two launches at the smallest shape that forces the split: 2 x 2 planes are one workgroup each, 2^17 planes a sample: 64 samples a launch
    out.append(Case("two_launches-uint8-cf-131072x2x2-B65", GATHER, np.uint8, True, 1 << 17, 2, 2, 65, 0, 0))
    return out


CASES = _cases()


def coeff_sets(H, W):
    """float32 [17, 6]: identity; shifts of +-1, +-1/2 and +-(n + 5); a quarter and a half turn; 2x and 1/2x; 37 degrees with a shear; far
    out and not finite."""
    q = min(H, W) - 1
    sets = [[1, 0, 0, 0, 1, 0],
            [1, 0, 1, 0, 1, 0], [1, 0, 0, 0, 1, -1], [1, 0, 0.5, 0, 1, 0.5], [1, 0, -0.5, 0, 1, -0.5],
            [1, 0, W + 5, 0, 1, 0], [1, 0, 0, 0, 1, -(H + 5)],
            [0, 1, 0, -1, 0, q], [-1, 0, W - 1, 0, -1, H - 1],
            [0.5, 0, 0, 0, 0.5, 0], [2, 0, -W / 2.0, 0, 2, -H / 2.0]]
    rot = coeffs_f64(np.array([[1, 1.5, -0.75, 37.0, 1.1, 0.9, 8.0, -4.0]], dtype=F32), H, W)[0]
    sets.append(list(rot))
    sets += [[1, 0, 1e30, 0, 1, 0], [1e30, 0, 0, 0, 1, 0], [1, 0, float("inf"), 0, 1, 0], [1, 0, 0, float("-inf"), 1, 0], [1, float("nan"), 0, 0, 1, 0]]
    return np.array(sets, dtype=F32)


def case_coeffs(case):
    sets = coeff_sets(case.H, case.W)
    if case.B == 1:
        return sets[11:12].copy()                                                # the rotation with a shear
    if case.B == 5:
        return sets[[0, 3, 7, 11, 16]].copy()
    return sets[np.arange(case.B) % len(sets)].copy()


def case_input(case, n_samples=None):
    n = case.B if n_samples is None else n_samples
    shape = (n, case.C, case.H, case.W) if case.channels_first else (n, case.H, case.W, case.C)
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    if case.dtype == np.uint8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return (rng.random(shape, dtype=np.float32) * F32(255)).astype(F32)


def case_apply(case):
    apply = np.ones(case.B, F32)
    if case.B > 1:
        apply[1] = 0                                                             # one sample passed through (a shift of 1 if it were applied)
    return apply


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _plan(case, in_ptr, out_ptr):
    capi = _capi()
    path, in_vec, chunks, lds, launches = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert capi.test_lib().tg_selftest_affine_plan(capi.AUGMENT_DTYPE[np.dtype(case.dtype).name], int(case.channels_first), case.C, case.H, case.W,
                                                   case.B, in_ptr, out_ptr, C.byref(path), C.byref(in_vec), C.byref(chunks), C.byref(lds),
                                                   C.byref(launches)) == 0
    return path.value, launches.value


def _call(case, x, coeffs, apply, rows=None):
    """One call on guarded buffers with coeffs_in and params_in: the output [B, ...] after every guard check."""
    capi = _capi()
    L = capi.lib()
    shape = (case.B,) + x.shape[1:]
    prm = np.zeros((case.B, 8), F32)
    prm[:, 0] = apply * F32(3.5)                                                   # any non-zero flag applies
    src = Guarded(x.nbytes, case.in_off, fill=x)
    out = Guarded(int(np.prod(shape)) * 4, case.out_off)
    pin, cin = Guarded(prm.nbytes, fill=prm), Guarded(coeffs.nbytes, fill=coeffs)
    pout, cout = Guarded(case.B * 32), Guarded(case.B * 24)
    rows_dev = torch.from_numpy(rows).cuda() if rows is not None else None
    assert src.ptr % 16 == case.in_off % 16 and out.ptr % 16 == case.out_off % 16
    path, launches = _plan(case, src.ptr, out.ptr)
    assert path == case.path, (case.name, path)
    assert launches == (2 if case.name.startswith("two_launches") else 1)
    stream = torch.cuda.current_stream().cuda_stream
    head = (src.ptr, out.ptr, capi.AUGMENT_DTYPE[np.dtype(case.dtype).name], int(case.channels_first), case.B, case.C, case.H, case.W) + NO_RANGES + (
        0.0, 0, 0, pin.ptr, pout.ptr, cin.ptr, cout.ptr)
    rc = L.tg_random_affine(*head, stream) if rows is None else L.tg_random_affine_rows(*head, rows_dev.data_ptr(), stream)
    assert rc == 0, L.tg_last_error().decode()
    torch.cuda.synchronize()
    assert out.guards_intact(), "the output's guard bytes were written"
    assert pout.guards_intact() and cout.guards_intact(), "the guard bytes of params_out / coeffs_out were written"
    assert src.guards_intact() and np.array_equal(src.host(x.dtype).reshape(x.shape), x), "the input was written"
    assert pin.guards_intact() and cin.guards_intact()
    got_p = pout.host(F32).reshape(case.B, 8)
    assert np.array_equal(got_p[:, 0], apply) and not got_p[:, 1:].any()
    assert np.array_equal(cout.host(np.uint32), coeffs.reshape(-1).view(np.uint32))  # the coefficients used are the ones given, NaN included
    return out.host(F32).reshape(shape)


def _check(case, x, coeffs, apply, got):
    ref = warp_f32(x, coeffs, apply, case.channels_first)
    if not _bits_equal(got, ref):
        bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).reshape(case.B, -1).any(axis=1))
        raise AssertionError(f"{case.name}: {len(bad)} samples differ from the restatement, first {bad[:8]}, coefficients {coeffs[bad[:4]]}")
    keep = apply == 0
    assert _bits_equal(got[keep], x[keep].astype(F32))
    dead = ~keep & ~np.isfinite(coeffs).all(axis=1)
    assert not got[dead].any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_given_coefficients_on_every_path(case):
    x, coeffs, apply = case_input(case), case_coeffs(case), case_apply(case)
    _check(case, x, coeffs, apply, _call(case, x, coeffs, apply))


@pytest.mark.parametrize("case", [c for c in CASES if c.B == 17 or c.B == 5 and c.path == STAGED], ids=lambda c: c.name)
def test_row_table_equals_gather_then_warp(case):
    """A source of more samples than B behind a table with repeats, out of order, holding the last source sample."""
    n_src = case.B + 3
    x = case_input(case, n_samples=n_src)
    rows = (np.arange(case.B, dtype=np.int64)[::-1] * 2) % n_src
    rows[0] = n_src - 1
    rows[-1] = rows[-2]
    assert len(set(rows.tolist())) < case.B and rows.max() == n_src - 1
    coeffs, apply = case_coeffs(case), case_apply(case)
    _check(case, x[rows], coeffs, apply, _call(case, x, coeffs, apply, rows=rows))


def test_error_returns():
    capi = _capi()
    L = capi.lib()
    x = torch.zeros(4 * 1 * 8 * 8, dtype=torch.uint8, device="cuda")
    o = torch.zeros(4 * 1 * 8 * 8, dtype=torch.float32, device="cuda")
    good = dict(inp=x.data_ptr(), out=o.data_ptr(), dtype=0, cf=1, B=4, C=1, H=8, W=8, ax=0.1, ay=0.1, d0=-5.0, d1=5.0, s0=0.9, s1=1.1, s2=0.0,
                s3=0.0, h0=0.0, h1=0.0, h2=0.0, h3=0.0, p=0.5)

    def call(**kw):
        a = dict(good, **kw)
        return L.tg_random_affine(a["inp"], a["out"], a["dtype"], a["cf"], a["B"], a["C"], a["H"], a["W"], a["ax"], a["ay"], a["d0"], a["d1"],
                                  a["s0"], a["s1"], a["s2"], a["s3"], a["h0"], a["h1"], a["h2"], a["h3"], a["p"], 1, 2, None, None, None, None,
                                  torch.cuda.current_stream().cuda_stream)

    assert call() == 0 and call(B=0) == 0 and call(B=0, inp=None, out=None) == 0
    nan, inf = float("nan"), float("inf")
    bad = [(dict(dtype=2), "dtype"), (dict(B=-1), "B >= 0"), (dict(C=0), "C >= 1"), (dict(H=1), "H >= 2"), (dict(W=1), "W >= 2"),
           (dict(C=1 << 20, H=64, W=64), "2\\^30"), (dict(ax=1.5), "translate"), (dict(ay=-0.1), "translate"), (dict(ax=nan), "translate"),
           (dict(d0=5.0, d1=-5.0), "degrees"), (dict(d1=inf), "degrees"), (dict(d0=nan), "degrees"),
           (dict(s0=0.0), "scale"), (dict(s0=1.2, s1=1.1), "scale"), (dict(s1=inf), "scale"), (dict(s0=-1.0, s1=1.0), "scale"),
           (dict(s2=1.2, s3=1.1), "scale of y"), (dict(s2=0.0, s3=1.0), "scale of y"), (dict(s2=-1.0, s3=0.0), "scale of y"), (dict(s3=nan), "scale of y"),
           (dict(h0=1.0, h1=0.0), "shear"), (dict(h2=1.0, h3=0.0), "shear"), (dict(h3=inf), "shear"),
           (dict(p=1.5), "p must"), (dict(p=-0.5), "p must"), (dict(p=nan), "p must"),
           (dict(inp=None), "NULL"), (dict(out=None), "NULL"), (dict(out=x.data_ptr(), inp=x.data_ptr()), "overlaps")]
    for kw, what in bad:
        assert call(**kw) == -1, kw
        msg = L.tg_last_error().decode()
        assert msg.startswith("tg_random_affine") and re.search(what, msg), (kw, msg)
    torch.cuda.synchronize()
