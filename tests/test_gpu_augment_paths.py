"""k_random_translate (csrc/tg_augment.hip) on every case of tests/augment_cases.py: tg_random_translate / tg_random_translate_rows called through
ctypes on raw pointers into flat torch byte buffers - that is where the misaligned pointers come from: an offset INSIDE a larger buffer, nothing
is read or written outside an allocation - with guard bytes round the output and round params_out.

Per case: the output equals tests/augment_ref.py's float32 restatement bit for bit (samples that are not applied: the converted input), the
rows of finite parameters also agree with kornia's float64 path within tolerance(x), the guard bytes and the input are untouched, and the
launcher took the path the table is there for (asked of tg_selftest_translate_plan with the real addresses).

float32 inputs come in two kinds: uniform [0, 255), and signed values of magnitudes 2^-20 .. 2^20 next to each other.  tolerance() has no
honest value for the second kind (it is an absolute 1e-3 above max|x| = 1, while a float32 rounding at 2^20 is 0.06), so those runs are
compared with the restatement only - bit for bit, which is the stronger check anyway."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import augment_cases as AC  # noqa: E402
from augment_ref import draw_params, tolerance, warp_f32, warp_f32_batched, warp_kornia  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import Guarded  # noqa: E402


def _capi():
    from tactile_gym_amd import _capi
    return _capi


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _plan(case, in_ptr, out_ptr):
    capi = _capi()
    path, chunks, lds, launches = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    assert capi.test_lib().tg_selftest_translate_plan(capi.AUGMENT_DTYPE[case.dtype.name], int(case.channels_first), case.C, case.H, case.W, case.B,
                                                      in_ptr, out_ptr, C.byref(path), C.byref(chunks), C.byref(lds), C.byref(launches)) == 0
    return path.value, chunks.value, launches.value


def _call(case, x, params=None, rows=None, draw=None):
    """One call on guarded buffers: (output [like a batch of case.B samples], params_out [B, 3]) after every guard check."""
    capi = _capi()
    L = capi.lib()
    shape = (case.B,) + x.shape[1:]
    n = int(np.prod(shape))
    src = Guarded(x.nbytes, case.in_off, fill=x)
    out = Guarded(n * 4, case.out_off)
    pout = Guarded(case.B * 12)
    pin = Guarded(case.B * 12, fill=params) if params is not None else None
    rows_dev = torch.from_numpy(rows).cuda() if rows is not None else None
    assert src.ptr % 16 == case.in_off % 16 and out.ptr % 16 == case.out_off % 16
    path, chunks, launches = _plan(case, src.ptr, out.ptr)
    if case.cls != "multi_launch":                       # (2 x 2 planes: staged for float32, per element for uint8)
        assert path == (1 if case.cls.startswith("staged") else 0), (case.name, path)
    assert (launches > 1) == (case.cls == "multi_launch")
    ax, ay, p, seed, counter = draw if draw else (0.0, 0.0, 0.0, 0, 0)
    stream = torch.cuda.current_stream().cuda_stream
    head = (src.ptr, out.ptr, capi.AUGMENT_DTYPE[case.dtype.name], int(case.channels_first), case.B, case.C, case.H, case.W, ax, ay, p, seed, counter,
            pin.ptr if pin else None, pout.ptr)
    if rows is None:
        rc = L.tg_random_translate(*head, stream)
    else:
        rc = L.tg_random_translate_rows(*head, rows_dev.data_ptr(), stream)
    assert rc == 0, L.tg_last_error().decode()
    torch.cuda.synchronize()
    assert out.guards_intact(), "the output's guard bytes were written"
    assert pout.guards_intact(), "the guard bytes of params_out were written"
    assert src.guards_intact() and np.array_equal(src.host(x.dtype).reshape(x.shape), x), "the input was written"
    if pin:
        assert pin.guards_intact() and np.array_equal(pin.host(np.uint32), params.reshape(-1).view(np.uint32))
    return out.host(np.float32).reshape(shape), pout.host(np.float32).reshape(case.B, 3)


def _reference(case, x, prm):
    return (warp_f32_batched if AC.is_huge(case) else warp_f32)(x, prm, case.channels_first)


def _check(case, kind, x, prm, got):
    """got against the references for the gathered input x [B, ...] and rows prm."""
    ref = _reference(case, x, prm)
    if not _bits_equal(got, ref):
        bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).reshape(case.B, -1).any(axis=1))
        raise AssertionError(f"{case.name} {kind}: {len(bad)} samples differ from the restatement, first {bad[:8]}, params {prm[bad[:4]]}")
    keep = prm[:, 0] == 0
    assert _bits_equal(got[keep], x[keep].astype(np.float32))
    finite = np.isfinite(prm[:, 1]) & np.isfinite(prm[:, 2])
    assert not got[~keep & ~finite].any()
    if kind != "signed_wide":
        err = float(np.abs(got[finite] - warp_kornia(x[finite], prm[finite], case.channels_first)).max())
        print(f"{case.name} {kind}: max |device - kornia| {err:.3e}, tolerance {tolerance(x):.3e}")
        assert err <= tolerance(x)


def _runs():
    return [pytest.param(c, k, id=f"{c.name}-{k}") for c in AC.CASES for k in AC.DATA_KINDS[c.dtype]]


@pytest.mark.parametrize("case,kind", _runs())
def test_explicit_params_on_every_path(case, kind):
    x = AC.case_input(case, kind)
    prm = AC.case_params(case)
    got, pout = _call(case, x, params=prm)
    assert np.array_equal(pout[:, 1:].view(np.uint32), prm[:, 1:].view(np.uint32)) and np.array_equal(pout[:, 0], (prm[:, 0] != 0).astype(np.float32))
    _check(case, kind, x, prm, got)


@pytest.mark.parametrize("case,kind", [r for r in _runs() if r.values[0].rows])
def test_row_table_equals_gather_then_translate(case, kind):
    """A source of more samples than B behind a table with repeats, descending order and the last source sample."""
    n_src = case.B + 9
    x = AC.case_input(case, kind, n_samples=n_src)
    rows = AC.row_table(case, n_src)
    assert len(rows) == case.B and rows[0] == n_src - 1 and len(set(rows.tolist())) < case.B and (np.diff(rows) < 0).sum() > case.B // 2
    prm = AC.case_params(case)
    got, _ = _call(case, x, params=prm, rows=rows)
    _check(case, kind, x[rows], prm, got)


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.cls == "multi_launch" or c.name.startswith("staged_ragged-uint8-cl-6x96x96")],
                         ids=lambda c: c.name)
def test_drawn_params_equal_the_numpy_draws(case):
    """No params_in: the kernel draws.  The sample index enters the draw, so a second launch must go on where the first ended."""
    kind = AC.DATA_KINDS[case.dtype][0]
    x = AC.case_input(case, kind)
    seed, counter = 2 ** 63 + AC.case_seed(case), 2 ** 40 + 5
    got, pout = _call(case, x, draw=AC.DRAW["translate"] + (AC.DRAW["p"], seed, counter))
    prm = draw_params(seed, counter, case.B, AC.DRAW["translate"], AC.DRAW["p"], case.H, case.W)
    assert _bits_equal(pout, prm)
    assert 0 < prm[:, 0].sum() < case.B
    _check(case, kind, x, prm, got)
