"""The case table of tests/augment_cases.py without a GPU: that it reaches every path of k_random_translate (csrc/tg_augment.hip) for each of the
kernel's four instantiations - asked of the launcher's own decision through tg_selftest_translate_plan -, every channel count and every shift
class, and that on its inputs the two references of tests/augment_ref.py agree: the float32 restatement with kornia's float64 path within
tolerance(x), with a plain integer shift where the shift is one, and with its batched form bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import augment_cases as AC  # noqa: E402
from augment_ref import split_shift, tolerance, warp_f32, warp_f32_batched, warp_kornia  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

BASE = 0x7F0000001000      # a 16-byte aligned address: the table's offsets are added to it


def plan(case, in_addr=None, out_addr=None, B=None):
    """(path, chunks per plane, LDS bytes, launches) of a case from the launcher's own function."""
    T = _capi.test_lib()
    path, chunks, lds, launches = C.c_int32(-9), C.c_int32(-9), C.c_int32(-9), C.c_int64(-9)
    rc = T.tg_selftest_translate_plan(_capi.AUGMENT_DTYPE[case.dtype.name], int(case.channels_first), case.C, case.H, case.W,
                                      case.B if B is None else B, BASE + case.in_off if in_addr is None else in_addr,
                                      BASE + (1 << 32) + case.out_off if out_addr is None else out_addr, C.byref(path), C.byref(chunks),
                                      C.byref(lds), C.byref(launches))
    assert rc == 0, T.tg_selftest_last_error().decode()
    return path.value, chunks.value, lds.value, launches.value


def geometry(case):
    R = case.W if case.channels_first else case.W * case.C
    S = 1 if case.channels_first else case.C
    return case.H * R, R, S, 16 // case.dtype.itemsize


def classify(case):
    """The path classes a case is in, from the launcher's answers: its path, and for the per-element path the one condition whose removal
    gives the staged path back."""
    HR, R, S, V = geometry(case)
    path, chunks, lds, launches = plan(case)
    assert chunks == -(-HR // AC.CHUNK)
    got = set()
    if launches > 1:
        got.add("multi_launch")
    if path == 1:
        assert lds >= 4 * (AC.CHUNK + R + S) and case.in_off % 16 == 0 and case.out_off % 16 == 0
        got.add("staged_single" if chunks == 1 else "staged_whole" if HR % AC.CHUNK == 0 else "staged_ragged")
        return got
    assert lds == 0
    aligned = plan(case, BASE, BASE + (1 << 32))[0]
    if HR % V:
        got.add("elem_plane")
    if R + S > AC.MAX_ROW:
        got.add("elem_row")
    if case.in_off % 16 and plan(case, out_addr=BASE + (1 << 32))[0] == 0 and aligned == 1:
        got.add("elem_in")
    if case.out_off % 16 and plan(case, in_addr=BASE)[0] == 0 and aligned == 1:
        got.add("elem_out")
    assert aligned == (0 if HR % V or R + S > AC.MAX_ROW else 1)
    return got


def coverage_gaps(cases):
    """What a table lacks: (class, dtype, layout) without a case, (layout, C) without a case, a case without a shift class."""
    return path_gaps(cases) + [(c.name, k) for c in cases for k, problem in shift_gaps(c).items() if problem]


def shift_gaps(case):
    """{shift class: True when the case's rows do not hold it}, from the rows themselves."""
    p = case_rows(case)
    H, W = case.H, case.W
    on, tx, ty = p[:, 0] != 0, p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)

    def has(mask):
        return bool((on & mask).any())

    def both_signs(t, v):
        return has(t == v) and has(t == -v)

    frac = lambda t: np.isfinite(t) & (t != np.floor(t))   # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = tx * W / (W - 1), ty * H / (H - 1)          # the shifts, as split_shift forms them
        ex, ey = sx - np.floor(sx), sy - np.floor(sy)
    gaps = {
        "zero": not has((tx == 0) & (ty == 0)),
        "n_minus_1": not (both_signs(tx, W - 1) and both_signs(ty, H - 1)),
        "n": not (both_signs(tx, W) and both_signs(ty, H)),
        "half_fractional": not (has((tx > W / 2) & (tx < W / 2 + 1) & frac(tx)) and has((tx < -W / 2) & (tx > -W / 2 - 1) & frac(tx))
                                and has((ty > H / 2) & (ty < H / 2 + 1) & frac(ty)) and has((ty < -H / 2) & (ty > -H / 2 - 1) & frac(ty))),
        "n_plus_5": not (both_signs(tx, W + 5) and both_signs(ty, H + 5)),
        "huge": not (both_signs(tx, np.float64(np.float32(1e30))) and both_signs(ty, np.float64(np.float32(1e30)))),
        "non_finite": not (both_signs(tx, np.inf) and both_signs(ty, np.inf) and has(np.isnan(tx)) and has(np.isnan(ty))),
        "integer": not has((ex == 0) & (ey == 0) & (np.abs(sx) < W) & (np.abs(sy) < H) & ((sx != 0) | (sy != 0))),   # a whole shift inside
        "half": not has((ex == 0.5) & (ey == 0.5)),
        "unapplied_huge": not bool((~on & ~(np.abs(tx) < 1e29) & ~(np.abs(ty) < 1e29)).any()),
    }
    assert tuple(gaps) == AC.SHIFT_CLASSES
    n_explicit = sum(len(v) for v in AC.explicit_rows(H, W).values())
    gaps["draws"] = case.B - n_explicit < 8
    return gaps


_rows = {}


def case_rows(case):
    if case.name not in _rows:
        _rows[case.name] = AC.case_params(case)
    return _rows[case.name]


def test_names_are_unique_and_every_case_is_in_its_class():
    assert len({c.name for c in AC.CASES}) == len(AC.CASES)
    for c in AC.CASES:
        assert c.cls in AC.CLASSES and c.cls in classify(c), (c.name, classify(c))
        assert c.in_off % c.dtype.itemsize == 0 and c.out_off % 4 == 0, c.name      # misaligned for the vector path, not for the element type
        launches = plan(c)[3]
        assert (launches > 1) == (c.cls == "multi_launch") and launches == -(-c.B // (AC.MAX_BLOCKS // (plan(c)[1] * (c.C if c.channels_first else 1))))


def test_table_covers_every_path_channel_count_and_shift_class():
    assert coverage_gaps(AC.CASES) == []


def test_coverage_check_notices_a_missing_case():
    """The check above is not vacuous: without the last case of a class, of a channel count or of a shift class it reports the gap."""
    for cls in AC.CLASSES:
        for dtype in (np.uint8, np.float32):
            for cf in (True, False):
                rest = [c for c in AC.CASES if not (c.cls == cls and c.dtype == dtype and c.channels_first == cf)]
                assert (cls, np.dtype(dtype).name, cf) in path_gaps(rest), (cls, dtype, cf)
    for cf in (True, False):
        for ch in (1, 2, 3, 6):
            rest = [c for c in AC.CASES if not (c.channels_first == cf and c.C == ch)]
            assert ("channels", cf, ch) in path_gaps(rest)
    c = AC.CASES[0]
    for cls in AC.SHIFT_CLASSES:
        sl = AC.explicit_slice(c, cls)
        saved = case_rows(c).copy()
        try:
            _rows[c.name] = np.delete(saved, np.arange(sl.start, sl.stop), axis=0)
            assert shift_gaps(c)[cls], cls
        finally:
            _rows[c.name] = saved
    assert not any(shift_gaps(c).values())


def path_gaps(cases):
    have = {(cls, c.dtype.name, c.channels_first) for c in cases for cls in classify(c) if cls == c.cls or cls == "multi_launch"}
    gaps = [(cls, d, cf) for cls in AC.CLASSES for d in ("uint8", "float32") for cf in (True, False) if (cls, d, cf) not in have]
    return gaps + [("channels", cf, ch) for cf in (True, False) for ch in (1, 2, 3, 6)
                   if not any(c.channels_first == cf and c.C == ch for c in cases)]


def test_plan_entry_refuses_what_the_call_refuses():
    T = _capi.test_lib()
    out = [C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()]
    refs = [C.byref(o) for o in out]
    assert T.tg_selftest_translate_plan(0, 1, 1, 1, 16, 4, BASE, BASE * 2, *refs) == -1        # H < 2
    assert T.tg_selftest_translate_plan(2, 1, 1, 16, 16, 4, BASE, BASE * 2, *refs) == -1       # unknown dtype
    assert T.tg_selftest_translate_plan(0, 1, 1 << 20, 1 << 6, 1 << 6, 4, BASE, BASE * 2, *refs) == -1   # more than 2^30 elements
    assert T.tg_selftest_translate_plan(0, 1, 1, 16, 16, -1, BASE, BASE * 2, *refs) == -1
    assert T.tg_selftest_translate_plan(0, 1, 1, 16, 16, 0, BASE, BASE * 2, *refs) == 0 and out[3].value == 0
    assert T.tg_selftest_translate_plan(1, 0, 2, 128, 128, AC.MAX_BLOCKS // 8 + 1, BASE, BASE * 2, *refs) == 0
    assert (out[0].value, out[1].value, out[3].value) == (1, 8, 2)
    assert out[2].value == 4 * ((4096 + 256 + 2 + 2 * 4 + 12 + 3) // 4 * 4)


def _kinds(case):
    return AC.DATA_KINDS[case.dtype]


def _plain_shift(x, oy, ox):
    """out[b, c, y, x] = in[b, c, y + oy, x + ox], 0 outside: slices only."""
    Cn, H, W = x.shape
    out = np.zeros((Cn, H, W), np.float32)
    for y in range(H):
        if 0 <= y + oy < H:
            lo, hi = max(0, -ox), min(W, W - ox)
            if lo < hi:
                out[:, y, lo:hi] = x[:, y + oy, lo + ox:hi + ox]
    return out


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c.name)
def test_references_agree_on_the_table(case):
    """warp_f32 against warp_kornia within tolerance(x) on every row of finite parameters; an all-zero sample for the rows that are not finite;
    a plain integer shift where fx = fy = 0 (the restatement's split_shift and taps against slices); the converted input where not applied.
    The cases of millions of samples take warp_f32_batched, which every other case holds to warp_f32 bit for bit."""
    prm = case_rows(case)
    finite = np.isfinite(prm[:, 1]) & np.isfinite(prm[:, 2])
    on = prm[:, 0] != 0
    for kind in _kinds(case):
        x = AC.case_input(case, kind)
        if AC.is_huge(case):
            ref = warp_f32_batched(x, prm, case.channels_first)
            edge = np.r_[0:2048, case.B - 2048:case.B]                       # both ends by the loop as well: the explicit rows are last
            assert np.array_equal(ref[edge].view(np.uint32), warp_f32(x[edge], prm[edge], case.channels_first).view(np.uint32))
        else:
            ref = warp_f32(x, prm, case.channels_first)
            assert np.array_equal(ref.view(np.uint32), warp_f32_batched(x, prm, case.channels_first).view(np.uint32))
        if kind != "signed_wide":       # (tolerance() has no honest value for magnitudes 2^-20 .. 2^20 side by side: tests/test_gpu_augment_paths.py)
            k64 = warp_kornia(x[finite], prm[finite], case.channels_first)
            err = float(np.abs(ref[finite] - k64).max())
            print(f"{case.name} {kind}: max |restatement - kornia| {err:.3e}, tolerance {tolerance(x):.3e}")
            assert err <= tolerance(x)
        assert not ref[on & ~finite].any() and (on & ~finite).sum() >= 8
        assert np.array_equal(ref[~on], x[~on].astype(np.float32)) and (~on).sum() >= 3
        xc = x if case.channels_first else x.transpose(0, 3, 1, 2)
        rc = ref if case.channels_first else ref.transpose(0, 3, 1, 2)
        n_int = n_inside = 0
        some = np.flatnonzero(on & finite)
        for b in (some[-4096:] if case.explicit_last else some[:4096]):
            (ox, fx), (oy, fy) = split_shift(prm[b, 1], case.W), split_shift(prm[b, 2], case.H)
            if fx == 0 and fy == 0:
                sx, sy = -float(prm[b, 1]) * case.W / (case.W - 1), -float(prm[b, 2]) * case.H / (case.H - 1)
                assert ox == min(max(sx, -(case.W + 2)), case.W + 2) and oy == min(max(sy, -(case.H + 2)), case.H + 2)
                assert np.array_equal(rc[b], _plain_shift(xc[b].astype(np.float32), oy, ox)), (case.name, b)
                n_int += 1
                n_inside += (ox, oy) != (0, 0) and abs(ox) < case.W and abs(oy) < case.H
        assert n_int >= 8 and n_inside >= 2, (n_int, n_inside)
