"""The block raster's hit predicate (csrc/tg_raster_dev.hpp: pixel_hit) against the chained compares it replaced, restated in numpy float32
over the full grid of special values - the identity argument of the helper's comment, cell by cell.  No GPU needed; the device evaluates
both forms on 2^22 cases per seed in tests/test_gpu_raster_issue.py (tg_selftest_pixel_predicate).

    chained:  box = (fx >= xmin) & (fx <= xmax);  pos = all e_k >= 0;  neg = all e_k <= 0;  hit = box & (pos | neg) & (s != 0) & (d < z)
    helper:   box = med3(fx, xmin, xmax) == fx;   lo = min(min(e0, e1), e2);  hi = max(max(e0, e1), e2);
              hit = box & ((lo >= 0) | (hi <= 0)) & (d < z)

The hardware's rules, as the argument uses them: v_min_f32 / v_max_f32 return the other operand when one is NaN (numpy's fmin / fmax);
v_med3_f32 returns min3 of its operands when any is NaN and the median otherwise.  s = (e0 + e1) + e2 in float32.  d is NaN wherever the
argument says it must be - s == +-0 (div_mid_range's reciprocal step is 0 x inf), s NaN (a NaN or two opposite infinities among the e_k), or
a NaN bound (both bounds are then NaN: all three x_k are, and every e_k with them) - and runs over a set of values everywhere else, +-inf
among them.  The bounds are emit()'s: xmin <= xmax, or both NaN."""
import itertools

import numpy as np

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
TINY = F(1e-45)                                     # the smallest denormal
E_VALUES = [-INF, F(-1), -TINY, F(-0.0), F(0.0), TINY, F(1), INF, NAN]
FX = F(36.5)                                        # a pixel centre: finite, never zero
BOXES = [(F(10.25), F(80.0)), (FX, F(80.0)), (F(10.25), FX), (FX, FX), (F(40.0), F(80.0)), (F(10.0), F(30.0)), (-INF, INF), (-INF, FX), (FX, INF),
         (INF, INF), (-INF, -INF), (F(-0.0), F(0.0)), (F(-0.0), F(80.0)), (np.nextafter(FX, INF), F(80.0)), (F(10.0), np.nextafter(FX, -INF)),
         (NAN, NAN)]
D_VALUES = [-INF, F(-1), F(0.0), F(0.02), F(0.03), INF, NAN]
Z_VALUES = [F(0.03), F(0.05), INF]


def _med3(a, b, c):
    if np.isnan(a) or np.isnan(b) or np.isnan(c):
        return np.fmin(np.fmin(a, b), c)
    return sorted([a, b, c])[1]


def _chained(fx, xmin, xmax, e0, e1, e2, s, d, z):
    box = (fx >= xmin) & (fx <= xmax)
    pos = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    neg = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
    return bool(box & (pos | neg) & (s != 0) & (d < z))


def _helper(fx, xmin, xmax, e0, e1, e2, d, z):
    box = _med3(fx, xmin, xmax) == fx
    lo, hi = np.fmin(np.fmin(e0, e1), e2), np.fmax(np.fmax(e0, e1), e2)
    return bool(box & ((lo >= 0) | (hi <= 0)) & (d < z))


def test_division_by_zero_gives_nan():
    """div_mid_range(a, +-0): rcp = +-inf, the Newton step on it is fma(-/+0, +-inf, 1) = NaN, and NaN stays: d < z is false, which is why
    the helper needs no s != 0."""
    with np.errstate(all="ignore"):
        for b in (F(0.0), F(-0.0)):
            for a in (F(0.0), F(-0.0), F(1.0), F(-3.5), INF, NAN):
                y = F(1.0) / b
                assert np.isinf(y)
                y = (-b * y + F(1.0)) * y + y
                q = a * y
                q = (-b * q + a) * y + q
                q = (-b * q + a) * y + q
                assert np.isnan(q) and not (q < INF)


def test_the_two_forms_agree_on_the_grid_of_special_values():
    cells = differing_coverage = hits = 0
    with np.errstate(all="ignore"):
        for (xmin, xmax), (e0, e1, e2) in itertools.product(BOXES, itertools.product(E_VALUES, repeat=3)):
            s = F(F(e0 + e1) + e2)
            forced_nan = bool(np.isnan(s) or s == 0 or np.isnan(xmin) or np.isnan(xmax))
            cov_a = _chained(FX, xmin, xmax, e0, e1, e2, s, F(0.0), F(1.0))
            cov_b = _helper(FX, xmin, xmax, e0, e1, e2, F(0.0), F(1.0))
            if cov_a != cov_b:
                differing_coverage += 1
                assert forced_nan, (xmin, xmax, e0, e1, e2, s)              # the booleans differ only where d is NaN
            for d in ([NAN] if forced_nan else D_VALUES):
                for z in Z_VALUES:
                    a = _chained(FX, xmin, xmax, e0, e1, e2, s, d, z)
                    b = _helper(FX, xmin, xmax, e0, e1, e2, d, z)
                    assert a == b, (xmin, xmax, e0, e1, e2, s, d, z, a, b)
                    cells += 1
                    hits += a
    assert cells > 20000 and hits > 500 and differing_coverage > 100, (cells, hits, differing_coverage)     # not vacuous


def test_bounds_as_emit_makes_them_are_ordered_or_both_nan():
    """xmin = fminf(x0, fminf(x1, x2)), xmax = fmaxf(x0, fmaxf(x1, x2)): ordered, or both NaN exactly when all three x_k are - the domain the
    median form of `box` is argued on."""
    xs = [-INF, F(-2.5), F(-0.0), F(0.0), F(36.5), INF, NAN]
    for x0, x1, x2 in itertools.product(xs, repeat=3):
        xmin, xmax = np.fmin(x0, np.fmin(x1, x2)), np.fmax(x0, np.fmax(x1, x2))
        if np.isnan(xmin) or np.isnan(xmax):
            assert np.isnan(xmin) and np.isnan(xmax) and np.isnan(x0) and np.isnan(x1) and np.isnan(x2)
        else:
            assert xmin <= xmax
