"""Exact geometry for the broadphase guard's tests: a bracket (lower, upper) on the distance between a convex hull, given as world vertices, and an
oriented box, in numpy float64, each bound carried by a CERTIFICATE and re-evaluated from it by direct arithmetic:

    upper   the distance from an explicit convex combination of hull vertices (a witness point of the hull) to the box, in closed form;
    lower   the gap along an explicit unit axis g: min(hull . g) - max(box corners . g), a separating axis; 0 when none was found.

Whatever search proposes the certificates (the box's own axes and the nearest single vertex first, then oracle/gjk_epa.py's gjk), a wrong proposal
can only widen the bracket, never make a bound untrue.  Nothing here comes from oracle/broadphase.py or the kernel: the guard is held to this, not to
its own arithmetic.

A pair is MUST-HIT at D if upper <= D, MUST-CLEAR if lower > D, UNDECIDED otherwise (classify); tally() counts the three, the tests cap the share
of the third.  The guard's D is 2 * MARGIN: two boxes, each grown by MARGIN, must overlap when the shapes inside them come that close."""
import dataclasses

import numpy as np

HIT, CLEAR, UNDECIDED = "hit", "clear", "undecided"
_SIGNS = np.array([[(i >> 2 & 1) * 2 - 1, (i >> 1 & 1) * 2 - 1, (i & 1) * 2 - 1] for i in range(8)], dtype=np.float64)


@dataclasses.dataclass(frozen=True)
class Bracket:
    lower: float
    upper: float
    index: tuple                         # the witness: hull vertices ...
    weight: tuple                        # ... and their weights (>= 0, sum 1)
    axis: tuple                          # the separating unit axis, box -> hull; None: none found (lower = 0)

    @property
    def width(self):
        return self.upper - self.lower


def box_corners(center, axes, half):
    """The 8 corners of the box centre + axes @ (+-half) (axes: columns)."""
    return np.asarray(center, float) + (_SIGNS * np.asarray(half, float)) @ np.asarray(axes, float).T


def point_box_distance(x, center, axes, half):
    """Closed form: the part of the point's box-frame coordinates that sticks out of the half extents."""
    l = np.asarray(axes, float).T @ (np.asarray(x, float) - np.asarray(center, float))
    return float(np.linalg.norm(np.maximum(np.abs(l) - np.asarray(half, float), 0.0)))


def upper_bound(hull, index, weight, box):
    """Re-evaluates a witness: sum weight_i hull[index_i] (weights checked to be a convex combination) -> its distance to the box."""
    w = np.asarray(weight, float)
    assert (w >= 0).all() and abs(w.sum() - 1.0) < 1e-12 and len(index) == len(w) >= 1
    return point_box_distance(w @ np.asarray(hull, float)[list(index)], *box)


def lower_bound(hull, axis, box):
    """Re-evaluates a separating axis: min(hull . g) - max(box corners . g) for the unit axis g, never below 0."""
    if axis is None:
        return 0.0
    g = np.asarray(axis, float)
    assert abs(g @ g - 1.0) < 1e-12
    return max(0.0, float((np.asarray(hull, float) @ g).min() - (box_corners(*box) @ g).max()))


def _gjk_certificates(hull, box):
    """oracle/gjk_epa.py's GJK on (hull, box) -> (indices, weights, axis or None): the witness as a combination of the hull vertices its final
    simplex holds, the axis from the box's witness to the hull's."""
    from oracle import gjk_epa
    center, axes, half = box
    _, pa, pb, simplex = gjk_epa.gjk(gjk_epa.hull_support(hull), gjk_epa.box_support(center, axes, half))
    _, lam = gjk_epa._closest_on_simplex([s[0] for s in simplex])
    lam = np.maximum(np.asarray(lam, float), 0.0)
    lam = lam / lam.sum()
    weight = {}                                                                  # a vertex may sit in the simplex twice (with two box corners)
    for s, l in zip(simplex, lam):
        k = int(np.flatnonzero((hull == s[1]).all(1))[0])
        weight[k] = weight.get(k, 0.0) + float(l)
    index, lam = list(weight), np.array(list(weight.values()))
    axis = None
    if pa is not None and np.linalg.norm(pa - pb) > 0:
        axis = (pa - pb) / np.linalg.norm(pa - pb)
        axis = axis / np.linalg.norm(axis)
    return index, lam, axis


def bracket(hull, box, decide_at=None):
    """Bracket on the distance between conv(hull) ([n][3] world vertices) and box = (centre, axes as columns, half extents).  decide_at = D: the search
    stops at the first certificates that decide the pair at D (the bracket is then true but may be wide); None: always the full search."""
    hull = np.ascontiguousarray(hull, dtype=np.float64)
    center, axes, half = (np.asarray(v, dtype=np.float64) for v in box)
    box = (center, axes, half)
    l = (hull - center) @ axes                                                   # the hull in the box's frame
    out = np.maximum(np.abs(l) - half, 0.0)
    k = int(np.argmin((out * out).sum(1)))                                       # the single vertex nearest the box: a witness
    index, weight = (k,), (1.0,)
    gaps = np.concatenate([l.min(0) - half, -half - l.max(0)])                   # the box's own six face axes
    f = int(np.argmax(gaps))
    axis = (axes[:, f % 3] * (1.0 if f < 3 else -1.0)) if gaps[f] > 0 else None
    axis = None if axis is None else axis / np.linalg.norm(axis)
    lo, up = lower_bound(hull, axis, box), upper_bound(hull, index, weight, box)
    if decide_at is None or not (up <= decide_at or lo > decide_at):
        gi, gw, ga = _gjk_certificates(hull, box)
        gup, glo = upper_bound(hull, gi, gw, box), lower_bound(hull, ga, box)
        if gup < up:
            up, index, weight = gup, tuple(gi), tuple(float(w) for w in gw)
        if glo > lo:
            lo, axis = glo, ga
    assert lo <= up + 1e-9, (lo, up)                                             # two true bounds cannot cross (beyond the witness's own rounding)
    return Bracket(lo, up, tuple(index), tuple(weight), None if axis is None else tuple(float(a) for a in axis))


def classify(b, D):
    return HIT if b.upper <= D else CLEAR if b.lower > D else UNDECIDED


def tally(brackets, D):
    """{"hit", "clear", "undecided"} counts of an iterable of brackets at D."""
    out = {HIT: 0, CLEAR: 0, UNDECIDED: 0}
    for b in brackets:
        out[classify(b, D)] += 1
    return out
