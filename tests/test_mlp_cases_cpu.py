"""The case table of tests/test_gpu_mlp_matrix.py without a GPU (tests/mlp_cases.py): it reaches every named edge of csrc/tg_mlp.hip and loses
one with any case deleted; every exact variant is exact under the seed the GPU test uses; no case holds more than 64 MiB on the device; and
numpy mutants - what a kernel wrong at ONE edge would return - change the exact cases' float32 bits in the outputs that edge owns."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlp_cases as mc  # noqa: E402
import mlp_ref as ref  # noqa: E402

f32, f64 = np.float32, np.float64
PATTERN_F32 = np.frombuffer(bytes([0xA5] * 4), f32)[0]      # what an unwritten float of a guarded buffer holds (tests/device_guard.py)


def _named(name, B=None):
    return next(case for n, case in mc.NAMED if n == name and (B is None or case[0] == B))


def test_the_table_reaches_every_edge_and_every_case_owns_one():
    everything = mc.reached()
    assert everything == set(mc.EDGES), (everything ^ set(mc.EDGES))
    assert len(set(mc.EDGES)) == len(mc.EDGES)
    for name in mc.TABLE:
        lost = everything - mc.reached(without=name)
        print(f"{name}: alone in reaching {sorted(lost)}")
        assert lost, name                                                    # a deleted case is noticed
    # the edges the issue names, case by case
    assert mc.paths(_named("four-mixed", 65)) >= {"T=4", "mixed depths", "staging: partial second block", "outT=255", "outT=31", "outT=32",
                                                  "second block crosses column 128", "second block starts inside a 32-column group",
                                                  "straddling tile, both blocks", "reduce with the dx row", "reduce: more than 12 segments"}
    assert mc.paths(_named("widest-in")) >= {"K0=1024", "fwd: 32 staging chunks", "bwd: four k tiles a wave", "T=1: dx written by k_mlp_bwd"}
    assert mc.paths(_named("odd-in-three")) >= {"T=3", "K0=1023", "in odd", "in%32=31", "bwd: four k tiles a wave"}
    assert mc.paths(_named("three-tiles")) >= {"a workgroup walks three tiles", "G=64, 2 or 3 tiles each", "partial reload, more than two dweight tiles",
                                               "partial reload, K0>32", "reduce without the dx row"}
    assert mc.plan(_named("three-tiles"))["slab_floats"] == 132353
    assert mc.plan(_named("full-grid")) == dict(mc.plan(_named("full-grid")), n_tiles=64, G=64, min_tiles=1, max_tiles=1)
    assert mc.plan(_named("grid-plus-one")) == dict(mc.plan(_named("grid-plus-one")), n_tiles=65, G=64, min_tiles=1, max_tiles=2)
    assert mc.paths(_named("rows-32")) >= {"G=1", "no reduce", "last tile full, G=1", "Ka=1"}
    # the option runs: which tiles the dx skip passes over
    K0 = 40
    tower0 = mc.TABLE["four-mixed"][3][:1]
    assert mc.skipped_dx_tiles((65, K0, 33, tower0), (True, False)) == [] and mc.skipped_dx_tiles((65, K0, 33, tower0), (False, True)) == [0]
    assert mc.skipped_dx_tiles((65, K0, 1, tower0), (True, False)) == [1] and mc.skipped_dx_tiles((65, K0, 1, tower0), (False, True)) == []
    assert mc.skipped_dx_tiles((65, K0, 32, tower0), (True, False)) == [1] and mc.skipped_dx_tiles((65, K0, 32, tower0), (False, True)) == [0]
    assert [mc.straddling_tile(K0, Ka) for Ka in (33, 1, 32, 40)] == [1, 0, None, None]


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_exact_variants_are_exact_under_the_gpu_tests_seeds_and_fit_the_byte_cap(case):
    B, K0, Ka, spec = case
    (x, towers), _ = mc.forward_variants(case)
    for tower in towers:
        ref.assert_exact_forward(x, tower)
    (x, towers, hs, dys), _ = mc.backward_variants(case)
    for tower, h, dy in zip(towers, hs, dys):
        ref.assert_exact_backward(x, tower, h, dy)
    if B >= 33:
        relu = [h for t, (w, a, two) in enumerate(spec) for h, name in zip(hs[t], a) if name == "relu"]
        assert all(0.3 < float((h == 0).mean()) < 0.7 for h in relu)         # about half of the ReLU units are off
    nbytes = mc.device_bytes(case)
    print(f"{mc.case_id(case)}: {nbytes / 2**20:.1f} MiB on the device, workspace {mc.workspace_bytes(case)} bytes")
    assert nbytes < mc.BYTE_CAP


def test_the_workspace_restatement_equals_the_library_where_it_is_built():
    """tg_mlp_backward_workspace needs no device; the GPU test repeats the comparison."""
    from tactile_gym_amd import _capi
    L = _capi.lib()
    for case in mc.CASES + [c for _, c, _ in mc.option_runs()]:
        B, K0, Ka, _ = case
        arr = (_capi.TgMlpTower * len(case[3]))()
        for t, tower in enumerate(mc.layers_of(case)):
            arr[t].n_layers = len(tower)
            for l, (k, out, out2) in enumerate(tower):
                arr[t].layer[l].in_, arr[t].layer[l].out, arr[t].layer[l].out2 = k, out, out2
        assert L.tg_mlp_backward_workspace(B, Ka, K0 - Ka, arr, len(case[3])) == mc.workspace_bytes(case), mc.case_id(case)


# ---------------------------------------------------------------------------------------------------------------------- path mutants
def _rows(x, hs, dy, rows):
    return tuple(b[rows] if b is not None else None for b in x), [h[rows] for h in hs], dy[rows]


def _grads_over(x, tower, hs, dy, rows):
    """The sums over `rows` only: what a kernel that loses the other rows' terms returns (rows are independent terms of every sum)."""
    xs, hss, dys = _rows(x, hs, dy, rows)
    return ref.tower_backward(xs, tower, hss, dys)[0]


def _row_mask(case, tiles):
    m = np.zeros(case[0], bool)
    for tile in tiles:
        m[tile * mc.ROWS:(tile + 1) * mc.ROWS] = True
    return m


def _overwritten_partials(case):
    """Only each workgroup's LAST tile survives when the later tiles overwrite the partial instead of continuing it."""
    return _row_mask(case, [mc.tiles_of_group(case, g)[-1] for g in range(mc.plan(case)["G"])])


def _last_slab_left_out(case):
    G = mc.plan(case)["G"]
    return ~_row_mask(case, mc.tiles_of_group(case, G - 1))


def _zero_w(ly, rows=None, cols=None):
    """The layer with W's rows from `rows` on (over both row blocks), or its columns from `cols` on, read as zeros."""
    w, _ = ref.full_w(ly)
    w = w.copy()
    if rows is not None:
        w[rows:] = 0
    if cols is not None:
        w[:, cols:] = 0
    out = ly["w"].shape[0]
    new = dict(ly, w=w[:out].astype(f32))
    if ly["w2"] is not None:
        new["w2"] = w[out:].astype(f32)
    return new


def _report(name, what, factor, changed):
    note = "" if factor > 1000 else "  (below 1000: the exact case carries this edge)"
    print(f"{name}: {what}: exact bits changed: {changed}; random case {factor:.3g} bounds{note}")
    assert changed, (name, what)


def _forward_mutants(case, name, mutate, owned):
    """mutate(tower) -> (layer index, mutated tower) or None; owned(h) picks the outputs the edge owns."""
    (xe, te), (xr, tr) = mc.forward_variants(case)
    seen = 0
    for t in range(len(te)):
        hit = mutate(te[t])
        if hit is None:
            continue
        l, bad = hit
        want, got = ref.tower_forward(xe, te[t])[l][0], ref.tower_forward(xe, bad)[l][0]
        changed = not np.array_equal(owned(want).astype(f32).view(np.uint32), owned(got).astype(f32).view(np.uint32))
        (h, bound), bad_r = ref.tower_forward(xr, tr[t])[l], ref.tower_forward(xr, mutate(tr[t])[1])[l][0]
        factor = float((np.abs(owned(bad_r) - owned(h)) / owned(bound)).max())
        _report(name, f"{mc.case_id(case)} tower {t} layer {l}", factor, changed)
        seen += 1
    assert seen, (name, "no layer of the case has the edge")


def test_forward_mutants_unstaged_rows_and_dropped_chunks():
    def unstaged(tower):                                                     # rows co >= 128 of a layer with 128 < outT < 256 left unstaged
        for l, ly in enumerate(tower):
            outT = ref.full_w(ly)[0].shape[0]
            if 128 < outT < 256:
                return l, [_zero_w(v, rows=128) if i == l else v for i, v in enumerate(tower)]
        return None

    def dropped(tower):                                                      # layer 0's k chunks beyond the eighth: in <= 256 assumed
        if tower[0]["w"].shape[1] <= 256:
            return None
        return 0, [_zero_w(tower[0], cols=256)] + list(tower[1:])

    for nm in ("four-mixed", "odd-in-three", "grid-plus-one"):
        case = _named(nm)
        _forward_mutants((33,) + case[1:], "W rows from 128 on left unstaged", unstaged, lambda h: h[:, 128:])
    for nm in ("widest-in", "odd-in-three"):
        _forward_mutants(_named(nm), "k chunks beyond the eighth dropped", dropped, lambda h: h)


def _backward_mutant(case, name, keep):
    """keep: the rows whose terms the mutant still sums.  Every dweight and dbias of the case belongs to the edge."""
    (xe, te, he, de), (xr, tr, hr, dr) = mc.backward_variants(case)
    changed, factor = True, 0.0
    for t in range(len(te)):
        want, got = ref.tower_backward(xe, te[t], he[t], de[t])[0], _grads_over(xe, te[t], he[t], de[t], keep)
        for l in range(len(te[t])):
            # per layer: dweight or dbias differs (a one-element dbias may lose terms that happen to add up to zero)
            changed = changed and any(not np.array_equal(a.astype(f32).view(np.uint32), b.astype(f32).view(np.uint32)) for a, b in zip(want[l], got[l]))
        grads, bounds, _, _ = ref.tower_backward(xr, tr[t], hr[t], dr[t])
        bad = _grads_over(xr, tr[t], hr[t], dr[t], keep)
        for l in range(len(tr[t])):
            for a, b, e in zip(grads[l], bad[l], bounds[l]):
                factor = max(factor, float((np.abs(a - b) / np.maximum(e, 1e-300)).max()))
    _report(name, f"{mc.case_id(case)}: every dweight and dbias ({int((~keep).sum())} of {case[0]} rows lost)", factor, changed)


def test_backward_mutants_overwritten_partials_and_a_slab_left_out():
    for nm in ("grid-plus-one", "three-tiles"):
        case = _named(nm)
        keep = _overwritten_partials(case)
        assert not keep.all()
        _backward_mutant(case, "a workgroup's later tiles overwrite its partial", keep)
    for case in (_named("four-mixed", 65), _named("three-tiles")):
        keep = _last_slab_left_out(case)
        assert not keep.all() and keep.any()
        _backward_mutant(case, "the last slab left out of the reduction", keep)


def _dh0(x, towers, hs, dys):
    outs = [ref.tower_backward(x, tower, h, dy) for tower, h, dy in zip(towers, hs, dys)]
    return [o[2] for o in outs], [o[3] for o in outs]


def test_dx_mutants_straddling_columns_unwritten_and_a_tower_left_out():
    for case, want in mc.dx_runs():
        B, K0, Ka, spec = case
        kt = mc.straddling_tile(K0, Ka)
        if len(spec) != 1 or kt is None or not any(want):
            continue
        (xe, te, he, de), (xr, tr, hr, dr) = mc.backward_variants(case)
        cols = [k for k in range(kt * 32, min(kt * 32 + 32, K0)) if want[0 if k < Ka else 1]]   # the straddling tile's columns that ARE asked for
        assert cols
        total = ref.sum_dx(*_dh0(xe, te, he, de))[0].astype(f32)
        bad = total.copy()
        bad[:, cols] = PATTERN_F32
        changed = bool((bad[:, cols].view(np.uint32) != total[:, cols].view(np.uint32)).any(axis=0).all())    # every such column shows it
        tr_total, tr_bound = ref.sum_dx(*_dh0(xr, tr, hr, dr))
        live = tr_bound[:, cols] > 0                                          # a row whose last-layer units are all off has dh_0 = 0 exactly
        factor = float((np.abs(f64(PATTERN_F32) - tr_total[:, cols])[live] / tr_bound[:, cols][live]).max())
        _report("the straddling tile's columns left unwritten", f"Ka = {Ka}, want_dx = {want}", factor, changed)
    for case in (_named("four-mixed", 65), _named("odd-in-three")):
        (xe, te, he, de), (xr, tr, hr, dr) = mc.backward_variants(case)
        dh0s, e0s = _dh0(xe, te, he, de)
        total, bad = ref.sum_dx(dh0s, e0s)[0], sum(dh0s[:2])
        changed = not np.array_equal(total.astype(f32).view(np.uint32), bad.astype(f32).view(np.uint32))
        dh0s, e0s = _dh0(xr, tr, hr, dr)
        tot, bound = ref.sum_dx(dh0s, e0s)
        factor = float((np.abs(tot - sum(dh0s[:2])) / bound).max())
        _report("dh_0 of the towers from 2 on left out of dx", mc.case_id(case), factor, changed)
