"""tg_mlp_forward and tg_mlp_backward (csrc/tg_mlp.hip) on raw pointers between guard bytes at every path edge tests/mlp_cases.py names: three
and four towers of mixed depth, widths between 128 and 256, K0 up to 1024, a full grid of 64 workgroups and workgroups that walk two and three
row tiles on their own partial sums, dx blocks cut inside a k tile, frozen parameters on many slabs, and non-finite values.

As in tests/test_gpu_mlp_abi.py: on the exact variants float32 arithmetic is exact in every order (tests/test_mlp_cases_cpu.py asserts it with
these seeds), so the float64 restatement IS the required bits; the random variants (activations rotated, tanh everywhere) lie within the
derived bounds of tests/mlp_ref.py from the device's own h_{l-1} bits.

Non-finite values.  ReLU is z > 0 ? z : (z != z ? z : 0): a NaN stays a NaN (torch.relu), where fmaxf(z, 0) returned 0.  A poisoned row
changes no other row: the padded MFMA operands make NaNs only in lanes that are not stored."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlp_cases as mc  # noqa: E402
import mlp_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from device_guard import PATTERN  # noqa: E402
from mlp_device import _backward, _bits, _check_backward, _forward, _within  # noqa: E402

f32, f64 = np.float32, np.float64
FOUR_MIXED = next(case for name, case in mc.NAMED if name == "four-mixed" and case[0] == 65)
GRID_PLUS_ONE = next(case for name, case in mc.NAMED if name == "grid-plus-one")


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_forward_exact_bits_and_random_bounds(case):
    B, K0, Ka, spec = case
    (x, towers), (xr, towers_r) = mc.forward_variants(case)
    for tower in towers:
        ref.assert_exact_forward(x, tower)
    saved, last = _forward(x, towers, B, True), _forward(x, towers, B, False)
    for t, tower in enumerate(towers):
        want = ref.tower_forward(x, tower)
        for l in range(len(tower)):
            assert _bits(saved.layer_h(t, l), want[l][0].astype(f32)), (t, l)
            assert (last.layer_h(t, l) is None) == (l < len(tower) - 1)
        assert _bits(last.layer_h(t, len(tower) - 1), want[-1][0].astype(f32))
        if any(ly["act"] == "relu" and ly["w"].shape[0] >= 33 for ly in tower):
            h = np.concatenate([want[l][0].reshape(-1) for l, ly in enumerate(tower) if ly["act"] == "relu"])
            assert (h == 0).any() and (h > 0).any()                          # the clamp is exercised
    x, towers = xr, towers_r
    saved, last = _forward(x, towers, B, True), _forward(x, towers, B, False)
    for t, tower in enumerate(towers):
        want = ref.tower_forward(x, tower)
        hprev = ref.cat_input(x)
        for l, ly in enumerate(tower):
            got = saved.layer_h(t, l)
            h, bound = ref.layer_forward(hprev, ly)                           # from the device's own h_{l-1} bits
            _within(got, h, bound, f"tower {t} h_{l + 1} ({ly['act']})")
            hprev = got
        _within(got, want[-1][0], want[-1][1], f"tower {t} output, propagated")
        assert _bits(last.layer_h(t, len(tower) - 1), got)                    # the same bits whether or not the hidden layers are saved


@pytest.mark.parametrize("case", mc.CASES, ids=mc.case_id)
def test_backward_exact_bits_random_bounds_and_repeat(case):
    B, K0, Ka, spec = case
    (x, towers, hs, dys), (xr, towers_r, hs_r, dys_r) = mc.backward_variants(case)
    for tower, h, dy in zip(towers, hs, dys):
        ref.assert_exact_backward(x, tower, h, dy)
    call, dx = _backward(x, towers, hs, dys, B)
    assert call.workspace_bytes == mc.workspace_bytes(case)                   # the restatement of mlp_plan against the C entry's answer
    _check_backward(call, dx, x, towers, hs, dys, exact=True)
    call, dx = _backward(xr, towers_r, hs_r, dys_r, B, twice=True)
    _check_backward(call, dx, xr, towers_r, hs_r, dys_r, exact=False)


def _written(call):
    """{(t, l, i): host bits} of every gradient buffer of the call."""
    return {(t, l, i): g.host(f32).copy() for t, row in enumerate(call.grad) for l, gb in enumerate(row) for i, g in enumerate(gb) if g is not None}


@pytest.mark.parametrize("split", mc.STRADDLES, ids=lambda s: f"ka{s[0]}+{s[1]}")
def test_dx_blocks_cut_inside_a_k_tile(split):
    """One block of dx asked for, or none, where the blocks meet inside a 32-wide k tile (Ka = 33, Ka = 1) or at its edge (Ka = 32): with one
    tower k_mlp_bwd writes dx itself and skips the tiles that hold no asked-for column; with four the towers' dh_0 go through k_mlp_reduce."""
    Ka, Kb = split
    B, K0, _, spec = FOUR_MIXED
    assert Ka + Kb == K0
    for towers_spec in (spec[:1], spec):
        case = (B, K0, Ka, towers_spec)
        for exact, (x, towers, hs, dys) in zip((True, False), mc.backward_variants(case)):
            if exact:
                for tower, h, dy in zip(towers, hs, dys):
                    ref.assert_exact_backward(x, tower, h, dy)
            full, full_dx = _backward(x, towers, hs, dys, B)
            _check_backward(full, full_dx, x, towers, hs, dys, exact=exact)
            for want in mc.PARTIAL_DX:
                call, dx = _backward(x, towers, hs, dys, B, want_dx=want)
                cols = np.r_[np.arange(Ka) if want[0] else [], np.arange(Ka, K0) if want[1] else []].astype(int)
                assert np.isnan(np.delete(dx, cols, axis=1)).all()            # the block that was not asked for has no buffer to write
                assert _bits(dx[:, cols], full_dx[:, cols]), (len(towers), want)   # the other has the bits of the full run
                got, ref_bits = _written(call), _written(full)
                assert all(_bits(got[k], ref_bits[k]) for k in ref_bits), (len(towers), want)
                if exact:
                    _check_backward(call, dx, x, towers, hs, dys, exact=True, want_dx=want)


def test_frozen_parameters_on_many_slabs():
    """grid-plus-one (65 row tiles, 64 slabs): layer (0, 0) frozen whole, (3, 0) given only dweight2 and dbias2, (1, 2) only dbias, tower 2's
    dy NULL.  What is written has the bits of the run with nothing frozen; what is not asked for is not written."""
    case = GRID_PLUS_ONE
    B = case[0]
    names = ("dweight", "dbias", "dweight2", "dbias2")
    for exact, (x, towers, hs, dys) in zip((True, False), mc.backward_variants(case)):
        dys = [None if t in mc.FROZEN_NULL_DY else dy for t, dy in enumerate(dys)]
        full, full_dx = _backward(x, towers, hs, dys, B)
        _check_backward(full, full_dx, x, towers, hs, dys, exact=exact)       # a NULL dy with G > 1: zeros for its tower

        def freeze(call):
            for (t, l), kept in mc.FROZEN.items():
                for name in names:
                    if name not in kept:
                        setattr(call.arr[t].layer[l], name, None)
        call, dx = _backward(x, towers, hs, dys, B, edit=freeze)
        assert _bits(dx, full_dx)
        got, ref_bits = _written(call), _written(full)
        for (t, l, i), bits in ref_bits.items():
            if (t, l) in mc.FROZEN and names[i] not in mc.FROZEN[(t, l)]:
                assert bool((call.grad[t][l][i].payload() == PATTERN).all()), (t, l, names[i])     # not asked for: not written
            else:
                assert _bits(got[(t, l, i)], bits), (t, l, names[i])
        assert any(ly[2] for ly in mc.layers_of(case)[3]) and call.grad[3][0][2] is not None         # (3, 0) does have a second block


def test_a_row_alone_equals_the_row_in_a_batch_of_65_and_each_tower_alone():
    B, K0, Ka, spec = FOUR_MIXED
    rng = np.random.default_rng(7)
    xfull = ref.random_input(rng, B, K0)
    for at in (0, 31, 32, 64):
        xfull[at] = xfull[5]
    towers = [ref.random_tower(rng, K0, w, mc.random_acts(a, t), two) for t, (w, a, two) in enumerate(spec)]
    assert {ly["act"] for tower in towers for ly in tower} == {"none", "tanh", "relu"}
    batch = _forward(ref.split_input(xfull, Ka), towers, B)
    alone = _forward(ref.split_input(xfull[5:6].copy(), Ka), towers, 1)
    singles = [_forward(ref.split_input(xfull, Ka), [tower], B) for tower in towers]
    for t, tower in enumerate(towers):
        for l in range(len(tower)):
            h = batch.layer_h(t, l)
            for at in (0, 5, 31, 32, 64):
                assert _bits(h[at], alone.layer_h(t, l)[0]), (t, l, at)
            assert _bits(h, singles[t].layer_h(0, l)), (t, l)


# ---------------------------------------------------------------------------------------------------------------------- non-finite values
POISONED = 40


def _relu_nan(z):
    return np.where(z > 0, z, np.where(np.isnan(z), z, 0.0))


def _forward64(x, tower):
    """Every layer's h in float64 with the kernel's ReLU: a NaN stays a NaN."""
    h, out = ref.cat_input(x), []
    with np.errstate(all="ignore"):
        for ly in tower:
            w, b = ref.full_w(ly)
            z = (h[:, None, :] * w[None, :, :]).sum(axis=2) + b               # term by term: no BLAS shortcut decides where a NaN lands
            h = np.tanh(z) if ly["act"] == "tanh" else _relu_nan(z) if ly["act"] == "relu" else z
            out.append(h)
    return out


def test_forward_a_poisoned_row_is_nan_and_changes_no_other_row():
    B, K0, Ka, spec = FOUR_MIXED
    _, (x, towers) = mc.forward_variants(FOUR_MIXED)
    clean = _forward(x, towers, B)
    xfull = ref.cat_input(x).astype(f32)
    xfull[POISONED, 0], xfull[POISONED, K0 - 1] = np.inf, np.nan
    xp = ref.split_input(xfull, Ka)
    dirty = _forward(xp, towers, B)
    others = np.arange(B) != POISONED
    relu_layers = 0
    for t, tower in enumerate(towers):
        want = _forward64(xp, tower)
        for l, ly in enumerate(tower):
            got = dirty.layer_h(t, l)
            assert _bits(got[others], clean.layer_h(t, l)[others]), (t, l)    # every other row keeps the clean run's bits
            assert not np.isnan(got[others]).any()
            assert np.array_equal(np.isnan(got[POISONED]), np.isnan(want[l][POISONED])), (t, l, ly["act"])
            assert np.isnan(want[l][POISONED]).all()                          # inf w + ... + NaN w: every unit of the row
            relu_layers += ly["act"] == "relu"
    assert relu_layers >= 3


def _backward64(x, tower, hs, dy):
    """(grads, dh_0) in float64 with the kernel's selects: ReLU passes dh where h > 0 and 0 elsewhere, whatever dh is."""
    grads = [None] * len(tower)
    with np.errstate(all="ignore"):
        dh = np.asarray(dy, f64)
        for l in range(len(tower) - 1, -1, -1):
            ly = tower[l]
            w, _ = ref.full_w(ly)
            h, hprev = np.asarray(hs[l], f64), (np.asarray(hs[l - 1], f64) if l else ref.cat_input(x))
            g = dh * (1.0 - h * h) if ly["act"] == "tanh" else np.where(h > 0, dh, 0.0) if ly["act"] == "relu" else dh
            grads[l] = ((g[:, :, None] * hprev[:, None, :]).sum(axis=0), g.sum(axis=0))
            dh = (g[:, :, None] * w[None, :, :]).sum(axis=1)
    return grads, dh


def test_backward_a_poisoned_dy_row_changes_no_other_row_of_dx():
    B, K0, Ka, spec = FOUR_MIXED
    _, (x, towers, hs, dys) = mc.backward_variants(FOUR_MIXED)
    clean, clean_dx = _backward(x, towers, hs, dys, B)
    dys = [dy.copy() for dy in dys]
    for dy in dys:
        dy[POISONED, 0] = np.inf
        dy[POISONED, -1] = np.nan                                             # a one-column dy: the NaN alone
    call, dx = _backward(x, towers, hs, dys, B)
    others = np.arange(B) != POISONED
    assert _bits(dx[others], clean_dx[others]) and not np.isnan(dx[others]).any()
    total = 0.0
    for t, tower in enumerate(towers):
        grads, dh0 = _backward64(x, tower, hs[t], dys[t])
        total = total + dh0
        for l in range(len(tower)):
            dw, db = call.layer_grads(t, l)
            assert np.array_equal(np.isnan(dw), np.isnan(grads[l][0])), (t, l, "dweight")
            assert np.array_equal(np.isnan(db), np.isnan(grads[l][1])), (t, l, "dbias")
    assert np.array_equal(np.isnan(dx[POISONED]), np.isnan(total[POISONED])) and np.isnan(dx[POISONED]).any()
