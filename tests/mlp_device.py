"""The device side of the MLP towers' raw-pointer tests (tests/test_gpu_mlp_abi.py, tests/test_gpu_mlp_matrix.py): one call's buffers between
guard bytes, tg_mlp_forward and tg_mlp_backward behind their memory checks, and the comparison of a backward call with the float64 restatement
(tests/mlp_ref.py)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mlp_ref as ref  # noqa: E402
from device_guard import PATTERN, Guarded  # noqa: E402

f32 = np.float32
ACT = {"none": 0, "tanh": 1, "relu": 2}


def _lib():
    from tactile_gym_amd import _capi
    return _capi, _capi.lib()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _g(a):
    a = np.ascontiguousarray(a, f32)
    return Guarded(a.nbytes, fill=a)


class Call:
    """The device side of one call: guarded copies of the input blocks and the towers' parameters, guarded h / gradient buffers, and the
    tg_mlp_tower array over them."""

    def __init__(self, x, towers, B, save_all=True, hs=None, dys=None, backward=False, skip=()):
        capi, _ = _lib()
        self.x, self.towers, self.B = x, towers, B
        self.gx = [_g(b) if b is not None else None for b in x]
        self.inputs, self.outputs = [(g, b) for g, b in zip(self.gx, x) if g is not None], []
        self.arr = (capi.TgMlpTower * len(towers))()
        self.h, self.grad = [], []
        for t, tower in enumerate(towers):
            self.arr[t].n_layers = len(tower)
            hrow, grow = [], []
            for l, ly in enumerate(tower):
                d = self.arr[t].layer[l]
                out, out2 = ly["w"].shape[0], (ly["w2"].shape[0] if ly["w2"] is not None else 0)
                d.in_, d.out, d.out2, d.act = ly["w"].shape[1], out, out2, ACT[ly["act"]]
                for name, src in (("weight", ly["w"]), ("bias", ly["b"]), ("weight2", ly["w2"]), ("bias2", ly["b2"])):
                    if src is not None:
                        g = _g(src)
                        self.inputs.append((g, src))
                        setattr(d, name, g.ptr)
                bufs = [None, None]
                if save_all or l == len(tower) - 1:
                    for i, (n, name) in enumerate(((out, "h"), (out2, "h2"))):
                        if n:
                            given = None if hs is None else np.ascontiguousarray(hs[t][l][:, :out] if i == 0 else hs[t][l][:, out:])
                            bufs[i] = Guarded(4 * B * n, fill=given)
                            setattr(d, name, bufs[i].ptr)
                            (self.outputs if hs is None else self.inputs).append((bufs[i], given) if hs is not None else bufs[i])
                hrow.append(bufs)
                gb = [None] * 4
                if backward and (t, l) not in skip:
                    for i, (n, name) in enumerate(((out * d.in_, "dweight"), (out, "dbias"), (out2 * d.in_, "dweight2"), (out2, "dbias2"))):
                        if n:
                            gb[i] = Guarded(4 * n)
                            setattr(d, name, gb[i].ptr)
                            self.outputs.append(gb[i])
                grow.append(gb)
            if dys is not None and dys[t] is not None:
                out = tower[-1]["w"].shape[0]
                g0 = _g(dys[t][:, :out])
                self.inputs.append((g0, np.ascontiguousarray(dys[t][:, :out])))
                self.arr[t].dy = g0.ptr
                if dys[t].shape[1] > out:
                    g1 = _g(dys[t][:, out:])
                    self.inputs.append((g1, np.ascontiguousarray(dys[t][:, out:])))
                    self.arr[t].dy2 = g1.ptr
            self.h.append(hrow)
            self.grad.append(grow)
        self.Ka = x[0].shape[1]
        self.Kb = x[1].shape[1] if x[1] is not None else 0

    def xargs(self):
        return (C.c_void_p(self.gx[0].ptr), self.Ka, C.c_void_p(self.gx[1].ptr if self.gx[1] is not None else None), self.Kb, self.B, self.arr,
                len(self.towers))

    def check_memory(self, extra=()):
        torch.cuda.synchronize()
        for g, src in self.inputs:
            assert g.guards_intact() and _bits(g.host(f32), np.ascontiguousarray(src, f32).reshape(-1))       # inputs are unchanged
        for g in list(self.outputs) + list(extra):
            assert g.guards_intact()

    def layer_h(self, t, l):
        """[B, out + out2] float32 of layer l, or None where it was not saved."""
        bufs = self.h[t][l]
        if bufs[0] is None:
            return None
        parts = [b.host(f32).reshape(self.B, -1) for b in bufs if b is not None]
        return np.concatenate(parts, axis=1)

    def layer_grads(self, t, l):
        """(dweight [out + out2, in], dbias [out + out2]) float32."""
        gb, k = self.grad[t][l], self.towers[t][l]["w"].shape[1]
        return (np.concatenate([b.host(f32).reshape(-1, k) for b in (gb[0], gb[2]) if b is not None]),
                np.concatenate([b.host(f32) for b in (gb[1], gb[3]) if b is not None]))


def _forward(x, towers, B, save_all=True):
    capi, L = _lib()
    call = Call(x, towers, B, save_all=save_all)
    capi.check(L.tg_mlp_forward(*call.xargs(), int(save_all), _stream()))
    call.check_memory()
    return call


def _backward(x, towers, hs, dys, B, want_dx=(True, True), shrink=0, twice=False, skip=(), edit=None):
    """One tg_mlp_backward call (two with twice=True, into fresh outputs) with a workspace of exactly the queried size less `shrink` bytes
    -> (call, dx [B, K0] with NaN where a block was not asked for), or the return code when shrink > 0.  edit(call), where given, changes the
    call's descriptors before the launch (the matrix tests take single gradient pointers out)."""
    capi, L = _lib()
    results = []
    for _ in range(2 if twice else 1):
        call = Call(x, towers, B, hs=hs, dys=dys, backward=True, skip=skip)
        if edit is not None:
            edit(call)
        nbytes = L.tg_mlp_backward_workspace(call.B, call.Ka, call.Kb, call.arr, len(towers))
        assert nbytes >= 0
        gws = Guarded(max(nbytes - shrink, 0) + 16)          # 16 spare bytes of the pattern behind the workspace: nothing may reach them
        gdx = [Guarded(4 * B * k) if k and w else None for k, w in zip((call.Ka, call.Kb), want_dx)]
        rc = L.tg_mlp_backward(*call.xargs(), C.c_void_p(gdx[0].ptr if gdx[0] else None), C.c_void_p(gdx[1].ptr if gdx[1] else None),
                               C.c_void_p(gws.ptr), nbytes - shrink, _stream())
        call.check_memory([g for g in gdx if g] + [gws])
        assert bool((gws.payload()[max(nbytes - shrink, 0):] == PATTERN).all())
        if shrink:
            assert rc != 0 and L.tg_last_error().decode().startswith("tg_mlp_backward:")
            for g in call.outputs + [g for g in gdx if g] + [gws]:
                assert bool((g.payload() == PATTERN).all())
            return rc
        capi.check(rc)
        dx = np.concatenate([g.host(f32).reshape(B, -1) if g else np.full((B, k), np.nan, f32)
                             for g, k in zip(gdx, (call.Ka, call.Kb)) if k], axis=1)
        call.workspace_bytes = nbytes
        results.append((call, dx))
    if twice:
        (c1, d1), (c2, d2) = results
        assert _bits(d1, d2)
        for t, tower in enumerate(towers):
            for l in range(len(tower)):
                assert all(_bits(a, b) for a, b in zip(c1.layer_grads(t, l), c2.layer_grads(t, l)))
    return results[0]


def _within(got, want, bound, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: largest error / bound = {ratio:.3g}")
    assert (err <= bound).all(), (what, ratio)


def _check_backward(call, dx, x, towers, hs, dys, exact, want_dx=(True, True)):
    dh0s, dh0_bounds = [], []
    for t, tower in enumerate(towers):
        dy = dys[t] if dys[t] is not None else np.zeros((call.B, hs[t][-1].shape[1]), f32)
        grads, bounds, dh0, e0 = ref.tower_backward(x, tower, hs[t], dy)
        dh0s.append(dh0)
        dh0_bounds.append(e0)
        for l in range(len(tower)):
            dw, db = call.layer_grads(t, l)
            if exact:
                assert _bits(dw, grads[l][0].astype(f32)), (t, l, "dweight")
                assert _bits(db, grads[l][1].astype(f32)), (t, l, "dbias")
            else:
                _within(dw, grads[l][0], bounds[l][0], f"tower {t} layer {l} dweight")
                _within(db, grads[l][1], bounds[l][1], f"tower {t} layer {l} dbias")
    total, bound = ref.sum_dx(dh0s, dh0_bounds)
    Ka = call.Ka
    cols = np.r_[np.arange(Ka) if want_dx[0] else [], np.arange(Ka, total.shape[1]) if want_dx[1] else []].astype(int)
    assert np.isnan(np.delete(dx, cols, axis=1)).all()                        # a block that was not asked for is not written
    if exact:
        assert float(sum(np.abs(d) for d in dh0s).max()) < ref.EXACT_LIMIT
        assert _bits(dx[:, cols], total.astype(f32)[:, cols])
    else:
        _within(dx[:, cols], total[:, cols], bound[:, cols], "dx")
