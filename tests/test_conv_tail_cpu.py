"""The device NatureCNN tail without a GPU: the float64 restatement (tests/conv_tail_ref.py) against torch's own float64 conv2d / linear and
autograd on every case the GPU tests use, the exact-arithmetic generators' conditions, the order probes' arithmetic, the ABI's declarations,
the checks that raise, the CPU path of conv_relu / linear_relu, and NatureCNN(device_tail=True) against the module it stands for."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import build_units  # noqa: E402
import conv_tail_ref as ref  # noqa: E402

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_conv_relu"]                  # at import: the whole file needs the feature
SB3_KEYS = ["cnn.0.weight", "cnn.0.bias", "cnn.2.weight", "cnn.2.bias", "cnn.4.weight", "cnn.4.bias", "linear.0.weight", "linear.0.bias"]
f32 = np.float32


class _Space:
    def __init__(self, shape):
        self.shape, self.dtype = tuple(shape), np.uint8


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("case", ref.CASES + ref.PATH_CASES, ids=ref.case_id)
def test_reference_equals_torch_float64_autograd(case):
    Cin, H, W, Cout, KH, KW, stride, B = case
    rng = np.random.default_rng(1)
    x, w, b, _, _ = ref.random_case(rng, case)
    xt = torch.from_numpy(x).double().requires_grad_()
    wt, bt = torch.from_numpy(w).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    y = F.relu(F.conv2d(xt, wt, bt, stride=stride))
    got, bound = ref.forward(x, w, b, stride)
    OH, OW = ref.out_hw(H, W, KH, KW, stride)
    assert got.shape == (B, Cout, OH, OW) and bound.shape == got.shape and (bound >= 0).all()
    _close(got, y.detach().numpy())
    if OH == OW == 1 and KH == H and KW == W:                                 # the linear layer IS this convolution
        lin = F.relu(F.linear(xt.detach().reshape(B, -1), wt.detach().reshape(Cout, -1), bt.detach()))
        _close(got.reshape(B, Cout), lin.numpy())
    dy = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(dy))
    r = ref.backward(x, w, y.detach().numpy(), dy, stride)
    _close(r["dw"], wt.grad.numpy())
    _close(r["db"], bt.grad.numpy())
    _close(r["dx"], xt.grad.numpy())
    for name in ("dw", "db", "dx"):
        assert r[name + "_bound"].shape == r[name].shape and (r[name + "_bound"] >= 0).all()
    assert (r["dx"][:, :, ref.unread(case)] == 0).all()


@pytest.mark.parametrize("case", ref.CASES + ref.PATH_CASES, ids=ref.case_id)
def test_grid_cases_are_exact_in_float32(case):
    Cin, H, W, Cout, KH, KW, stride, B = case
    x, w, b, y, dy = ref.grid_case(np.random.default_rng(2), case)        # asserts its magnitude conditions
    assert x.min() >= 0 and x.max() <= 15 and np.abs(w).max() <= 8 and np.abs(dy).max() <= 4
    assert (y == 0).any() and (y > 0).any()
    got, _ = ref.forward(x, w, b, stride)
    r = ref.backward(x, w, y, dy, stride)
    for a in (got, r["dw"], r["db"], r["dx"]):
        assert np.array_equal(a.astype(f32).astype(np.float64), a) and np.abs(a).max() < 2 ** 24       # a grid case's result is a float32 integer


def test_grid_generator_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):
        ref.grid_case(np.random.default_rng(0), (2, 3, 3, 32, 2, 2, 1, 70000))       # M 4 15 >= 2^24
    ref.grid_case(np.random.default_rng(0), (64, 16, 16, 512, 16, 16, 1, 1))           # the family's largest K and J are exact: 1966080, 4194304


def test_parts_rule_and_the_walking_cases():
    assert ref.parts(64, 512, 9216) == 1 and ref.parts(1024, 512, 9216) == 4 and ref.parts(10 ** 6, 512, 9216) == 7
    assert ref.parts(64 * 196, 64, 512) == 49 and ref.parts(64 * 144, 64, 576) == 36 and ref.parts(1024 * 196, 64, 512) == 64
    walks = []
    for case in ref.CASES:
        Cin, H, W, Cout, KH, KW, stride, B = case
        OH, OW = ref.out_hw(H, W, KH, KW, stride)
        M = B * OH * OW
        walks.append(-(-M // ref.BWD_CHUNK) / ref.parts(M, Cout, Cin * KH * KW))
    assert max(walks) > 4 and sum(w >= 4 for w in walks) >= 2                 # workgroups that walk four chunks and more
    L = _capi.lib()
    for case in ref.CASES:
        Cin, H, W, Cout, KH, KW, stride, B = case
        assert L.tg_conv_relu_bwd_workspace(B, Cin, H, W, Cout, KH, KW, stride) == ref.workspace_bytes(case), case
    # the header comment's worst cases at NatureCNN's shapes
    sizes = [L.tg_conv_relu_bwd_workspace(B, *s[:3], *s[3:]) for B in (64, 1024) for s in ref.REAL_128]
    assert sizes == [6472704, 5345280, 18882560, 8454144, 9502720, 75530240]


def test_the_partials_cap_in_the_workspace_query():
    """conv_parts' cap 2^25 / (Cout K), asked of the library itself (the query needs no device)."""
    L = _capi.lib()
    for case, P in (((64, 12, 12, 512, 12, 12, 1, 4096), 7), ((64, 16, 16, 512, 16, 16, 1, 2000), 4), (ref.CAP_CASE, 4)):
        Cin, H, W, Cout, KH, KW, stride, B = case
        K = Cin * KH * KW
        r = ref.route(case)
        assert r["cap_bound"] and r["P"] == P == ref.BWD_MAX_FLOATS // (Cout * K) and P < min(-(-B // ref.BWD_SHARE), ref.BWD_MAX_PARTS)
        got = L.tg_conv_relu_bwd_workspace(B, Cin, H, W, Cout, KH, KW, stride)
        assert got == 4 * P * (Cout * K + 4 * Cout) == ref.workspace_bytes(case), case
    assert L.tg_conv_relu_bwd_workspace(4096, 64, 12, 12, 512, 12, 12, 1) == 4 * 7 * (512 * 9216 + 4 * 512)
    assert L.tg_conv_relu_bwd_workspace(2000, 64, 16, 16, 512, 16, 16, 1) == 4 * 4 * (512 * 16384 + 4 * 512)
    assert not any(ref.route(c)["cap_bound"] for c in ref.CASES + ref.PATH_CASES)
    for case in ref.PATH_CASES:
        Cin, H, W, Cout, KH, KW, stride, B = case
        assert L.tg_conv_relu_bwd_workspace(B, Cin, H, W, Cout, KH, KW, stride) == ref.workspace_bytes(case), case


# Each path of csrc/tg_conv.hip's launchers and kernels as a predicate on conv_tail_ref.route's table
ROUTES = {
    "fwd generic, four channel tiles a workgroup (Cout >= 128)": lambda r: r["fwd"] == "generic" and r["fwd_cl"] == 2,
    "fwd generic, four channel tiles, a second channel block partly active": lambda r: (r["fwd"] == "generic" and r["fwd_cl"] == 2
                                                                                         and r["fwd_cblocks"] == 2 and r["fwd_last_cblock_partial"]),
    "fwd generic, a short last chunk behind full chunks": lambda r: r["fwd"] == "generic" and len(r["fwd_chunks"]) > 1 and r["fwd_chunks"][-1] < 32,
    "bwd, K > 64 with K % 64 in 1..32": lambda r: r["n_kblocks"] > 1 and r["k_mod_64"] == "1..32",
    "bwd, K > 64 with K % 64 in 33..63": lambda r: r["n_kblocks"] > 1 and r["k_mod_64"] == "33..63",
    "bwd, several partials over several channel blocks": lambda r: r["P"] > 1 and r["n_cblocks"] > 1,
    "dx generic, two channel tiles, the second partly valid": lambda r: r["dx"] == "generic" and r["dx_cl"] == 1 and r["dx_last_ctile_partial"],
    "dx generic, ky / stride = 15": lambda r: r["dx"] == "generic" and r["dx_max_ky_div"] == 15,
    "dx generic, ky % stride = 3 (stride 4)": lambda r: r["dx"] == "generic" and r["dx_max_ky_mod"] == 3 and r["stride"] == 4,
    "dx lin, a partly valid k tile over several batch tiles": lambda r: r["dx"] == "lin" and r["lin_dx_last_ktile"] > 0 and r["batch_tiles"] > 1,
    "the linear pair at a stride above 1": lambda r: r["fwd"] == "lin" and r["dx"] == "lin" and r["stride"] > 1,
}
# what CASES reached before PATH_CASES: everything else of this table
OLD_ROUTES = {
    "fwd lin": lambda r: r["fwd"] == "lin",
    "fwd generic, one, two and two-of-three channel tiles": lambda r: r["fwd"] == "generic" and r["fwd_cl"] in (0, 1),
    "bwd, several partials": lambda r: r["P"] == 64,
    "bwd, several channel blocks": lambda r: r["n_cblocks"] == 8,
    "dx generic, two full channel tiles": lambda r: r["dx"] == "generic" and r["dx_cl"] == 1 and not r["dx_last_ctile_partial"],
    "dx lin, full k tiles over several batch tiles": lambda r: r["dx"] == "lin" and r["lin_dx_last_ktile"] == 0 and r["batch_tiles"] == 3,
}


def test_route_table_names_the_paths_that_only_the_path_cases_reach():
    old = [ref.route(c) for c in ref.CASES]
    new = [ref.route(c) for c in ref.PATH_CASES]
    for name, reached in {**ROUTES, **OLD_ROUTES}.items():
        assert any(reached(r) for r in old + new), name
    for name, reached in OLD_ROUTES.items():
        assert any(reached(r) for r in old), name
    for name, reached in ROUTES.items():                                      # the reason PATH_CASES exists: CASES alone reaches none of them
        assert not any(reached(r) for r in old) and any(reached(r) for r in new), name
    assert any(r["dx"] == "lin" and r["lin_dx_last_ktile"] > 0 for r in old)  # K = 18 at B = 1: one batch tile
    # the forward's fall-back: a linear layer whose bases are not 16-byte aligned takes the generic kernel, with the layout its Cout gives
    for case in ((64, 3, 3, 64, 3, 3, 1, 5), (64, 1, 1, 32, 1, 1, 1, 33)):
        a, u = ref.route(case), ref.route(case, aligned=False)
        assert a["fwd"] == "lin" and a["fwd_cl"] is None and u["fwd"] == "generic" and u["fwd_cl"] == (1 if case[3] == 64 else 0)
        assert u["fwd_chunks"] == [32] * (a["K"] // 32) and u["dx"] == a["dx"] == "lin"
    # the table against the issue's figures for each case
    r = dict(zip(ref.PATH_CASES, new))
    c = r[(32, 8, 8, 128, 4, 4, 2, 3)]
    assert (c["K"], c["M"], c["fwd_cl"], c["fwd_cblocks"], c["fwd_last_cblock_partial"]) == (512, 27, 2, 1, False)
    c = r[(5, 9, 9, 160, 4, 4, 1, 15)]
    assert (c["fwd_chunks"], c["k_mod_64"], c["M"], c["P"], c["n_cblocks"], c["n_kblocks"], c["walks"]) == ([32, 32, 16], "1..32", 540, 3, 3, 2, [3])
    c = r[(40, 6, 6, 32, 3, 3, 1, 5)]
    assert (c["K"], c["fwd_chunks"][-1], c["k_mod_64"], c["fwd_cl"], c["dx_cl"]) == (360, 8, "33..63", 0, 1)
    c = r[(2, 17, 18, 32, 16, 16, 1, 2)]
    assert (c["K"], c["dx_max_ky_div"], c["dx_max_ky_mod"]) == (512, 15, 0)
    c = r[(2, 23, 21, 64, 7, 6, 4, 3)]
    assert (c["K"], c["fwd_chunks"], c["dx_max_ky_div"], c["dx_max_ky_mod"]) == (84, [32, 32, 20], 1, 3)
    assert int(ref.unread((2, 23, 21, 64, 7, 6, 4, 3)).sum()) == 69           # three unread input columns
    c = r[(6, 3, 3, 32, 3, 3, 1, 33)]
    assert (c["K"], c["fwd"], c["dx"], c["lin_dx_last_ktile"], c["batch_tiles"]) == (54, "generic", "lin", 22, 2)
    c = r[(2, 5, 5, 32, 2, 2, 1, 8)]
    assert c["M"] == 128 and c["walks"] == [2]
    c = ref.route(ref.CAP_CASE)
    assert c["cap_bound"] and c["P"] == 4 and c["walks"] == [5, 4]
    # the launchers themselves say what route restates (the source is the specification of these decisions)
    src = open(os.path.join(ROOT, "tactile_gym_amd", "csrc", "tg_conv.hip")).read()
    for text in ("conv_is_linear(a) && a.K % 32 == 0 && ((uintptr_t)x_dev | (uintptr_t)weight_dev) % 16 == 0",
                 "const int32_t cl = Cout >= 128 ? 2 : (Cout >= 64 ? 1 : 0), MP = (4 >> cl) * 32, CW = 32 << cl;",
                 "const int32_t n_kblocks = (a.K + 63) / 64, n_cblocks = (Cout + 63) / 64;",
                 "const int32_t cl = Cin > 32 ? 1 : 0, NP = (4 >> cl) * 32;",
                 "static bool conv_is_linear(const ConvArgs& a) { return a.H == a.KH && a.W == a.KW; }"):
        assert text in src, text


def test_order_probe_arithmetic():
    o = ref.probe_orders()
    assert o["ascending"] == 0 and o["reversed"] == 1 and o["pairwise"] == 1 and o["split"] == 1
    assert all(v.dtype == f32 for v in o.values())
    for shape, triples in ref.forward_probe_sets() + ref.path_forward_probe_sets():
        Cin, H, W, Cout, KH, KW, stride = shape
        K, khw = Cin * KH * KW, KH * KW
        assert all(0 <= a < b < c < K for a, b, c in triples)
        assert any(a % 2 == 0 and b == a + 1 for a, b, c in triples) and any(a % 2 == 1 and b == a + 1 for a, b, c in triples)   # in and across a pair
        assert any(a // khw != c // khw for a, b, c in triples) and any(a // khw == c // khw for a, b, c in triples)           # channel boundary
        if K > 32:
            assert any(a // 32 != b // 32 for a, b, c in triples) and any(b // 32 != c // 32 for a, b, c in triples)           # staging chunks
        x, w, b, at = ref.forward_probe(shape, triples)
        want, _ = ref.forward(x, w, b, stride)                               # exact arithmetic: every probed element is 2^24 + 1 - 2^24 = 1
        for i, (oy, ox) in enumerate(at):
            assert want[i, i % Cout, oy, ox] == 1.0
    for shape, at in ref.dx_probe_sets() + ref.path_dx_probe_sets():
        Cin, H, W, Cout, KH, KW, stride = shape
        x, w, y, dy, B = ref.dx_probe(shape, at)
        want = ref.backward(x, w, y, dy, stride)["dx"]
        assert B >= 60
        for i in range(B):
            assert want[i, i % Cin, at[0], at[1]] == 1.0
    assert len(ref.dx_terms((4, 6, 6, 32, 3, 3, 1), 2, 2)) == 288 and len(ref.dx_terms((32, 8, 8, 64, 4, 4, 2), 2, 2)) == 256
    # the new chains: every window of three consecutive k of K = 80 and 360; 256 terms at stride 4, each alone in its MFMA (no two terms are
    # neighbours in j), and 192 of the 16 x 16 kernel, all with ky / stride of 14 or 15
    assert [len(t) for _, t in ref.path_forward_probe_sets()] == [78, 358]
    for (shape, at), n in zip(ref.path_dx_probe_sets(), (256, 192)):
        terms = ref.dx_terms(shape, *at)
        assert len(terms) == n and len(ref.dx_probe(shape, at)[0]) == n - 2
    (s4, at4), (k16, at16) = ref.path_dx_probe_sets()
    terms = ref.dx_terms(s4, *at4)
    assert all(b[0] - a[0] >= 2 for a, b in zip(terms, terms[1:])) and {t[4] % 4 for t in terms} == {0} and {t[4] for t in terms} == {0, 4}
    assert {t[4] for t in ref.dx_terms(k16, *at16)} == {14, 15}
    assert len(ref.dx_terms((64, 3, 3, 64, 3, 3, 1), 1, 2)) == 64 and ref.dx_terms((4, 10, 13, 96, 3, 2, 3), 9, 0) == []


def test_abi_declarations_and_build_line():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    macros = (("TG_CONV_MAX_CIN", 64), ("TG_CONV_COUT_STEP", 32), ("TG_CONV_MAX_COUT", 512), ("TG_CONV_MAX_KERNEL", 16), ("TG_CONV_MAX_STRIDE", 4),
              ("TG_CONV_MAX_POSITIONS", 2 ** 29 - 32))
    for name, value in macros:
        assert re.search(r"#define %s %d\b" % (name, value), header)
        assert getattr(_capi, name[3:]) == value
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16      # functions added, no struct changed
    for name, n_args in (("tg_conv_relu", 13), ("tg_conv_relu_bwd_workspace", 8), ("tg_conv_relu_bwd", 18)):
        decl = re.search(r"\b(?:int|int64_t) %s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
    L = _capi.lib()
    assert all(hasattr(L, n) for n in ("tg_conv_relu", "tg_conv_relu_bwd_workspace", "tg_conv_relu_bwd"))
    build_units.assert_exact_product_unit("tg_conv")
    # the workspace query needs no device: the error's code and a text naming the limit
    ok = dict(B=1, Cin=32, H=8, W=8, Cout=64, KH=4, KW=4, stride=2)
    assert L.tg_conv_relu_bwd_workspace(*ok.values()) == 4 * (64 * 512 + 4 * 64)
    for change, word in ((dict(Cin=0), "Cin"), (dict(Cin=65), "Cin"), (dict(Cout=48), "Cout"), (dict(Cout=0), "Cout"), (dict(Cout=544), "Cout"),
                         (dict(KH=0), "KH"), (dict(KW=9), "KW <= W"), (dict(KH=17, H=20), "KH"), (dict(stride=0), "stride"), (dict(stride=5), "stride"),
                         (dict(Cin=1, KH=3, KW=3), "even"), (dict(B=-1), "B >= 0"), (dict(B=2 ** 29 // 64), "positions")):
        assert L.tg_conv_relu_bwd_workspace(*dict(ok, **change).values()) < 0, change
        text = L.tg_last_error().decode()
        assert text.startswith("tg_conv_relu_bwd_workspace:") and word in text, (change, text)


def test_checks_raise():
    import tactile_gym_amd as tg
    x, w, b = torch.zeros(2, 32, 8, 8), torch.zeros(64, 32, 4, 4), torch.zeros(64)
    assert tg.conv_relu(x, w, b, 2).shape == (2, 64, 3, 3)
    with pytest.raises(TypeError):
        tg.conv_relu(x.double(), w, b, 2)
    with pytest.raises(TypeError):
        tg.conv_relu(x.numpy(), w, b, 2)
    with pytest.raises(TypeError, match="weight"):
        tg.conv_relu(x, w.double(), b, 2)
    with pytest.raises(ValueError, match="contiguous"):
        tg.conv_relu(torch.zeros(2, 8, 8, 32).permute(0, 3, 1, 2), w, b, 2)
    with pytest.raises(ValueError):
        tg.conv_relu(x[0], w, b, 2)
    with pytest.raises(ValueError, match="weight"):
        tg.conv_relu(x, torch.zeros(64, 31, 4, 4), b, 2)
    with pytest.raises(ValueError, match="bias"):
        tg.conv_relu(x, w, torch.zeros(63), 2)
    with pytest.raises(ValueError, match="odd"):
        tg.conv_relu(torch.zeros(1, 1, 8, 8), torch.zeros(32, 1, 3, 3), torch.zeros(32), 1)
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.conv_relu(x, torch.zeros(48, 32, 4, 4), torch.zeros(48), 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.conv_relu(x, torch.zeros(544, 32, 4, 4), torch.zeros(544), 2)
    with pytest.raises(ValueError, match="channels"):
        tg.conv_relu(torch.zeros(1, 65, 8, 8), torch.zeros(32, 65, 2, 2), torch.zeros(32), 1)
    with pytest.raises(ValueError, match="kernel"):
        tg.conv_relu(x, torch.zeros(64, 32, 9, 4), b, 1)
    with pytest.raises(ValueError, match="stride"):
        tg.conv_relu(x, w, b, 5)
    with pytest.raises(ValueError, match="stride"):
        tg.conv_relu(x, w, b, 0)
    with pytest.raises(ValueError, match="weight"):
        tg.linear_relu(torch.zeros(3, 64, 2, 2), torch.zeros(32, 255), torch.zeros(32))
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.linear_relu(torch.zeros(3, 64), torch.zeros(500, 64), torch.zeros(500))
    with pytest.raises(ValueError):
        tg.linear_relu(torch.zeros(3, 4, 4, 4, 4), torch.zeros(32, 256), torch.zeros(32))
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.ConvRelu(32, 48, 4, 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.LinearRelu(1024, 500)
    with pytest.raises(ValueError, match="multiple of 32"):
        tg.NatureCNN(_Space((1, 64, 64)), features_dim=500, device_tail=True)
    with pytest.raises(ValueError, match="512"):
        tg.NatureCNN(_Space((1, 64, 64)), features_dim=544, device_tail=True)
    assert tg.NatureCNN(_Space((1, 64, 64)), features_dim=500).features_dim == 500       # the torch tail has no such limit


def test_cpu_path_equals_torch():
    import tactile_gym_amd as tg
    from tactile_gym_amd import torch_layers
    for name in ("conv_relu", "linear_relu", "ConvRelu", "LinearRelu"):
        assert getattr(tg, name) is getattr(torch_layers, name) and name in torch_layers.__all__
    rng = np.random.default_rng(3)
    for case in ref.CASES[:8] + [ref.CASES[15]]:
        Cin, H, W, Cout, KH, KW, stride, B = case
        x, w, b, _, _ = ref.random_case(rng, case)
        xt, wt, bt = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w).requires_grad_(), torch.from_numpy(b).requires_grad_()
        y = tg.conv_relu(xt, wt, bt, stride)
        assert torch.equal(y, F.relu(F.conv2d(xt, wt, bt, stride=stride)))
        y.sum().backward()                                                    # the CPU path is differentiable through torch
        assert xt.grad is not None and wt.grad is not None and bt.grad is not None
    x, w, b = torch.randn(5, 64, 2, 3), torch.randn(32, 384), torch.randn(32)
    want = F.relu(F.linear(x.flatten(1), w, b))
    assert torch.equal(tg.linear_relu(x, w, b), want) and torch.equal(tg.linear_relu(x.flatten(1), w, b), want)
    conv, lin = tg.ConvRelu(32, 64, 4, 2), tg.LinearRelu(384, 32)
    plain_c, plain_l = nn.Conv2d(32, 64, 4, 2), nn.Linear(384, 32)
    assert [(k, tuple(v.shape)) for k, v in conv.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain_c.state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in lin.state_dict().items()] == [(k, tuple(v.shape)) for k, v in plain_l.state_dict().items()]
    plain_c.load_state_dict(conv.state_dict())
    plain_l.load_state_dict(lin.state_dict())
    xc = torch.randn(2, 32, 8, 8)
    assert torch.equal(conv(xc), F.relu(plain_c(xc))) and torch.equal(lin(x), F.relu(plain_l(x.flatten(1))))
    # nn.Conv2d's and nn.Linear's initialisation: uniform within 1 / sqrt(fan_in)
    assert float(conv.weight.detach().abs().max()) <= 1 / np.sqrt(512) and float(conv.bias.detach().abs().max()) <= 1 / np.sqrt(512)
    assert float(lin.weight.detach().abs().max()) <= 1 / np.sqrt(384) and float(lin.weight.detach().abs().max()) > 0.9 / np.sqrt(384)


@pytest.mark.parametrize("channels_first", [True, False])
def test_nature_cnn_device_tail_keys_checkpoints_and_cpu_features(channels_first):
    import tactile_gym_amd as tg
    torch.manual_seed(4)
    shape = (2, 64, 64) if channels_first else (64, 64, 2)
    tail = tg.NatureCNN(_Space(shape), features_dim=32, channels_first=channels_first, device_tail=True)
    plain = tg.NatureCNN(_Space(shape), features_dim=32, channels_first=channels_first, device_tail=False)
    assert list(tail.state_dict()) == SB3_KEYS == list(plain.state_dict())
    assert [tuple(v.shape) for v in tail.state_dict().values()] == [tuple(v.shape) for v in plain.state_dict().values()]
    assert isinstance(tail.cnn[2], tg.ConvRelu) and isinstance(tail.cnn[4], tg.ConvRelu) and isinstance(tail.linear[0], tg.LinearRelu)
    assert all(isinstance(tail.cnn[i], nn.Identity) for i in (1, 3, 5)) and isinstance(tail.cnn[6], nn.Flatten)
    assert isinstance(tail.linear[1], nn.Identity) and len(tail.cnn) == 7 and len(tail.linear) == 2
    assert tail.features_dim == 32 and tail.n_flatten == plain.n_flatten == 1024
    x = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (3,) + shape, dtype=np.uint8))
    with torch.no_grad():
        assert not torch.allclose(tail(x), plain(x))                          # two initialisations
        plain.load_state_dict(tail.state_dict(), strict=True)
        assert torch.allclose(tail(x), plain(x), rtol=1e-5, atol=1e-6)
        assert torch.allclose(tail.linear(tail.cnn(x)), tail(x), rtol=1e-5, atol=1e-6)       # the Sequentials say the same as forward
        torch.manual_seed(6)
        other = tg.NatureCNN(_Space(shape), features_dim=32, channels_first=channels_first)
        tail.load_state_dict(other.state_dict(), strict=True)                 # and back
        assert torch.allclose(tail(x), other(x), rtol=1e-5, atol=1e-6)
    tail(x).sum().backward()
    assert all(p.grad is not None for p in tail.parameters())


def test_nature_cnn_without_the_argument_is_the_torch_tail():
    import tactile_gym_amd as tg
    m = tg.NatureCNN(_Space((1, 64, 64)), features_dim=48)
    assert type(m.cnn[2]) is nn.Conv2d and type(m.cnn[4]) is nn.Conv2d and type(m.linear[0]) is nn.Linear
    assert type(m.cnn[3]) is nn.ReLU and type(m.cnn[5]) is nn.ReLU and type(m.linear[1]) is nn.ReLU and m.device_tail is False


def test_conv_tail_kernels_use_no_scratch(tmp_path):
    from test_conv_stem_cpu import LIB, _kernel_scratch
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = {k: v for k, v in _kernel_scratch(tmp_path).items() if "k_conv_" in k and "k_conv_stem" not in k}
    assert len(scratch) == 6, sorted(scratch)        # forward, partials, reduction, dx, and the linear layer's forward and dx
    assert all(v == 0 for v in scratch.values()), scratch
