"""The device conv stem without a GPU: the float64 restatement (tests/conv_stem_ref.py) against torch's own float64 conv2d and autograd on every
shape the GPU tests use, tactile_gym_amd.torch_layers' modules on their CPU path against the plain nn.Sequential they stand for, the checks
that raise, the ABI's declarations, and the kernels' scratch size read from the built library."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import build_units  # noqa: E402
import conv_stem_ref as ref  # noqa: E402

torch = pytest.importorskip("torch")
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

BOUND_ENTRY = _capi.SYMBOLS["tg_conv_stem"]                  # at import: the whole file needs the feature
LIB = os.path.join(ROOT, "tactile_gym_amd", "lib", "libtactile_gym_hip.so")
LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
SB3_KEYS = ["cnn.0.weight", "cnn.0.bias", "cnn.2.weight", "cnn.2.bias", "cnn.4.weight", "cnn.4.bias", "linear.0.weight", "linear.0.bias"]
f32 = np.float32


class _Space:
    def __init__(self, shape):
        self.shape, self.dtype = tuple(shape), np.uint8


def _id(case):
    H, W, Cn, B, cf, fl = case
    return f"{H}x{W}-c{Cn}-b{B}-{'chw' if cf else 'hwc'}-{'f32' if fl else 'u8'}"


def _nchw64(x, channels_first):
    t = torch.from_numpy(np.asarray(x).astype(np.float64))
    return t if channels_first else t.permute(0, 3, 1, 2)


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1e-300)


@pytest.mark.parametrize("case", ref.FWD_CASES, ids=_id)
def test_reference_forward_equals_torch_float64(case):
    H, W, Cn, B, cf, fl = case
    rng = np.random.default_rng(1)
    for maker in (ref.grid_forward_case, ref.random_forward_case):
        x, w, b, scale = maker(rng, B, Cn, H, W, cf, fl)
        want = F.relu(F.conv2d(_nchw64(x, cf) * float(scale), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=4))
        got, bound = ref.forward(x, w, b, scale, cf)
        assert got.shape == (B, 32) + ref.out_hw(H, W) and bound.shape == got.shape and (bound >= 0).all()
        _close(got, want.numpy())
    x, w, b, scale = ref.grid_forward_case(rng, B, Cn, H, W, cf, fl)
    got, _ = ref.forward(x, w, b, scale, cf)
    assert np.array_equal(got.astype(f32).astype(np.float64), got)       # a grid case's result is a float32 number


@pytest.mark.parametrize("case", ref.BWD_CASES, ids=_id)
def test_reference_backward_equals_torch_float64_autograd(case):
    H, W, Cn, B, cf, fl = case
    rng = np.random.default_rng(2)
    x, w, b, scale = ref.random_forward_case(rng, B, Cn, H, W, cf, fl)
    wt, bt = torch.from_numpy(w).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    y = F.relu(F.conv2d(_nchw64(x, cf) * float(scale), wt, bt, stride=4))
    dy = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(dy))
    dw, db, dw_bound, db_bound = ref.backward(x, y.detach().numpy(), dy, scale, cf)
    _close(dw, wt.grad.numpy())
    _close(db, bt.grad.numpy())
    assert dw_bound.shape == dw.shape and db_bound.shape == db.shape and (dw_bound >= 0).all()
    x, yg, dyg, scale = ref.grid_backward_case(rng, B, Cn, H, W, cf, fl, gmax=ref.gmax_of(case))
    dw, db, _, _ = ref.backward(x, yg, dyg, scale, cf)
    assert np.array_equal(dw.astype(f32).astype(np.float64), dw) and np.array_equal(db.astype(f32).astype(np.float64), db)
    assert (yg == 0).any() and (yg > 0).any()


def _plain(Cn, n_flatten, features_dim):
    """SB3's NatureCNN as it is written there."""
    cnn = nn.Sequential(nn.Conv2d(Cn, 32, kernel_size=8, stride=4, padding=0), nn.ReLU(), nn.Conv2d(32, 64, kernel_size=4, stride=2, padding=0),
                        nn.ReLU(), nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=0), nn.ReLU(), nn.Flatten())

    class Plain(nn.Module):
        def __init__(self):
            super().__init__()
            self.cnn, self.linear = cnn, nn.Sequential(nn.Linear(n_flatten, features_dim), nn.ReLU())

        def forward(self, x):
            return self.linear(self.cnn(x))
    return Plain()


@pytest.mark.parametrize("size,n_flatten", [(64, 1024), (128, 9216), (256, 50176)])
def test_state_dict_keys_and_n_flatten(size, n_flatten):
    import tactile_gym_amd as tg
    from tactile_gym_amd import torch_layers
    assert tg.torch_layers is torch_layers and tg.NatureCNN is torch_layers.NatureCNN and tg.ConvStem is torch_layers.ConvStem
    assert tg.conv_stem is torch_layers.conv_stem
    m = tg.NatureCNN(_Space((1, size, size)), features_dim=16)
    assert list(m.state_dict()) == SB3_KEYS and m.n_flatten == n_flatten and m.features_dim == 16
    assert tuple(m.state_dict()["cnn.0.weight"].shape) == (32, 1, 8, 8) and tuple(m.state_dict()["linear.0.weight"].shape) == (16, n_flatten)
    assert isinstance(m.cnn[1], nn.Identity) and m.cnn[0].channels_first
    assert tg.NatureCNN(_Space((size, size, 2))).cnn[0].channels_first is False          # SB3's rule: the smallest dimension is the channels


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_module_on_cpu_matches_the_plain_sequential(channels_first, dtype):
    import tactile_gym_amd as tg
    torch.manual_seed(3)
    Cn, H, W, B = 3, 40, 52, 3
    shape = (Cn, H, W) if channels_first else (H, W, Cn)
    m = tg.NatureCNN(_Space(shape), features_dim=32, channels_first=channels_first, float_scale=1.0 / 255.0)
    plain = _plain(Cn, m.n_flatten, 32)
    m.load_state_dict(plain.state_dict())                                 # a checkpoint of the plain module loads ...
    plain.load_state_dict(m.state_dict())                                 # ... and the other way round
    rng = np.random.default_rng(4)
    x8 = rng.integers(0, 256, (B,) + shape, dtype=np.uint8)
    x = torch.from_numpy(x8 if dtype == "uint8" else x8.astype(f32))      # float32 in 0 ... 255: this project's buffers, float_scale 1 / 255
    nchw = (x if channels_first else x.permute(0, 3, 1, 2)).float() / 255.0   # SB3's preprocess_obs
    with torch.no_grad():
        stem, stem_plain = m.cnn[0](x), plain.cnn[1](plain.cnn[0](nchw))
        want, bound = ref.forward(x8, m.cnn[0].weight.numpy(), m.cnn[0].bias.numpy(), ref.U8_SCALE, channels_first)
        for got in (stem, stem_plain):                                    # both float32 evaluations lie within the bound of the exact result
            assert (np.abs(got.numpy().astype(np.float64) - want) <= bound).all()
        feats, feats_plain = m(x), plain(nchw)
    assert feats.shape == (B, 32) and feats.dtype == torch.float32
    assert torch.allclose(feats, feats_plain, rtol=1e-5, atol=1e-6)
    loss = m(x).sum()                                                     # the CPU path is differentiable through torch
    loss.backward()
    assert m.cnn[0].weight.grad is not None and m.cnn[0].bias.grad is not None and m.cnn[0].weight.grad.abs().sum() > 0


def test_float_scale_rule():
    import tactile_gym_amd as tg
    torch.manual_seed(5)
    rng = np.random.default_rng(6)
    x8 = torch.from_numpy(rng.integers(0, 256, (2, 2, 36, 36), dtype=np.uint8))
    unit = tg.ConvStem(2)                                                 # float_scale = 1: float32 input that SB3 has divided already
    scaled = tg.ConvStem(2, float_scale=1.0 / 255.0)                      # float32 input in 0 ... 255
    scaled.load_state_dict(unit.state_dict())
    with torch.no_grad():
        from_u8 = unit(x8)
        assert torch.equal(scaled(x8), from_u8)                           # uint8 is scaled by 1 / 255 whatever float_scale says
        assert torch.equal(scaled(x8.float()), from_u8)
        assert torch.allclose(unit(x8.float() / 255.0), from_u8, rtol=1e-5, atol=1e-6)
        assert not torch.allclose(unit(x8.float()), from_u8)
        w, b = unit.weight, unit.bias
        assert torch.equal(tg.conv_stem(x8, w, b), from_u8) and torch.equal(tg.conv_stem(x8.float(), w, b, scale=1.0 / 255.0), from_u8)
        hwc = x8.permute(0, 2, 3, 1).contiguous()
        assert torch.equal(tg.conv_stem(hwc, w, b, channels_first=False), from_u8)


def test_checks_raise():
    import tactile_gym_amd as tg
    w, b = torch.zeros(32, 2, 8, 8), torch.zeros(32)
    x = torch.zeros(1, 2, 16, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="gradient"):
        tg.conv_stem(torch.zeros(1, 2, 16, 16, requires_grad=True), w, b)
    with pytest.raises(TypeError):
        tg.conv_stem(x.to(torch.int32), w, b)
    with pytest.raises(TypeError):
        tg.conv_stem(x.double(), w, b)
    with pytest.raises(TypeError):
        tg.conv_stem(x.numpy(), w, b)
    with pytest.raises(ValueError, match="4-D"):
        tg.conv_stem(x[0], w, b)
    with pytest.raises(ValueError, match="contiguous"):
        tg.conv_stem(torch.zeros(1, 16, 16, 2, dtype=torch.uint8).permute(0, 3, 1, 2), w, b)
    with pytest.raises(ValueError, match="H, W >= 8"):
        tg.conv_stem(torch.zeros(1, 2, 7, 16, dtype=torch.uint8), w, b)
    with pytest.raises(ValueError, match="weight"):
        tg.conv_stem(x, torch.zeros(32, 3, 8, 8), b)
    with pytest.raises(ValueError, match="16 channels"):
        tg.conv_stem(x, w, b, channels_first=False)                       # read as [B, H, W, C]
    with pytest.raises(ValueError, match="weight"):
        tg.conv_stem(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), w, b, channels_first=False)
    with pytest.raises(ValueError, match="bias"):
        tg.conv_stem(x, w, torch.zeros(31))
    with pytest.raises(TypeError, match="weight"):
        tg.conv_stem(x, w.double(), b)
    with pytest.raises(ValueError, match="channels"):
        tg.conv_stem(torch.zeros(1, 13, 16, 16, dtype=torch.uint8), torch.zeros(32, 13, 8, 8), b)
    with pytest.raises(ValueError):
        tg.ConvStem(13)
    with pytest.raises(ValueError, match="image space"):
        tg.NatureCNN(_Space((128, 128)))
    with pytest.raises(ValueError, match="H, W >= 36"):
        tg.NatureCNN(_Space((1, 35, 64)))
    with pytest.raises(ValueError, match="channels_first"):
        tg.NatureCNN(_Space((1, 64, 64)), channels_first="yes")


def test_abi_declarations_and_build_line():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    for name, value in (("TG_STEM_KERNEL", 8), ("TG_STEM_STRIDE", 4), ("TG_STEM_OUT", 32), ("TG_STEM_MAX_CIN", 12)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
    assert (_capi.STEM_KERNEL, _capi.STEM_STRIDE, _capi.STEM_OUT, _capi.STEM_MAX_CIN) == (8, 4, 32, 12)
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16      # functions added, no struct changed
    for name, n_args in (("tg_conv_stem", 12), ("tg_conv_stem_bwd_workspace", 4), ("tg_conv_stem_bwd", 15)):
        decl = re.search(r"\b(?:int|int64_t) %s\s*\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args == len(_capi.SYMBOLS[name][1]), name
    L = _capi.lib()
    assert all(hasattr(L, n) for n in ("tg_conv_stem", "tg_conv_stem_bwd_workspace", "tg_conv_stem_bwd"))
    build_units.assert_exact_product_unit("tg_conv_stem")
    # the workspace query needs no device: a size for valid shapes, the error's code otherwise
    assert L.tg_conv_stem_bwd_workspace(64, 1, 128, 128) > 0
    assert L.tg_conv_stem_bwd_workspace(1, 1, 8, 8) == 4 * (2 * 32 * 64 + 8 * 32)
    assert L.tg_conv_stem_bwd_workspace(1, 13, 8, 8) < 0 and L.tg_last_error().decode().startswith("tg_conv_stem_bwd_workspace:")


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def _kernel_scratch(tmp_path):
    """{kernel symbol: private segment bytes} over every gfx950 code object in the library (the method of test_kstep_quad_resources_cpu.py)."""
    objcopy, bundler, readelf = _tool("llvm-objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not (objcopy and bundler and readelf):
        pytest.skip("LLVM tools of the ROCm install not found")
    fatbin = tmp_path / "fatbin"
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fatbin}", LIB, str(tmp_path / "stripped")], check=True)
    data = fatbin.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for k, s in enumerate(starts):
        chunk = tmp_path / f"b{k}"
        chunk.write_bytes(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        co = tmp_path / f"b{k}.co"
        r = subprocess.run([bundler, "--unbundle", "--type=o", f"--input={chunk}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"],
                           capture_output=True)
        if r.returncode != 0 or not co.exists() or co.stat().st_size == 0:
            continue
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.", notes):
            name = re.search(r"\.name:\s+(\S+)", block)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            if name and scratch:
                out[name.group(1)] = int(scratch.group(1))
    return out


def test_conv_stem_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    scratch = _kernel_scratch(tmp_path)
    stem = {k: v for k, v in scratch.items() if "k_conv_stem" in k}
    assert len(stem) == 9, sorted(stem)              # forward and backward x {uint8, float32} x {channels first, last}, and the reduction
    assert all(v == 0 for v in stem.values()), stem


# ---------------------------------------------------------------------------------------------------------------------- the backward's walk
def _position_mask(case, keep_region):
    """bool [B, OH, OW]: the output positions of the regions keep_region(index, geometry) picks."""
    H, W, Cn, B, cf, fl = case
    g = ref.geometry(B, H, W)
    mask = np.zeros((B, g["OH"], g["OW"]), bool)
    for index in range(g["regions"]):
        if keep_region(index, g):
            b, oy0, ox0, rv, cv = ref.region(g, index)
            mask[b, oy0:oy0 + rv, ox0:ox0 + cv] = True
    return mask


def test_geometry_restates_stem_geom_and_the_backward_cases_reach_every_edge_of_the_walk():
    assert ref.geometry(1, 128, 128) == dict(OH=31, OW=31, Cw=31, n_chunks=1, R=4, n_strips=8, regions=8, G=8)       # DESIGN 4.14's example
    assert ref.geometry(129, 16, 176) == dict(OH=3, OW=43, Cw=43, n_chunks=1, R=2, n_strips=2, regions=258, G=256)
    assert ref.geometry(129, 8, 530) == dict(OH=1, OW=131, Cw=128, n_chunks=2, R=1, n_strips=1, regions=258, G=256)
    L = _capi.lib()
    reached = set()
    for case in ref.BWD_CASES:
        H, W, Cn, B, cf, fl = case
        g = ref.geometry(B, H, W)
        assert L.tg_conv_stem_bwd_workspace(B, Cn, H, W) == 4 * (g["G"] * 2 * 32 * 64 * Cn + g["G"] * 8 * 32)          # stem_workspace on this G
        regions = [ref.region(g, i) for i in range(g["regions"])]
        assert sum(rv * cv for _, _, _, rv, cv in regions) == B * g["OH"] * g["OW"] and max(rv * cv for _, _, _, rv, cv in regions) <= ref.POS
        assert _position_mask(case, lambda i, g: True).all()                  # the regions tile every image
        wrap = g["regions"] > g["G"]
        reached |= {name for name, hit in (
            ("regions > G", wrap), ("regions % G != 0", wrap and g["regions"] % g["G"] != 0),
            ("a workgroup with three regions", -(-g["regions"] // g["G"]) >= 3), ("n_chunks > 1", g["n_chunks"] > 1),
            ("n_strips > 1 with regions > G", g["n_strips"] > 1 and wrap), ("n_chunks > 1 with regions > G", g["n_chunks"] > 1 and wrap),
            ("a last chunk smaller than the others", g["OW"] % g["Cw"] != 0), ("a last strip smaller than the others", g["OH"] % g["R"] != 0),
            ("npos <= 64", min(rv * cv for _, _, _, rv, cv in regions) <= 64)) if hit}
    assert reached == {"regions > G", "regions % G != 0", "a workgroup with three regions", "n_chunks > 1", "n_strips > 1 with regions > G",
                       "n_chunks > 1 with regions > G", "a last chunk smaller than the others", "a last strip smaller than the others", "npos <= 64"}
    with pytest.raises(AssertionError):                                       # the exactness check does refuse what is not exact
        ref.grid_backward_case(np.random.default_rng(0), 129, 1, 16, 176, True, False, gmax=4)
    with pytest.raises(AssertionError):
        ref.grid_backward_case(np.random.default_rng(0), 6, 1, 128, 128, True, False, gmax=18)


def test_mutants_of_the_backward_walk_change_the_grid_cases_bits():
    """What k_conv_stem_bwd would return were it wrong at one edge of its walk over the regions: the sums are linear in g = dy (y > 0), so a
    lost region is a masked dy."""
    def bits(a):
        return np.asarray(a).astype(f32).view(np.uint32)

    seen = {"first": 0, "chunk": 0, "bias": 0}
    for case in ref.BWD_CASES:
        H, W, Cn, B, cf, fl = case
        g = ref.geometry(B, H, W)
        wrap, chunks = g["regions"] > g["G"], g["n_chunks"] > 1
        if not (wrap or chunks):
            continue
        rng = np.random.default_rng(hash(case) % 2**32)                       # the GPU test's draw
        x, y, dy, scale = ref.grid_backward_case(rng, B, Cn, H, W, cf, fl, gmax=ref.gmax_of(case))
        dw, db, _, _ = ref.backward(x, y, dy, scale, cf)

        def masked(keep):
            m = _position_mask(case, keep)
            assert not m.all()
            return ref.backward(x, y, dy * m[:, None], scale, cf)[:2]
        if wrap:
            dw1, db1 = masked(lambda i, g: i < g["G"])                        # only each workgroup's first region contributes
            assert (bits(dw1) != bits(dw)).any() and (bits(db1) != bits(db)).any(), case
            last = lambda i, g: i + g["G"] >= g["regions"]   # noqa: E731        the bias sum restarted at every region: the last one is left
            _, db3 = masked(last)
            assert (bits(db3) != bits(db)).any(), case
            seen["first"] += 1
            seen["bias"] += 1
        if chunks:
            dw2, db2 = masked(lambda i, g: i % g["n_chunks"] != 1)            # the second column chunk dropped
            assert (bits(dw2) != bits(dw)).any() and (bits(db2) != bits(db)).any(), case
            seen["chunk"] += 1
    assert seen == {"first": 4, "chunk": 2, "bias": 4}, seen
