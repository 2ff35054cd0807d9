"""tactile_gym_amd.augment without a GPU: the two references of tests/augment_ref.py against each other, the draws' statistics, the kornia-style
constructor's argument rules, the CPU refusal, the C ABI entry, the kernel's resources and the one C call of the device buffers' fused gather."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from augment_ref import draw_params, split_shift, tolerance, uniforms, warp_f32, warp_kornia  # noqa: E402

from tactile_gym_amd import _capi  # noqa: E402

SIZES = [(64, 64), (128, 128), (256, 256), (48, 80)]


def _batch(rng, B, C, H, W, dtype, channels_first):
    shape = (B, C, H, W) if channels_first else (B, H, W, C)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    return rng.random(shape, dtype=np.float32)


@pytest.mark.parametrize("channels_first", [True, False])
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_restatement_matches_kornia_path(hw, channels_first, dtype):
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W + (7 if channels_first else 0))
    B, C = 6, 2
    x = _batch(rng, B, C, H, W, dtype, channels_first)
    params = draw_params(seed=11, counter=3, B=B, translate=(0.05, 0.05), p=1.0, H=H, W=W)
    params[1, 0] = 0.0                                        # one sample passed through
    got = warp_f32(x, params, channels_first)
    ref = warp_kornia(x, params, channels_first)
    assert got.dtype == np.float32 and got.shape == x.shape
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= tolerance(x), (err, tolerance(x))
    assert np.array_equal(got[1], x[1].astype(np.float32))     # bit for bit: not a resampled copy


def test_tolerance_is_not_vacuous():
    """The kornia path moves the image: a warped sample differs from the input by far more than the tolerance."""
    rng = np.random.default_rng(1)
    x = _batch(rng, 1, 1, 64, 64, np.uint8, True)
    params = np.array([[1.0, 2.5, -1.25]], dtype=np.float32)
    assert np.abs(warp_kornia(x, params) - x).max() > 10.0


@pytest.mark.parametrize("channels_first", [True, False])
def test_integer_shift_is_an_exact_copy(channels_first):
    """W = H = 64: tx = k 63 / 64 is exact in float32 and gives sx = k exactly (tx W / (W - 1)): the output is the shifted input with zeros."""
    rng = np.random.default_rng(2)
    x = _batch(rng, 4, 3, 64, 64, np.uint8, channels_first)
    ks = [(1, 0), (-3, 2), (0, -5), (7, 7)]
    params = np.array([[1.0, kx * 63 / 64, ky * 63 / 64] for kx, ky in ks], dtype=np.float32)
    got = warp_f32(x, params, channels_first)
    xc = x if channels_first else x.transpose(0, 3, 1, 2)
    gc = got if channels_first else got.transpose(0, 3, 1, 2)
    for b, (kx, ky) in enumerate(ks):
        assert split_shift(params[b, 1], 64) == (-kx, np.float32(0)) and split_shift(params[b, 2], 64) == (-ky, np.float32(0))
        exp = np.zeros((3, 64, 64), np.float32)
        exp[:, max(0, ky):64 + min(0, ky), max(0, kx):64 + min(0, kx)] = xc[b, :, max(0, -ky):64 - max(0, ky), max(0, -kx):64 - max(0, kx)]
        assert np.array_equal(gc[b], exp), b
    err = np.abs(got - warp_kornia(x, params, channels_first)).max()
    assert err <= 1e-3


@pytest.mark.parametrize("shift", [(64.0, 0.0), (0.0, -64.0), (-100.0, 3.0), (1e30, 0.0), (0.0, float("nan"))])
def test_shift_past_the_image_gives_zeros(shift):
    """A shift of at least W (or H) pixels - and anything non-finite - leaves every tap outside the image."""
    rng = np.random.default_rng(3)
    x = _batch(rng, 1, 2, 64, 64, np.float32, True) + 1.0
    got = warp_f32(x, np.array([[1.0, shift[0], shift[1]]], dtype=np.float32))
    assert not got.any()


def test_draw_statistics():
    n, p = 1_000_000, 0.5
    H = W = 128
    prm = draw_params(seed=5, counter=9, B=n, translate=(0.05, 0.05), p=p, H=H, W=W)
    rate = prm[:, 0].mean()
    assert abs(rate - p) < 5 * np.sqrt(p * (1 - p) / n), rate                 # binomial, 5 sigma
    lim = np.float32(0.05 * W)
    for col in (1, 2):
        t = prm[:, col]
        assert t.min() >= -lim and t.max() < lim
        hist, _ = np.histogram(t, bins=20, range=(-float(lim), float(lim)))
        expect = n / 20
        assert np.abs(hist - expect).max() < 6 * np.sqrt(expect), hist        # flat
    u = uniforms(5, 9, 3 * n).astype(np.float64)
    for lag in (1, 3):                                                         # consecutive elements, consecutive samples
        r = np.corrcoef(u[:-lag], u[lag:])[0, 1]
        assert abs(r) < 5 / np.sqrt(len(u)), (lag, r)
    a, b = uniforms(5, 9, 1000), uniforms(5, 10, 1000)
    assert not np.array_equal(a, b) and abs(np.corrcoef(a, b)[0, 1]) < 0.2   # the next counter is another draw
    p0 = draw_params(5, 9, 1000, (0.05, 0.05), 0.0, H, W)
    p1 = draw_params(5, 9, 1000, (0.05, 0.05), 1.0, H, W)
    assert not p0[:, 0].any() and p1[:, 0].all()


def test_random_affine_arguments():
    torch = pytest.importorskip("torch")
    import tactile_gym_amd.augment as K
    aug = torch.nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5))   # the reference's exact line
    m = aug[0]
    assert isinstance(m, K.RandomTranslate) and m.translate == (0.05, 0.05) and m.p == 0.5 and m.counter == 0
    assert isinstance(K.RandomAffine(degrees=(0, 0), translate=(0.1, 0.2)), K.RandomTranslate)
    assert K.RandomAffine(0, translate=[0.05, 0.05], seed=3).seed == 3
    torch.manual_seed(0)
    s0 = K.RandomAffine(0, translate=[0.05, 0.05]).seed
    torch.manual_seed(0)
    assert K.RandomAffine(0, translate=[0.05, 0.05]).seed == s0
    bad = [(dict(degrees=10), "degrees"), (dict(degrees=(-5, 5)), "degrees"), (dict(degrees=0, scale=(0.9, 1.1)), "scale"),
           (dict(degrees=0, shear=5), "shear"), (dict(degrees=0, same_on_batch=True), "same_on_batch"),
           (dict(degrees=0, align_corners=True), "align_corners"), (dict(degrees=0, padding_mode="border"), "padding_mode"),
           (dict(degrees=0, resample="nearest"), "resample")]
    for kw, name in bad:
        with pytest.raises(NotImplementedError, match=name):
            K.RandomAffine(translate=[0.05, 0.05], **kw)
    with pytest.raises(ValueError):
        K.RandomAffine(0, translate=[1.5, 0.0])
    with pytest.raises(ValueError):
        K.RandomAffine(0, translate=[0.05, 0.05], p=2.0)


def test_cpu_and_bad_tensors_raise():
    torch = pytest.importorskip("torch")
    import tactile_gym_amd as tg
    K = tg.augment
    with pytest.raises(ValueError, match="device"):
        K.random_translate(torch.zeros((2, 1, 16, 16), dtype=torch.uint8))
    with pytest.raises(ValueError, match="device"):
        K.RandomAffine(0, translate=[0.05, 0.05])(torch.zeros((2, 1, 16, 16)))
    with pytest.raises(TypeError):
        K.random_translate(torch.zeros((2, 1, 16, 16), dtype=torch.float64))
    with pytest.raises(TypeError):
        K.random_translate(np.zeros((2, 1, 16, 16), np.float32))


def test_c_abi_entry_is_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "tactile_gym_hip.h")).read()
    assert re.search(r"\bint tg_random_translate\s*\(", header)
    assert "tg_random_translate" in _capi.SYMBOLS
    assert re.search(r"#define TG_ABI_VERSION 16\b", header) and _capi.ABI_VERSION == 16
    assert re.search(r"#define TG_AUGMENT_UINT8 0\b", header) and re.search(r"#define TG_AUGMENT_FLOAT32 1\b", header)
    assert _capi.AUGMENT_DTYPE == {"uint8": 0, "float32": 1}
    assert len(_capi.SYMBOLS["tg_random_translate"][1]) == 16
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("library not built")
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tg_random_translate\b", nm)


def test_random_translate_kernels_use_no_scratch(tmp_path):
    """Every instantiation of k_random_translate (uint8 / float32 input, channels first / last) keeps its registers: no scratch memory."""
    from test_kstep_quad_resources_cpu import LIB, _kernel_scratch
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    ks = {k: v for k, v in _kernel_scratch(tmp_path).items() if "k_random_translate" in k}
    assert len(ks) == 4, sorted(ks)
    assert all(v == 0 for v in ks.values()), ks


@pytest.mark.parametrize("channels_first", [True, False])
def test_fused_gather_entry_issues_the_one_call(monkeypatch, channels_first):
    """augment._gather_images, the image-key branch of DeviceRolloutBuffer._gather and DeviceReplayBuffer.sample: for no module, a RandomTranslate
    and a RandomWarp it issues exactly one C call with the arguments those branches laid out by hand, moves the module's counter on by one and
    sets `_params` under kornia's names.  The library is replaced by a recorder, so CPU tensors do (the stream is an argument)."""
    torch = pytest.importorskip("torch")
    import ctypes
    import tactile_gym_amd.augment as K

    calls = []

    class Recorder:
        def __getattr__(self, name):
            def entry(*args):
                calls.append((name, tuple(a.value if isinstance(a, (ctypes.c_void_p, ctypes.c_uint64)) else a for a in args)))
                return 0
            return entry

    monkeypatch.setattr(_capi, "lib", lambda: Recorder())
    B, c, h, w, stream, M64 = 3, 2, 4, 4, 0x1234, 2**64 - 1
    sample = (c, h, w) if channels_first else (h, w, c)
    src = torch.zeros((5,) + sample, dtype=torch.uint8)
    out = torch.empty((B,) + sample, dtype=torch.float32)
    rows = torch.tensor([4, 0, 2], dtype=torch.int64)
    head = (src.data_ptr(), out.data_ptr(), _capi.AUGMENT_DTYPE["uint8"], int(channels_first), B, c, h, w)

    K._gather_images(None, src, out, rows, B, c, h, w, channels_first, stream)       # the plain uint8 -> float32 gather: a translate with p = 0
    assert calls == [("tg_random_translate_rows", head + (0.0, 0.0, 0.0, 0, 0, None, None, rows.data_ptr(), stream))]

    del calls[:]
    t = K.RandomTranslate(translate=(0.05, 0.1), p=0.25, seed=2**64 + 5)
    t.counter = 7
    K._gather_images(t, src, out, rows, B, c, h, w, channels_first, stream)
    assert t.counter == 8 and set(t._params) == {"batch_prob", "translations"}
    assert t._params["batch_prob"].shape == (B,) and t._params["batch_prob"].dtype == torch.bool and t._params["translations"].shape == (B, 2)
    prm = t._params["translations"].data_ptr() - 4                                    # translations = prm[:, 1:3] of the [B, 3] the call wrote
    assert calls == [("tg_random_translate_rows", head + (0.05, 0.1, 0.25, (2**64 + 5) & M64, 7, None, prm, rows.data_ptr(), stream))]

    del calls[:]
    wp = K.RandomWarp(degrees=10, translate=(0.1, 0.2), scale=(0.9, 1.1), shear=5, p=0.5, seed=-1)
    wp.counter = 2**64 + 3
    K._gather_images(wp, src, out, rows, B, c, h, w, channels_first, stream)
    assert wp.counter == 2**64 + 4 and set(wp._params) == {"batch_prob", "translations", "center", "scale", "angle", "sx", "sy"}
    assert wp._params["translations"].shape == (B, 2) and wp._params["scale"].shape == (B, 2) and wp._params["angle"].shape == (B,)
    assert wp._coeffs.shape == (B, 6) and wp._coeffs.dtype == torch.float32
    prm = wp._params["translations"].data_ptr() - 4
    assert calls == [("tg_random_affine_rows", head + (0.1, 0.2, -10.0, 10.0, 0.9, 1.1, 0.0, 0.0, -5.0, 5.0, 0.0, 0.0, 0.5, M64, 3, None, prm, None,
                                                       wp._coeffs.data_ptr(), rows.data_ptr(), stream))]
