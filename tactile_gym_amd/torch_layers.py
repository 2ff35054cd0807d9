"""stable_baselines3.common.torch_layers' NatureCNN with its first layer on the device conv stem (csrc/tg_conv_stem.hip: k_conv_stem,
k_conv_stem_bwd).

Every params file of the reference builds its policy with `CustomCombinedExtractor(cnn_base=NatureCNN)`; with `cnn_base=tg.NatureCNN` the
same line builds this module.  Its first stage - SB3's preprocess_obs (obs.float() / 255), Conv2d(C, 32, kernel_size=8, stride=4), ReLU - is
ONE launch that reads the uint8 image once and writes the activated float32 output once; everything after it stays on torch unless
`device_tail=True` puts the second and third convolution and the linear layer on csrc/tg_conv.hip too (conv_relu, linear_relu; DESIGN.md
4.21: one launch a layer, the same rule for the bits, gradients for input, weight and bias in a fixed summation order).  Each output
element is one float32 fmaf chain over k = (c 8 + ky) 8 + kx ascending, then fmaxf(fmaf(acc, scale, bias), 0): an image's features do not
depend on the batch it sits in, so PPO's first-epoch ratio exp(log_prob_new - log_prob_old) of a minibatch row is computed from the very bits
the collection batch produced.  The input is data and gets no gradient; the backward pass is dweight and dbias, summed in a fixed order
(the same bits on every run).

What reaches the module, and the scale that goes with it:

    uint8 images (collect.py's loops, buf.get(out_dtype=torch.uint8), rb.sample(...))   scale 1 / 255, always
    float32 in [0, 1] (SB3's own preprocess_obs has divided already)                    float_scale=1 (the default)
    float32 in 0 ... 255 (this project's buffers: get / sample with float32 output,     float_scale=1 / 255
                          the augmentation's output)

Device tensors run the HIP kernels on torch's current stream.  CPU tensors take a plain-torch path of the same meaning (F.conv2d on
x.float() * scale, then relu) that is not bit-specified: SB3 can save, load and evaluate the module on the host.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _capi as capi
from ._device import check_f32_like, check_images, launch, ptr, workspace
from .vec_env import _optional_base

__all__ = ["conv_stem", "ConvStem", "conv_relu", "linear_relu", "ConvRelu", "LinearRelu", "NatureCNN"]

_U8_SCALE = float(np.float32(1.0) / np.float32(255.0))      # 1 / 255f
_FeaturesBase = _optional_base("stable_baselines3.common.torch_layers", "BaseFeaturesExtractor")


def _check_stem(x, weight, bias, channels_first):
    """(Cn, H, W) of the batch x after _device.check_images' checks (a CPU tensor is allowed here), its own, and the parameters'."""
    check_images(x, allow_cpu=True)
    if x.requires_grad:
        raise ValueError("x requires a gradient: the conv stem treats its input as data and computes none")
    Cn, H, W = tuple(x.shape[1:]) if channels_first else (x.shape[3], x.shape[1], x.shape[2])
    if not 1 <= Cn <= capi.STEM_MAX_CIN:
        raise ValueError(f"x has {Cn} channels (channels_first={bool(channels_first)}): 1 to {capi.STEM_MAX_CIN} are built")
    if H < capi.STEM_KERNEL or W < capi.STEM_KERNEL:
        raise ValueError(f"x is {H} x {W}: the 8 x 8 kernel needs H, W >= 8")
    for t, name, shape in ((weight, "weight", (capi.STEM_OUT, Cn, capi.STEM_KERNEL, capi.STEM_KERNEL)), (bias, "bias", (capi.STEM_OUT,))):
        check_f32_like(t, name, shape, x)
    return Cn, H, W


def _out_hw(H, W):
    return (H - capi.STEM_KERNEL) // capi.STEM_STRIDE + 1, (W - capi.STEM_KERNEL) // capi.STEM_STRIDE + 1


class _ConvStem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, channels_first, scale):
        B = x.shape[0]
        Cn, H, W = tuple(x.shape[1:]) if channels_first else (x.shape[3], x.shape[1], x.shape[2])
        y = torch.empty((B, capi.STEM_OUT) + _out_hw(H, W), dtype=torch.float32, device=x.device)
        launch("tg_conv_stem", x.device, ptr(x), int(x.dtype == torch.float32), int(channels_first), B, Cn, H, W, ptr(weight.detach()),
               ptr(bias.detach()), scale, ptr(y))
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:          # under no_grad, or with frozen parameters, nothing is kept
            ctx.save_for_backward(x, y)
            ctx.stem = (bool(channels_first), scale, Cn, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        channels_first, scale, Cn, H, W = ctx.stem
        B = x.shape[0]
        dy = dy.contiguous()
        if dy.dtype != torch.float32:
            raise TypeError(f"the output's gradient must be float32, got {dy.dtype}")
        alloc = torch.empty if B else torch.zeros                         # B = 0 launches nothing: the gradients are zero
        dweight = alloc((capi.STEM_OUT, Cn, capi.STEM_KERNEL, capi.STEM_KERNEL), dtype=torch.float32, device=x.device)
        dbias = alloc((capi.STEM_OUT,), dtype=torch.float32, device=x.device)
        nbytes = workspace("tg_conv_stem_bwd_workspace", B, Cn, H, W)
        work = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        launch("tg_conv_stem_bwd", x.device, ptr(x), int(x.dtype == torch.float32), int(channels_first), B, Cn, H, W, ptr(y), ptr(dy), scale,
               ptr(dweight), ptr(dbias), ptr(work), nbytes)
        return None, dweight, dbias, None, None


def conv_stem(x, weight, bias, channels_first=True, scale=None):
    """relu(conv2d(x * scale, weight, bias, stride=4)) for the 8 x 8 kernel and 32 output channels of NatureCNN's first layer: float32
    [B, 32, (H - 8) // 4 + 1, (W - 8) // 4 + 1] from x, a contiguous uint8 or float32 batch [B, C, H, W] (channels_first) or [B, H, W, C].
    scale: None is 1 / 255 for uint8 and 1 for float32 (see the module's table).  Differentiable in weight and bias; x must not require a
    gradient.  On the device: one launch forward, two backward, on torch's current stream.  On the CPU: plain torch, not bit-specified."""
    Cn, H, W = _check_stem(x, weight, bias, channels_first)
    if scale is None:
        scale = _U8_SCALE if x.dtype == torch.uint8 else 1.0
    scale = float(np.float32(scale))
    if not x.is_cuda:
        xf = x.float() * scale
        return F.relu(F.conv2d(xf if channels_first else xf.permute(0, 3, 1, 2), weight, bias, stride=capi.STEM_STRIDE))
    return _ConvStem.apply(x, weight, bias, bool(channels_first), scale)


class ConvStem(nn.Module):
    """NatureCNN's Conv2d(n_input_channels, 32, kernel_size=8, stride=4) with SB3's preprocessing in front and the ReLU behind it, as
    `conv_stem`.  weight [32, C, 8, 8] and bias [32] are nn.Conv2d's parameters under nn.Conv2d's names and initialisation.  uint8 input is
    scaled by 1 / 255, float32 input by float_scale."""

    def __init__(self, n_input_channels, channels_first=True, float_scale=1.0):
        super().__init__()
        if not 1 <= int(n_input_channels) <= capi.STEM_MAX_CIN:
            raise ValueError(f"n_input_channels={n_input_channels}: 1 to {capi.STEM_MAX_CIN} are built")
        self.n_input_channels, self.channels_first, self.float_scale = int(n_input_channels), bool(channels_first), float(float_scale)
        conv = nn.Conv2d(self.n_input_channels, capi.STEM_OUT, kernel_size=capi.STEM_KERNEL, stride=capi.STEM_STRIDE)
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x):
        return conv_stem(x, self.weight, self.bias, self.channels_first, _U8_SCALE if x.dtype == torch.uint8 else self.float_scale)

    def extra_repr(self):
        return f"{self.n_input_channels}, 32, kernel_size=8, stride=4, channels_first={self.channels_first}, float_scale={self.float_scale}"


# ---------------------------------------------------------------------------------------------------------------- the device tail
def _check_conv(x, weight, bias, stride):
    """(Cin, H, W, Cout, KH, KW) of relu(conv2d(x, weight, bias, stride)) after the checks of the device tail (tg_conv_relu's limits)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError("x must be a float32 torch tensor")
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous [B, Cin, H, W] tensor, got shape {tuple(x.shape)}")
    if not isinstance(weight, torch.Tensor) or weight.dim() != 4:
        raise ValueError("weight must be a [Cout, Cin, KH, KW] tensor")
    Cin, H, W = (int(v) for v in x.shape[1:])
    Cout, _, KH, KW = (int(v) for v in weight.shape)
    check_f32_like(weight, "weight", (Cout, Cin, KH, KW), x)
    check_f32_like(bias, "bias", (Cout,), x)
    if not 1 <= Cin <= capi.CONV_MAX_CIN:
        raise ValueError(f"x has {Cin} channels: 1 to {capi.CONV_MAX_CIN} are built")
    if Cout % capi.CONV_COUT_STEP or not 0 < Cout <= capi.CONV_MAX_COUT:
        raise ValueError(f"weight has {Cout} output channels: a multiple of {capi.CONV_COUT_STEP} up to {capi.CONV_MAX_COUT} is built")
    if not (1 <= KH <= min(H, capi.CONV_MAX_KERNEL) and 1 <= KW <= min(W, capi.CONV_MAX_KERNEL)):
        raise ValueError(f"the kernel is {KH} x {KW} on a {H} x {W} input: 1 to {capi.CONV_MAX_KERNEL}, and no larger than the input")
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 1 <= stride <= capi.CONV_MAX_STRIDE:
        raise ValueError(f"stride={stride!r}: an integer from 1 to {capi.CONV_MAX_STRIDE}")
    if (Cin * KH * KW) % 2:
        raise ValueError(f"K = Cin KH KW = {Cin * KH * KW} is odd: the MFMA takes two k per instruction, an even K is built")
    return Cin, H, W, Cout, KH, KW


class _ConvRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        B, Cin, H, W = x.shape
        Cout, _, KH, KW = weight.shape
        y = torch.empty((B, Cout, (H - KH) // stride + 1, (W - KW) // stride + 1), dtype=torch.float32, device=x.device)
        launch("tg_conv_relu", x.device, ptr(x.detach()), B, Cin, H, W, ptr(weight.detach()), ptr(bias.detach()), Cout, KH, KW, stride, ptr(y))
        if any(ctx.needs_input_grad[:3]):                                 # under no_grad, or with everything frozen, nothing is kept
            ctx.save_for_backward(x, weight, y)
            ctx.stride = stride
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        stride = ctx.stride
        B, Cin, H, W = x.shape
        Cout, _, KH, KW = weight.shape
        dy = dy.contiguous()
        if dy.dtype != torch.float32:
            raise TypeError(f"the output's gradient must be float32, got {dy.dtype}")
        alloc = torch.empty if B else torch.zeros                         # B = 0 launches nothing: the gradients are zero
        dweight = alloc(tuple(weight.shape), dtype=torch.float32, device=x.device)
        dbias = alloc((Cout,), dtype=torch.float32, device=x.device)
        dx = alloc(tuple(x.shape), dtype=torch.float32, device=x.device) if ctx.needs_input_grad[0] else None   # None: no dx launch
        nbytes = workspace("tg_conv_relu_bwd_workspace", B, Cin, H, W, Cout, KH, KW, stride)
        work = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=x.device)
        launch("tg_conv_relu_bwd", x.device, ptr(x.detach()), B, Cin, H, W, ptr(weight.detach()), ptr(y), ptr(dy), Cout, KH, KW, stride, ptr(dweight),
               ptr(dbias), ptr(dx), ptr(work), nbytes)
        return dx, dweight, dbias, None


def conv_relu(x, weight, bias, stride=1):
    """relu(conv2d(x, weight, bias, stride)), unpadded: float32 [B, Cout, (H - KH) // stride + 1, (W - KW) // stride + 1] from a contiguous
    float32 x [B, Cin, H, W], weight [Cout, Cin, KH, KW] and bias [Cout].  Each output element is one float32 fmaf chain over
    k = (c KH + ky) KW + kx ascending, then + bias and relu (csrc/tg_conv.hip): its bits do not depend on the batch around it.  Built for
    Cin <= 64, Cout a multiple of 32 up to 512, kernels up to 16 x 16, strides up to 4 and an even Cin KH KW.  Differentiable in x (computed
    only when x requires it), weight and bias.  On the device: one launch forward, two or three backward, on torch's current stream.  On the
    CPU: plain torch, not bit-specified."""
    _check_conv(x, weight, bias, stride)
    if not x.is_cuda:
        return F.relu(F.conv2d(x, weight, bias, stride=int(stride)))
    return _ConvRelu.apply(x, weight, bias, int(stride))


def linear_relu(x, weight, bias):
    """relu(linear(flatten(x), weight, bias)): float32 [B, F] from x [B, C, h, w] (conv3's output: Flatten is part of the call) or [B, K],
    weight [F, K] and bias [F], with the arithmetic and limits of `conv_relu`: it IS the convolution of [B, C, h, w] with an h x w kernel
    (C <= 64, h, w <= 16; a [B, K] input is split the same way, K = C h w with the smallest such C)."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 4):
        raise ValueError("x must be a [B, C, h, w] or [B, K] tensor")
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError("weight must be a [F, K] tensor")
    B, K = int(x.shape[0]), int(np.prod(x.shape[1:]))
    if int(weight.shape[1]) != K:
        raise ValueError(f"weight must be [F, {K}] for x of shape {tuple(x.shape)}, got {tuple(weight.shape)}")
    if x.dim() == 4:
        C, h, w = (int(v) for v in x.shape[1:])
    else:
        C, h, w = _split_k(K)
    if not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("x and weight must be contiguous")
    n_out = int(weight.shape[0])
    x4, w4 = x.view(B, C, h, w), weight.view(n_out, C, h, w)
    _check_conv(x4, w4, bias, 1)
    if not x.is_cuda:
        return F.relu(F.linear(x.view(B, K), weight, bias))
    return _ConvRelu.apply(x4, w4, bias, 1).view(B, n_out)


def _split_k(K):
    """(C, h, w) with C h w = K inside the device tail's limits, the smallest C first; a ValueError where there is none."""
    for C in range(1, capi.CONV_MAX_CIN + 1):
        if K % C == 0:
            r = K // C
            for h in range(min(r, capi.CONV_MAX_KERNEL), 0, -1):
                if r % h == 0 and r // h <= capi.CONV_MAX_KERNEL:
                    return C, h, r // h
    raise ValueError(f"K = {K} is no product C h w with C <= {capi.CONV_MAX_CIN} and h, w <= {capi.CONV_MAX_KERNEL}")


class ConvRelu(nn.Module):
    """nn.Conv2d(cin, cout, kernel_size, stride) with the ReLU behind it, as `conv_relu`: weight [cout, cin, k, k] and bias [cout] are
    nn.Conv2d's parameters under nn.Conv2d's names and initialisation."""

    def __init__(self, cin, cout, kernel_size, stride=1):
        super().__init__()
        conv = nn.Conv2d(int(cin), int(cout), kernel_size=kernel_size, stride=int(stride))
        self.cin, self.cout, self.kernel_size, self.stride = int(cin), int(cout), tuple(conv.kernel_size), int(stride)
        if self.cout % capi.CONV_COUT_STEP or not 0 < self.cout <= capi.CONV_MAX_COUT:
            raise ValueError(f"cout={cout}: a multiple of {capi.CONV_COUT_STEP} up to {capi.CONV_MAX_COUT} is built")
        self.weight, self.bias = conv.weight, conv.bias

    def forward(self, x):
        if not x.is_cuda:                   # the stem's torch path hands on conv2d's own layout
            x = x.contiguous()
        return conv_relu(x, self.weight, self.bias, self.stride)

    def extra_repr(self):
        return f"{self.cin}, {self.cout}, kernel_size={self.kernel_size}, stride={self.stride}"


class LinearRelu(nn.Module):
    """nn.Linear(in_features, out_features) with the ReLU behind it, as `linear_relu`: weight [out, in] and bias [out] are nn.Linear's
    parameters under nn.Linear's names and initialisation."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = int(in_features), int(out_features)
        if self.out_features % capi.CONV_COUT_STEP or not 0 < self.out_features <= capi.CONV_MAX_COUT:
            raise ValueError(f"out_features={out_features}: a multiple of {capi.CONV_COUT_STEP} up to {capi.CONV_MAX_COUT} is built")
        lin = nn.Linear(self.in_features, self.out_features)
        self.weight, self.bias = lin.weight, lin.bias

    def forward(self, x):
        if not x.is_cuda:
            x = x.contiguous()
        return linear_relu(x, self.weight, self.bias)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}"


class NatureCNN(_FeaturesBase if _FeaturesBase is not object else nn.Module):
    """stable_baselines3's NatureCNN (a BaseFeaturesExtractor subclass when SB3 is importable, the same surface where it is not) over an
    image space: `cnn_base=tg.NatureCNN` in the reference's CustomCombinedExtractor.

    cnn = Sequential(ConvStem, Identity, Conv2d(32, 64, 4, 2), ReLU, Conv2d(64, 64, 3, 1), ReLU, Flatten), linear = Sequential(Linear, ReLU):
    the state_dict keys are SB3's (cnn.0, cnn.2, cnn.4, linear.0: the Identity stands where SB3 has the first ReLU), so a checkpoint loads
    either way.  channels_first: the layout of the observations, [C, H, W] or [H, W, C] per sample; None applies SB3's rule as
    DeviceRolloutBuffer does (the smallest of the three dimensions comes first).  normalized_image is accepted for SB3's signature.

    Inputs (see the module's table): uint8 images are scaled by 1 / 255; float32 images that SB3's preprocess_obs has divided already need
    float_scale=1 (the default), float32 images in 0 ... 255 from this project's buffers and augmentation need float_scale=1 / 255.

    device_tail=True puts the second and third convolution and the linear layer on the device tail as well (csrc/tg_conv.hip; DESIGN.md
    4.21): cnn = Sequential(ConvStem, Identity, ConvRelu(32, 64, 4, 2), Identity, ConvRelu(64, 64, 3, 1), Identity, Flatten), linear =
    Sequential(LinearRelu, Identity), the same state_dict keys, so both kinds and SB3's own load each other's checkpoints.  Then a row's
    FEATURES are one arithmetic order per element whatever the batch.  features_dim must be a multiple of 32 up to 512."""

    def __init__(self, observation_space, features_dim=512, normalized_image=False, channels_first=None, float_scale=1.0, device_tail=False):
        shape = tuple(int(s) for s in observation_space.shape)
        if len(shape) != 3:
            raise ValueError(f"NatureCNN needs an image space [C, H, W] or [H, W, C], got shape {shape}")
        if channels_first is not None and not isinstance(channels_first, (bool, np.bool_)):
            raise ValueError(f"channels_first={channels_first!r}: True, False or None")
        cf = bool(np.argmin(shape) == 0) if channels_first is None else bool(channels_first)
        Cn, H, W = shape if cf else (shape[2], shape[0], shape[1])
        if H < 36 or W < 36:
            raise ValueError(f"NatureCNN's three convolutions need H, W >= 36, got {H} x {W} (channels_first={cf})")
        if device_tail and (int(features_dim) % capi.CONV_COUT_STEP or not 0 < int(features_dim) <= capi.CONV_MAX_COUT):
            raise ValueError(f"features_dim={features_dim} with device_tail=True: a multiple of {capi.CONV_COUT_STEP} up to "
                             f"{capi.CONV_MAX_COUT} is built")
        if _FeaturesBase is not object:
            super().__init__(observation_space, features_dim)
        else:
            super().__init__()
            self._observation_space, self._features_dim = observation_space, int(features_dim)
        h, w = _out_hw(H, W)
        h, w = (h - 4) // 2 + 1, (w - 4) // 2 + 1
        h, w = h - 2, w - 2
        self.n_flatten = 64 * h * w
        self.device_tail = bool(device_tail)
        if self.device_tail:
            if h > capi.CONV_MAX_KERNEL or w > capi.CONV_MAX_KERNEL:
                raise ValueError(f"device_tail=True: conv3's output is {h} x {w}, the linear layer is built up to {capi.CONV_MAX_KERNEL} x "
                                 f"{capi.CONV_MAX_KERNEL} (observations up to 163 x 163)")
            self.cnn = nn.Sequential(ConvStem(Cn, cf, float_scale), nn.Identity(), ConvRelu(32, 64, 4, 2), nn.Identity(), ConvRelu(64, 64, 3, 1),
                                     nn.Identity(), nn.Flatten())
            self.linear = nn.Sequential(LinearRelu(self.n_flatten, int(features_dim)), nn.Identity())
            return
        self.cnn = nn.Sequential(ConvStem(Cn, cf, float_scale), nn.Identity(), nn.Conv2d(32, 64, kernel_size=4, stride=2, padding=0), nn.ReLU(),
                                 nn.Conv2d(64, 64, kernel_size=3, stride=1, padding=0), nn.ReLU(), nn.Flatten())
        self.linear = nn.Sequential(nn.Linear(self.n_flatten, int(features_dim)), nn.ReLU())

    if _FeaturesBase is object:
        @property
        def features_dim(self):
            return self._features_dim

    def forward(self, observations):
        if self.device_tail:                # Flatten is part of linear_relu: conv3's [B, 64, h, w] output goes to the kernel as it is
            return self.linear[0](self.cnn[4](self.cnn[2](self.cnn[0](observations))))
        return self.linear(self.cnn(observations))
