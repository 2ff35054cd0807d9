"""RAD's image augmentation on the device: kornia's RandomAffine(degrees=0, translate=..., scale=[1, 1], p) over torch tensors on the ROCm
device (csrc/tg_augment.hip: k_random_translate, one launch per call on torch's current stream).

Every params file of the reference builds (sb3_helpers/params/*_params.py:7-9, train_agent.py:35, simple_sb3_example.py:68)

    augmentations = nn.Sequential(K.RandomAffine(degrees=0, translate=[0.05, 0.05], scale=[1.0, 1.0], p=0.5))

with `import kornia.augmentation as K`; with `import tactile_gym_amd.augment as K` the same line builds the device module, and RAD_PPO / RAD_SAC
apply it to the image observations of every training minibatch as before.

Semantics (kornia's defaults: same_on_batch=False, bilinear, zero padding, align_corners=False): sample b is warped with probability p by
tx ~ U(-ax W, ax W), ty ~ U(-ay H, ay H) pixels - out[y][x] = bilinear(in, x - tx W / (W - 1), y - ty H / (H - 1)), taps outside the image 0,
every channel alike - and otherwise passed through unchanged (its values converted to float32).  The draws are counter based (seed, counter):
the same distribution as kornia's, not the same numbers.  Inputs: contiguous 4-D uint8 or float32 tensors on the device, [B, C, H, W]
(channels_first) or [B, H, W, C]; the output is a new float32 tensor of the same shape.  The input is never written, so obs_mode="torch"
observations can be augmented directly.  There is no CPU path: anything else raises.
"""
import ctypes as C

import torch

from . import _capi as capi

__all__ = ["random_translate", "RandomTranslate", "RandomAffine", "augment_images"]

_DTYPES = {torch.uint8: capi.AUGMENT_DTYPE["uint8"], torch.float32: capi.AUGMENT_DTYPE["float32"]}


def _pair(v, name):
    if isinstance(v, (int, float)):
        return float(v), float(v)
    v = tuple(float(x) for x in v)
    if len(v) != 2:
        raise ValueError(f"{name} must be a number or a pair, got {v}")
    return v


def _check_images(x, name="x"):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise TypeError(f"{name} must be uint8 or float32, got {x.dtype}")
    if not x.is_cuda:
        raise ValueError(f"{name} must be on the ROCm device (there is no CPU path), got {x.device}")
    if x.dim() != 4:
        raise ValueError(f"{name} must be a 4-D image batch, got shape {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def random_translate(x, translate=(0.05, 0.05), p=0.5, seed=0, counter=0, params=None, channels_first=True, out=None, return_params=False):
    """One draw of the augmentation over the batch x ([B, C, H, W], or [B, H, W, C] with channels_first=False): a new float32 tensor (or `out`).

    translate: (ax, ay) in [0, 1], fractions of W and H; p: the probability that a sample is warped.  (seed, counter) pick the draws: element
    3 b + k of tg_sample_actions' generator.  params: an optional float32 [B, 3] device tensor of (apply, tx, ty) per sample (tx, ty in pixels)
    used instead of the draws.  return_params=True returns (out, params) with the [B, 3] values that were used."""
    _check_images(x)
    ax, ay = _pair(translate, "translate")
    if not (0.0 <= ax <= 1.0 and 0.0 <= ay <= 1.0):
        raise ValueError(f"translate must lie in [0, 1], got {(ax, ay)}")
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"p must lie in [0, 1], got {p}")
    B = x.shape[0]
    if channels_first:
        Cn, H, W = x.shape[1], x.shape[2], x.shape[3]
    else:
        H, W, Cn = x.shape[1], x.shape[2], x.shape[3]
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    else:
        _check_images(out, "out")
        if out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device:
            raise ValueError("out must be a float32 tensor of the input's shape on its device")
    if params is not None:
        if not isinstance(params, torch.Tensor) or params.dtype != torch.float32:
            raise TypeError("params must be a float32 torch tensor")
        if tuple(params.shape) != (B, 3) or params.device != x.device or not params.is_contiguous():
            raise ValueError(f"params must be a contiguous [{B}, 3] tensor on the input's device")
    pout = torch.empty((B, 3), dtype=torch.float32, device=x.device) if return_params else None
    L = capi.lib()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        capi.check(L.tg_random_translate(
            C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), _DTYPES[x.dtype], int(bool(channels_first)), B, Cn, H, W, ax, ay, p,
            C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint64(int(counter) & 0xFFFFFFFFFFFFFFFF),
            C.c_void_p(params.data_ptr() if params is not None else None), C.c_void_p(pout.data_ptr() if pout is not None else None),
            C.c_void_p(stream)))
    return (out, pout) if return_params else out


def _draw_seed():
    return int(torch.randint(0, 2**62, (1,)).item())   # torch's default generator: torch.manual_seed makes the module's draws repeat


class RandomTranslate(torch.nn.Module):
    """kornia's RandomAffine(degrees=0, translate, scale=(1, 1), p) on the device.  Call k (from 0) draws with (seed, k), so successive
    minibatches differ and a seeded run repeats.  After a call, `_params` holds kornia's names: `batch_prob` (bool [B]) and `translations`
    (float32 [B, 2], pixels)."""

    def __init__(self, translate=(0.05, 0.05), p=0.5, seed=None, channels_first=True):
        super().__init__()
        self.translate = _pair(translate, "translate")
        if not all(0.0 <= t <= 1.0 for t in self.translate):
            raise ValueError(f"translate must lie in [0, 1], got {self.translate}")
        self.p = float(p)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError(f"p must lie in [0, 1], got {self.p}")
        self.seed = _draw_seed() if seed is None else int(seed)
        self.channels_first = bool(channels_first)
        self.counter = 0
        self._params = None

    def forward(self, x):
        out, prm = random_translate(x, self.translate, self.p, self.seed, self.counter, channels_first=self.channels_first, return_params=True)
        self.counter += 1
        self._params = {"batch_prob": prm[:, 0] != 0, "translations": prm[:, 1:3]}
        return out

    def extra_repr(self):
        return f"translate={self.translate}, p={self.p}, seed={self.seed}, channels_first={self.channels_first}"


def _is_zero_pair(v):
    if isinstance(v, (int, float)):
        return float(v) == 0.0
    v = tuple(v)
    return len(v) == 2 and all(float(t) == 0.0 for t in v)


def RandomAffine(degrees, translate=None, scale=None, shear=None, p=0.5, same_on_batch=False, align_corners=False, padding_mode="zeros",
                 resample="bilinear", seed=None):
    """The drop-in for kornia.augmentation.RandomAffine in the form the reference uses: degrees 0, a translate range, scale None or (1, 1),
    no shear, kornia's defaults otherwise.  Returns a RandomTranslate (translate None: no shift).  Any other argument raises NotImplementedError
    naming it: the rotation, scale and shear paths are not built."""
    if not _is_zero_pair(degrees):
        raise NotImplementedError(f"RandomAffine: degrees={degrees!r} (only 0 is built)")
    if scale is not None and tuple(float(s) for s in scale) != (1.0, 1.0):
        raise NotImplementedError(f"RandomAffine: scale={scale!r} (only None or (1, 1) is built)")
    if shear is not None:
        raise NotImplementedError(f"RandomAffine: shear={shear!r} (only None is built)")
    if same_on_batch:
        raise NotImplementedError("RandomAffine: same_on_batch=True (only per-sample draws are built)")
    if align_corners:
        raise NotImplementedError("RandomAffine: align_corners=True (only False is built)")
    if str(getattr(padding_mode, "name", padding_mode)).lower() != "zeros":
        raise NotImplementedError(f"RandomAffine: padding_mode={padding_mode!r} (only 'zeros' is built)")
    if str(getattr(resample, "name", resample)).lower() != "bilinear":
        raise NotImplementedError(f"RandomAffine: resample={resample!r} (only 'bilinear' is built)")
    return RandomTranslate(translate=(0.0, 0.0) if translate is None else translate, p=p, seed=seed)


def augment_images(obs, module):
    """Apply `module` to the 4-D image keys of an observation dict ("tactile", "visual"), one independent call per key; vector keys are
    returned as they are.  A new dict; the observation tensors are not written."""
    return {k: module(v) if isinstance(v, torch.Tensor) and v.dim() == 4 else v for k, v in obs.items()}
