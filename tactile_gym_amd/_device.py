"""The one call path of the torch-facing device ops (rollout, replay, vecnorm, action_head, loss_head, torch_layers, mlp, augment; DESIGN.md
4.18): how a torch tensor becomes a C argument, how a C entry of the library is launched, and what these wrappers refuse.

    launch("tg_rollout_gae", dev, ptr(rewards), ..., T, N, gamma, lam)      # one launch: dev current, torch's stream of dev last, rc checked

    with on_device(dev):                                                    # several launches under one guard
        stream = stream_of(dev)
        call("tg_replay_draw", ..., stream)
        call("tg_rollout_gather", ..., stream)

What the path guarantees: the tensors' device is the current one during the call, torch's current stream of that device is the entry's last
argument, a non-zero return code raises TactileGymHipError with the library's message, and None becomes NULL.  A new wrapper uses it; it
does not write these steps out again.
"""
import contextlib
import ctypes as C

import torch

from . import _capi as capi

_CURRENT = contextlib.nullcontext()


# ---------------------------------------------------------------------------------------------------------------- arguments
def ptr(t):
    """A tensor's address as a c_void_p; NULL for None."""
    return C.c_void_p(None if t is None else t.data_ptr())


def addr(t):
    """A tensor's address as an integer, None for None: what a ctypes structure's pointer fields take (tg_mlp_tower)."""
    return None if t is None else t.data_ptr()


def ptrs(tensors):
    """A host array of device addresses (NULL for None): how the C entries take the critics' separate tensors and the tables."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


# ---------------------------------------------------------------------------------------------------------------- launches
def on_device(dev):
    """torch.cuda.device(dev), or nothing when it is the current device already (the context manager costs more than the launch)."""
    return _CURRENT if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def stream_of(dev):
    """torch's current stream of `dev` as a c_void_p (`.value`: the integer that augment's _fused takes)."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def call(entry, *args):
    """The library's entry of that name with `args` as they are (the stream among them); a non-zero return code raises."""
    capi.check(getattr(capi.lib(), entry)(*args))


def launch(entry, dev, *args):
    """One whole launch: `dev` made current if it is not, torch's current stream of it appended to `args`, the return code checked."""
    with on_device(dev):
        call(entry, *args, stream_of(dev))


def workspace(entry, *args):
    """The byte count that a *_workspace entry answers; a negative answer is an error code and raises.  The caller allocates."""
    nbytes = int(getattr(capi.lib(), entry)(*args))
    if nbytes < 0:
        capi.check(nbytes)
    return nbytes


# ---------------------------------------------------------------------------------------------------------------- refusals
def checked_f32(x, name, shapes, device=None, where="the device", is_device=None):
    """`x` itself (with its autograd history: the caller detaches) after the checks of the action and loss heads, in this order: a torch
    tensor, float32, of one of `shapes`, on the ROCm device (is_device: the predicate that the heads' CPU tests replace), on `device` when
    one is given (`where`: the caller's words for it), contiguous."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {x.dtype}")
    if tuple(x.shape) not in shapes:
        raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shapes)}, got {tuple(x.shape)}")
    if not (x.is_cuda if is_device is None else is_device(x)):
        raise ValueError(f"{name} must be on the ROCm device (there is no CPU path), got {x.device}")
    if device is not None and x.device != device:
        raise ValueError(f"{name} must be on {where} {device}, got {x.device}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous (a copy would be a launch and a temporary of its own)")
    return x


def check_f32_like(t, name, shape, x, where="x's device", got=True):
    """`t` as a contiguous float32 tensor of `shape` on the device of the tensor `x` (`where`: the caller's words for that device; got: whether
    the refusal also says what it found)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 torch tensor")
    if tuple(t.shape) != tuple(shape) or t.device != x.device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {list(shape)} tensor on {where}" + (f", got {list(t.shape)} on {t.device}" if got else ""))


def check_images(x, name="x", allow_cpu=False):
    """`x` as a contiguous 4-D uint8 or float32 image batch on the ROCm device (allow_cpu: or on the host, for the conv stem's torch path)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{name} must be uint8 or float32, got {x.dtype}")
    if not (allow_cpu or x.is_cuda):
        raise ValueError(f"{name} must be on the ROCm device (there is no CPU path), got {x.device}")
    if x.dim() != 4:
        raise ValueError(f"{name} must be a 4-D image batch, got shape {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
