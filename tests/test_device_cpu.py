"""tactile_gym_amd._device without a GPU: the one call path of the torch-facing wrappers with the library replaced by a
recorder and the module's guard and stream functions replaced by fakes, the shared refusals with the texts of both callers, and the base of
the two device buffers on the refusal paths that end before any allocation."""
import contextlib
import ctypes
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from tactile_gym_amd import _capi, spaces  # noqa: E402

torch = pytest.importorskip("torch")
from tactile_gym_amd import _device  # noqa: E402

STREAM = 0x1234


class Recorder:
    """A library whose every entry records (name, arguments) and answers `rc`; tg_last_error answers `error`."""

    def __init__(self, rc=0, error=b""):
        self.calls, self.rc, self.error = [], rc, error

    def __getattr__(self, name):
        def entry(*args):
            if name == "tg_last_error":
                return self.error
            self.calls.append((name, tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args)))
            return self.rc
        return entry


@pytest.fixture
def path(monkeypatch):
    """(recorder, the devices the guard was asked for): the library, the guard and the stream of the call path replaced."""
    rec, guarded = Recorder(), []

    def on_device(dev):
        guarded.append(dev)
        return contextlib.nullcontext()

    monkeypatch.setattr(_capi, "lib", lambda: rec)
    monkeypatch.setattr(_device, "on_device", on_device)
    monkeypatch.setattr(_device, "stream_of", lambda dev: ctypes.c_void_p(STREAM))
    return rec, guarded


def test_launch_passes_the_arguments_through_with_the_stream_last(path):
    rec, guarded = path
    x, table, dev = torch.zeros(3), (ctypes.c_int64 * 2)(5, 6), torch.device("cuda", 1)
    assert _device.launch("tg_some_entry", dev, _device.ptr(x), 7, 0.5, table, _device.ptr(None)) is None
    assert guarded == [dev]                                                    # the guard was asked for the caller's device, once
    (name, args), = rec.calls
    assert name == "tg_some_entry" and args == (x.data_ptr(), 7, 0.5, table, None, STREAM)
    assert args[3] is table                                                    # passed on as it is, not copied
    del rec.calls[:], guarded[:]
    _device.call("tg_other", 1, ctypes.c_void_p(99))                           # the guard-plus-stream form's half: no guard, no stream of its own
    assert rec.calls == [("tg_other", (1, 99))] and guarded == []


def test_a_return_code_raises_with_the_librarys_text(path):
    rec, _ = path
    rec.rc, rec.error = -3, b"tg_some_entry: rows is NULL"
    with pytest.raises(_capi.TactileGymHipError, match="tg_some_entry: rows is NULL"):
        _device.launch("tg_some_entry", torch.device("cuda", 0), 1)
    assert rec.calls == [("tg_some_entry", (1, STREAM))]
    with pytest.raises(_capi.TactileGymHipError, match="rows is NULL"):
        _device.call("tg_some_entry", 1, ctypes.c_void_p(STREAM))


def test_none_is_null_and_tensors_give_their_address():
    a, b = torch.zeros(4), torch.zeros((2, 3), dtype=torch.uint8)
    assert isinstance(_device.ptr(a), ctypes.c_void_p) and _device.ptr(a).value == a.data_ptr() and _device.ptr(None).value is None
    assert _device.ptr(a[1:]).value == a.data_ptr() + 4
    assert _device.addr(b) == b.data_ptr() and _device.addr(None) is None
    arr = _device.ptrs([a, None, b])
    assert isinstance(arr, ctypes.c_void_p * 3) and list(arr) == [a.data_ptr(), None, b.data_ptr()]
    assert len(_device.ptrs([])) == 0


def test_workspace_answers_an_int_and_raises_on_an_error_code(path):
    rec, guarded = path
    rec.rc = 4096
    n = _device.workspace("tg_some_workspace", 64, 2)
    assert n == 4096 and type(n) is int and rec.calls == [("tg_some_workspace", (64, 2))] and guarded == []
    rec.rc = 0
    assert _device.workspace("tg_some_workspace", 0, 2) == 0
    rec.rc, rec.error = -1, b"tg_some_workspace: B = 0"
    with pytest.raises(_capi.TactileGymHipError, match="tg_some_workspace: B = 0"):
        _device.workspace("tg_some_workspace", 0, 2)


HEAD = dict(where="the head's device")             # action_head._DeviceHead._checked's words
LOSS = dict()                                      # loss_head's


@pytest.mark.parametrize("words", [HEAD, LOSS], ids=["head", "loss"])
def test_the_float32_check_refuses_in_order(words):
    """Each refusal is reached with everything behind it wrong as well: a wrong dtype on a wrong shape on the CPU, and so on."""
    shapes = [(2,), (5, 2)]
    with pytest.raises(TypeError, match="mean must be a torch tensor, got ndarray"):
        _device.checked_f32(np.zeros((3, 3)), "mean", shapes, **words)
    with pytest.raises(ValueError, match=r"mean must be float32, got torch\.float64"):
        _device.checked_f32(torch.zeros((3, 3), dtype=torch.float64), "mean", shapes, **words)
    with pytest.raises(ValueError, match=r"mean must have shape \(2,\) or \(5, 2\), got \(3, 3\)"):
        _device.checked_f32(torch.zeros((3, 3)), "mean", shapes, **words)
    with pytest.raises(ValueError, match=r"mean must be on the ROCm device \(there is no CPU path\), got cpu"):
        _device.checked_f32(torch.zeros((2, 5)).t(), "mean", shapes, **words)      # [5, 2], not contiguous: the device comes first


def test_the_float32_check_with_the_device_predicate_replaced():
    """As tests/test_action_head_cpu.py's stubbed heads do: every tensor counts as a device tensor."""
    everything = lambda t: True  # noqa: E731
    shapes, cpu = [(5, 2)], torch.device("cpu")
    x = torch.zeros((5, 2), requires_grad=True)
    assert _device.checked_f32(x, "mean", shapes, cpu, is_device=everything) is x          # the tensor itself: the caller detaches
    for words in (HEAD, LOSS):
        with pytest.raises(ValueError, match=r"mean must be contiguous \(a copy would be a launch and a temporary of its own\)"):
            _device.checked_f32(torch.zeros((2, 5)).t(), "mean", shapes, cpu, is_device=everything, **words)
    other = torch.device("cuda", 1)                                                         # only compared, never touched
    with pytest.raises(ValueError, match="mean must be on the head's device cuda:1, got cpu"):
        _device.checked_f32(torch.zeros((2, 5)).t(), "mean", shapes, other, is_device=everything, **HEAD)
    with pytest.raises(ValueError, match="mean must be on the device cuda:1, got cpu"):
        _device.checked_f32(torch.zeros((2, 5)).t(), "mean", shapes, other, is_device=everything, **LOSS)


def test_the_parameter_and_image_checks_keep_each_callers_text():
    x = torch.zeros((2, 3))
    with pytest.raises(TypeError, match="weight must be a float32 torch tensor"):
        _device.check_f32_like(torch.zeros((4, 3), dtype=torch.float64), "weight", (4, 3), x)
    with pytest.raises(ValueError, match=r"weight must be a contiguous \[4, 3\] tensor on x's device, got \[3, 4\] on cpu$"):
        _device.check_f32_like(torch.zeros((3, 4)), "weight", (4, 3), x)
    with pytest.raises(ValueError, match=r"params must be a contiguous \[2, 3\] tensor on the input's device$"):
        _device.check_f32_like(torch.zeros((3, 2)).t(), "params", (2, 3), x, where="the input's device", got=False)
    assert _device.check_f32_like(torch.zeros((4, 3)), "weight", [4, 3], x) is None
    img = torch.zeros((1, 1, 8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="out must be on the ROCm device"):
        _device.check_images(img, "out")
    assert _device.check_images(img, allow_cpu=True) is None
    with pytest.raises(TypeError, match="x must be uint8 or float32, got torch.int64"):
        _device.check_images(img.long(), allow_cpu=True)
    with pytest.raises(ValueError, match=r"x must be a 4-D image batch, got shape \(1, 8, 8\)"):
        _device.check_images(img[0], allow_cpu=True)
    with pytest.raises(ValueError, match="x must be contiguous"):
        _device.check_images(img.expand(2, 3, 8, 8), allow_cpu=True)


# ---------------------------------------------------------------------------------------------------------------- the buffers' base
IMG = spaces.Box(low=0, high=255, shape=(1, 8, 8), dtype=np.uint8)
VEC = spaces.Box(low=-1.0, high=1.0, shape=(3,), dtype=np.float32)
ACT = spaces.Box(low=-1.0, high=1.0, shape=(2,), dtype=np.float32)
OBS = spaces.Dict({"tactile": IMG, "oracle": VEC})
REFUSED = [                                         # (constructor arguments, exception, the message's words): all end before any allocation
    (dict(buffer_size=0), ValueError, "buffer_size must be a positive integer, got 0"),
    (dict(buffer_size=True), ValueError, "buffer_size must be a positive integer, got True"),
    (dict(buffer_size=2.5), ValueError, "buffer_size must be a positive integer, got 2.5"),
    (dict(n_envs=-1), ValueError, "n_envs must be a positive integer, got -1"),
    (dict(device="cpu"), ValueError, "device must be the ROCm device (there is no CPU path), got cpu"),
    (dict(observation_space=spaces.Dict({"a": spaces.Dict({"b": VEC})})), TypeError, "observation_space['a'] must be a Box"),
    (dict(observation_space=spaces.Dict({"a": spaces.Box(low=0, high=1, shape=(3,), dtype=np.float64)})), TypeError,
     "observation_space['a'] must be uint8 or float32, got float64"),
    (dict(action_space=spaces.Box(low=0, high=3, shape=(2,), dtype=np.uint8)), TypeError, "action_space must be a float32 Box of one dimension"),
    (dict(action_space=OBS), TypeError, "action_space must be a float32 Box of one dimension"),
    (dict(channels_first=1), ValueError, "channels_first=1: True, False or None"),
    (dict(observation_space=spaces.Dict({"tactile": spaces.Box(low=0, high=255, shape=(1, 8, 8), dtype=np.uint8)}), channels_first=False),
     ValueError, "observation_space key 'tactile': image keys need H, W >= 2, got shape (1, 8, 8) (channels_first=False)"),
    (dict(observation_space=spaces.Box(low=0, high=255, shape=(4, 1, 8), dtype=np.uint8)), ValueError,
     "observation_space key None: image keys need H, W >= 2, got shape (4, 1, 8) (channels_first=False)"),
]


def _buffer_classes():
    from tactile_gym_amd.replay import DeviceReplayBuffer
    from tactile_gym_amd.rollout import DeviceRolloutBuffer
    return DeviceRolloutBuffer, DeviceReplayBuffer


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_both_buffers_refuse_the_same_arguments_with_the_same_words(case):
    kwargs, exc, words = REFUSED[case]
    kwargs = dict(dict(buffer_size=4, observation_space=OBS, action_space=ACT, device="cuda", n_envs=2), **kwargs)
    texts = []
    for cls in _buffer_classes():
        with pytest.raises(exc) as info:
            cls(**kwargs)
        texts.append(str(info.value))
    assert texts[0] == texts[1] and words in texts[0], texts


def test_the_replay_buffer_borrows_no_method_of_the_rollout_buffer():
    from tactile_gym_amd.rollout import _DeviceBuffer
    rollout, replay = _buffer_classes()
    assert issubclass(rollout, _DeviceBuffer) and issubclass(replay, _DeviceBuffer) and not issubclass(replay, rollout)
    own = {id(v.__func__ if isinstance(v, (classmethod, staticmethod)) else v) for v in vars(rollout).values()
           if isinstance(v, (types.FunctionType, classmethod, staticmethod))}
    assert len(own) >= 8                                                        # __init__, for_env, reset, add, ... are looked at
    for name in dir(replay):
        attr = getattr(replay, name)
        assert id(getattr(attr, "__func__", attr)) not in own, name
    for name in ("_alloc", "size", "_input", "_place", "_device_index", "_obs_inputs", "_image_options", "_gather_plain"):
        assert name in vars(_DeviceBuffer) and name not in vars(rollout) and name not in vars(replay), name
    from tactile_gym_amd import augment, rollout as rollout_module
    assert rollout_module._unwrap_augment is augment._unwrap_augment           # importable from both, as the buffers' callers do
