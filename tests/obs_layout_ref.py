"""stable_baselines3's VecTransposeImage restated in numpy, composed with the VecFrameStack restatement of frame_stack_ref.StackRef: what
channels_first=True (with frame_stack=n) must hand out (tests/test_obs_layout_cpu.py, tests/test_gpu_obs_layout.py).

VecTransposeImage (stable_baselines3/common/vec_env/vec_transpose.py):
- observation_space: every image Box (uint8, three axes, bounds 0 and 255) of shape (H, W, C) becomes Box(0, 255, (C, H, W), uint8);
- observations: the image keys of the batch are transposed (0, 3, 1, 2); a terminal observation's image keys (2, 0, 1); other keys untouched.
VecTransposeImage(VecFrameStack(venv, n)) therefore hands out [N, C * n, H, W] with channel index C * s + c (stack slot s, oldest first).
"""
import numpy as np

from frame_stack_ref import expected_from_single

IMAGE_KEYS = ("tactile", "visual")


def is_image_space(space):
    """stable_baselines3.common.preprocessing.is_image_space(space) with check_channels=False."""
    return (not hasattr(space, "spaces") and len(space.shape) == 3 and np.dtype(space.dtype) == np.uint8
            and bool(np.all(space.low == 0)) and bool(np.all(space.high == 255)))


def is_image_space_channels_first(space):
    """stable_baselines3.common.preprocessing.is_image_space_channels_first: the smallest axis is the first."""
    return int(np.argmin(space.shape)) == 0


def transpose_space_shape(shape):
    h, w, c = shape
    return (c, h, w)


def transpose_image(image):
    """VecTransposeImage.transpose_image: (H, W, C) -> (C, H, W); a batch (N, H, W, C) -> (N, C, H, W).  C-contiguous here (the device's arrays are)."""
    if image.ndim == 3:
        return np.ascontiguousarray(np.transpose(image, (2, 0, 1)))
    return np.ascontiguousarray(np.transpose(image, (0, 3, 1, 2)))


def transpose_obs(obs, keys=IMAGE_KEYS):
    return {k: transpose_image(v) if k in keys else v for k, v in obs.items()}


class TransposeRef:
    """VecTransposeImage over a recorded VecEnv's outputs: reset observations, step observations and info["terminal_observation"]."""

    def __init__(self, keys=IMAGE_KEYS):
        self.keys = keys

    def reset(self, obs):
        return transpose_obs(obs, self.keys)

    def step(self, obs, terminal):
        """terminal: {env: {key: frame}}.  Returns (observations, terminal observations)."""
        return transpose_obs(obs, self.keys), {i: transpose_obs(t, self.keys) for i, t in terminal.items()}


def expected_layout(events, n, channels_first):
    """Apply VecFrameStack(n) (n > 1) and then, with channels_first, VecTransposeImage to a frame_stack=1, channels-last rollout
    (frame_stack_ref.rollout's event list): the events the run with frame_stack=n, channels_first must produce."""
    ev = expected_from_single(events, n) if n > 1 else events
    if not channels_first:
        return ev
    ref, out = TransposeRef(), []
    for e in ev:
        if e[0] == "reset":
            out.append(("reset", e[1], ref.reset(e[2])))
        else:
            _, a, obs, rew, done, term = e
            o, t = ref.step(obs, term)
            out.append(("step", a, o, rew, done, t))
    return out
