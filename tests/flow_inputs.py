"""Seeded inputs of the optical-flow tests (tests/test_flow_host.py, tests/test_flow_gpu.py) and their reference, computed
once per process: `vdx.compat.cv2_shim` imported explicitly (float64 numpy / scipy), never through `metrics._cv2()`.

An image is three independent standard-normal fields blurred with a Gaussian of sigma 3 and rescaled to 0..255; frame i of a
clip is that field moved by i * (dx, dy) with a cubic spline, cropped 20 px inside: 2-D texture everywhere, so Farneback's
2 x 2 systems are well conditioned and a difference from the shim far above fp32 rounding is a bug.

Generated video is not like that, so `content_clip` adds 72 x 104 frames of integer pixel values (no spline) with straight
edges, flat areas and noise, where the window's 2 x 2 system is close to singular or the two frames share no motion at all:
CONTENT_ROWS move, ZERO_ROWS are one-dimensional or flat and give a flow of ~0 in exact arithmetic."""
import functools

import numpy as np
from scipy import ndimage

from vdx.compat import cv2_shim

MARGIN = 20
FARNEBACK = (0.5, 3, 15, 3, 5, 1.2, 0)
# (H, W), (dx, dy): what each row exercises is listed in tests/test_flow_gpu.py
SMALL_ROWS = [((24, 40), (1.0, 0.5)), ((72, 104), (1.5, -0.75)), ((72, 104), (6.0, -3.0)), ((97, 131), (-2.25, 1.5)),
              ((64, 200), (3.0, 3.0))]
LARGE_ROW = ((576, 1024), (1.5, -0.75))


@functools.lru_cache(maxsize=None)
def clip(n, H, W, dx, dy, seed=0):
    """uint8 RGB (n, H, W, 3): frame i shows the seeded field moved by i * (dx, dy)."""
    rng = np.random.default_rng(seed)
    field = np.stack([ndimage.gaussian_filter(rng.standard_normal((H + 2 * MARGIN, W + 2 * MARGIN)), 3.0) for _ in range(3)], -1)
    field = (field - field.min()) / (field.max() - field.min()) * 255.0
    frames = []
    for i in range(n):
        moved = field if i == 0 else np.stack(
            [ndimage.shift(field[..., c], (i * dy, i * dx), order=3, mode="nearest") for c in range(3)], -1)
        frames.append(np.clip(np.rint(moved[MARGIN:-MARGIN, MARGIN:-MARGIN]), 0, 255).astype(np.uint8))
    out = np.stack(frames)
    out.setflags(write=False)
    return out


def pair(hw, shift, seed=0):
    return clip(2, hw[0], hw[1], shift[0], shift[1], seed)


@functools.lru_cache(maxsize=None)
def shim_flow(n, H, W, dx, dy, seed=0, bgr=False):
    """The float64 shim's flows of the clip's consecutive pairs, float32 (n-1, H, W, 2) as it returns them."""
    code = cv2_shim.COLOR_BGR2GRAY if bgr else cv2_shim.COLOR_RGB2GRAY
    grey = [cv2_shim.cvtColor(f, code) for f in clip(n, H, W, dx, dy, seed)]
    out = np.stack([cv2_shim.calcOpticalFlowFarneback(a, b, None, *FARNEBACK) for a, b in zip(grey[:-1], grey[1:])])
    out.setflags(write=False)
    return out


# ---- content rows: what tests/test_flow_gpu.py lists for each ------------------------------------------------------------
CONTENT_HW = (72, 104)
CONTENT_ROWS = ["diagonal", "square", "noise_roll", "noise_pair", "mixed"]     # the reference flow is far from 0
ZERO_ROWS = ["step", "bars", "ramp", "constant"]                               # the reference flow is ~0 (asserted < 1e-6 px)


def _diagonal(i, H, W):
    y, x = np.mgrid[:H, :W]
    return np.where(x + y < 90 + 3 * i, 245, 10)


@functools.lru_cache(maxsize=None)
def content_clip(name, n=2, seed=0):
    """uint8 RGB (n, 72, 104, 3): frame i of the named content, moved by i times its shift.  The structured rows have three
    equal channels (grey = the value, under either channel order); the noise rows and the textured half have three different ones."""
    H, W = CONTENT_HW
    rng = np.random.default_rng(seed + 100)
    y, x = np.mgrid[:H, :W]
    noise = rng.integers(0, 256, (n + 1, H, W, 3))
    frames = []
    for i in range(n):
        if name == "diagonal":                       # edge x + y < 90 -> x + y < 93, grey 10 / 245
            f = _diagonal(i, H, W)
        elif name == "square":                       # white 24 x 32 square on black, +3 px in x
            f = np.where((y >= 24) & (y < 48) & (x >= 30 + 3 * i) & (x < 62 + 3 * i), 255, 0)
        elif name == "step":                         # vertical step, +2 px
            f = np.where(x < 50 + 2 * i, 10, 245)
        elif name == "bars":                         # 8-px bars, +1 px
            f = np.where(((x - i) // 8) % 2 == 0, 10, 245)
        elif name == "ramp":                         # horizontal ramp of 2 grey levels per px, +2 px
            f = np.clip(2 * (x - 2 * i) + 20, 0, 255)
        elif name == "constant":
            f = np.full((H, W), 128)
        elif name == "noise_roll":                   # uniform noise against itself rolled by 2 px
            f = np.roll(noise[0], 2 * i, axis=1)
        elif name == "noise_pair":                   # noise against unrelated noise
            f = noise[i + 1]
        elif name == "mixed":                        # left half texture, right half a diagonal edge
            f = np.array(clip(n, H, W, 1.5, -0.75, seed)[i], dtype=np.int64)
            f[:, W // 2:] = _diagonal(i, H, W)[:, W // 2:, None]
        else:
            raise KeyError(name)
        frames.append(np.broadcast_to(f if f.ndim == 3 else f[..., None], (H, W, 3)).astype(np.uint8))
    out = np.stack(frames)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def content_shim_flow(name, n=2, seed=0, bgr=False):
    """The float64 shim's flows of the content clip's consecutive pairs, float32 (n-1, 72, 104, 2)."""
    code = cv2_shim.COLOR_BGR2GRAY if bgr else cv2_shim.COLOR_RGB2GRAY
    grey = [cv2_shim.cvtColor(f, code) for f in content_clip(name, n, seed)]
    out = np.stack([cv2_shim.calcOpticalFlowFarneback(a, b, None, *FARNEBACK) for a, b in zip(grey[:-1], grey[1:])])
    out.setflags(write=False)
    return out
