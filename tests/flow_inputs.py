"""Seeded inputs of the optical-flow tests (tests/test_flow_host.py, tests/test_flow_gpu.py) and their reference, computed
once per process: `vdx.compat.cv2_shim` imported explicitly (float64 numpy / scipy), never through `metrics._cv2()`.

An image is three independent standard-normal fields blurred with a Gaussian of sigma 3 and rescaled to 0..255; frame i of a
clip is that field moved by i * (dx, dy) with a cubic spline, cropped 20 px inside: 2-D texture everywhere, so Farneback's
2 x 2 systems are well conditioned and a difference from the shim far above fp32 rounding is a bug."""
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
