"""Seeded inputs of the frame-interpolation tests (tests/test_interp_host.py, tests/test_interp_gpu.py), computed once per
process and read-only.

`canvas` is a smooth textured image: a few low-frequency sinusoids plus seeded noise blurred with a Gaussian of sigma 2, three
different channels.  `moving_pair` cuts A and B out of it 4 px / 2 px apart and the true middle frame half-way between them:
the quality claim is measured against that truth, not against anyone's restatement.

`stage_case(size, name)` is one input of the stage-parity test: two frames and explicit fp32 flows."""
import functools

import numpy as np
from scipy import ndimage

STAGE_SIZES = [(1, 5), (5, 1), (16, 16), (17, 19), (33, 130)]          # (H, W): tails, single rows and columns, several blocks
STAGE_CASES = ["zero", "const_int", "const_half", "smooth", "outside", "wild"]
# t = 1/3, 2/3 and 1/4, 1/2, 3/4.  The 0.5-px flows get dyadic t only: there every product is exact in fp32 and fp64 alike, so
# the ties are exact ties; at t = 1/3 the same flows give values n / 108, true ties among them, that no float type evaluates
# exactly, and which way those round says nothing about the kernel.
STAGE_FACTORS = {"const_half": (2, 4)}
DEFAULT_FACTORS = (3, 4)


def stage_factors(name):
    return STAGE_FACTORS.get(name, DEFAULT_FACTORS)


MOVE = (4, 2)                                                           # (dx, dy) between A and B of the moving pair
QUALITY_HW = (64, 96)
QUALITY_BORDER = 24


@functools.lru_cache(maxsize=None)
def canvas(H, W, seed=0):
    """uint8 RGB (H, W, 3)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    ch = []
    for c in range(3):
        s = sum(np.sin(2 * np.pi * (x * fx + y * fy) + ph) for fx, fy, ph in rng.uniform(-0.04, 0.04, (4, 3)) * (1, 1, 80))
        n = ndimage.gaussian_filter(rng.standard_normal((H, W)), 2.0, mode="wrap")
        v = s / 4 + 1.5 * n / n.std() * 0.35
        ch.append((v - v.min()) / (v.max() - v.min()) * 255.0)
    out = np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def crop(H, W, ox, oy, seed=0, pad=32):
    """The H x W window of the canvas whose top-left corner is (pad + ox, pad + oy)."""
    return canvas(H + 2 * pad, W + 2 * pad, seed)[pad + oy:pad + oy + H, pad + ox:pad + ox + W]


@functools.lru_cache(maxsize=None)
def moving_pair(seed=0):
    """-> (A, B, truth), uint8 (64, 96, 3): the content moves by MOVE from A to B, and by half of it to the truth."""
    H, W = QUALITY_HW
    dx, dy = MOVE
    return crop(H, W, 0, 0, seed), crop(H, W, -dx, -dy, seed), crop(H, W, -dx // 2, -dy // 2, seed)


def interior_mae(img, truth):
    b = QUALITY_BORDER
    return float(np.mean(np.abs(np.asarray(img, np.float64) - np.asarray(truth, np.float64))[b:-b, b:-b]))


def _smooth_flow(rng, H, W, amp):
    """fp32 (H, W, 2), each component a blurred field rescaled to [-amp, amp]."""
    f = np.stack([ndimage.gaussian_filter(rng.standard_normal((H + 16, W + 16)), 4.0)[8:8 + H, 8:8 + W] for _ in range(2)], -1)
    f = f / max(np.abs(f).max(), 1e-12) * amp
    return f.astype(np.float32)


@functools.lru_cache(maxsize=None)
def stage_case(size, name, seed=0):
    """-> (frames uint8 (2, H, W, 3), fab fp32 (1, H, W, 2), fba fp32 (1, H, W, 2))."""
    H, W = size
    rng = np.random.default_rng([seed, H, W, STAGE_CASES.index(name)])
    A, B = crop(H, W, 0, 0, seed + 1), crop(H, W, 3, -2, seed + 2)
    const = lambda dx, dy: np.broadcast_to(np.array([dx, dy], np.float32), (H, W, 2)).copy()
    if name == "zero":                                  # A = B and no motion: every output frame is A
        B, fab, fba = A, const(0, 0), const(0, 0)
    elif name == "const_int":                           # B is A moved by the flow: both samples agree away from the border.
        # a multiple of 4, so that every position at t = k / 4 is a whole pixel: half-pixel positions give samples of x.5 on
        # both sides, ties that the 1e-6 of a penalised side cannot separate in any float type
        B, fab, fba = crop(H, W, -4, 4, seed + 1), const(4, -4), const(-4, 4)
    elif name == "const_half":                          # with t = 1/2 every weight is a multiple of 1/8: exact ties
        fab, fba = const(0.5, 0.5), const(-0.5, -0.5)
    elif name == "smooth":
        fab, fba = _smooth_flow(rng, H, W, 6.0), _smooth_flow(rng, H, W, 6.0)
    elif name == "outside":                             # every sampling position of every t >= 1/4 lies outside the frames
        fab, fba = const(8 * W + 3.25, -(8 * H + 1.5)), const(-(8 * W + 3.25), 8 * H + 1.5)
    elif name == "wild":                                # +-1e4, NaN and inf entries among smooth flows
        fab, fba = _smooth_flow(rng, H, W, 6.0), _smooth_flow(rng, H, W, 6.0)
        for fl in (fab, fba):
            flat = fl.reshape(-1)
            pick = rng.permutation(flat.size)[:max(flat.size // 4, 5)]
            flat[pick] = np.resize(np.array([1e4, -1e4, np.nan, np.inf, -np.inf], np.float32), pick.size)
    else:
        raise KeyError(name)
    frames = np.stack([A, B])
    for a in (frames, fab, fba):
        a.setflags(write=False)
    return frames, fab[None], fba[None]
