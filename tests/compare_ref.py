"""The definition of the full-reference clip comparison (vdx/compare.py, csrc/compare.hip) in float64 numpy: the yardstick of
tests/test_compare_host.py and tests/test_compare_gpu.py.  Restated from the published definitions (Wang, Bovik, Sheikh,
Simoncelli 2004 for SSIM; Wang, Simoncelli, Bovik 2003 for MS-SSIM); nothing but numpy.

Inputs are two uint8 RGB clips a, b of one shape (F, H, W, 3); everything is per frame.  Every R, G, B plane is treated on its
own and the three plane results are averaged: no grey conversion.

PSNR     sse = the exact integer sum of (a - b)^2 over the frame's 3 H W bytes; psnr = 10 log10(255^2 / (sse / (3 H W))) in
         float64, inf for sse == 0.
SSIM     the 11 x 11 Gaussian window, sigma 1.5, weights normalised to sum 1, separable, as a "valid" correlation: the map is
         (H - 10) x (W - 10), no padding.  C1 = (0.01 255)^2, C2 = (0.03 255)^2; mx, my, sx2 = E[x^2] - mx^2, sy2, sxy;
         cs = (2 sxy + C2) / (sx2 + sy2 + C2); ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) cs.  A plane's value is the mean of its
         map, the frame's the mean of the three planes' (they hold equally many positions).  min(H, W) >= 11.
MS-SSIM  5 scales, weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); between scales a 2 x 2 mean of both planes (real valued
         from scale 1 on; an odd last row or column is dropped).  Per plane: the mean cs of scales 0..3 and the mean ssim of
         scale 4, each clamped at 0 from below before its power (a negative mean gives 0, not NaN); the product of the five
         powers, averaged over the three planes.  min(H, W) >= 176, so that the fifth scale still holds one window.
"""
import math

import numpy as np

WIN, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = WIN
MS_MIN_SIDE = WIN << (len(MS_WEIGHTS) - 1)            # 176


def window() -> np.ndarray:
    d = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def _valid(p: np.ndarray) -> np.ndarray:
    """(H, W) float64 -> (H-10, W-10): the window as a valid correlation, columns first, then rows."""
    w = window()
    H, W = p.shape
    v = np.zeros((H - WIN + 1, W), np.float64)
    for k in range(WIN):
        v += w[k] * p[k:k + H - WIN + 1, :]
    o = np.zeros((H - WIN + 1, W - WIN + 1), np.float64)
    for k in range(WIN):
        o += w[k] * v[:, k:k + W - WIN + 1]
    return o


def ssim_maps(x: np.ndarray, y: np.ndarray):
    """Two planes (H, W) -> (ssim map, cs map), float64 (H-10, W-10)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape or x.ndim != 2 or min(x.shape) < MIN_SIDE:
        raise ValueError(f"ssim: planes {x.shape} / {y.shape}: one shape with min(H, W) >= {MIN_SIDE}")
    mx, my = _valid(x), _valid(y)
    sx2, sy2, sxy = _valid(x * x) - mx * mx, _valid(y * y) - my * my, _valid(x * y) - mx * my
    cs = (2.0 * sxy + C2) / (sx2 + sy2 + C2)
    return (2.0 * (mx * my) + C1) / (mx * mx + my * my + C1) * cs, cs


def down2(p: np.ndarray) -> np.ndarray:
    """2 x 2 mean of a plane (H, W) in float64; an odd last row or column is dropped."""
    p = np.asarray(p, np.float64)
    h, w = p.shape[0] // 2, p.shape[1] // 2
    p = p[:2 * h, :2 * w]
    return ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])) * 0.25


def plane_means(x: np.ndarray, y: np.ndarray, scales: int = 1) -> np.ndarray:
    """Two planes -> float64 (scales, 2): mean ssim and mean cs of every scale."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.zeros((scales, 2), np.float64)
    for s in range(scales):
        if s:
            x, y = down2(x), down2(y)
        m, c = ssim_maps(x, y)
        out[s] = m.mean(), c.mean()
    return out


def frame_means(a: np.ndarray, b: np.ndarray, scales: int = 1) -> np.ndarray:
    """Two uint8 RGB frames (H, W, 3) -> float64 (3, scales, 2)."""
    return np.stack([plane_means(a[..., c], b[..., c], scales) for c in range(3)])


def sse(a: np.ndarray, b: np.ndarray) -> int:
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def psnr_from_sse(s: int, n: int) -> float:
    return math.inf if s == 0 else 10.0 * math.log10(255.0 ** 2 / (s / n))


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    return psnr_from_sse(sse(a, b), a.size)


def ssim_from_means(means: np.ndarray) -> float:
    """(3, scales, 2) -> the frame's SSIM: the mean over the planes of the scale-0 ssim means."""
    return float((means[0, 0, 0] + means[1, 0, 0] + means[2, 0, 0]) / 3.0)


def ms_ssim_from_means(means: np.ndarray) -> float:
    """(3, 5, 2) -> the frame's MS-SSIM."""
    vals = []
    for c in range(3):
        v = 1.0
        for s, w in enumerate(MS_WEIGHTS):
            m = means[c, s, 1] if s < len(MS_WEIGHTS) - 1 else means[c, s, 0]
            v *= max(float(m), 0.0) ** w
        vals.append(v)
    return (vals[0] + vals[1] + vals[2]) / 3.0


def ssim(a: np.ndarray, b: np.ndarray) -> float:
    """Two uint8 RGB frames (H, W, 3) -> SSIM."""
    _check(a, b, MIN_SIDE, "ssim")
    return ssim_from_means(frame_means(a, b, 1))


def ms_ssim(a: np.ndarray, b: np.ndarray) -> float:
    """Two uint8 RGB frames (H, W, 3) -> MS-SSIM."""
    _check(a, b, MS_MIN_SIDE, "ms_ssim")
    return ms_ssim_from_means(frame_means(a, b, len(MS_WEIGHTS)))


def _check(a, b, side, what):
    if a.shape != b.shape or a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or b.dtype != np.uint8:
        raise ValueError(f"{what}: expected two uint8 RGB frames of one shape, got {a.dtype} {a.shape} / {b.dtype} {b.shape}")
    if min(a.shape[:2]) < side:
        raise ValueError(f"{what}: frames of {a.shape[0]}x{a.shape[1]} are too small (min(H, W) >= {side})")


def compare_clip(a: np.ndarray, b: np.ndarray, want_ms: bool = True) -> dict:
    """Two clips (F, H, W, 3) -> {"sse", "psnr", "ssim"[, "ms_ssim"]}: per-frame lists."""
    out = {"sse": [], "psnr": [], "ssim": []}
    if want_ms:
        out["ms_ssim"] = []
    for fa, fb in zip(a, b):
        _check(fa, fb, MS_MIN_SIDE if want_ms else MIN_SIDE, "compare_clip")
        m = frame_means(fa, fb, len(MS_WEIGHTS) if want_ms else 1)
        out["sse"].append(sse(fa, fb))
        out["psnr"].append(psnr(fa, fb))
        out["ssim"].append(ssim_from_means(m))
        if want_ms:
            out["ms_ssim"].append(ms_ssim_from_means(m))
    return out


# ---- the inputs tests/test_compare_gpu.py and tools/compare_parity.py share ------------------------------------------------
TILE_H, TILE_W = 16, 32                               # csrc/compare.hip's output tile
PSNR_SIZES = ((11, 11), (12, 13), (TILE_H + 9, TILE_W + 11), (TILE_H + 11, TILE_W + 9), (TILE_H + 10, TILE_W + 10), (61, 117))
SSIM_SIZES = ((11, 11), (11, 43), (43, 11), (TILE_H + 9, TILE_W + 9), (TILE_H + 10, TILE_W + 10), (TILE_H + 11, TILE_W + 11), (61, 117))
SSIM_KINDS = ("noise", "perturbed", "flat_bright", "step", "anticorrelated")
MS_SIZES = ((176, 177), (191, 176))
MS_KINDS = ("perturbed", "flat_bright", "anticorrelated")


def _seed(kind: str, size) -> int:
    return 1000 * SSIM_KINDS.index(kind) + 7 * size[0] + size[1]


def pair(kind: str, size, frames: int = 2):
    """Two seeded uint8 RGB clips (frames, H, W, 3) of `kind`:
      noise           two independent uniform byte noises;
      perturbed       noise, and the same plus an integer perturbation in -3..3 (clipped);
      flat_bright     250 +- 1 each, independently: the cancellation regime (variances of order 1 under E[x^2] of 62500);
      step            a vertical step edge 40 | 220 a third into the frame, against the same edge one pixel further and 3 darker;
      anticorrelated  noise x against 255 - x: negative cs and ssim."""
    H, W = size
    g = np.random.default_rng(_seed(kind, size))
    shape = (frames, H, W, 3)
    if kind == "noise":
        a, b = g.integers(0, 256, shape), g.integers(0, 256, shape)
    elif kind == "perturbed":
        a = g.integers(0, 256, shape)
        b = np.clip(a + g.integers(-3, 4, shape), 0, 255)
    elif kind == "flat_bright":
        a, b = 250 + g.integers(-1, 2, shape), 250 + g.integers(-1, 2, shape)
    elif kind == "step":
        a, b = np.full(shape, 40), np.full(shape, 37)
        a[:, :, W // 3:], b[:, :, W // 3 + 1:] = 220, 217
    elif kind == "anticorrelated":
        a = g.integers(0, 256, shape)
        b = 255 - a
    else:
        raise ValueError(kind)
    return a.astype(np.uint8), b.astype(np.uint8)


def clip_means(a: np.ndarray, b: np.ndarray, scales: int) -> np.ndarray:
    """Two clips -> float64 (F, 3, scales, 2)."""
    return np.stack([frame_means(fa, fb, scales) for fa, fb in zip(a, b)])
