"""The temporal filter of vdx/deflicker.py (csrc/deflicker.hip), stated once in float64 numpy: the tests pin the kernel to this
expression (tests/test_deflicker_gpu.py).  The reference has no counterpart, and no external tool is meant.

uint8 RGB frames I[t] (F, H, W, 3); flows fab[t] (frame t -> t+1) and fba[t] (frame t+1 -> t), float32 (F-1, H, W, 2) = (dx, dy),
or with `loop` (F, H, W, 2), entry F-1 being the pair (F-1, 0).  For frame t, its neighbours n = t-1 then t+1 (those inside the
clip; with `loop` both, mod F), f = fba[t-1] towards t-1 and fab[t] towards t+1, at pixel q = (column, row):

    c     = q + f(q), each coordinate clamped by fmin(fmax(., 0), hi): NaN -> 0, +inf -> hi
    Wn(q) = bilinear sample of I[n] at c: (v00 (1-fx) + v01 fx) (1-fy) + (v10 (1-fx) + v11 fx) fy, neighbours clamped to the frame
    en(q) = the sum over R, G, B of (I[t](q) - Wn(q))^2
    dn(p) = (the sum of en over the 3 x 3 patch around p, row-major, border replicate) / 27
    wn(p) = 1 / (1 + dn(p) / sigma^2)
    out(p) = (I[t](p) + strength (w- W-(p) + w+ W+(p))) / (1 + strength (w- + w+));  byte = floor(out + 0.5) clamped to [0, 255]

A further pass filters the pass before with the same flows."""
import numpy as np


def warp(img, flow):
    """img (H, W, 3) float64 sampled at q + flow(q), flow float32 (H, W, 2) -> (H, W, 3)."""
    H, W = img.shape[:2]
    ys, xs = np.mgrid[:H, :W]
    with np.errstate(all="ignore"):
        cx = np.fmin(np.fmax(xs + flow[..., 0].astype(np.float64), 0.0), float(W - 1))
        cy = np.fmin(np.fmax(ys + flow[..., 1].astype(np.float64), 0.0), float(H - 1))
    flx, fly = np.floor(cx), np.floor(cy)
    x0, y0 = np.clip(flx.astype(np.int64), 0, W - 1), np.clip(fly.astype(np.int64), 0, H - 1)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (cx - flx)[..., None], (cy - fly)[..., None]
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def patch_mean(e):
    """(H, W) -> the mean over the 3 x 3 patch (border replicate) and the 3 channels whose squares `e` already sums."""
    H, W = e.shape
    p = np.pad(e, 1, mode="edge")
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) / 27.0


def deflicker_pass(frames, fab, fba, strength, sigma, loop=False):
    """One pass -> uint8 (F, H, W, 3)."""
    frames = np.asarray(frames)
    F = len(frames)
    out = np.empty_like(frames)
    for t in range(F):
        I = frames[t].astype(np.float64)
        acc, wsum = np.zeros_like(I), np.zeros(I.shape[:2])
        for n, flow in ((t - 1, fba[(t - 1) % F] if loop or t > 0 else None), (t + 1, fab[t] if loop or t < F - 1 else None)):
            if flow is None:
                continue
            Wn = warp(frames[n % F].astype(np.float64), np.asarray(flow, np.float32))
            w = 1.0 / (1.0 + patch_mean(((I - Wn) ** 2).sum(-1)) / (float(sigma) * float(sigma)))
            acc, wsum = acc + w[..., None] * Wn, wsum + w
        num, den = I + strength * acc, 1.0 + strength * wsum
        out[t] = np.clip(np.floor(num / den[..., None] + 0.5), 0, 255).astype(np.uint8)
    return out


def deflicker_clip(frames, fab, fba, strength, sigma, passes=1, loop=False):
    for _ in range(passes):
        frames = deflicker_pass(frames, fab, fba, strength, sigma, loop)
    return frames
