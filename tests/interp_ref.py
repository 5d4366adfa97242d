"""The frame interpolation of vdx/interp.py (csrc/interp.hip), stated once in float64 numpy: the tests pin the kernel to this
expression (tests/test_interp_host.py, tests/test_interp_gpu.py).  The reference has no counterpart.

For uint8 RGB frames A, B (H, W, 3), flows Fab (A -> B) and Fba (B -> A), float32 (H, W, 2) = (dx, dy), a factor N and
k = 1 .. N-1, with t = k / N and a = (N - k) / N (two quotients of integers: (A, B, k) and (B, A, N - k) are then the same
arithmetic, which is the swap symmetry), at output pixel x = (column, row):

    gA = (t t) Fba(x) - (a t) Fab(x)          gB = (a a) Fab(x) - (a t) Fba(x)        Super SloMo's intermediate flows

and for each side (frame I with its own flow `own`, leaving I, and the flow `other` that comes back to it):

    a g with a non-finite component counts as 0;  p = x + g;  c = p clamped to [0, W-1] x [0, H-1]
    S  = bilinear sample of I at c: (v00 (1-fx) + v01 fx) (1-fy) + (v10 (1-fx) + v11 fx) fy, neighbours clamped to the frame
    cf = the same sample of `own` at c;  r = cf + the same sample of `other` at clamp(c + cf)
    v  = 1 / (1 + (rx rx + ry ry)), 0 when that sum is not finite;
         times 1e-6 when g was not finite or p lies outside [-0.5, W-0.5] x [-0.5, H-0.5]

    wA = a vA, wB = t vB; when wA + wB is not positive, wA = a and wB = t
    out = (wA SA + wB SB) / (wA + wB);  byte = floor(out + 0.5) clamped to [0, 255]

`clamp` is fmin(fmax(., 0), hi): a NaN becomes 0, +inf the upper end.  `dtype` evaluates the same expression in another float
type (float32: what the kernel computes in, without mul-add contraction)."""
import numpy as np


def _clamp(v, hi):
    return np.fmin(np.fmax(v, v.dtype.type(0)), v.dtype.type(hi))


def _taps(cx, cy, W, H):
    flx, fly = np.floor(cx), np.floor(cy)
    x0 = np.clip(flx.astype(np.int64), 0, W - 1)
    y0 = np.clip(fly.astype(np.int64), 0, H - 1)
    return x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1), cx - flx, cy - fly


def _sample(img, taps):
    """img (H, W, C) in the working type -> (H, W, C) sampled at the taps."""
    x0, x1, y0, y1, fx, fy = taps
    one = fx.dtype.type(1)
    fx, fy = fx[..., None], fy[..., None]
    gx, gy = one - fx, one - fy
    return (img[y0, x0] * gx + img[y0, x1] * fx) * gy + (img[y1, x0] * gx + img[y1, x1] * fx) * fy


def _side(img, own, other, g):
    """-> (S (H, W, 3), v (H, W)) of one side; img, own, other, g in the working type."""
    T = g.dtype.type
    H, W = img.shape[:2]
    with np.errstate(all="ignore"):
        fin = np.isfinite(g[..., 0]) & np.isfinite(g[..., 1])
        ys, xs = np.mgrid[:H, :W]
        px = xs.astype(T) + np.where(fin, g[..., 0], T(0))
        py = ys.astype(T) + np.where(fin, g[..., 1], T(0))
        inside = fin & (px >= T(-0.5)) & (px <= T(W) - T(0.5)) & (py >= T(-0.5)) & (py <= T(H) - T(0.5))
        cx, cy = _clamp(px, W - 1), _clamp(py, H - 1)
        taps = _taps(cx, cy, W, H)
        S = _sample(img, taps)
        cf = _sample(own, taps)
        back = _sample(other, _taps(_clamp(cx + cf[..., 0], W - 1), _clamp(cy + cf[..., 1], H - 1), W, H))
        r = cf + back
        n2 = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
        v = np.where(np.isfinite(n2), T(1) / (T(1) + n2), T(0))
        v = np.where(inside, v, v * T(1e-6))
    return S, v.astype(T)


def interp_pair(A, B, fab, fba, k, N, dtype=np.float64):
    """The frame at t = k / N between uint8 RGB A and B -> uint8 (H, W, 3)."""
    T = np.dtype(dtype).type
    A, B = np.asarray(A), np.asarray(B)
    fab, fba = np.asarray(fab, np.float32).astype(T), np.asarray(fba, np.float32).astype(T)
    t, a = T(k) / T(N), T(N - k) / T(N)
    tt, aa, at = t * t, a * a, a * t
    with np.errstate(all="ignore"):
        SA, vA = _side(A.astype(T), fab, fba, tt * fba - at * fab)
        SB, vB = _side(B.astype(T), fba, fab, aa * fab - at * fba)
        wA, wB = a * vA, t * vB
        dead = ~(wA + wB > T(0))
        wA, wB = np.where(dead, a, wA).astype(T), np.where(dead, t, wB).astype(T)
        out = (wA[..., None] * SA + wB[..., None] * SB) / (wA + wB)[..., None]
        return np.fmin(np.fmax(np.floor(out + T(0.5)), T(0)), T(255)).astype(np.uint8)


def interp_clip(frames, fab, fba, N, dtype=np.float64):
    """uint8 (F, H, W, 3), flows (F-1, H, W, 2) each -> uint8 ((F-1) N + 1, H, W, 3); frame i N is frame i."""
    frames = np.asarray(frames)
    out = []
    for i in range(len(frames) - 1):
        out.append(frames[i])
        out += [interp_pair(frames[i], frames[i + 1], fab[i], fba[i], k, N, dtype) for k in range(1, N)]
    out.append(frames[-1])
    return np.stack(out)


def blend_pair(A, B, k, N):
    """The plain blend a A + t B, rounded the same way: what the interpolation must beat on a moving texture."""
    t = k / N
    return np.clip(np.floor((1 - t) * np.asarray(A, np.float64) + t * np.asarray(B, np.float64) + 0.5), 0, 255).astype(np.uint8)
