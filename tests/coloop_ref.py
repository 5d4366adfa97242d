"""Torch-CPU restatement of the ring-window kernels (csrc/codenoise.hip, its RING flag): the yardstick of tests/test_coloop_host.py and
tests/test_coloop_gpu.py.  It does not import the product's kernels.

A window (s, L) holds the frames (s + arange(L)) % T of the clip.  Per element (c, t, p), over the windows k = 0..K-1 IN
ASCENDING ORDER that hold frame t (f = (t - s_k) mod T < L_k):
    U  = sum_k wn[k][t] * fp32(u_k[f])        Cc = sum_k wn[k][t] * fp32(c_k[f])
every product one fp32 operation and every add another, the sum STARTING with the first product; then u = fp16(U), c = fp16(Cc)
and the chains tests/codenoise_ref.py and tests/dpm_ref.py already restate (imported, not copied).  All of it is correctly
rounded fp32 arithmetic in a stated order, so the kernels' fp16 bits EQUAL these: nothing is measured.
"""
import numpy as np
import torch

import codenoise_ref as R
import dpm_ref


def ring_frames(s, L, T):
    """The frames of the ring window (s, L) of a clip of T, in the window's order."""
    return (s + torch.arange(L)) % T


def take(z, s, L):
    """z (..., C, T, h, w) with T at dim 2 -> the window's frames, by index_select."""
    return z.index_select(2, ring_frames(s, L, z.shape[2]))


def fuse(windows, table, wn, shape):
    """windows[k]: fp16 (2,C,L_k,h,w) = [u; c]; table[k] = (s_k, L_k), a ring window; wn: fp32 (K,T) -> eps2 fp16 (2,C,T,h,w),
    the fused [u; c] of the whole clip.  A frame in no window is an error."""
    _, C, T, h, w = shape
    out = torch.empty((2, C, T, h, w), dtype=torch.float16)
    wn = wn.float()
    for t in range(T):
        acc = None
        for k, (s, L) in enumerate(table):
            f = (t - s) % T
            if f >= L:
                continue
            prod = wn[k, t] * windows[k][:, :, f].float()                  # fp32 product, rounded
            acc = prod if acc is None else acc + prod                      # fp32 add, rounded
        if acc is None:
            raise ValueError(f"frame {t} is in no window")
        out[:, :, t] = acc.half()
    return out


def coloop_ddim(z, windows, table, wn, gs, coeffs):
    """The whole-clip DDIM step over ring windows: z fp16 (1,C,T,h,w) -> z' fp16."""
    return R.ddim_chain(dpm_ref.cfg_combine(fuse(windows, table, wn, z.shape), gs), z, coeffs)


def coloop_dpm(z, windows, table, wn, gs, k, x0_prev=None):
    """The whole-clip DPM-Solver++ step over ring windows from tests/dpm_ref.py's scalars `k` -> (z' fp16, x0 fp16)."""
    return dpm_ref.step(dpm_ref.cfg_combine(fuse(windows, table, wn, z.shape), gs), z, x0_prev, k)


def cfg_input_loop(z, ctx, weight, s, L):
    """cat([z[:, :, (s + arange(L)) % T]]*2) (+ fp16(weight * ctx), then fp16(x + that)) -> fp16 (2,C,L,h,w)."""
    x = take(z, s, L)
    if ctx is not None:
        t = R.r16(ctx.float() * float(np.float32(weight)))
        x = R.r16(x.float() + t).half()
    return torch.cat([x, x], dim=0).contiguous()
