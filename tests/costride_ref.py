"""Torch-CPU restatement of the strided-window kernels (csrc/codenoise.hip, its `costride_tab`): the yardstick of
tests/test_costride_host.py and tests/test_costride_gpu.py.  It does not import the product's kernels.

A window (s, L, d) holds the frames s + d * arange(L) of the clip.  Per element (c, t, p), over the windows k = 0..K-1 IN
ASCENDING ORDER that hold frame t (q = t - s_k >= 0, q % d_k == 0, f = q / d_k < L_k):
    U  = sum_k wn[k][t] * fp32(u_k[f])        Cc = sum_k wn[k][t] * fp32(c_k[f])
every product one fp32 operation and every add another, the sum STARTING with the first product; then u = fp16(U), c = fp16(Cc)
and the chains tests/codenoise_ref.py and tests/dpm_ref.py already restate (imported, not copied).  All of it is correctly
rounded fp32 arithmetic in a stated order, so the kernels' fp16 bits EQUAL these: nothing is measured.  With every d = 1 the
membership rule is s <= t < s + L and the functions below are tests/codenoise_ref.py's.
"""
import numpy as np
import torch

import codenoise_ref as R
import dpm_ref


def stride_frames(s, L, d):
    """The frames of the strided window (s, L, d), in the window's order."""
    return s + d * torch.arange(L)


def take(z, s, L, d):
    """z (..., C, T, h, w) with T at dim 2 -> the window's frames, by index_select."""
    return z.index_select(2, stride_frames(s, L, d))


def fuse(windows, table, wn, shape):
    """windows[k]: fp16 (2,C,L_k,h,w) = [u; c]; table[k] = (s_k, L_k, d_k); wn: fp32 (K,T) -> eps2 fp16 (2,C,T,h,w), the fused
    [u; c] of the whole clip.  A frame in no window is an error."""
    _, C, T, h, w = shape
    out = torch.empty((2, C, T, h, w), dtype=torch.float16)
    wn = wn.float()
    for t in range(T):
        acc = None
        for k, (s, L, d) in enumerate(table):
            q = t - s
            if q < 0 or q % d or q // d >= L:
                continue
            prod = wn[k, t] * windows[k][:, :, q // d].float()             # fp32 product, rounded
            acc = prod if acc is None else acc + prod                      # fp32 add, rounded
        if acc is None:
            raise ValueError(f"frame {t} is in no window")
        out[:, :, t] = acc.half()
    return out


def costride_ddim(z, windows, table, wn, gs, coeffs):
    """The whole-clip DDIM step over strided windows: z fp16 (1,C,T,h,w) -> z' fp16."""
    return R.ddim_chain(dpm_ref.cfg_combine(fuse(windows, table, wn, z.shape), gs), z, coeffs)


def costride_dpm(z, windows, table, wn, gs, k, x0_prev=None):
    """The whole-clip DPM-Solver++ step over strided windows from tests/dpm_ref.py's scalars `k` -> (z' fp16, x0 fp16)."""
    return dpm_ref.step(dpm_ref.cfg_combine(fuse(windows, table, wn, z.shape), gs), z, x0_prev, k)


def cfg_input_stride(z, ctx, weight, s, L, d):
    """cat([z[:, :, s + d * arange(L)]]*2) (+ fp16(weight * ctx), then fp16(x + that)) -> fp16 (2,C,L,h,w)."""
    x = take(z, s, L, d)
    if ctx is not None:
        t = R.r16(ctx.float() * float(np.float32(weight)))
        x = R.r16(x.float() + t).half()
    return torch.cat([x, x], dim=0).contiguous()
