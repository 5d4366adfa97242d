"""Torch-CPU restatement of the co-denoising kernels (csrc/codenoise.hip): the yardstick of tests/test_codenoise_host.py and
tests/test_codenoise_gpu.py.  It does not import the product's kernels.

Per element (c, t, p), over the windows k = 0..K-1 IN ASCENDING ORDER that hold frame t (s_k <= t < s_k + L_k):
    U  = sum_k wn[k][t] * fp32(u_k)        Cc = sum_k wn[k][t] * fp32(c_k)
Every product is one fp32 operation and every add another (torch's fp32 `*` and `+` on the CPU are correctly rounded, and two
tensor operations cannot contract into an fma); the sum STARTS with the first product, nothing is added to a zero.  Then
u = fp16(U), c = fp16(Cc), and from there the plain fused steps' chains: u + gs*(c - u) with fp16 after every tensor
operation, then DDIM (`ddim_chain`, the expression of oracle/ddim_ref.py `step_gpu_rules` in coefficient form) or DPM-Solver++
(tests/dpm_ref.py `step`).  All of it is correctly rounded fp32 arithmetic in a stated order, so the kernels' fp16 bits EQUAL
these: nothing is measured.
"""
import numpy as np
import torch

import dpm_ref


def r16(x):
    return x.half().float()


def fuse(windows, table, wn, shape):
    """windows[k]: fp16 (2,C,L_k,h,w) = [u; c]; table[k] = (s_k, L_k); wn: fp32 (K,T) -> eps2 fp16 (2,C,T,h,w), the fused
    [u; c] of the whole clip.  A frame in no window is an error."""
    _, C, T, h, w = shape
    out = torch.empty((2, C, T, h, w), dtype=torch.float16)
    wn = wn.float()
    for t in range(T):
        acc = None
        for k, (s, L) in enumerate(table):
            if not s <= t < s + L:
                continue
            prod = wn[k, t] * windows[k][:, :, t - s].float()              # fp32 product, rounded
            acc = prod if acc is None else acc + prod                      # fp32 add, rounded
        if acc is None:
            raise ValueError(f"frame {t} is in no window")
        out[:, :, t] = acc.half()
    return out


def inv32(x):
    """1.0f / x in fp32, as the C entry point forms 1/sqrt(a_t)."""
    return float(np.float32(1.0) / np.float32(x))


def ddim_chain(eps, x, coeffs):
    """DDIM (eta 0) on fp16 tensors from (sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)) as fp32-valued floats: fp16
    after every tensor operation, `/ sqrt(a_t)` as `* (1/sqrt(a_t))` -> x' fp16."""
    s1, sa, sp, s1p = (float(np.float32(c)) for c in coeffs)
    e, x = eps.float(), x.float()
    x0 = r16(r16(x - r16(s1 * e)) * inv32(sa))
    return r16(r16(sp * x0) + r16(s1p * e)).half()


def cofuse_ddim(z, windows, table, wn, gs, coeffs):
    """The whole-clip DDIM step: z fp16 (1,C,T,h,w) -> z' fp16."""
    eps2 = fuse(windows, table, wn, z.shape)
    return ddim_chain(dpm_ref.cfg_combine(eps2, gs), z, coeffs)


def cofuse_dpm(z, windows, table, wn, gs, k, x0_prev=None):
    """The whole-clip DPM-Solver++ step from tests/dpm_ref.py's scalars `k` -> (z' fp16, x0 fp16)."""
    eps2 = fuse(windows, table, wn, z.shape)
    return dpm_ref.step(dpm_ref.cfg_combine(eps2, gs), z, x0_prev, k)


def cfg_input_window(z, ctx, weight, s, e):
    """cat([z[:, :, s:e]]*2) (+ fp16(weight * ctx), then fp16(x + that)) -> fp16 (2,C,e-s,h,w)."""
    x = z[:, :, s:e]
    if ctx is not None:
        t = r16(ctx.float() * float(np.float32(weight)))
        x = r16(x.float() + t).half()
    return torch.cat([x, x], dim=0).contiguous()
