"""Torch-CPU restatement of the tiled co-denoising kernels (csrc/cotile.hip): the yardstick of tests/test_cotile_host.py and
tests/test_cotile_gpu.py.  It does not import the product's kernels.

A window is (time window kt, row band ky, column band kx); its UNet output is fp16 (2,C,L_kt,th,tw) = [u; c] for frames
[s_kt, s_kt + L_kt), rows [y0_ky, y0_ky + th), columns [x0_kx, x0_kx + tw).  Per element (c, t, y, x), over the windows that hold
it IN ASCENDING (kt, ky, kx):
    w  = fp32(fp32(wn[kt][t] * wyn[ky][y]) * wxn[kx][x])
    U  = sum w * fp32(u_k)        Cc = sum w * fp32(c_k)
Every product is one fp32 operation and every add another (torch's fp32 `*` and `+` on the CPU are correctly rounded, and two
tensor operations cannot contract into an fma); the sum STARTS with the first product.  Then u = fp16(U), c = fp16(Cc) and the
chains of tests/codenoise_ref.py, unchanged.  With one spatial tile both spatial weights are 1.0f, w = wn[kt][t], and every line
reduces to tests/codenoise_ref.py's (tests/test_cotile_host.py checks that on the CPU).
"""
import numpy as np
import torch

import codenoise_ref as R
import dpm_ref


def fuse(windows, table, wn, ys, xs, th, tw, wyn, wxn, shape):
    """windows[kt][ky][kx]: fp16 (2,C,L_kt,th,tw); table[kt] = (s_kt, L_kt); wn fp32 (Kt,T), wyn fp32 (ny,H), wxn fp32 (nx,W)
    -> eps2 fp16 (2,C,T,H,W), the fused [u; c] of the whole clip.  A cell in no window is an error."""
    _, C, T, H, W = shape
    wn, wyn, wxn = wn.float(), wyn.float(), wxn.float()
    acc = torch.zeros((2, C, T, H, W), dtype=torch.float32)
    seen = torch.zeros((T, H, W), dtype=torch.bool)
    for kt, (s, L) in enumerate(table):
        for ky, y0 in enumerate(ys):
            wty = wn[kt, s:s + L].view(L, 1, 1) * wyn[ky, y0:y0 + th].view(1, th, 1)            # fp32 product, rounded
            for kx, x0 in enumerate(xs):
                w = wty * wxn[kx, x0:x0 + tw].view(1, 1, tw)                                    # fp32 product, rounded
                prod = w * windows[kt][ky][kx].float()                                          # fp32 product, rounded
                box = (slice(None), slice(None), slice(s, s + L), slice(y0, y0 + th), slice(x0, x0 + tw))
                first = ~seen[box[2:]]
                acc[box] = torch.where(first, prod, acc[box] + prod)                            # fp32 add, rounded; none onto a zero
                seen[box[2:]] = True
    if not bool(seen.all()):
        raise ValueError(f"cell {tuple(int(i) for i in (~seen).nonzero()[0])} is in no window")
    return acc.half()


def cotile_ddim(z, windows, table, wn, ys, xs, th, tw, wyn, wxn, gs, coeffs):
    """The whole-clip DDIM step: z fp16 (1,C,T,H,W) -> z' fp16."""
    eps2 = fuse(windows, table, wn, ys, xs, th, tw, wyn, wxn, z.shape)
    return R.ddim_chain(dpm_ref.cfg_combine(eps2, gs), z, coeffs)


def cotile_dpm(z, windows, table, wn, ys, xs, th, tw, wyn, wxn, gs, k, x0_prev=None):
    """The whole-clip DPM-Solver++ step from tests/dpm_ref.py's scalars `k` -> (z' fp16, x0 fp16)."""
    eps2 = fuse(windows, table, wn, ys, xs, th, tw, wyn, wxn, z.shape)
    return dpm_ref.step(dpm_ref.cfg_combine(eps2, gs), z, x0_prev, k)


def cfg_input_tile(z, ctx, weight, s, e, y0, th, x0, tw):
    """cat([z[:, :, s:e, y0:y0+th, x0:x0+tw]]*2) (+ fp16(weight * ctx crop), then fp16(x + that)) -> fp16 (2,C,e-s,th,tw)."""
    x = z[:, :, s:e, y0:y0 + th, x0:x0 + tw]
    if ctx is not None:
        t = R.r16(ctx[:, :, :, y0:y0 + th, x0:x0 + tw].float() * float(np.float32(weight)))
        x = R.r16(x.float() + t).half()
    return torch.cat([x, x], dim=0).contiguous()
