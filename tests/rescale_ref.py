"""Torch-CPU restatement of classifier-free guidance with CFG rescale (Lin et al. 2023, section 3.4; diffusers'
`rescale_noise_cfg`) as csrc/rescale.hip computes it: the yardstick of tests/test_rescale_host.py and tests/test_rescale_gpu.py.
It does not import the product's kernels.  Over ONE sample (what one scheduler step advances), eps2 = [u; c] fp16:

    g    = fp16(u + fp16(gs * fp16(c - u)))                                   tests/dpm_ref.py `cfg_combine`
    sd_c = fp16(sqrt(var(c))),  sd_g = fp16(sqrt(var(g)))                     var: unbiased (divisor N - 1), float64, TWO passes
                                                                              (mean, then squared deviations); ONE rounding to fp16
    r    = fp16(fp32(sd_c) / fp32(sd_g))
    g'   = fp16(fp16(phi * fp16(g * r)) + fp16(phi1 * g))                     phi = fp32(rescale), phi1 = fp32(1.0 - rescale)

and g' goes where g went (DDIM: tests/codenoise_ref.py `ddim_chain`; DPM-Solver++: tests/dpm_ref.py `step`).  The kernels form
the variance from fp64 SUMS instead ((N*S2 - S1*S1) / (N*(N-1))): the two float64 values differ in their last bits and round to
the same fp16 unless one lands on a rounding tie.  Everything after `r` is correctly rounded fp32 arithmetic in a stated order:
`rescale_with_r` takes r as an input, so that part is pinned bit for bit whatever the reduction did.
"""
import numpy as np
import torch

import codenoise_ref
import dpm_ref

r16 = dpm_ref.r16


def f32(v):
    """A Python double rounded once to fp32, as a Python float."""
    return float(np.float32(v))


def factors(rescale):
    """(phi, phi1): fp32(rescale) and fp32(1.0 - rescale), the subtraction in Python double."""
    return f32(float(rescale)), f32(1.0 - float(rescale))


def to_f16(x64):
    """float64 -> fp16 in ONE rounding (numpy converts directly; torch goes through fp32) -> numpy float16 scalar."""
    with np.errstate(all="ignore"):
        return np.float64(x64).astype(np.float16)


def std64(x):
    """Unbiased standard deviation of the fp16 tensor x over all its elements in float64, two passes -> Python float (NaN for
    one element, as 0/0 is)."""
    v = x.double().reshape(-1)
    n = v.numel()
    mean = v.sum() / n
    with np.errstate(all="ignore"):
        var = np.float64(float(((v - mean) ** 2).sum())) / np.float64(n - 1)
        return float(np.sqrt(var))


def sums64(eps2, gs):
    """[sum c, sum c*c, sum g, sum g*g] in float64 and the sums of the terms' magnitudes (the error bound's scale)."""
    c = eps2[1:].double().reshape(-1)
    g = dpm_ref.cfg_combine(eps2, gs).double().reshape(-1)
    terms = (c, c * c, g, g * g)
    return [float(t.sum()) for t in terms], [float(t.abs().sum()) for t in terms]


def stats(eps2, gs):
    """-> (sd_c, sd_g, r) as numpy float16 scalars."""
    sd_c, sd_g = to_f16(std64(eps2[1:])), to_f16(std64(dpm_ref.cfg_combine(eps2, gs)))
    with np.errstate(all="ignore"):
        r = (np.float32(sd_c) / np.float32(sd_g)).astype(np.float16)
    return sd_c, sd_g, r


def rescale_with_r(eps2, gs, r, rescale):
    """g' fp16 from eps2 fp16 (2,...), the fp16-valued scalar r and `rescale` (the Python number of the public interface)."""
    phi, phi1 = factors(rescale)
    g = dpm_ref.cfg_combine(eps2, gs).float()
    h1 = r16(g * float(np.float32(r)))
    return r16(r16(phi * h1) + r16(phi1 * g)).half()


def rescaled(eps2, gs, rescale):
    return rescale_with_r(eps2, gs, stats(eps2, gs)[2], rescale)


def ddim_step(eps2, x, gs, rescale, coeffs, r=None):
    """The rescaled fused CFG + DDIM step -> x' fp16.  `r`: the scalar to use instead of the restatement's own."""
    g2 = rescaled(eps2, gs, rescale) if r is None else rescale_with_r(eps2, gs, r, rescale)
    return codenoise_ref.ddim_chain(g2, x, coeffs)


def dpm_step(eps2, x, x0_prev, gs, rescale, k, r=None):
    """The rescaled fused CFG + DPM-Solver++ step from tests/dpm_ref.py's scalars `k` -> (x' fp16, x0 fp16)."""
    g2 = rescaled(eps2, gs, rescale) if r is None else rescale_with_r(eps2, gs, r, rescale)
    return dpm_ref.step(g2, x, x0_prev, k)


def rescale_f64(eps2, gs, rescale):
    """The expression before any rounding of its own (float64 throughout, from the fp16 g and c): the property test's subject."""
    c = eps2[1:].double()
    g = dpm_ref.cfg_combine(eps2, gs).double()
    r = c.std() / g.std()
    return rescale * (g * r) + (1.0 - rescale) * g
