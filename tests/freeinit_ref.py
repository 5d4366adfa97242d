"""FreeInit's filter and frequency mix restated in float64 with torch.fft on the CPU (not a test): the definition
vdx/freeinit.py's docstring gives, written from the published method (Wu et al. 2023) and diffusers' free_init_utils, in the
SHIFT form, literally.  The kernels (csrc/freeinit.hip) run the difference form eta + Re IDFT3(ifftshift(H) DFT3(z - eta)), so
this is an independent route to the same numbers."""
import math

import numpy as np
import torch

DIMS = (-3, -2, -1)


def lowpass_filter(shape, method="butterworth", d_s=0.25, d_t=0.25, order=4):
    """H over (T, h, w) in fftshift-ed index coordinates, float64, point by point as the definition reads."""
    T, h, w = shape
    H = torch.zeros((T, h, w), dtype=torch.float64)
    if d_s == 0 or d_t == 0:
        return H
    for t in range(T):
        for y in range(h):
            for x in range(w):
                d2 = ((d_s / d_t) * (2 * t / T - 1)) ** 2 + (2 * y / h - 1) ** 2 + (2 * x / w - 1) ** 2
                if method == "butterworth":
                    H[t, y, x] = 1 / (1 + (d2 / d_s ** 2) ** order)
                elif method == "gaussian":
                    H[t, y, x] = math.exp(-d2 / (2 * d_s ** 2))
                elif method == "ideal":
                    H[t, y, x] = 1.0 if d2 <= d_s ** 2 else 0.0
                else:
                    raise ValueError(method)
    return H


def mix_complex(z_T, eta, H):
    """ifftn(ifftshift(fftshift(fftn(z_T)) H + fftshift(fftn(eta)) (1 - H))) over the last three axes, complex128."""
    z, e, H = z_T.double(), eta.double(), H.double()
    zf = torch.fft.fftshift(torch.fft.fftn(z, dim=DIMS), dim=DIMS)
    ef = torch.fft.fftshift(torch.fft.fftn(e, dim=DIMS), dim=DIMS)
    return torch.fft.ifftn(torch.fft.ifftshift(zf * H + ef * (1 - H), dim=DIMS), dim=DIMS)


def mix(z_T, eta, H):
    """The definition's real part, float64."""
    return mix_complex(z_T, eta, H).real


def mix_difference_form(z_T, eta, H):
    """eta + Re IDFT3(ifftshift(H) . DFT3(z_T - eta)), float64: what the kernels compute."""
    z, e = z_T.double(), eta.double()
    Hs = torch.fft.ifftshift(H.double(), dim=DIMS)
    return e + torch.fft.ifftn(Hs * torch.fft.fftn(z - e, dim=DIMS), dim=DIMS).real


def fp16_ulp(x16):
    """The spacing of fp16 at |x| (the subnormal spacing 2^-24 below 2^-14), float64."""
    a = x16.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)


def compare_fp16(got16, want64):
    """-> (largest |got - fp16(want)| in ulps of fp16(want), share of elements that differ at all)."""
    want16 = torch.from_numpy(want64.numpy().astype(np.float16))          # numpy rounds float64 to fp16 once, not through fp32
    d = (got16.double() - want16.double()).abs()
    return float((d / fp16_ulp(want16)).max()), float((got16 != want16).double().mean())
