"""FreeLong restated in float64 (no test of its own): the spectrally blended temporal attention of include/vdx.h
`vdx_temporal_attn_blend_f16`, and the blend matrix written out in un-shifted DFT coordinates with numpy.fft."""
import numpy as np
import torch


def temporal_gain(F, method, d_t, order=4):
    """g[k] for the un-shifted DFT index k.  `freeinit.lowpass_filter` evaluates its temporal coordinate at the fftshift-ed
    index i as 2 i / F - 1; fftshift puts un-shifted index k at i = (k + F // 2) mod F, so k's coordinate is
    2 ((k + F // 2) mod F) / F - 1: 0 at k = 0 for even F, -1 / F for odd F (the filter is not Hermitian there)."""
    if d_t == 0:
        return np.zeros(F)
    x2 = np.array([((2.0 * ((k + F // 2) % F) / F - 1.0) / d_t) ** 2 for k in range(F)])
    if method == "gaussian":
        return np.exp(-x2 / 2.0)
    if method == "butterworth":
        return 1.0 / (1.0 + x2 ** order)
    return (x2 <= 1.0).astype(np.float64)


def blend_matrix(F, method, d_t, order=4):
    """Lp = Re(IDFT diag(g) DFT): column s is the real part of the filtered unit impulse at s."""
    g = temporal_gain(F, method, d_t, order)
    return torch.from_numpy(np.fft.ifft(g[:, None] * np.fft.fft(np.eye(F), axis=0), axis=0).real.copy())


def blended_attention(q, k, v, scale, r, lp):
    """q, k, v (..., F, d) -> (..., F, d) float64: Zl + Lp (Zg - Zl), Zg over all keys, Zl inside the band |t - j| <= r."""
    q, k, v = q.double(), k.double(), v.double()
    F = q.shape[-2]
    s = scale * q @ k.transpose(-1, -2)
    t = torch.arange(F)
    band = (t[:, None] - t[None, :]).abs() <= r
    zg = torch.softmax(s, dim=-1) @ v
    zl = torch.softmax(s.masked_fill(~band, float("-inf")), dim=-1) @ v
    return zl + lp.double() @ (zg - zl)
