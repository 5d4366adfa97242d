"""FreeInit noise re-initialisation (Wu et al. 2023, "FreeInit: Bridging Initialization Gap in Video Diffusion Models";
diffusers' `FreeInitMixin.enable_free_init`) on libvdx_hip.so.

The reference has nothing of the kind: it samples once from white noise (fsdp_chunked_coherent.py:180-182).  A text-to-video
UNet is trained on noised videos whose low temporal frequencies still carry signal at t = 999; at inference it starts from
white noise.  FreeInit samples, noises the result back to t = 999 with the SAME initial noise, keeps the low spatio-temporal
frequencies of that latent, takes the high ones from fresh noise, and samples again.  In the chunked job the blended whole-clip
latent is what gets re-noised and the new start is again ONE tensor for the whole clip that every window slices, so overlapping
frames still start identical (vdx/pipeline.py, `DiffuserConfig.free_init_iters`, `--free_init N`).

Definition (tests/freeinit_ref.py states it in float64 with torch.fft).  The filter over a latent of extent (T, h, w) with stop
frequencies d_s (spatial) and d_t (temporal), in fftshift-ed index coordinates t in [0, T), y in [0, h), x in [0, w):
  d2 = ((d_s / d_t) (2 t / T - 1))^2 + (2 y / h - 1)^2 + (2 x / w - 1)^2
  butterworth (order n, default 4)   H = 1 / (1 + (d2 / d_s^2)^n)
  gaussian                           H = exp(-d2 / (2 d_s^2))
  ideal                              H = 1 if d2 <= d_s^2 else 0
  H = 0 everywhere when d_s == 0 or d_t == 0.  Defaults (diffusers'): butterworth, order 4, d_s = d_t = 0.25, 3 iterations.
The mix over the last three axes, z_T and eta taken to fp32 first:
  mix(z_T, eta, H) = Re ifftn(ifftshift(fftshift(fftn(z_T)) H + fftshift(fftn(eta)) (1 - H)))
(for odd extents H is not Hermitian and the discarded imaginary part is not small: the real part is part of the definition).
One re-initialisation, between iteration i - 1 and iteration i >= 1 of a job:
  z_T   = scheduler.add_noise(fp16(blended latent of iteration i - 1), base noise, num_train_timesteps - 1)
  eta   = fp32 N(0, 1) of the same shape, seeded by i (`pipeline.iteration_noise`)
  start of iteration i = fp16(mix(z_T, eta, H))
What is pinned: the kernels (csrc/freeinit.hip) against that restatement (tests/test_freeinit_gpu.py,
profiles/freeinit_parity.txt).  What is not: the restatement against diffusers (not installed where it was written): restated
from the published definition, not pinned against an external implementation.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ._lib import VdxError

METHODS = ("butterworth", "gaussian", "ideal")
DEFAULT_METHOD, DEFAULT_STOP, DEFAULT_ORDER, DEFAULT_ITERS = "butterworth", 0.25, 4, 3


def check_filter_args(method: str, d_s: float, d_t: float, order: int) -> None:
    """`ValueError` for an unknown method, a negative (or non-finite) stop frequency or a non-positive order."""
    if method not in METHODS:
        raise ValueError(f"free_init: unknown filter {method!r}: expected one of {METHODS}")
    for name, v in (("d_s", d_s), ("d_t", d_t)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) or v < 0:
            raise ValueError(f"free_init: stop frequency {name} must be a finite number >= 0, got {v!r}")
    if isinstance(order, bool) or not isinstance(order, int) or order < 1:
        raise ValueError(f"free_init: the filter order must be a positive integer, got {order!r}")


def lowpass_filter(shape: Sequence[int], method: str = DEFAULT_METHOD, d_s: float = DEFAULT_STOP, d_t: float = DEFAULT_STOP,
                   order: int = DEFAULT_ORDER) -> torch.Tensor:
    """The low-pass table H of a (T, h, w) latent in fftshift-ed coordinates: fp32 (T, h, w) on the host, evaluated in float64."""
    check_filter_args(method, d_s, d_t, order)
    if len(shape) != 3 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in shape):
        raise ValueError(f"free_init: the filter's shape must be three positive integers (T, h, w), got {tuple(shape)}")
    T, h, w = (int(v) for v in shape)
    if d_s == 0 or d_t == 0:
        return torch.zeros((T, h, w), dtype=torch.float32)
    t = (float(d_s) / float(d_t)) * (2.0 * np.arange(T, dtype=np.float64) / T - 1.0)
    y = 2.0 * np.arange(h, dtype=np.float64) / h - 1.0
    x = 2.0 * np.arange(w, dtype=np.float64) / w - 1.0
    d2 = (t * t)[:, None, None] + (y * y)[None, :, None] + (x * x)[None, None, :]
    s2 = float(d_s) ** 2
    if method == "butterworth":
        H = 1.0 / (1.0 + (d2 / s2) ** order)
    elif method == "gaussian":
        H = np.exp(-d2 / (2.0 * s2))
    else:
        H = (d2 <= s2).astype(np.float64)
    return torch.from_numpy(H.astype(np.float32))


def freq_mix(z_T: torch.Tensor, eta: torch.Tensor, filt: torch.Tensor) -> torch.Tensor:
    """mix(z_T, eta, filt) on the GPU: z_T fp16 and eta fp32 (B, C, T, h, w) on one GPU, filt fp32 (T, h, w) (anywhere: a host
    table is uploaded) -> the fp16 start latent on that GPU.  `VdxError` for what the kernels do not take, before any launch."""
    from . import ops
    ops.freeinit_check_sizes(z_T.shape)
    if not torch.is_tensor(filt) or filt.dtype != torch.float32 or tuple(filt.shape) != tuple(z_T.shape[2:]):
        raise VdxError(f"freq_mix: the filter must be fp32 {tuple(z_T.shape[2:])}, got "
                       f"{getattr(filt, 'dtype', type(filt).__name__)} {tuple(getattr(filt, 'shape', ()))}")
    return ops.freeinit_mix(z_T.contiguous(), eta.contiguous(), filt.to(z_T.device).contiguous())


def reinit(z0: torch.Tensor, base_noise: torch.Tensor, scheduler, iteration: int, filt: torch.Tensor, noise_device=None, seed=None):
    """One whole re-initialisation: the blended latent `z0` (any float dtype, (B, C, T, h, w)) of iteration `iteration - 1` and
    the job's base noise (fp16, the same shape) -> the fp16 start latent of iteration `iteration` >= 1 (0 is the seed of the
    base noise itself).  `noise_device` and `seed` (the portable generator's, None: torch's stream) as in `pipeline.seeded_noise`."""
    from .pipeline import iteration_noise
    if isinstance(iteration, bool) or not isinstance(iteration, int) or iteration < 1:
        raise ValueError(f"free_init: reinit starts iteration 1 or later, got {iteration!r}")
    if z0.shape != base_noise.shape:
        raise VdxError(f"free_init: latent {tuple(z0.shape)} and base noise {tuple(base_noise.shape)} differ in shape")
    dev = base_noise.device
    z_T = scheduler.add_noise(z0.to(dev, torch.float16).contiguous(), base_noise, scheduler.config.num_train_timesteps - 1)
    eta = iteration_noise(tuple(z0.shape), iteration, dev, noise_device, **({"seed": seed} if seed is not None else {}))
    return freq_mix(z_T, eta, filt)
