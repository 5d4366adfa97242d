"""The second caller of the same UNet / DDIM surface: the InferNet miner's denoising loop
(`InferNet/neurons/miner.py:516-586`) — batch 1, no classifier-free guidance, every intermediate latent z_t and
noise prediction eps_t recorded, because their fp16 BYTES are hashed into the Merkle leaves the validator later
re-checks (`miner.py:180-209`: leaf = sha256(t as 2 big-endian bytes + z bytes + eps bytes)).

Only the loop and the leaf hash are here (the denoising path and the exact bytes it commits to); the Merkle tree /
proof / network protocol around them are InferNet's own product and stay out of scope.  What matters for that
caller is bit-stability: the same inputs must give the same bytes on every run — all kernels on this path use
fixed-order reductions (tests/test_miner_gpu.py runs the loop twice and compares hashes).
"""
from __future__ import annotations

import hashlib
from typing import Dict, List

import torch

from ._lib import VdxError


def leaf_hash(t: int, z: torch.Tensor, eps: torch.Tensor) -> bytes:
    """miner.py:196-203 — sha256 over (timestep as 2 big-endian bytes, z fp16 bytes, eps fp16 bytes)."""
    return hashlib.sha256(int(t).to_bytes(2, "big") + z.cpu().numpy().tobytes() + eps.cpu().numpy().tobytes()).digest()


def seeded_latent(seed: int, shape, device, frames=None) -> torch.Tensor:
    """The start latent `denoise_with_trace` takes, from the validator's 64-bit seed (`proof.py:11-15`) alone: the base stream of
    the portable generator "philox4x32-10/v1" (vdx/noise.py) over the logical (1, C, T, h, w) `shape`, fp16, unscaled (the
    miner's DDIM has init_noise_sigma 1).  `frames` = (t0, t1): only the frames [t0, t1) of it, (1, C, t1 - t0, h, w), with the
    bits the whole latent has there; a validator's frame-0 spot check regenerates `frames=(0, 1)` without the clip."""
    from . import noise, ops
    shape = tuple(shape)
    if len(shape) != 5 or shape[0] != 1:
        raise VdxError(f"seeded_latent: shape must be (1, C, T, h, w), got {shape}")
    box = None
    if frames is not None:
        if (not isinstance(frames, (tuple, list)) or len(frames) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in frames)
                or not 0 <= frames[0] < frames[1] <= shape[2]):
            raise ValueError(f"seeded_latent: frames must be (t0, t1) with 0 <= t0 < t1 <= {shape[2]}, got {frames!r}")
        t0, t1 = frames
        box = ((0, 0, t0, 0, 0), (1, shape[1], t1 - t0, shape[3], shape[4]))
    return ops.philox_normal(shape, noise.check_seed(seed), noise.STREAM_BASE, box=box, device=device)


@torch.no_grad()
def denoise_with_trace(unet, scheduler, z: torch.Tensor, encoder_hidden_states: torch.Tensor, num_steps: int) -> Dict:
    """miner.py:516-586.  z (1,4,T,h,w) fp16 initial noise on the GPU; encoder_hidden_states (1,77,D) fp16.
    Returns {"z": final latent, "latents": [z_t], "noise_preds": [eps_t], "timesteps": [t], "alphas": [abar_t]}."""
    if z.dim() != 5 or z.shape[0] != 1 or z.dtype != torch.float16:
        raise VdxError(f"denoise_with_trace: z must be (1,C,T,h,w) fp16, got {tuple(z.shape)} {z.dtype}")
    scheduler.set_timesteps(num_steps, device=z.device)
    if hasattr(scheduler, "reset"):         # a multistep scheduler starts every trace without history
        scheduler.reset()
    timesteps: List[int] = list(scheduler._host_timesteps)
    if timesteps and not 0 <= max(timesteps) < len(scheduler.alphas_cumprod):
        raise ValueError(f"denoise_with_trace: timestep {max(timesteps)} of this {num_steps}-step schedule is outside the "
                         f"{len(scheduler.alphas_cumprod)} training steps")
    alphas = [float(scheduler.alphas_cumprod[t]) for t in timesteps]                     # :534-544
    latents, noise_preds = [], []
    z = z.contiguous()
    for t in timesteps:                                                                   # :573-586
        latents.append(z)
        eps = unet(z, t, encoder_hidden_states=encoder_hidden_states).sample
        noise_preds.append(eps)
        z = scheduler.step(eps, t, z).prev_sample
    return {"z": z, "latents": latents, "noise_preds": noise_preds, "timesteps": timesteps, "alphas": alphas}
