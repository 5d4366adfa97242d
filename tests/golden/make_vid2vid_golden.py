"""Writes tests/golden/vid2vid_encoder_full.npz: the fp32 CPU encoder restatement (tests/vae_encoder_ref.py) at Stable-Diffusion
VAE widths on one seeded 576x1024 uint8 frame -> the posterior moments (8, 72, 128) as fp16 (mean 0..3, logvar 4..7).
Weights: vdx.weights.synthetic_vae_encoder_state_dict(VaeConfig.sd(), seed=8), fp16 values.  Frame:
numpy default_rng(2024).integers(0, 256, (576, 1024, 3), uint8).  Run from the repository root:
    python tests/golden/make_vid2vid_golden.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import vdx  # noqa: E402,F401
from vdx.vae import VaeConfig  # noqa: E402
from vdx.weights import synthetic_vae_encoder_state_dict  # noqa: E402

import vae_encoder_ref as ref  # noqa: E402

FRAME_SEED, WEIGHT_SEED, H, W = 2024, 8, 576, 1024


def frame():
    return np.random.default_rng(FRAME_SEED).integers(0, 256, (H, W, 3), dtype=np.uint8)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sd = synthetic_vae_encoder_state_dict(VaeConfig.sd(), seed=WEIGHT_SEED)
    m = ref.AutoencoderKLEncoderRef(ref.VaeConfig.sd()).eval()
    m.load_state_dict({k: v.float() for k, v in sd.items()})
    x = ref.unit_map(torch.from_numpy(frame())[None])
    with torch.no_grad():
        mom = m.moments(x)[0]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vid2vid_encoder_full.npz")
    np.savez_compressed(out, moments=mom.half().numpy(), frame_seed=FRAME_SEED, weight_seed=WEIGHT_SEED)
    print(out, tuple(mom.shape), float(mom.abs().max()))


if __name__ == "__main__":
    main()
