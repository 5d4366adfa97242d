"""The job's noise: which generator draws it, under which seed, on which stream.

Two generators.  "torch" is the reference's (`fsdp_chunked_coherent.py:180-182`): `torch.manual_seed(0); randn` on the job's device
(or `noise_device`), a stream that depends on the device and on the torch build; its seeds are fixed, as they always were.
"philox" is the portable one, "philox4x32-10/v1" (csrc/noise.hip, `ops.philox_normal`; tests/noise_ref.py is its definition):
element i of stream s under seed k is a pure function of (k, s, i), the same bits on every device, rank and batch, for the whole
tensor or for any box of it, with no state to carry.  A chosen seed (`DiffuserConfig.seed`, `--seed N`) always means "philox".

Streams of one seed, 64-bit:
    STREAM_BASE        0          the base noise (the start latent, `add_noise`'s and the masked job's re-noising)
    1 .. 2^32 - 1                 FreeInit's fresh noise of iteration k (`stream_of_iteration`)
    STREAM_POSTERIOR   2^32       the video-to-video posterior sample
    STREAM_SAMPLER     2^33 ...   reserved for per-step sampler noise (no sampler here draws any yet)
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

GENERATOR = "philox4x32-10/v1"
GENERATORS = ("torch", "philox")
STREAM_BASE = 0
STREAM_ITERATION_MAX = 2 ** 32 - 1
STREAM_POSTERIOR = 2 ** 32
STREAM_SAMPLER = 2 ** 33


def check_seed(seed) -> int:
    """`seed` when it is an integer in [0, 2^64); `ValueError` otherwise."""
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must lie in [0, 2^64), got {seed}")
    return seed


def stream_of_iteration(iteration: int) -> int:
    """FreeInit iteration k >= 1 -> its stream, k itself."""
    if isinstance(iteration, bool) or not isinstance(iteration, int) or not 1 <= iteration <= STREAM_ITERATION_MAX:
        raise ValueError(f"FreeInit iteration must be an integer in [1, {STREAM_ITERATION_MAX}], got {iteration!r}")
    return iteration


def generator_of(cfg) -> Optional[int]:
    """The philox seed of a config (`noise` "philox": `seed`, 0 without one), None for the torch stream."""
    if getattr(cfg, "noise", "torch") != "philox":
        return None
    seed = getattr(cfg, "seed", None)
    return 0 if seed is None else check_seed(seed)


def normal(shape, device, *, seed: Optional[int] = None, stream: int = STREAM_BASE, sigma: float = 1.0, dtype=torch.float16, box=None,
           torch_draw=None):
    """The job's N(0, 1) * sigma of `shape` on `device`.  `seed` None: `torch_draw()`, the torch stream's draw as the caller always
    made it.  Else the portable generator's `stream` under `seed` (`box`: only that box of the logical `shape`)."""
    if seed is None:
        return torch_draw()
    return ops.philox_normal(shape, check_seed(seed), stream, box=box, sigma=sigma, dtype=dtype, device=device)


def record(seed: int) -> dict:
    """The entry `info`, the result and the JSON records gain under "noise"."""
    return {"generator": GENERATOR, "seed": int(seed)}
