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
    STREAM_SAMPLER     2^33 ...   per-step sampler noise, drawn by the stochastic samplers (`DiffuserConfig.eta`: DDIM with eta > 0,
                                  SDE-DPM-Solver++; vdx/scheduler.py `seed_noise`): 2^33 + round 2^16 + i (`stream_of_step`)
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
STREAM_STEP_MAX = 2 ** 16 - 1          # a step's index in its schedule
STREAM_ROUND_MAX = 2 ** 30 - 1         # a sampling round (the FreeInit iteration less one)


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


def stream_of_step(round: int, i: int) -> int:
    """The stream a stochastic sampler draws step `i` of sampling round `round` from: STREAM_SAMPLER + round 2^16 + i.  `i`: the
    timestep's index in the scheduler's FULL schedule (a video-to-video run starts at its first timestep's index, not at 0);
    `round`: the FreeInit iteration less one, 0 without FreeInit."""
    for name, v, hi in (("round", round, STREAM_ROUND_MAX), ("step index", i, STREAM_STEP_MAX)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= hi:
            raise ValueError(f"sampler noise: the {name} must be an integer in [0, {hi}], got {v!r}")
    return STREAM_SAMPLER + round * 2 ** 16 + i


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
