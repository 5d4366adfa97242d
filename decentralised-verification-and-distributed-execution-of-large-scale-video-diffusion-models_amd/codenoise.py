"""Temporal co-denoising: the host side (integers, weights and the per-step loop; the arithmetic is csrc/codenoise.hip).

The job's default keeps one trajectory per window and lets the windows meet once, after the loop, in the ramp blend.  With
`DiffuserConfig(co_denoise=True)` / `--co_denoise` there is ONE latent for the whole clip instead (MultiDiffusion, Bar-Tal et al.
2023, applied along time; Gen-L-Video's "temporal co-denoising", Wang et al. 2023; what AnimateDiff's context windows do): at
every step each window predicts noise for its slice of that latent, the predictions are averaged where windows overlap, and one
scheduler step advances the whole clip.  Frames that two windows share cannot diverge: there is one copy of them.  DDIM (eta 0)
and DPM-Solver++ 2M are linear in the noise and the weights sum to 1, so averaging the predictions is averaging the stepped
latents.  The reference has no counterpart: the option is off by default, and without it nothing here runs.

Pinned (tests/test_codenoise_gpu.py, bit for bit): the kernels against the torch restatement of tests/codenoise_ref.py, a
one-window job against `DistributedVideoDiffuser.denoise`, a several-window job against a Python loop over the same windows, and
a two-rank job against the one-rank job.  NOT pinned and not claimed: agreement with any external implementation, and any
seam-quality effect on real Zeroscope weights.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .planner import ChunkPlan


def fuse_weights(length: int, overlap: int) -> List[float]:
    """Raw weight of frame j of a window: `min(j + 1, length - j, overlap + 1) / (overlap + 1)`: a ramp of `overlap` frames at
    either end and 1 between, STRICTLY positive.  (The reference's blend ramp has exact zeros at a window's ends, which survive
    its division only through `clamp(min=1e-6)`; a frame that only such an end covers would have no noise to step with.)"""
    if length < 1 or overlap < 0:
        raise ValueError(f"fuse_weights: length {length} must be >= 1 and overlap {overlap} >= 0")
    return [min(j + 1, length - j, overlap + 1) / (overlap + 1) for j in range(length)]


@dataclass(frozen=True)
class WindowTable:
    """`fused`: (index in the plan, s, e) of the windows that enter the fuse, in plan order; `wn`: fp32 (K, T), the normalised
    weights, zero outside a window."""
    fused: Tuple[Tuple[int, int, int], ...]
    wn: torch.Tensor

    def rows(self, world: int, per_rank: int, slot_elems: int) -> List[Tuple[int, int, int]]:
        """(element offset, first frame, length) per fused window in the packed buffer `[world][per_rank][slot]`: window i of
        the plan sits at rank i % world, slot i // world."""
        return [(((i % world) * per_rank + i // world) * slot_elems, s, e - s) for i, s, e in self.fused]


def window_table(chunk_plan: ChunkPlan, T: int) -> WindowTable:
    """The plan's windows in plan order.  A range that repeats an earlier one (the planner's repeated tail window) is still
    DENOISED by its rank, so that all ranks make the same number of UNet calls and the sharded parameters' gathers stay in
    lockstep, but it is left out of the fuse.  `wn[k][t] = w_k[t - s_k] / sum over the fused windows that hold t`, in float64,
    then rounded to fp32: exactly 1.0 where one window covers a frame.  A frame in no window is a `ValueError`."""
    seen, fused = set(), []
    for i, (s, e) in enumerate(chunk_plan.ranges):
        if not 0 <= s < e <= T:
            raise ValueError(f"window_table: window {i} = [{s}, {e}) leaves the {T} frames")
        if (s, e) not in seen:
            seen.add((s, e))
            fused.append((i, s, e))
    if len(fused) > ops.COFUSE_MAX_WINDOWS:
        raise ValueError(f"window_table: {len(fused)} windows, the fused step takes {ops.COFUSE_MAX_WINDOWS}")
    raw = np.zeros((len(fused), T), dtype=np.float64)
    for k, (_, s, e) in enumerate(fused):
        raw[k, s:e] = fuse_weights(e - s, chunk_plan.overlap)
    total = raw.sum(axis=0)
    if (total <= 0).any():
        raise ValueError(f"window_table: frame {int(np.argmin(total > 0))} is in no window")
    return WindowTable(tuple(fused), torch.from_numpy((raw / total).astype(np.float32)))


def check_co_denoise(cfg, exchange: str = "allgather") -> bool:
    """`cfg.co_denoise`; `ValueError` before any work when it is asked for together with the halo exchange: every rank holds the
    whole latent at every step anyway, there are no owned segments to return."""
    if getattr(cfg, "co_denoise", False) and exchange == "halo":
        raise ValueError("co_denoise needs exchange=\"allgather\": every rank holds the whole clip's latent at every step")
    return bool(getattr(cfg, "co_denoise", False))


def co_denoise_round(d, start: torch.Tensor, cp: ChunkPlan):
    """One co-denoised sampling round of `d` (a `DistributedVideoDiffuser`) from the whole clip's start latent -> (z.float(),
    the round's seconds and bytes under `info`'s names, the `info["co_denoise"]` record).  Per step: this rank's windows go
    through `ops.cfg_input_window` -> UNet into one packed buffer `[per_rank][2][C][cp.chunk][h][w]` (a window shorter than the
    chunk fills the front of its slot; the rest is never read); with more than one rank, one `all_gather_into_tensor` of that
    buffer; then every rank runs the fused step on its own copy of z (identical bits on every rank: no broadcast; with
    `guidance_rescale` the step's statistic is taken over that same gathered buffer, so every rank gets the same r).  There is no
    final blend, so the zeroed first and last frame of the reference's ramp blend does not occur."""
    from .pipeline import emu_gather_delay_s
    cfg, sched = d.cfg, d.scheduler
    _, C, T, H, W = start.shape
    table = window_table(cp, T)
    per, world, rank = cp.per_rank, d.world, d.rank
    slot = 2 * C * cp.chunk * H * W
    rows = table.rows(world, per, slot)
    wn = table.wn.to(start.device)
    mine = cp.for_rank(rank)
    emb = torch.cat([d.uncond_emb, d.cond_emb], dim=0)
    local = torch.zeros((per, slot), dtype=torch.float16, device=start.device)
    packed = torch.zeros((world, per, slot), dtype=torch.float16, device=start.device) if world > 1 else local
    payload_step = sum((e - s) * C * 2 for s, e in mine)          # the reference's formula (:194), per exchange
    actual_step = sum(2 * C * (e - s) * H * W * 2 for s, e in mine)
    bytes_step = (world - 1) * per * slot * 2
    z = start.clone()
    reset = getattr(sched, "reset", None)
    if reset is not None:                                         # ONE x0 history for the whole clip, fresh per round
        reset()
    spent = {"denoise_s": 0.0, "emu_gather_delay_s": 0.0, "net_gather_s": 0.0, "network_bytes": 0, "payload_bytes": 0,
             "payload_bytes_actual": 0}
    t_round = time.time()
    for i, t in enumerate(d.schedule):
        for j, (s, e) in enumerate(mine):
            x = ops.cfg_input_window(z, d.ctx, cfg.context_weight, s, e)
            noise = d.unet(x, t, encoder_hidden_states=emb).sample
            local[j, :noise.numel()].copy_(noise.reshape(-1))
        delay = emu_gather_delay_s(payload_step, cfg)             # per step: one exchange per step is what the method costs
        if delay > 0:
            d._sync()
            time.sleep(delay)
            spent["emu_gather_delay_s"] += delay
        if world > 1:
            d._sync()
            t0 = time.time()
            dist.all_gather_into_tensor(packed.view(-1), local.view(-1))
            d._sync()
            spent["net_gather_s"] += time.time() - t0
        z = sched.step_cfg_windows(packed, rows, wn, t, z, cfg.guidance_scale, **d._rescale_kw)
        if d.latent_mask is not None:                             # masked video-to-video (vdx/inpaint.py): the whole clip, s = 0
            d._mask_step(z, i, 0)
        spent["network_bytes"] += bytes_step
        spent["payload_bytes"] += payload_step
        spent["payload_bytes_actual"] += actual_step
    if world > 1:
        dist.barrier()
    d._sync()
    spent["denoise_s"] = time.time() - t_round - spent["net_gather_s"] - spent["emu_gather_delay_s"]
    rec = {"windows": len(table.fused), "steps": len(d.schedule), "exchange_s": spent["net_gather_s"], "bytes_per_step": bytes_step}
    return z.float(), spent, rec
