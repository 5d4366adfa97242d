"""`DistributedVideoDiffuser` — the hybrid FSDP + frame-chunked denoiser of
`Distribution/strategies/fsdp_chunked_coherent.py:47-276`, re-built on the HIP kernels.

Same configuration names as the reference's argparse (`:281-300`): num_frames, steps,
guidance_scale, chunk_size, overlap, height, width, mode {fsdp, chunk, hybrid, hybrid_ctx},
context_weight.  Differences in mechanism (results identical):
  * the per-step arithmetic (ctx injection, CFG combine, DDIM step) runs as two fused kernels;
  * denoised chunks stay on the device.  `__call__(exchange="allgather")` — the DEFAULT — keeps the reference's
    everyone-gets-everything semantics (`all_gather_object`, :201) as one fixed-shape `all_gather` and returns the whole
    blended latent.  `exchange="halo"` (vdx/halo.py) returns a DIFFERENT type — the list of (s, e, latent) segments this rank owns:
    every frame of the video has ONE owning rank (the rank of the first window that starts at or before it and whose
    successor starts after it); a rank sends only the frames of its windows that another rank owns — the `overlap`
    halo frames, 288 KiB per neighbour at XL size — as fixed-shape point-to-point transfers (RCCL send/recv over xGMI,
    issued on a side HIP stream with event hand-off; `comm=` routes them through the C-ABI entry point
    `vdx_halo_exchange` instead of torch.distributed) and blends and decodes only the frames it owns.  The per-frame
    accumulation order is the reference's (`for lst in gathered: for s,e,latc in lst`, :208-216), so the owned frames
    carry exactly the bits of the reference's full blend.
    `info["network_bytes"]` = bytes this rank RECEIVES in the exchange (allgather: (world-1) fixed-shape chunk lists;
    halo: the halo frames).  The reference's CSV column of the same name is `payload_bytes` (:194): frames x channels x 2
    of the rank's own chunk list (the formula leaves the h x w extent out; kept, it is what the reference's rows hold):
    both modes report that one as `info["payload_bytes"]` (and the real byte count as `payload_bytes_actual`), and
    a caller that writes the reference's CSV row (`metrics.append_csv`) passes it as the `network_bytes` column;
  * the linear-ramp blend (:204-217) runs on the device, in the reference's accumulation order.
"""
from __future__ import annotations

import json
import time
from dataclasses import dataclass, fields
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist

from . import noise as _noise
from . import ops
from .codenoise import co_denoise_round, loop_plan_of, tile_plan
from .inpaint import known_coefficients, mask_record
from .halo import HaloPlan, blend_owned, exchange_halos, ramp_weights
from .options import JobOptions, check_cfg_mimic, check_eta, check_free_init, check_freeu, check_guidance_rescale, check_noise, check_tome  # the checks' home is vdx/options.py
from .options import info_options, job_texts, lora_record, mimic_record, noise_record, prompt_record, record_options, region_record, resolve, sampler_noise_record, travel_record, world_size
from .planner import ChunkPlan, plan


@dataclass
class DiffuserConfig:
    num_frames: int = 32
    steps: int = 50
    guidance_scale: float = 7.5
    chunk_size: int = 0
    overlap: int = 4
    height: int = 576
    width: int = 1024
    mode: str = "hybrid_ctx"
    context_weight: float = 0.35
    device: str = "cuda"
    noise_device: Optional[str] = None     # None = like the reference: generate on `device`
    overlap_rule: str = "coherent"
    # the rest of the reference's argparse (`:281-300`): the job's front end (`run_job` / `main` below)
    model_id: str = "cerspense/zeroscope_v2_XL"
    prompt: str = "a rocket in space, 4k"
    fps: int = 8
    out_csv: str = "results.csv"
    # network emulation (`:195-199,257-258`): sleeps in front of the chunk exchange and the memory reduction
    emu_bw_mbps: float = 0.0               # throttle: payload_bytes / (Mbps * 1e6 / 8) seconds before the gather (0 = off)
    emu_rtt_ms: float = 0.0                # one-way latency: gauss(rtt, jitter) ms before the gather, rtt ms before the reduction
    emu_jitter_ms: float = 0.0
    # video-to-video refinement (diffusers VideoToVideoSDPipeline; unpinned): start from an encoded clip noised to the first
    # timestep of the schedule truncated by `strength`, instead of pure noise.  None = text-to-video, as the reference runs
    init_video: Optional[str] = None       # .npy uint8 (T,H,W,3) or a directory of image files (sorted by name)
    strength: float = 0.6
    posterior: str = "sample"              # "sample" | "mode" of the encoder's diagonal Gaussian
    gpu_flow: bool = False                 # flow_err (and MD-VQS' TC) from the HIP Farneback kernels instead of the host path
    scheduler: str = "ddim"                # "ddim" | "dpmpp_2m" (DPM-Solver++ 2M) | "dpmpp_2m_sde" (its SDE form; see `eta`): the sampler `run_job` uses
    interpolate: int = 1                   # N > 1: write (F-1) N + 1 motion-interpolated frames at fps N (vdx/interp.py); 1 = as always
    # FreeInit (vdx/freeinit.py; diffusers' enable_free_init, unpinned): sample, noise the blend back to t = 999 with the same
    # base noise, keep its low frequencies, take the high ones from fresh noise, sample again.  1 = one sampling pass, as always
    free_init_iters: int = 1
    free_init_method: str = "butterworth"  # "butterworth" | "gaussian" | "ideal"
    free_init_spatial: float = 0.25        # stop frequency d_s
    free_init_temporal: float = 0.25       # stop frequency d_t
    free_init_order: int = 4               # butterworth only
    # FreeU (UNet3DConditionModel.enable_freeu; diffusers' enable_freeu, unpinned): (b1, b2, s1, s2), the backbone factors and the
    # skip filter's scales of up blocks 0 and 1, on every denoising step of the job.  None = off, as always
    freeu: Optional[Tuple[float, float, float, float]] = None
    # token merging (UNet3DConditionModel.enable_tome; tomesd's apply_patch(ratio, max_downsample=1, sx=2, sy=2), unpinned): the share
    # of the level-0 spatial self-attentions' tokens merged away on every denoising step of the job.  None = off, as always
    tome: Optional[float] = None
    tome_seed: Optional[int] = None        # draw the cells' destination offsets once from this seed (None: every cell's first token)
    # temporal co-denoising (vdx/codenoise.py; MultiDiffusion along time, unpinned): ONE latent for the whole clip, the windows'
    # noise predictions averaged at every step where they overlap, one scheduler step for the clip; no final blend.  False = one
    # trajectory per window and the ramp blend after the loop, as always
    co_denoise: bool = False
    # masked video-to-video (vdx/inpaint.py; the replacement method / RePaint / diffusers' 4-channel inpainting, unpinned): hold
    # part of `init_video` fixed and generate the rest.  `mask`: a .npy path (or an array) of uint8 / bool (T,H,W), (H,W) or (T,),
    # nonzero = regenerate; `keep_frames`: "0:8,20:24", the frames to KEEP; one of the two.  None, None = off, as always
    mask: Optional[object] = None
    keep_frames: Optional[str] = None
    mask_rule: str = "nearest"             # pixel -> latent mask: "nearest" (pixel (8y, 8x)) | "any" (any of the cell's 64 pixels)
    mask_paste: bool = True                # the written frames' kept pixels are the input clip's bytes
    # the guidance itself (both arguments of every diffusers pipeline call; unpinned).  `negative_prompt`: the text of the
    # unconditional branch ("" = the empty prompt, as always).  `guidance_rescale`: phi of Lin et al. 2023 / diffusers'
    # `rescale_noise_cfg`, in [0, 1]: the guided noise is pulled towards the conditional one's standard deviation, per sample and
    # step (vdx/scheduler.py, csrc/rescale.hip).  0 = off, as always
    negative_prompt: str = ""
    guidance_rescale: float = 0.0
    # spatially tiled co-denoising (vdx/codenoise.py `tile_plan`, csrc/cotile.hip; MultiDiffusion along space, unpinned; needs
    # `co_denoise`): every window is run per tile of `tile` = (TH, TW) pixels, a crop at a size the UNet was trained at, and the
    # tiles' noise predictions are averaged where they overlap.  `tile_overlap` = (OY, OX) pixels, None = a quarter of the tile.
    # All four are multiples of 8.  None = the UNet runs on the whole frame, as always
    tile: Optional[Tuple[int, int]] = None
    tile_overlap: Optional[Tuple[int, int]] = None
    # seamless looping (vdx/codenoise.py `loop_plan`, csrc/codenoise.hip, its RING flag; AnimateDiff's `closed_loop` context option, unpinned; needs
    # `co_denoise`): the windows lie on a ring, the last wrapping over the clip's end into its first frames, so frames T-1 and 0
    # are denoised together at every step.  False = the windows stop at the clip's end, as always
    loop: bool = False
    # strided context windows (vdx/codenoise.py `stride_plan`, csrc/codenoise.hip, its `costride_tab`; AnimateDiff-Evolved's
    # `context_stride`, unpinned; needs `co_denoise`): the number of stride levels 1, 2, 4, ...; every level above the first adds
    # windows that take every 2nd, 4th, ... frame, so frames further apart than a window are denoised together at every step, at
    # the price of those windows' UNet calls.  1 = consecutive frames only, as always
    context_stride: int = 1
    # prompt travel (vdx/travel.py, csrc/travel.hip; AnimateDiff-Evolved's batch prompt schedule, unpinned): ((frame, text), ...),
    # key frames and their prompts; `prompt` is the key at frame 0 unless a key names frame 0.  A frame between two keys is
    # conditioned on the linear blend of their CLIP embeddings, a frame after the last key on the last key (with `loop`: on the
    # blend back to the first), in every window of every mode.  None = one prompt for the whole clip, as always
    prompt_travel: Optional[Tuple[Tuple[int, str], ...]] = None
    # regional prompts (vdx/region.py, csrc/region.hip; "attention couple" / regional conditioning, unpinned): ((mask, text), ...),
    # up to 7; a mask is a uint8 / bool array (H, W) or (T, H, W) in pixels, 0..255 (soft edges allowed), or the path of a .npy
    # file that holds one.  In every spatial cross-attention the conditional item's pixels under a mask are conditioned on that
    # region's text, the rest on `prompt`, in every window of every mode.  Not with `tile` or `prompt_travel`.  None = one prompt
    # for the whole frame, as always
    regions: Optional[tuple] = None
    # LoRA adapters (vdx/lora.py, csrc/lora.hip; diffusers' load_lora_weights / set_adapters, unpinned): ((path, scale), ...), up to
    # 8 local adapter files (.safetensors or torch.load; peft / diffusers or kohya keys) and their weights.  They are merged into
    # the UNet's and the text encoder's weights on the GPU before those are packed, moved and sharded; the forward itself is the
    # one it always was.  Goes with every other option.  None = the checkpoint's weights, as always
    lora: Optional[tuple] = None
    # weighted and long prompts (vdx/prompt.py, csrc/prompt.hip; the AUTOMATIC1111 web UI's prompt emphasis and 75-token chunks,
    # unpinned): "a1111" reads `(text:1.3)`, `(text)`, `[text]` and `BREAK` in the prompt, the negative prompt, every prompt-travel
    # key and every region text, and encodes a text of more than 75 tokens as up to four 77-position chunks side by side (all texts
    # of a job at the same length); the UNet's cross-attentions then see up to 308 rows.  A text of at most 75 tokens without
    # emphasis gives the same job bit for bit.  "plain" = one 77-position sequence, the rest truncated, every token alike, as always
    prompt_syntax: str = "plain"
    # dynamic thresholding of the guided noise (vdx/scheduler.py, csrc/dynthresh.hip; the A1111 / ComfyUI "Dynamic Thresholding (CFG
    # Scale Fix)" with its mimic scale, restated and unpinned): at every step each channel of the guided noise, less its mean, is
    # clamped at the `cfg_mimic_percentile` quantile of its magnitude and squeezed into the range the same prediction has at the
    # scale `cfg_mimic`, so a high `guidance_scale` keeps its direction without saturating.  No extra UNet call.  Needs
    # `guidance_scale` > 1; not with `guidance_rescale`, `tile`, `loop` or `context_stride` > 1.  None = off, as always
    cfg_mimic: Optional[float] = None
    cfg_mimic_percentile: float = 1.0
    # the noise generator (vdx/noise.py, csrc/noise.hip; Philox4x32-10 + Box-Muller, restated in tests/noise_ref.py and unpinned):
    # "philox" draws the start latent, FreeInit's fresh noise and the video-to-video posterior sample from the portable generator
    # "philox4x32-10/v1" under `seed` (an integer in [0, 2^64), None = 0): the same bits on every device, rank and torch build, and any
    # box of them can be regenerated from the seed alone.  A seed needs "philox" (`--seed N` alone selects it).  "torch", None = the
    # reference's `torch.manual_seed(0)` stream on the device, as always
    seed: Optional[int] = None
    noise: str = "torch"
    # stochastic sampling (vdx/scheduler.py, csrc/step_noise.h; diffusers' `DDIMScheduler.step(eta=)` and
    # `algorithm_type="sde-dpmsolver++"` / A1111's "DPM++ 2M SDE", restated in tests/sde_ref.py and unpinned): with "ddim", eta in
    # (0, 1] adds eta times the DDPM posterior's noise at every step; the scheduler "dpmpp_2m_sde" is SDE-DPM-Solver++ 2M (eta 0 or
    # 1 there, run and recorded as 1).  Every step's noise is drawn inside the step kernel from the portable generator, at the
    # element's place in the whole clip, so overlapping windows and any number of ranks draw the same noise: needs `noise`
    # "philox" (`--seed`).  Not with `guidance_rescale`, `cfg_mimic`, `tile`, `loop` or `context_stride` > 1.  0 = deterministic, as always
    eta: float = 0.0

    @property
    def use_fsdp(self):
        return self.mode in ("fsdp", "hybrid", "hybrid_ctx")

    @property
    def no_chunking(self):
        return self.mode == "fsdp"

    @property
    def use_ctx(self):
        return self.mode == "hybrid_ctx"


def emu_gather_delay_s(payload_bytes: int, cfg, rng=None) -> float:
    """Seconds the reference sleeps in front of `all_gather_object` (:195-199): `payload_bytes / (emu_bw_mbps * 1e6 / 8)` when
    a bandwidth is given, plus `max(0, gauss(emu_rtt_ms, emu_jitter_ms)) / 1000` when a latency is (the reference draws from
    the `random` module's global generator; `rng` = a `random.Random` for a reproducible draw)."""
    import random
    d = 0.0
    if cfg.emu_bw_mbps > 0:
        d += payload_bytes / (cfg.emu_bw_mbps * 1e6 / 8)
    if cfg.emu_rtt_ms > 0:
        d += max(0.0, (rng or random).gauss(cfg.emu_rtt_ms, cfg.emu_jitter_ms) / 1000.0)
    return d


def emu_reduce_delay_s(cfg) -> float:
    """Seconds the reference sleeps in front of the peak-memory `all_reduce` (:257-258)."""
    return cfg.emu_rtt_ms / 1000.0 if cfg.emu_rtt_ms > 0 else 0.0


def _world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _noise_device(device, noise_device=None) -> torch.device:
    """The device noise is generated on: `noise_device`, or like the reference `device` itself."""
    return torch.device(device if noise_device is None else noise_device)


def seeded_noise(shape, sigma, device, noise_device=None, dtype=torch.float16, seed: Optional[int] = None):
    """`torch.manual_seed(0); randn(...) * init_noise_sigma` (:180-182).  RNG streams are
    device-specific, so parity runs pass noise_device="cpu" (SURVEY.md §8 a2).  `seed` (the portable generator, vdx/noise.py):
    its base stream under that seed instead, times sigma, on `device`: no torch generator is touched."""
    if seed is not None:
        return _noise.normal(shape, device, seed=seed, stream=_noise.STREAM_BASE, sigma=sigma, dtype=dtype)
    nd = _noise_device(device, noise_device)
    torch.manual_seed(0)
    base = torch.randn(*shape, device=nd, dtype=dtype)
    base *= sigma
    return base.to(device)


def iteration_noise(shape, iteration: int, device, noise_device=None, seed: Optional[int] = None):
    """FreeInit's fresh noise of iteration `iteration` >= 1: fp32 N(0, 1) from a generator of its own seeded with the iteration
    number (seed 0 is `seeded_noise`'s), generated on `noise_device` like the base noise; the global generator is left alone.
    `seed` (the portable generator): stream `iteration` under that seed instead."""
    if seed is not None:
        return _noise.normal(shape, device, seed=seed, stream=_noise.stream_of_iteration(int(iteration)), dtype=torch.float32)
    nd = _noise_device(device, noise_device)
    g = torch.Generator(device=nd).manual_seed(int(iteration))
    return torch.randn(*shape, generator=g, device=nd, dtype=torch.float32).to(device)


SCHEDULERS = ("ddim", "dpmpp_2m", "dpmpp_2m_sde")


def make_scheduler(name: str, base):
    """The sampler `name` of `DiffuserConfig.scheduler` / `--scheduler`: "ddim" is `base` itself (the pipeline's scheduler,
    untouched); "dpmpp_2m" is `DPMSolverMultistepScheduler.from_config(base.config)`, as Zeroscope's published recipe builds it;
    "dpmpp_2m_sde" the same with `algorithm_type="sde-dpmsolver++"`."""
    if name == "ddim":
        return base
    if name == "dpmpp_2m_sde":
        from .scheduler import DPMSolverMultistepScheduler
        if isinstance(base, DPMSolverMultistepScheduler) and base.stochastic:
            return base
        return DPMSolverMultistepScheduler.from_config(base.config, algorithm_type="sde-dpmsolver++")
    if name == "dpmpp_2m":
        from .scheduler import DPMSolverMultistepScheduler
        if isinstance(base, DPMSolverMultistepScheduler):
            return base if not base.stochastic else DPMSolverMultistepScheduler.from_config(base.config, algorithm_type="dpmsolver++")
        return DPMSolverMultistepScheduler.from_config(base.config)
    raise ValueError(f"unknown scheduler {name!r}: expected one of {SCHEDULERS}")


def vid2vid_timesteps(scheduler, steps: int, strength: float) -> List[int]:
    """diffusers VideoToVideoSDPipeline.get_timesteps: init = min(int(steps*strength), steps), t_start = max(steps - init, 0),
    the tail `timesteps[t_start:]` of a schedule set for `steps` (the DDIM step's prev_t keeps the full `steps` spacing).
    `scheduler` must have had set_timesteps(steps)."""
    if steps <= 0:
        raise ValueError(f"vid2vid_timesteps: steps must be positive, got {steps}")
    if not (0.0 < strength <= 1.0):
        raise ValueError(f"vid2vid_timesteps: strength must be in (0, 1], got {strength}")
    if scheduler.num_inference_steps != steps:
        raise ValueError(f"vid2vid_timesteps: the scheduler is set for {scheduler.num_inference_steps} steps, not {steps}")
    init = min(int(steps * strength), steps)
    t_start = max(steps - init, 0)
    return list(scheduler._host_timesteps[t_start:])


def load_init_video(path: str):
    """--init_video: a .npy uint8 (T,H,W,3) array, or a directory of image files sorted by name (needs Pillow) -> numpy uint8."""
    import os

    import numpy as np
    if os.path.isdir(path):
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f"--init_video {path}: a directory of images needs Pillow, which is not installed "
                               "(pass a .npy uint8 (T,H,W,3) array instead)") from e
        names = sorted(n for n in os.listdir(path) if not n.startswith("."))
        if not names:
            raise ValueError(f"--init_video {path}: no image files")
        arr = np.stack([np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names])
    else:
        arr = np.load(path)
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[-1] != 3:
        raise ValueError(f"--init_video {path}: expected uint8 (T,H,W,3), got {arr.dtype} {arr.shape}")
    return np.ascontiguousarray(arr)


def gather_chunks(mine: List[torch.Tensor], chunk_plan: ChunkPlan, rank: int, world: int):
    """Exchange denoised chunks; returns [(s, e, tensor)] in the reference's blend order
    (rank-major, then the rank's own order — `for lst in gathered: for s,e,latc in lst`, :208-209).
    Fixed-shape exchange: every chunk is padded to `chunk_plan.chunk` frames."""
    per = chunk_plan.per_rank
    assert len(mine) == per
    if world == 1:
        return [(s, e, t) for (s, e), t in zip(chunk_plan.for_rank(0), mine)]
    ref = mine[0]
    _, C, _, H, W = ref.shape
    buf = ref.new_zeros((per, C, chunk_plan.chunk, H, W))
    for i, t in enumerate(mine):
        buf[i, :, :t.shape[2]] = t[0]
    bufs = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf)
    out = []
    for r in range(world):
        for i, (s, e) in enumerate(chunk_plan.for_rank(r)):
            out.append((s, e, bufs[r][i:i + 1, :, :e - s].contiguous()))
    return out


class DistributedVideoDiffuser:
    def __init__(self, cfg: DiffuserConfig, unet, scheduler, uncond_emb, cond_emb, init_latents=None, latent_mask=None, travel=None,
                 regions=None):
        """`init_latents` (video-to-video): the scaled clean latent (1,C,T,h,w) fp16 of the whole clip (every rank encodes the
        whole clip: identical bits on every rank, no collective).  The denoise then runs `vid2vid_timesteps(cfg.strength)`
        from add_noise(init_latents, base, t_first) (base = the seeded noise of text-to-video); with `hybrid_ctx`, ctx is the
        frame-mean of that start latent.  None: text-to-video, unchanged.
        `latent_mask` (masked video-to-video, vdx/inpaint.py; needs `init_latents`): uint8 (T,h,w) on the device, 1 = regenerate,
        0 = keep, identical on every rank.  After every scheduler step the kept cells are set to `init_latents` noised to the
        next timestep with `base` (to `init_latents` itself after the last one), and pasted again after the blend.  None: off.
        `travel` (prompt travel, vdx/travel.py): (key_embs, plan), the keys' text embeddings fp16 (n_keys, N, D) on the device in
        the order of the plan's frames and the `travel.TravelPlan` of the clip.  Every window's UNet text is then built once, by
        `ops.text_travel` (`window_text`), and passed where `cat([uncond_emb, cond_emb])` is passed without it.  None: off.
        `regions` (regional prompts, vdx/region.py): (region_embs, plan), the regions' text embeddings fp16 (R, N, D) and the
        `region.RegionPlan` of the clip.  Every UNet call then gains `regions=(region_embs, plan, its window)` (`region_kw`).
        None: off."""
        self.cfg = cfg
        check_noise(cfg)
        self._seed = _noise.generator_of(cfg)                         # the portable generator's seed; None: torch's stream, as always
        self._seed_kw = {"seed": self._seed} if self._seed is not None else {}
        self._sde = check_eta(cfg)                                    # a stochastic sampler's {"eta", "algorithm"}; None: deterministic, as always
        if self._sde is not None:
            if self._sde["algorithm"] == "ddim":
                if not hasattr(scheduler, "eta") or getattr(scheduler, "_dpm", False):
                    raise ValueError("eta > 0 with scheduler \"ddim\" needs a DDIMScheduler")
                scheduler.eta = self._sde["eta"]
            elif not getattr(scheduler, "stochastic", False):
                raise ValueError("scheduler \"dpmpp_2m_sde\" needs an SDEDPMSolverMultistepScheduler")
            scheduler.seed_noise(self._seed, 0)
        elif getattr(scheduler, "eta", 0.0) != 0.0:
            scheduler.eta = 0.0                                       # the pipeline's own scheduler, after a stochastic job
        check_freeu(cfg)
        check_tome(cfg)
        phi = check_guidance_rescale(cfg)
        self._rescale_kw = {"guidance_rescale": phi} if phi != 0 else {}     # off: the step is called as it always was
        mimic = check_cfg_mimic(cfg)
        if mimic is not None:                   # never with rescale (`check_cfg_mimic`): the step's one set of extra keywords
            self._rescale_kw = {"cfg_mimic": mimic["scale"], "cfg_mimic_percentile": mimic["percentile"]}
        if check_free_init(cfg) > 1 and init_latents is not None:
            raise ValueError("free_init_iters > 1 and init_latents exclude each other: FreeInit re-initialises a start from pure noise")
        self.free_init_starts: List[torch.Tensor] = []             # the start latents of iterations 1.. of the last call
        self.rank, self.world = _world()
        self.unet, self.scheduler = unet, scheduler
        self.uncond_emb, self.cond_emb = uncond_emb, cond_emb
        # reference :63-78 — modes fsdp / hybrid / hybrid_ctx shard the UNet's parameters
        if cfg.use_fsdp and self.world > 1 and isinstance(getattr(unet, "W", None), dict):
            unet.shard_(self.rank, self.world)
        scheduler.set_timesteps(cfg.steps, device=cfg.device)
        self.ctx = None
        self.init_latents = init_latents
        self.timesteps = None                                         # video-to-video only: the truncated schedule
        self._start = None
        self._base = self._x0 = None                                  # video-to-video only: the seeded noise, the clean latent
        self.latent_mask = None
        self._known = None                                            # masked only: add_noise's scalars of each step's NEXT timestep
        self.travel = None                                            # prompt travel only: (key_embs, the plan's device arrays)
        self._travel_text = {}                                        # (s, L, d, ring) -> that window's (2, L, N, D) text
        if travel is not None:
            key_embs, tplan = travel
            if key_embs.dim() != 3 or key_embs.shape[0] != len(tplan.frames) or tplan.T != cfg.num_frames:
                raise ValueError(f"travel: {tuple(key_embs.shape)} key embeddings for a plan of {len(tplan.frames)} keys and {tplan.T} "
                                 f"frames; the clip has {cfg.num_frames}")
            self.travel = (key_embs.to(cfg.device, torch.float16).contiguous(), tplan.to(cfg.device))
        self.regions = None                                           # regional prompts only: (region_embs, the plan on the device)
        if regions is not None:
            if travel is not None:
                raise ValueError("regions cannot be combined with prompt travel")
            region_embs, rplan = regions
            if (region_embs.dim() != 3 or region_embs.shape[0] != rplan.n_texts - 1 or rplan.T != cfg.num_frames
                    or (rplan.h, rplan.w) != (cfg.height // 8, cfg.width // 8)):
                raise ValueError(f"regions: {tuple(region_embs.shape)} text embeddings for a plan of {rplan.n_texts - 1} regions, {rplan.T} "
                                 f"frames and latent {rplan.h}x{rplan.w}; the clip has {cfg.num_frames} frames of {cfg.height // 8}x{cfg.width // 8}")
            self.regions = (region_embs.to(cfg.device, torch.float16).contiguous(), rplan.to(cfg.device))
        shape = self.latent_shape if init_latents is not None or cfg.use_ctx else None
        if init_latents is not None:
            if tuple(init_latents.shape) != shape:
                raise ValueError(f"init_latents {tuple(init_latents.shape)} != {shape}")
            self.timesteps = vid2vid_timesteps(scheduler, cfg.steps, cfg.strength)
            base = seeded_noise(shape, scheduler.init_noise_sigma, cfg.device, cfg.noise_device, **self._seed_kw)
            self._x0, self._base = init_latents.to(cfg.device, torch.float16).contiguous(), base
            self._start = scheduler.add_noise(self._x0, base, self.timesteps[0])
            if cfg.use_ctx:                                           # the frame-mean of the whole clip's start latent
                self.ctx = self._start.mean(dim=2, keepdim=True).contiguous()
        elif cfg.use_ctx:                                             # reference :105-127
            if self.rank == 0:
                full = seeded_noise(shape, scheduler.init_noise_sigma, cfg.device, cfg.noise_device, **self._seed_kw)
                ctx = full.mean(dim=2, keepdim=True)
            else:
                ctx = torch.empty(shape[:2] + (1,) + shape[3:], device=cfg.device, dtype=torch.float16)
            if self.world > 1:
                dist.broadcast(ctx, src=0)
            self.ctx = ctx.contiguous()
        if latent_mask is not None:
            if init_latents is None:
                raise ValueError("latent_mask needs init_latents: the kept content is that clip's")
            self.latent_mask = ops.check_latent_mask(latent_mask, *shape[2:])
            self._known = known_coefficients(scheduler, self.timesteps, self._x0)

    @property
    def latent_shape(self) -> Tuple[int, int, int, int, int]:
        cfg = self.cfg
        return (1, self.unet.config.in_channels, cfg.num_frames, cfg.height // 8, cfg.width // 8)

    @property
    def schedule(self) -> List[int]:
        """The timesteps this job runs: the scheduler's, or video-to-video's truncated ones."""
        return self.scheduler._host_timesteps if self.timesteps is None else self.timesteps

    def _mask_step(self, z: torch.Tensor, i: int, s: int) -> None:
        """Masked video-to-video, after step i of the schedule, in place on the latent z of the clip's frames [s, s + L)."""
        k = self._known[i]
        sa, s1 = k if k is not None else (0.0, 0.0)
        ops.mask_renoise(z, self._x0, self._base, self.latent_mask, sa, s1, k is None, s)

    def window_text(self, s: int, L: int, d: int = 1, ring: bool = False) -> torch.Tensor:
        """Prompt travel: the (2, L, N, D) UNet text of the window of the clip frames `s + f * d` (`ring`: mod T), built on first
        use and then held: the UNet's text cache knows a text by the tensor it is handed."""
        key = (int(s), int(L), int(d), bool(ring))
        text = self._travel_text.get(key)
        if text is None:
            key_embs, (lo, hi, w) = self.travel
            text = self._travel_text[key] = ops.text_travel(key_embs, self.uncond_emb.to(key_embs.device, torch.float16).contiguous(),
                                                            lo, hi, w, *key)
        return text

    def region_kw(self, s: int, L: int, d: int = 1, ring: bool = False) -> dict:
        """Regional prompts: what the UNet call of the window of the clip frames `s + f * d` (`ring`: mod T) gains; {} when off."""
        if self.regions is None:
            return {}
        return {"regions": (*self.regions, (int(s), int(L), int(d), bool(ring)))}

    def denoise(self, lat: torch.Tensor, s: Optional[int] = None, text: Optional[torch.Tensor] = None, window=None) -> torch.Tensor:
        """Reference `_denoise` (:129-143) for one chunk.  `s` (masked video-to-video only, with a `latent_mask`): the chunk's
        first frame in the clip; None: the masked path is off; a stochastic sampler needs it too (the chunk draws the clip's noise at
        its frames).  `text` (prompt travel): the chunk's `window_text`.  `window`
        (regional prompts; required with them): the chunk's (s, L) in the clip."""
        if self.regions is not None and window is None:
            raise ValueError("denoise: with regions the chunk's window (s, L) in the clip must be given: the masks are per clip frame")
        region_kw = self.region_kw(*window) if window is not None else {}
        masked = s is not None and self.latent_mask is not None
        cfg, sched = self.cfg, self.scheduler
        step_kw = self._rescale_kw
        if self._sde is not None:
            if s is None:
                raise ValueError("denoise: a stochastic sampler needs the chunk's first frame s in the clip")
            step_kw = {"frames": (int(s), cfg.num_frames)}            # never with rescale or mimic (`check_eta`)
        emb = torch.cat([self.uncond_emb, self.cond_emb], dim=0) if text is None else text
        lat = lat.contiguous()
        reset = getattr(sched, "reset", None)
        if reset is not None:       # a multistep scheduler must not carry the previous chunk's history into this one
            reset()
        for i, t in enumerate(self.schedule):
            x = ops.cfg_input(lat, self.ctx, cfg.context_weight)
            noise = self.unet(x, t, encoder_hidden_states=emb, **region_kw).sample
            lat = sched.step_cfg(noise, t, lat, cfg.guidance_scale, **step_kw)
            if masked:
                self._mask_step(lat, i, s)
        return lat

    def plan(self) -> ChunkPlan:
        cfg = self.cfg
        if cfg.loop:                        # ring windows of one length; a range's end may exceed num_frames (codenoise.loop_plan)
            return loop_plan_of(cfg, self.world)
        return plan(cfg.num_frames, self.world, cfg.chunk_size, cfg.overlap, cfg.no_chunking, cfg.overlap_rule)

    def blend(self, chunks: List[Tuple[int, int, torch.Tensor]], like: torch.Tensor, ov: int) -> torch.Tensor:
        """Reference :204-217 on the device."""
        T = like.shape[2]
        full = torch.zeros_like(like)
        weight = torch.zeros(T, dtype=torch.float32, device=like.device)
        for s, e, lat in chunks:
            ops.blend_accumulate(full, weight, lat.contiguous(), ramp_weights(e - s, ov).to(like.device), s, e)
        return ops.blend_finalize(full, weight)

    def decode_frames(self, lat: torch.Tensor, vae, batch: int = 8, paste=None) -> List:
        """Reference :219-225: the blended latent (1,C,T,h,w) -> T uint8 (H,W,3) frames (numpy, host).
        `z/0.18215` is formed in the latent's dtype and cast to fp16 at the VAE boundary (what the reference's
        FSDP mixed-precision wrapper does to forward inputs); frames are decoded `batch` at a time instead of one
        by one (frames are independent samples of the decoder).  `paste` = (the original uint8 (T,H,W,3) frames, the pixel mask
        uint8 (T,H,W), nonzero = generated), both on the device (masked video-to-video): each batch's kept pixels take the
        originals' bytes before the copy to the host."""
        frames = []
        T = lat.shape[2]
        if self.cfg.tile is not None:   # a tiled job's frame may be many times the headline's: keep the headline decode's activations
            batch = min(batch, max(1, 8 * 576 * 1024 // (self.cfg.height * self.cfg.width)))
        for i0 in range(0, T, batch):
            z = lat[0, :, i0:i0 + batch].permute(1, 0, 2, 3) / 0.18215
            u8 = vae.decode_frames_u8(z.to(self.cfg.device, torch.float16).contiguous())
            if paste is not None:
                orig, pm = paste
                u8 = ops.mask_composite_u8(u8, orig[i0:i0 + batch], pm[i0:i0 + batch], out=u8)
            frames += [f for f in u8.cpu().numpy()]
        return frames

    def _sync(self):
        if torch.device(self.cfg.device).type == "cuda":
            torch.cuda.synchronize()

    def _round(self, start: torch.Tensor, cp: ChunkPlan, exchange: str, comm, co_recs: Optional[list] = None, tiles=None, strided=None):
        """One sampling round from the whole clip's start latent `start`: denoise this rank's windows, exchange, blend
        -> (the blend: the latent, or with "halo" the owned segments; that round's seconds and bytes, under `info`'s names).
        `co_recs` (`co_denoise`; the call's list of its rounds' records): the round is `codenoise.co_denoise_round` instead, with
        the call's `tiles` (a `TilePlan`) and `strided` (a `StridePlan`) where it has them: one latent, the windows meet at every
        step, no blend; its record is added to `co_recs`."""
        if co_recs is not None:
            out, spent, rec = co_denoise_round(self, start, cp, tiles, strided)
            co_recs.append(rec)
            return out, spent
        _, C, T, H, W = start.shape
        t0 = time.time()
        masked = self.latent_mask is not None or self._sde is not None        # who needs the chunk's first frame: `denoise` tells them apart
        if self.regions is not None:        # regional prompts: every window with its place in the clip
            mine = [self.denoise(start[:, :, s:e].clone(), s if masked else None, None, (s, e - s)) for s, e in cp.for_rank(self.rank)]
        elif self.travel is None:           # the call as it always was
            mine = [self.denoise(start[:, :, s:e].clone(), *((s,) if masked else ())) for s, e in cp.for_rank(self.rank)]
        else:                               # prompt travel: every window with its own text
            mine = [self.denoise(start[:, :, s:e].clone(), s if masked else None, self.window_text(s, e - s)) for s, e in cp.for_rank(self.rank)]
        if self.world > 1:
            dist.barrier()
        self._sync()
        denoise_s = time.time() - t0
        # `payload_bytes = sum((e-s) * in_channels * 2 ...)` (:194) — frames x channels x 2 bytes WITHOUT the h x w extent: the
        # value the reference's CSV column `network_bytes` carries (its executed rows: tests/golden/ref_exec_planner.json);
        # the bytes a rank's chunk list really has are `payload_bytes_actual`
        payload = sum(t.shape[2] * C * 2 for t in mine)
        delay = emu_gather_delay_s(payload, self.cfg)                       # :195-199, outside the timed gather like there
        if delay > 0:
            time.sleep(delay)
        t0 = time.time()
        if exchange == "allgather":
            chunks = gather_chunks(mine, cp, self.rank, self.world)
            self._sync()
            net_gather_s = time.time() - t0
            received = (self.world - 1) * cp.per_rank * C * cp.chunk * H * W * 2
            out = self.blend(chunks, start, cp.overlap)
            if self.latent_mask is not None:              # the ramp blend zeroes the clip's first and last frame and re-weights overlaps: kept cells again
                ops.mask_paste_f32(out, self._x0, self.latent_mask)
        else:
            hp = HaloPlan(cp, T)
            got, done = exchange_halos(mine, hp, self.rank, comm=comm) if self.world > 1 else ({}, None)
            out = blend_owned(mine, hp, got, done, start, self.rank)
            self._sync()
            net_gather_s = time.time() - t0
            received = sum(t.numel() * 2 for t in got.values())
        return out, {"denoise_s": denoise_s, "emu_gather_delay_s": delay, "net_gather_s": net_gather_s, "network_bytes": received,
                     "payload_bytes": payload, "payload_bytes_actual": sum(t.numel() * 2 for t in mine)}

    def __call__(self, exchange: str = "allgather", comm=None, options: Optional[JobOptions] = None):
        """exchange="allgather": every rank ends with the whole blended latent (reference semantics, :201-217)
        -> (lat fp32 (1,C,T,h,w), info).  exchange="halo": a rank ends with the frames it owns
        -> ([(s, e, lat fp32 (1,C,e-s,h,w))], info) — the same bits, 1/world of the blend and decode work.
        `comm` (vdx.comm.Comm): the halo transfers go through the C-ABI RCCL entry point instead of torch.distributed.
        `options`: the job's `options.resolve`d options (`run_job` has them); None: the call resolves, and so validates, itself.

        What each option does stands in `DiffuserConfig`'s field comments, what goes with what in vdx/options.py (`RULES`, the
        `check_*`).  `info` holds the plan (`chunk_size`, `overlap`, `ranges`: with `loop` each window clipped to the clip, with
        `context_stride` the level-0 plan's), the seconds and bytes of the rounds, `owned` with "halo", and one entry per option
        that is on (`freeu`, `tome`, `free_init`, `options.info_options`).  With `free_init_iters` > 1 the seconds, bytes and
        emulated delays are sums over the iterations, `info["free_init"]` holds the per-iteration `denoise_s` and `reinit_s`, and
        the UNet is handed back in the FreeU / ToMe state it came in.  With `co_denoise` the exchange happens once per STEP:
        `network_bytes`, `net_gather_s`, `payload_bytes` and the emulated delays are then sums over the steps too."""
        cfg = self.cfg
        opts = options or resolve(cfg, exchange, self.world)
        if self.latent_mask is not None and exchange == "halo":
            raise ValueError("latent_mask needs exchange=\"allgather\": the paste after the blend needs the whole latent on every rank")
        iters, freeu, tome = opts.free_init_iters, opts.freeu, opts.tome
        tiles = tile_plan(cfg.height // 8, cfg.width // 8, *opts.tile) if opts.tile is not None else None
        co_recs = [] if opts.co_denoise else None                      # co_denoise: the rounds' records
        cp = self.plan()
        if self._start is None:
            base = seeded_noise(self.latent_shape, self.scheduler.init_noise_sigma, cfg.device, cfg.noise_device, **self._seed_kw)
        else:                       # video-to-video: the constructor noised the encoded clip with this same seeded noise
            base = self._start
        T = cfg.num_frames
        info = {"chunk_size": cp.chunk, "overlap": cp.overlap, "ranges": [(s, min(e, T)) for s, e in cp.ranges] if opts.loop else list(cp.ranges),
                "world_size": self.world,
                "num_frames": cfg.num_frames, "denoise_s": 0.0, "exchange": exchange, "steps_run": len(self.schedule),
                "emu_gather_delay_s": 0.0, "net_gather_s": 0.0, "network_bytes": 0, "payload_bytes": 0, "payload_bytes_actual": 0}
        if iters > 1:
            from . import freeinit
            filt = freeinit.lowpass_filter(base.shape[2:], cfg.free_init_method, cfg.free_init_spatial, cfg.free_init_temporal,
                                           cfg.free_init_order).to(base.device)
            rec = {"iters": iters, "method": cfg.free_init_method, "d_s": cfg.free_init_spatial, "d_t": cfg.free_init_temporal,
                   "order": cfg.free_init_order, "denoise_s": [], "reinit_s": []}
        ctx0, start, starts = self.ctx, base, []
        if self.travel is not None:
            # a rank's windows alternate within a step (co_denoise) or follow one another (windowed): one slot of the UNet's text
            # cache per window, 8 at most (an entry is ~150 MB at XL widths); beyond that a call recomputes
            runs = len((opts.stride_plan or cp).for_rank(self.rank))
            slots0 = getattr(self.unet, "text_cache_slots", None)
            if slots0 is not None:
                self.unet.text_cache_slots = max(slots0, min(runs, 8))
        if freeu is not None:
            freeu0 = self.unet.freeu
            self.unet.enable_freeu(**freeu)
            info["freeu"] = freeu
        if tome is not None:
            # like FreeU: enabled for the length of the call, the UNet handed back in the state it came in
            tome0 = self.unet.tome
            self.unet.enable_tome(**tome)
            info["tome"] = tome
        try:
            for it in range(iters):
                if self._sde is not None:                              # every round draws streams of its own
                    self.scheduler.seed_noise(self._seed, it)
                out, spent = self._round(start, cp, exchange, comm, co_recs, tiles, opts.stride_plan)
                for k, v in spent.items():
                    info[k] += v
                if iters > 1:
                    rec["denoise_s"].append(spent["denoise_s"])
                if it + 1 < iters:
                    t0 = time.time()
                    start = freeinit.reinit(out, base, self.scheduler, it + 1, filt, cfg.noise_device, **self._seed_kw)
                    if cfg.use_ctx:
                        self.ctx = start.mean(dim=2, keepdim=True).contiguous()
                    self._sync()
                    rec["reinit_s"].append(time.time() - t0)
                    starts.append(start)
        finally:
            self.ctx = ctx0                                            # the next call's iteration 0 starts as this one did
            if self.travel is not None and slots0 is not None:
                self.unet.text_cache_slots = slots0
            if freeu is not None:
                self.unet.enable_freeu(**freeu0) if freeu0 is not None else self.unet.disable_freeu()
            if tome is not None:
                self.unet.enable_tome(**tome0) if tome0 is not None else self.unet.disable_tome()
        if iters > 1:
            self.free_init_starts = starts
            info["free_init"] = rec
        if exchange == "halo":
            info["owned"] = [(s, e) for s, e, _ in out]
        info.update(info_options(opts, co_recs))
        return out, info


# ---------------------------------------------------------------------------------------------
# the job's front end: the reference's `main()` (:279-340) on this build's own driver
# ---------------------------------------------------------------------------------------------
def build_arg_parser():
    """The reference's argparse, flag for flag and default for default (`fsdp_chunked_coherent.py:281-300`) — the sweep script
    `Distribution/full_experiments_ZeroscopeXL.sh` drives the job through these.  Every flag beyond the reference's is off by
    default, and without it every launch, byte, CSV row and record is the one it always was: what an option does stands in
    `DiffuserConfig`'s field comments and, flag by flag; what goes with what in vdx/options.py."""
    import argparse
    p = argparse.ArgumentParser(description="hybrid FSDP + frame-chunked video denoising on the HIP path")
    p.add_argument("--model_id", default="cerspense/zeroscope_v2_XL")
    p.add_argument("--prompt", default="a rocket in space, 4k")
    p.add_argument("--num_frames", type=int, default=32)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--guidance_scale", type=float, default=7.5)
    p.add_argument("--chunk_size", type=int, default=0)
    p.add_argument("--overlap", type=int, default=4)
    p.add_argument("--fps", type=int, default=8)
    p.add_argument("--height", type=int, default=576)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--device", default="cuda")
    p.add_argument("--mode", choices=["fsdp", "chunk", "hybrid", "hybrid_ctx"], default="hybrid_ctx")
    p.add_argument("--context_weight", type=float, default=0.35)
    p.add_argument("--emu_bw_mbps", type=float, default=0, help="throttle bandwidth in Mbps (0 = no throttle)")
    p.add_argument("--emu_rtt_ms", type=float, default=0, help="one-way latency in ms (0 = no extra delay)")
    p.add_argument("--emu_jitter_ms", type=float, default=0, help="jitter stddev in ms (0 = no jitter)")
    p.add_argument("--out_csv", default="results.csv")
    p.add_argument("--exchange", choices=["allgather", "halo"], default="allgather")
    p.add_argument("--noise_device", default=None)
    p.add_argument("--seed", type=int, default=None, metavar="N",
                   help="draw the job's noise from the portable generator philox4x32-10/v1 under seed N in [0, 2^64): the same start "
                        "latent on every device and rank (default: the reference's torch stream, seed 0)")
    p.add_argument("--noise", choices=list(_noise.GENERATORS), default=None,
                   help="the noise generator: torch (the reference's device-dependent stream, the default) or philox (the portable one; "
                        "--seed N selects it, alone it means seed 0)")
    p.add_argument("--out_video", default="out.mp4")
    p.add_argument("--clip_json", default=None, help="write the CLIP quality score of the decoded frames here (rank 0)")
    p.add_argument("--clip_model", default=None, help="local CLIP ViT-B/32 directory (transformers layout) for --clip_json")
    p.add_argument("--mdvqs_json", default=None, help="write the MD-VQS record of the decoded frames here (rank 0)")
    p.add_argument("--lpips_model", default=None, help="local LPIPS-AlexNet state dict (lpips layout) for --mdvqs_json")
    p.add_argument("--gpu_flow", action="store_true", help="Farneback flow of flow_err and of MD-VQS' TC on the GPU (vdx/flow.py)")
    p.add_argument("--video_restart_rows", type=int, default=0,
                   help="restart marker every N MCU rows in the mp4's JPEG frames (0: none, the bytes written without this flag)")
    p.add_argument("--gpu_video_write", action="store_true",
                   help="encode the mp4's JPEG frames on the GPU (vdx.video.write_frames): the same file as without this flag")
    p.add_argument("--out_gif", default=None,
                   help="also write the clip (what --out_video gets, interpolated frames included) as an animated GIF on the GPU (vdx/gif.py)")
    p.add_argument("--gif_dither", choices=["none", "bayer"], default="bayer", help="--out_gif: ordered 8x8 dither (default) or none")
    p.add_argument("--gif_loop", type=int, default=0, help="--out_gif: the repeat count, 0 (default) for ever")
    p.add_argument("--score_from_file", action="store_true",
                   help="--clip_json / --mdvqs_json score the frames decoded back from --out_video (vdx/video.py)")
    p.add_argument("--init_video", default=None,
                   help="video-to-video: refine this clip (.npy uint8 (T,H,W,3) or a directory of images) instead of starting from noise")
    p.add_argument("--strength", type=float, default=0.6, help="video-to-video: fraction of the schedule run (0, 1]")
    p.add_argument("--posterior", choices=["sample", "mode"], default="sample", help="video-to-video: encoder posterior")
    p.add_argument("--scheduler", choices=list(SCHEDULERS), default="ddim",
                   help="sampler: ddim (the reference's, default), dpmpp_2m (DPM-Solver++ 2M: fewer --steps for the same quality) or "
                        "dpmpp_2m_sde (its stochastic form, SDE-DPM-Solver++ 2M; needs --seed)")
    p.add_argument("--eta", type=float, default=0.0, metavar="E",
                   help="stochastic sampling: with ddim, E in (0, 1] adds E times the posterior's noise at every step (needs --seed; "
                        "0, the default: deterministic); dpmpp_2m_sde runs as 1")
    p.add_argument("--interpolate", type=int, default=1,
                   help="write N - 1 motion-interpolated frames between every two generated ones, at fps * N (1: none, the default)")
    p.add_argument("--free_init", type=int, default=1,
                   help="FreeInit: N sampling passes, the start of each re-initialised from the one before (1: none, the default)")
    p.add_argument("--free_init_method", choices=["butterworth", "gaussian", "ideal"], default="butterworth")
    p.add_argument("--free_init_spatial", type=float, default=0.25, help="FreeInit: spatial stop frequency d_s")
    p.add_argument("--free_init_temporal", type=float, default=0.25, help="FreeInit: temporal stop frequency d_t")
    p.add_argument("--free_init_order", type=int, default=4, help="FreeInit: order of the butterworth filter")
    p.add_argument("--freeu", type=float, nargs=4, default=None, metavar=("B1", "B2", "S1", "S2"),
                   help="FreeU in the UNet's up blocks 0 and 1: backbone factors B1 B2 (> 0), skip filter scales S1 S2 (default: off)")
    p.add_argument("--tome", type=float, default=None, metavar="RATIO",
                   help="token merging around the level-0 spatial self-attentions: share of the tokens merged away, in (0, 0.75] (default: off)")
    p.add_argument("--tome_seed", type=int, default=None, help="token merging: draw the cells' destination offsets once from this seed")
    p.add_argument("--co_denoise", action="store_true",
                   help="temporal co-denoising: one latent for the whole clip, window predictions averaged at every step (default: off)")
    p.add_argument("--tile", type=int, nargs=2, default=None, metavar=("TH", "TW"),
                   help="with --co_denoise: run the UNet on overlapping TH x TW pixel tiles (multiples of 8) of the frame (default: off)")
    p.add_argument("--tile_overlap", type=int, nargs=2, default=None, metavar=("OY", "OX"),
                   help="--tile: overlap of neighbouring tiles in pixels (multiples of 8; default: a quarter of the tile)")
    p.add_argument("--loop", action="store_true",
                   help="with --co_denoise: ring windows, so that the clip's last frame leads back into its first (default: off)")
    p.add_argument("--context_stride", type=int, default=1, metavar="N",
                   help="with --co_denoise: N stride levels; level l adds windows of every 2^l-th frame (1, the default: consecutive frames only)")
    p.add_argument("--mask", default=None,
                   help="masked video-to-video: .npy uint8 / bool (T,H,W), (H,W) or (T,), nonzero = regenerate, zero = keep (needs --init_video)")
    p.add_argument("--keep_frames", default=None,
                   help="masked video-to-video: frames of --init_video to KEEP, e.g. 0:8,20:24 (slices or indices; instead of --mask)")
    p.add_argument("--mask_rule", choices=["nearest", "any"], default="nearest",
                   help="pixel mask -> latent mask: pixel (8y, 8x) decides a cell (nearest), or any of its 64 pixels (any)")
    p.add_argument("--mask_paste", choices=["on", "off"], default="on",
                   help="masked video-to-video: kept pixels of the written frames are the input clip's bytes (on) or the decoder's (off)")
    p.add_argument("--negative_prompt", default="",
                   help="text of the unconditional branch of classifier-free guidance (default: the empty prompt)")
    p.add_argument("--guidance_rescale", type=float, default=0.0,
                   help="CFG rescale phi in [0, 1] (Lin et al. 2023): 0, the default, is off; needs --guidance_scale > 1")
    p.add_argument("--cfg_mimic", type=float, default=None, metavar="M",
                   help="dynamic thresholding of the guided noise towards the mimic scale M, per channel and step (default: off; needs "
                        "--guidance_scale > 1; not with --guidance_rescale, --tile, --loop or --context_stride > 1)")
    p.add_argument("--cfg_mimic_percentile", type=float, default=1.0, metavar="Q",
                   help="with --cfg_mimic: clamp each channel at this quantile of its magnitude, in (0, 1] (default 1.0: its maximum)")
    p.add_argument("--prompt_at", nargs=2, action="append", default=None, metavar=("FRAME", "TEXT"),
                   help="prompt travel: TEXT is the prompt at frame FRAME, frames between two such keys blend them (repeatable; "
                        "--prompt is the key at frame 0 unless one names it; default: off)")
    p.add_argument("--region", nargs=2, action="append", default=None, metavar=("MASK.npy", "TEXT"),
                   help="regional prompt: the pixels under the mask (uint8 (H, W) or (T, H, W), 0..255) are conditioned on TEXT, the "
                        "rest on --prompt (repeatable, up to 7; not with --tile or --prompt_at; default: off)")
    p.add_argument("--lora", nargs=2, action="append", default=None, metavar=("PATH", "SCALE"),
                   help="LoRA adapter: merge the local file PATH (.safetensors or torch.load; peft / diffusers or kohya keys) into the "
                        "UNet and text encoder at weight SCALE (repeatable, up to 8; default: off)")
    p.add_argument("--prompt_syntax", choices=["plain", "a1111"], default="plain",
                   help="a1111: (text:1.3) / (text) / [text] emphasis and BREAK in every text of the job, and texts of more than 75 tokens "
                        "as up to four 75-token chunks (default: plain, one truncated 77-position sequence)")
    p.add_argument("--compare_to", default=None,
                   help="compare the generated frames with this clip (.npy of uint8 frames or Motion-JPEG mp4); needs --compare_json")
    p.add_argument("--compare_json", default=None, help="write the PSNR / SSIM / MS-SSIM record of --compare_to here (rank 0)")
    return p


FLAG_OF_FIELD = {"free_init_iters": "free_init", "overlap_rule": None, "prompt_travel": "prompt_at", "regions": "region"}     # where the flag's name is not the field's; None: no flag


def config_from_args(a) -> DiffuserConfig:
    """The parsed flags as a `DiffuserConfig`: every field that has a flag takes that flag's value."""
    flag_of = {f.name: FLAG_OF_FIELD.get(f.name, f.name) for f in fields(DiffuserConfig)}
    cfg = DiffuserConfig(**{name: getattr(a, flag) for name, flag in flag_of.items() if flag is not None})
    if cfg.noise is None:                       # --seed N alone selects the portable generator; --noise torch --seed N is refused
        cfg.noise = "philox" if cfg.seed is not None else "torch"
    if cfg.freeu is not None:
        cfg.freeu = tuple(cfg.freeu)
    if cfg.tile is not None:
        cfg.tile = tuple(cfg.tile)
    if cfg.tile_overlap is not None:
        cfg.tile_overlap = tuple(cfg.tile_overlap)
    if isinstance(cfg.mask_paste, str):
        cfg.mask_paste = cfg.mask_paste == "on"
    if cfg.prompt_travel is not None:           # FRAME arrives as text; what is no integer stays as it came, for the check to refuse
        def frame(v):
            try:
                return int(v)
            except ValueError:
                return v
        cfg.prompt_travel = tuple((frame(f), text) for f, text in cfg.prompt_travel)
    if cfg.regions is not None:
        cfg.regions = tuple((mask, text) for mask, text in cfg.regions)
    if cfg.lora is not None:                    # SCALE arrives as text; what is no number stays as it came, for the check to refuse
        def number(v):
            try:
                return float(v)
            except ValueError:
                return v
        cfg.lora = tuple((path, number(scale)) for path, scale in cfg.lora)
    return cfg


def clip_score_record(frames, prompt: str, clip_model: Optional[str], pipe_tokenizer, device) -> dict:
    """The validator's quality score (InferNet/template/validator/scoring.py:87-147) of the decoded frames, as `--clip_json`
    writes it.  Weights: `clip_model` (a local transformers-layout directory) or seeded synthetic ViT-B/32 weights.  Tokenizer:
    the one in `clip_model` when it has tokenizer files, else the pipeline's."""
    from .clip_score import CLIPScorer
    scorer = CLIPScorer.from_local(clip_model, device=device) if clip_model else CLIPScorer.synthetic(seed=0, device=device)
    if scorer.tokenizer is not None:
        tok, tok_src = scorer.tokenizer, "clip_model"
    else:
        tok, tok_src = pipe_tokenizer, "pipeline"
    score, per = scorer.score(frames, prompt, tokenizer=tok)
    return {"clip_score": score, "per_frame": per.tolist(), "synthetic_weights": scorer.synthetic_weights,
            "tokenizer": f"{tok_src}:{type(tok).__name__}", "n_frames": len(frames)}


def mdvqs_record(frames, prompt: str, lpips_model: Optional[str], clip_model: Optional[str], pipe_tokenizer, device,
                 flow: str = "cpu") -> dict:
    """The validator's MD-VQS record (InferNet/template/validator/scoring.py:13-67, :154-343) of the decoded frames, as
    `--mdvqs_json` writes it.  Weights: `clip_model` / `lpips_model` (local), else seeded synthetic ones, recorded as such.
    Tokenizer: as for `clip_score_record`.  `flow="gpu"` (`--gpu_flow`): TC from the HIP Farneback kernels; the record then
    has one more key, "flow": "gpu"."""
    from .clip_score import CLIPScorer
    from .lpips import LPIPSAlex
    from .mdvqs import MDVQS, verify_video_authenticity
    clip = CLIPScorer.from_local(clip_model, device=device) if clip_model else CLIPScorer.synthetic(seed=0, device=device)
    lp = LPIPSAlex.from_local(lpips_model, device=device) if lpips_model else LPIPSAlex.synthetic(seed=0, device=device)
    m = MDVQS(clip, lp, flow=flow)
    tok = clip.tokenizer if clip.tokenizer is not None else pipe_tokenizer
    pf = m.compute_prompt_fidelity(frames, prompt, tokenizer=tok)
    vq, per = m.compute_video_quality(frames)
    tc = m.compute_temporal_consistency(frames)
    ok, stats = verify_video_authenticity(frames, device=device)
    rec = {"pf": pf, "vq": vq, "tc": tc, "total": m.alpha * pf + m.beta * vq + m.gamma * tc,
           "weights": {"alpha": m.alpha, "beta": m.beta, "gamma": m.gamma}, "lpips_per_pair": per.tolist(),
           "authentic": ok, "authenticity": stats, "synthetic_weights": m.synthetic_weights, "n_frames": len(frames)}
    if flow != "cpu":
        rec["flow"] = flow
    return rec


def check_compare_args(a) -> None:
    """`--compare_to` and `--compare_json` go together, and the clip must be there and, where its header says so, of the job's
    shape: `VdxError` before anything is loaded."""
    from ._lib import VdxError
    if bool(a.compare_to) != bool(a.compare_json):
        raise VdxError("--compare_to PATH and --compare_json OUT are given together or not at all")
    if a.compare_to:
        from .compare import check_target
        check_target(a.compare_to, (a.num_frames, a.height, a.width, 3))


def compare_record(frames, path: str, ranges, device) -> dict:
    """The record `--compare_json` writes: vdx/compare.py's comparison of the generated frames (a) with the clip at `path` (b),
    seam and interior means by the job's chunk ranges.  MS-SSIM is left out below 176 pixels."""
    from . import compare
    other = compare.load_clip(path, device)
    h, w = frames[0].shape[:2]
    rec = compare.compare_frames(frames, other, ms_ssim=min(h, w) >= compare.MS_MIN_SIDE, ranges=ranges, device=device)
    return {"compare_to": path, **rec}


def encode_init_video(cfg: DiffuserConfig, vae, dev, return_frames: bool = False):
    """--init_video -> the scaled clean latent (1,4,T,h,w) fp16 on `dev`, seconds (and with `return_frames` the uint8 (T,H,W,3)
    frames at job size the encoder saw, on `dev`: what masked video-to-video pastes back): the clip is loaded, resized on the GPU to
    (height, width) when its size differs (Image.resize, BICUBIC), and encoded (posterior noise: (T,4,h,w) fp16 from a
    torch.Generator seeded 1 on the noise device).  Encoder weights: `vae/` of a local checkpoint, else seeded synthetic ones."""
    import os

    from . import weights as _weights
    from .compat.diffusers_shim import _load_file
    clip = load_init_video(cfg.init_video)
    if clip.shape[0] != cfg.num_frames:
        raise ValueError(f"--init_video has {clip.shape[0]} frames, --num_frames is {cfg.num_frames}")
    if cfg.posterior not in ("sample", "mode"):
        raise ValueError(f"posterior must be 'sample' or 'mode', got {cfg.posterior!r}")
    d = str(cfg.model_id)
    sd = None
    if os.path.isdir(d):
        sd = _load_file([f"{d}/vae/diffusion_pytorch_model.safetensors", f"{d}/vae/diffusion_pytorch_model.bin"])
    if sd is None:
        sd = _weights.synthetic_vae_encoder_state_dict(vae.cfg, 8, "cpu")
    vae.load_diffusers_encoder_state_dict(sd, device=dev)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.time()
    frames = torch.from_numpy(clip).to(dev)
    if frames.shape[1:3] != (cfg.height, cfg.width):
        frames = ops.resize_u8(frames, cfg.height, cfg.width)
    noise = None
    if cfg.posterior == "sample" and _noise.generator_of(cfg) is not None:       # the portable generator's posterior stream
        noise = _noise.normal((cfg.num_frames, 4, cfg.height // 8, cfg.width // 8), dev, seed=_noise.generator_of(cfg),
                              stream=_noise.STREAM_POSTERIOR)
    elif cfg.posterior == "sample":
        nd = _noise_device(dev, cfg.noise_device)
        g = torch.Generator(device=nd).manual_seed(1)
        noise = torch.randn((cfg.num_frames, 4, cfg.height // 8, cfg.width // 8), generator=g, device=nd,
                            dtype=torch.float16).to(dev)
    lat = vae.encode_frames_u8(frames, posterior=cfg.posterior, noise=noise)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return (lat, time.time() - t0, frames) if return_frames else (lat, time.time() - t0)


def run_job(cfg: DiffuserConfig, exchange: str = "allgather", out_video: Optional[str] = "out.mp4", pipe=None,
            clip_inputs: Optional[dict] = None, video_restart_rows: int = 0, gpu_video_write: bool = False,
            out_gif: Optional[str] = None, gif_dither: str = "bayer", gif_loop: int = 0) -> dict:
    """The reference's `DistributedVideoDiffuser(cfg)()` (:47-276) end to end -> its result dict (:263-275): pipeline
    components (`model_id` = a local checkpoint directory in diffusers layout, else seeded synthetic weights: nothing can be
    downloaded here), text embeddings (:96-103), chunked denoising + exchange + blend, per-frame VAE decode (:219-225),
    boundary metrics (:227-247) and the mp4 (:250-253) on rank 0, peak memory reduced over the ranks (:255-261).  `out_gif`
    (no reference counterpart): rank 0 also writes the frames the mp4 gets, interpolated ones included, as an animated GIF on
    the GPU (vdx/gif.py) with `gif_dither` and the repeat count `gif_loop`; the result then carries "gif"."""
    import os

    from . import metrics
    from .compat.diffusers_shim import DiffusionPipeline
    from .compat import pynvml_shim
    opts = resolve(cfg, exchange, world_size(env=True), job=True)        # every refusal, before anything is loaded
    if out_gif:                                 # the GIF's own refusals that need no frames, before anything is loaded too
        from . import gif
        gif.check_job_args(cfg.fps * opts.interpolate, gif_dither, gif_loop)
    factor, loop, pixel_mask = opts.interpolate, opts.loop, opts.pixel_mask
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1 and not dist.is_initialized():
        # like the reference (:41-50): one process per GPU, backend "nccl" (= RCCL).  Rehearsal aids, never set by a real run:
        # VDX_DIST_BACKEND=gloo + VDX_SHARE_GPU=1 let several ranks of a real multi-process job compute on ONE GPU
        # (RCCL refuses two ranks per device), as `bench.py --backend gloo --share-gpu` does.
        from .shard import configure_rccl_env
        configure_rccl_env()
        torch.cuda.set_device(0 if os.environ.get("VDX_SHARE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group(os.environ.get("VDX_DIST_BACKEND", "nccl"))
    dev = torch.device(cfg.device if cfg.device != "cuda" else f"cuda:{torch.cuda.current_device()}")
    if pipe is None:
        pipe = DiffusionPipeline.from_pretrained(cfg.model_id, torch_dtype=torch.float16, low_cpu_mem_usage=True,
                                                 use_safetensors=False, device_map=None)
    if opts.lora is not None:
        # before the models move and shard: the job's adapters replace whatever the pipe had loaded, merged on this rank's GPU
        # (every rank reads the same files and merges the same bits: no collective)
        import dataclasses

        from .lora import apply_job_adapters
        opts = dataclasses.replace(opts, lora_found=tuple(apply_job_adapters(pipe, opts.lora, dev)))
    unet = pipe.unet
    unet.detect_cfg_duplicate = False           # this driver builds its CFG batch with ops.cfg_input: tagged, no compare needed
    for m in (unet, pipe.text_encoder, pipe.vae):
        m.to(dev)
    tok = pipe.tokenizer
    texts = job_texts(cfg, opts.prompt_travel, opts.regions)     # one text-encoder call (regions never with prompt travel: `check_regions`)
    if opts.prompt_syntax == "plain":
        ids = tok(texts, padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
        with torch.no_grad():
            emb = pipe.text_encoder(ids.to(dev))[0]
    else:                                       # weights and 75-token chunks: every text of the job at 77 k rows (vdx/prompt.py)
        import dataclasses

        from .prompt import encode_texts
        emb, pplan = encode_texts(pipe, texts, opts.prompt_syntax, dev, return_plan=True)
        opts = dataclasses.replace(opts, prompt_found=pplan.record(opts.prompt_syntax))
    cond, uncond = emb[:1].contiguous(), emb[1:2].contiguous()
    text_kw = {}
    if opts.prompt_travel is not None:
        from .travel import travel_plan
        text_kw = {"travel": (emb[2:].contiguous(), travel_plan(opts.prompt_travel, cfg.num_frames, loop=loop))}
    if opts.regions is not None:
        text_kw = {"regions": (emb[2:].contiguous(), opts.regions)}
    init_latents, encode_s, masking = None, 0.0, {}
    if pixel_mask is not None:
        init_latents, encode_s, originals = encode_init_video(cfg, pipe.vae, dev, return_frames=True)
        pixel_mask = torch.from_numpy(pixel_mask).to(dev)
        masking = {"latent_mask": ops.mask_to_latent(pixel_mask, cfg.mask_rule)}
    elif cfg.init_video is not None:
        init_latents, encode_s = encode_init_video(cfg, pipe.vae, dev)
    d = DistributedVideoDiffuser(cfg, unet, make_scheduler(cfg.scheduler, pipe.scheduler), uncond, cond, init_latents=init_latents,
                                 **masking, **text_kw)
    out, info = d(exchange=exchange, options=opts)
    ranges = info["ranges"]
    if exchange == "allgather":
        paste = {"paste": (originals.contiguous(), pixel_mask)} if pixel_mask is not None and cfg.mask_paste else {}
        frames = d.decode_frames(out, pipe.vae, **paste)
    else:                                       # every rank decodes the frames it owns; rank 0 collects them for the metrics / mp4
        mine = [(s, d.decode_frames(lat, pipe.vae)) for s, _e, lat in out]
        allf = [None] * d.world
        if d.world > 1:
            dist.all_gather_object(allf, mine)
        else:
            allf = [mine]
        frames = [f for _s, fr in sorted((x for lst in allf for x in lst), key=lambda x: x[0]) for f in fr]
    temp_instab = flow_err = None
    if d.rank == 0 and len(frames) > 1 and not cfg.no_chunking:
        temp_instab = metrics.boundary_l1(frames, ranges)
        flow_err = metrics.flow_warp_error(frames, ranges, device=dev) if cfg.gpu_flow else metrics.flow_warp_error(frames, ranges)
    if loop:                                    # the loop's seam beside the clip's ordinary frame-to-frame change, on the host
        wrap_l1, mean_l1 = metrics.loop_l1(frames)
        info["loop"] = {**info["loop"], "wrap_l1": wrap_l1, "mean_l1": mean_l1}
    frames_written = gif_info = None
    if d.rank == 0 and (out_video or out_gif):
        to_write, fps = frames, cfg.fps
        if factor > 1:
            # after the metrics above, which are numbers about the generated frames; `frames` itself (what --clip_json and
            # --mdvqs_json score) stays as it is
            from .interp import interpolate_frames
            to_write, fps = interpolate_frames(frames, factor, device=dev, **({"loop": True} if loop else {})), cfg.fps * factor
        if out_video:
            host = factor > 1 and not gpu_video_write
            metrics.write_video(list(to_write.cpu().numpy()) if host else to_write, out_video, fps, restart_rows=video_restart_rows,
                                device=dev if gpu_video_write else None)
            frames_written = len(to_write)
        if out_gif:                             # the same frames at the same rate; interpolated frames stay on the device
            from . import gif
            gif_info = gif.write_gif(out_gif, to_write, fps, loop=gif_loop, dither=gif_dither, device=dev)
    delay = emu_reduce_delay_s(cfg)             # :257-258
    if delay > 0:
        time.sleep(delay)
    peak_mb, reduce_s = metrics.peak_vram_mb(dev)
    pynvml_shim.nvmlInit()
    end_mb = pynvml_shim.nvmlDeviceGetMemoryInfo(pynvml_shim.nvmlDeviceGetHandleByIndex(dev.index or 0)).used // 1024 ** 2
    if d.rank == 0 and clip_inputs is not None:
        # what `clip_score_record` needs, handed to the caller: the score runs outside the job (and outside main()'s timing)
        clip_inputs.update(frames=frames, tokenizer=tok, device=dev, ranges=ranges)
    # the options' entries: what the call recorded in `info`, the mask's record, the guidance keys
    mask = {"mask": mask_record(d.latent_mask, cfg.mask_rule, cfg.mask_paste)} if pixel_mask is not None else {}
    return {"world_size": d.world, "chunk_size": info["chunk_size"], "overlap": info["overlap"], "num_frames": cfg.num_frames,
            "peak_vram_mb": peak_mb, "end_vram_mb": int(end_mb), "network_bytes": int(info["payload_bytes"]),
            "net_gather_s": info["net_gather_s"], "net_reduce_s": reduce_s, "temp_instab": temp_instab, "flow_err": flow_err,
            "denoise_s": info["denoise_s"], "exchange": exchange, "rank": d.rank, "synthetic_weights": pipe.synthetic_weights,
            "emu_gather_delay_s": info["emu_gather_delay_s"], "emu_reduce_delay_s": delay,
            "strength": cfg.strength if cfg.init_video is not None else None, "steps_run": info["steps_run"], "encode_s": encode_s,
            "scheduler": cfg.scheduler, "interpolate": factor, "frames_written": frames_written,
            **({"free_init": info["free_init"]} if "free_init" in info else {}),
            **record_options({**info, **mask, **opts.guidance}), **travel_record(info), **region_record(info), **mimic_record(info), **lora_record(info),
            **prompt_record(info), **noise_record(info), **sampler_noise_record(info), **({"gif": {k: gif_info[k] for k in GIF_RECORD_KEYS}} if gif_info else {})}


GIF_RECORD_KEYS = ("frames", "colors", "bytes", "delay_cs", "dither", "strip_rows")


def gif_record(res: dict) -> dict:
    """{"gif": what `--out_gif` wrote} of a job's result for the JSON records; {} for a job without the flag."""
    return {"gif": res["gif"]} if "gif" in res else {}


def write_record(path: str, rec: dict, dumps=lambda rec: json.dumps(rec, indent=1)) -> None:
    """One of `main`'s JSON records."""
    with open(path, "w") as f:
        f.write(dumps(rec))


def main(argv=None) -> int:
    """`python -m vdx.pipeline [the reference's flags]` (one process, or under torchrun like the reference's script): runs the
    job and appends the reference's CSV row (:313-333) to `--out_csv` on rank 0."""
    from . import metrics
    a = build_arg_parser().parse_args(argv)
    cfg = config_from_args(a)
    if torch.cuda.is_available():
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    check_compare_args(a)
    clip_inputs = {} if a.clip_json or a.mdvqs_json or a.compare_to else None
    t0 = time.time()
    if a.score_from_file and not a.out_video:
        raise ValueError("--score_from_file needs --out_video")
    res = run_job(cfg, exchange=a.exchange, out_video=a.out_video, clip_inputs=clip_inputs,
                  video_restart_rows=a.video_restart_rows, gpu_video_write=a.gpu_video_write,
                  **({"out_gif": a.out_gif, "gif_dither": a.gif_dither, "gif_loop": a.gif_loop} if a.out_gif else {}))
    if res["rank"] == 0:
        row = metrics.result_row(res, mode=cfg.mode, num_frames=cfg.num_frames, elapsed_s=time.time() - t0)
        metrics.append_csv(cfg.out_csv, row)
        print(f"Metrics appended ->  {cfg.out_csv}")
        source = {**record_options(res), **travel_record(res), **region_record(res), **mimic_record(res), **lora_record(res), **prompt_record(res),
                  **noise_record(res), **sampler_noise_record(res), **gif_record(res)}
        scored = cfg.prompt
        if "prompt_syntax" in res:
            # the scores know no weights and CLIP ViT-B/32 truncates at its own 77 tokens: they are taken against --prompt with the
            # syntax characters stripped, and the records say so
            from .prompt import strip_syntax
            scored = strip_syntax(cfg.prompt)
            source = {**source, "scored_prompt": scored}
        generated = clip_inputs["frames"] if clip_inputs is not None else None
        if clip_inputs is not None and a.score_from_file:
            # what a validator holding the file would score: the mp4 just written, decoded back on the GPU
            from .video import read_frames
            clip_inputs["frames"] = read_frames(a.out_video, device=clip_inputs["device"])[0]
            source = {**source, "source": "file"}
        if a.clip_json:
            # scored after the row took its latency and memory readings: the row is that of a run without --clip_json
            rec = clip_score_record(clip_inputs["frames"], scored, a.clip_model, clip_inputs["tokenizer"], clip_inputs["device"])
            write_record(a.clip_json, {**rec, **source})
        if a.mdvqs_json:
            # likewise after the row: MD-VQS (its optical flow runs on the CPU unless --gpu_flow) never shows in `latency_s`
            rec = mdvqs_record(clip_inputs["frames"], scored, a.lpips_model, a.clip_model, clip_inputs["tokenizer"],
                               clip_inputs["device"], **({"flow": "gpu"} if a.gpu_flow else {}))
            write_record(a.mdvqs_json, {**rec, **source})
        if a.compare_to:
            # likewise after the row; always the generated frames, whatever --score_from_file and --interpolate do to the file
            from . import compare
            rec = compare_record(generated, a.compare_to, clip_inputs["ranges"], clip_inputs["device"])
            rec.update({**record_options(res), **travel_record(res), **region_record(res), **mimic_record(res), **lora_record(res), **prompt_record(res),
                        **noise_record(res), **sampler_noise_record(res), **gif_record(res)})
            write_record(a.compare_json, rec, compare.dumps)
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
