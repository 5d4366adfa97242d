"""A job's options: `DiffuserConfig` -> one validated, frozen `JobOptions`, before any model or device is touched.

What each option IS stands once, in the comments of `DiffuserConfig`'s fields (vdx/pipeline.py); INTEGRATION.md is the long form.
What goes with what stands here: each option's own `check_*` below (its values), and `RULES`, the one table of what the
co-denoising family needs and excludes.  `resolve` runs the checks in the order the entry points always ran them, so a config
that breaks two rules keeps raising the message it always raised; `run_job` resolves once and hands the result to
`DistributedVideoDiffuser.__call__`, which resolves for itself only when called without one.  `RECORD_KEYS` / `record_options`
name the option entries of the result dict and the JSON records, `info_options` those of `info`.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import TYPE_CHECKING, Optional, Tuple

import torch.distributed as dist

from . import ops
from .planner import PlannerError

if TYPE_CHECKING:       # vdx/codenoise.py imports the checks from here: its plans are imported where a check builds one
    import numpy as np

    from .codenoise import StridePlan


def world_size(env: bool = False) -> int:
    """The initialised process group's size; else, with `env` (the job's front end, before it has initialised the group),
    `WORLD_SIZE` of the environment; else 1."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size()
    return int(os.environ.get("WORLD_SIZE", 1)) if env else 1


# ---- what the co-denoising family needs and excludes ------------------------------------------------------------------------------
_EVERY_RANK = "every rank holds the whole clip's latent at every step"
NEEDS_CO, NEEDS_ALLGATHER = "needs co_denoise", "needs allgather"
# option -> its refusals in the order they are raised: (NEEDS_CO | NEEDS_ALLGATHER | an option it excludes, the message).
# A pair that is not listed is allowed; a new option of the family adds its row (and its name to the rows that exclude it).
RULES = {
    "co_denoise": ((NEEDS_ALLGATHER, f"co_denoise needs exchange=\"allgather\": {_EVERY_RANK}"),),
    "tile": ((NEEDS_CO, "tile needs co_denoise: tiles meet at every step in the fused noise; the windowed job's blend has no tiled form"),
             (NEEDS_ALLGATHER, f"tile needs exchange=\"allgather\": {_EVERY_RANK}"),
             ("guidance_rescale", "tile and guidance_rescale exclude each other: the rescale's statistics pass has no tiled form yet")),
    "loop": ((NEEDS_CO, "loop needs co_denoise: ring windows meet at every step in the fused noise; the windowed job's blend has no ring form"),
             (NEEDS_ALLGATHER, f"loop needs exchange=\"allgather\": {_EVERY_RANK}"),
             ("tile", "loop and tile exclude each other: the tiled kernels have no ring form yet"),
             ("guidance_rescale", "loop and guidance_rescale exclude each other: the rescale's statistics pass has no ring form yet")),
    "context_stride": ((NEEDS_CO, "context_stride needs co_denoise: strided windows meet the others at every step in the fused noise; "
                                  "the windowed job's blend has no strided form"),
                       (NEEDS_ALLGATHER, f"context_stride needs exchange=\"allgather\": {_EVERY_RANK}"),
                       ("tile", "context_stride and tile exclude each other: the tiled kernels have no strided form yet"),
                       ("loop", "context_stride and loop exclude each other: ring windows have no strided form yet"),
                       ("guidance_rescale", "context_stride and guidance_rescale exclude each other: the rescale's statistics "
                                            "pass has no strided form yet")),
}
_IS_ON = {"tile": lambda cfg: cfg.tile is not None, "loop": lambda cfg: cfg.loop,
          "guidance_rescale": lambda cfg: cfg.guidance_rescale != 0}


def check_rules(option: str, cfg, exchange: str) -> None:
    """`ValueError` with the first of `RULES[option]` that `cfg` and `exchange` break."""
    for what, message in RULES[option]:
        if (not cfg.co_denoise if what == NEEDS_CO else exchange == "halo" if what == NEEDS_ALLGATHER else _IS_ON[what](cfg)):
            raise ValueError(message)


# ---- one check per option: its value when the job can run it, `ValueError` before any work otherwise ------------------------------
def check_free_init(cfg, exchange: str = "allgather") -> int:
    """`cfg.free_init_iters` when the job can run it; `ValueError` otherwise, before any work: the count is an integer >= 1,
    and with more than one iteration the filter's arguments are valid, the exchange is "allgather" (every rank must hold the
    whole blend to re-noise it) and there is no `init_video` (video-to-video starts from a clip, not from noise)."""
    k = cfg.free_init_iters
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"free_init_iters must be an integer >= 1, got {k!r}")
    if k > 1:
        from .freeinit import check_filter_args
        check_filter_args(cfg.free_init_method, cfg.free_init_spatial, cfg.free_init_temporal, cfg.free_init_order)
        if exchange == "halo":
            raise ValueError("free_init_iters > 1 needs exchange=\"allgather\": with \"halo\" no rank holds the whole blended latent")
        if cfg.init_video is not None:
            raise ValueError("free_init_iters > 1 and init_video exclude each other: FreeInit re-initialises a start from pure noise")
    return k


def check_freeu(cfg) -> Optional[dict]:
    """`cfg.freeu` as {"b1", "b2", "s1", "s2"} (None when off); `ValueError` before any work unless it is four finite numbers
    with b1, b2 > 0 (s may be any finite number: 0 removes the band)."""
    if cfg.freeu is None:
        return None
    v = tuple(cfg.freeu) if isinstance(cfg.freeu, (tuple, list)) else ()
    if len(v) != 4:
        raise ValueError(f"freeu must be four numbers (b1, b2, s1, s2), got {cfg.freeu!r}")
    rec = {}
    for name, x, positive in zip(("b1", "b2", "s1", "s2"), v, (True, True, False, False)):
        rec[name] = ops._freeu_number(f"freeu: {name}", x, positive)
    return rec


def check_guidance_rescale(cfg) -> float:
    """`cfg.guidance_rescale` as a float (0.0 when off); `ValueError` before any work unless it is a finite number in [0, 1], and
    when it is non-zero with `guidance_scale <= 1`: the job still runs the CFG combine there, as the reference does, but the
    guided noise then lies between the two predictions and rescale has nothing to correct, so refuse rather than guess."""
    phi = cfg.guidance_rescale
    ops.rescale_factors(phi)
    if phi != 0 and not cfg.guidance_scale > 1:
        raise ValueError(f"guidance_rescale {phi!r} needs guidance_scale > 1, got {cfg.guidance_scale!r}")
    return float(phi)


def check_cfg_mimic(cfg) -> Optional[dict]:
    """`cfg.cfg_mimic` / `cfg.cfg_mimic_percentile` as {"scale", "percentile"} (None when off); `ValueError` before any work for a
    scale that is not a finite number > 0, a percentile outside (0, 1] or given without a scale, `guidance_scale <= 1` (there is
    no high scale to tame), and together with `guidance_rescale` (both rewrite the guided noise, and no order is defined) or with
    `tile`, `loop` or `context_stride` > 1 (the statistics pass has no tiled, ring or strided form, as the rescale's has none).
    The option's refusals live here, as the regions' do in their check: `RULES` lists the co-denoising family only."""
    ms, q = getattr(cfg, "cfg_mimic", None), getattr(cfg, "cfg_mimic_percentile", 1.0)
    if ms is None:
        if q != 1.0:
            raise ValueError(f"cfg_mimic_percentile {q!r} needs cfg_mimic")
        return None
    ops.mimic_factors(ms, q, 1)
    if not cfg.guidance_scale > 1:
        raise ValueError(f"cfg_mimic {ms!r} needs guidance_scale > 1, got {cfg.guidance_scale!r}")
    if cfg.guidance_rescale != 0:
        raise ValueError("cfg_mimic and guidance_rescale exclude each other: both rewrite the guided noise, and no order is defined")
    for on, name, form in ((cfg.tile is not None, "tile", "tiled"), (cfg.loop, "loop", "ring"),
                           (cfg.context_stride != 1, "context_stride", "strided")):
        if on:
            raise ValueError(f"cfg_mimic and {name} exclude each other: the thresholding's statistics pass has no {form} form yet")
    return {"scale": float(ms), "percentile": float(q)}


def check_noise(cfg) -> Optional[dict]:
    """`cfg.noise` / `cfg.seed` as {"generator", "seed"} (None for "torch", the reference's stream, as always); `ValueError` before
    any work for a generator that is neither "torch" nor "philox", a seed that is no integer in [0, 2^64), a seed with "torch" (a
    chosen seed gets the portable generator; the torch stream stays what the reference draws: its seeds are fixed), and under
    "philox" a `noise_device` other than the job's device (the generator has no host form in the package).  "philox" without a
    seed is seed 0.  The front end's `--seed N` alone selects "philox" (`pipeline.config_from_args`)."""
    from . import noise as _noise
    gen, seed = getattr(cfg, "noise", "torch"), getattr(cfg, "seed", None)
    if gen not in _noise.GENERATORS:
        raise ValueError(f"noise must be one of {_noise.GENERATORS}, got {gen!r}")
    if seed is not None:
        _noise.check_seed(seed)
    if gen == "torch":
        if seed is not None:
            raise ValueError(f"seed {seed!r} needs noise=\"philox\" (--seed alone selects it): the torch stream's seeds are the "
                             "reference's and stay fixed")
        return None
    if cfg.noise_device is not None:
        import torch
        try:
            nd, dev = torch.device(cfg.noise_device), torch.device(cfg.device)
        except (RuntimeError, TypeError):
            raise ValueError(f"noise_device {cfg.noise_device!r} is no device") from None
        if nd.type != dev.type or (nd.index is not None and dev.index is not None and nd.index != dev.index):
            raise ValueError(f"noise=\"philox\" draws on the job's device {cfg.device!r}, noise_device is {cfg.noise_device!r}: the "
                             "generator has no host form in the package, and its bits do not depend on the device")
    return _noise.record(0 if seed is None else seed)


SDE_SCHEDULER = "dpmpp_2m_sde"


def check_eta(cfg) -> Optional[dict]:
    """`cfg.eta` / `cfg.scheduler` as {"eta", "algorithm"} (None for a deterministic job, as always); `ValueError` before any work
    unless eta is a finite number in [0, 1]; with the scheduler "dpmpp_2m_sde" (SDE-DPM-Solver++, which has no partial form) unless
    it is 0 or 1, and it is recorded as 1; with "dpmpp_2m" unless it is 0.  A stochastic job (DDIM with eta > 0, "dpmpp_2m_sde")
    draws every step's noise from the portable generator, so it needs `noise="philox"` (`--seed`): the torch stream has no
    per-step form (its draw depends on the device, the rank and the chunk).  Refused with `guidance_rescale`, `cfg_mimic`, `tile`,
    `loop` and `context_stride` > 1, whose steps have no noise form yet."""
    import math
    eta, sched = getattr(cfg, "eta", 0.0), getattr(cfg, "scheduler", "ddim")
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not math.isfinite(eta) or not 0 <= eta <= 1:
        raise ValueError(f"eta must be a finite number in [0, 1], got {eta!r}")
    if sched == SDE_SCHEDULER:
        if eta not in (0, 1):
            raise ValueError(f"scheduler {SDE_SCHEDULER!r} has no partial form: eta must be 0 or 1 (it runs as 1), got {eta!r}")
        rec = {"eta": 1.0, "algorithm": "sde-dpmsolver++"}
    elif eta == 0:
        return None
    elif sched != "ddim":
        raise ValueError(f"eta {eta!r} goes with scheduler \"ddim\" or {SDE_SCHEDULER!r}: {sched!r} is deterministic")
    else:
        rec = {"eta": float(eta), "algorithm": "ddim"}
    if getattr(cfg, "noise", "torch") != "philox":
        raise ValueError("a stochastic sampler (eta > 0, dpmpp_2m_sde) needs noise=\"philox\" (--seed N selects it): the torch stream "
                         "has no per-step form, its draw depends on the device, the rank and the chunk")
    for on, name, form in ((cfg.guidance_rescale != 0, "guidance_rescale", "rescaled"), (cfg.cfg_mimic is not None, "cfg_mimic", "thresholded"),
                           (cfg.tile is not None, "tile", "tiled"), (cfg.loop, "loop", "ring"),
                           (cfg.context_stride != 1, "context_stride", "strided")):
        if on:
            raise ValueError(f"eta and {name} exclude each other: the stochastic step has no {form} noise form yet")
    return rec


def check_tome(cfg) -> Optional[dict]:
    """`cfg.tome` / `cfg.tome_seed` as {"ratio", "sx", "sy", "seed", "max_downsample"} (None when off); `ValueError` before any work
    for a ratio `enable_tome` refuses, or a seed without a ratio."""
    if cfg.tome is None:
        if cfg.tome_seed is not None:
            raise ValueError("tome_seed needs tome")
        return None
    from .tome import check_params
    return check_params(cfg.tome, seed=cfg.tome_seed)


def check_co_denoise(cfg, exchange: str = "allgather") -> bool:
    """`cfg.co_denoise`; `ValueError` before any work when it is asked for together with the halo exchange: every rank holds the
    whole latent at every step anyway, there are no owned segments to return."""
    if cfg.co_denoise:
        check_rules("co_denoise", cfg, exchange)
    return bool(cfg.co_denoise)


MIN_TILE_CELLS = 8   # 2^(levels - 1) of the four-level UNet: below it the deepest level is a single ceil-rounded cell per side


def check_tile(cfg, exchange: str = "allgather") -> Optional[Tuple[int, int, int, int]]:
    """`cfg.tile` / `cfg.tile_overlap` (pixels) as (th, tw, oy, ox) in latent cells, None when off; `ValueError` before any work
    when the job cannot run it: `RULES["tile"]` (tiling exists only as co-denoising: the windowed job's ramp blend has no spatial
    form); a tile is two multiples of 8 pixels, no larger than the frame and no smaller than the UNet takes for a frame
    (`MIN_TILE_CELLS` latent cells a side); the overlap, multiples of 8 pixels too, lies in [0, tile) per axis and defaults to a
    quarter of the tile in latent cells."""
    tile, ov = cfg.tile, cfg.tile_overlap
    if tile is None:
        if ov is not None:
            raise ValueError("tile_overlap needs tile")
        return None

    def pair(v, what):
        if not isinstance(v, (tuple, list)) or len(v) != 2 or any(isinstance(x, bool) or not isinstance(x, int) for x in v):
            raise ValueError(f"{what} must be two integers (pixels), got {v!r}")
        if any(x % 8 for x in v):
            raise ValueError(f"{what} {tuple(v)} must be multiples of 8 pixels (one latent cell)")
        return v[0] // 8, v[1] // 8

    from .codenoise import tile_starts
    check_rules("tile", cfg, exchange)
    th, tw = pair(tile, "tile")
    h, w = cfg.height // 8, cfg.width // 8
    if cfg.height % 8 or cfg.width % 8:
        raise ValueError(f"tile: the frame {cfg.height}x{cfg.width} must be a multiple of 8 pixels")
    if th > h or tw > w:
        raise ValueError(f"tile {tuple(tile)} is larger than the frame {cfg.height}x{cfg.width}")
    if th < MIN_TILE_CELLS or tw < MIN_TILE_CELLS:
        raise ValueError(f"tile {tuple(tile)} is smaller than the UNet takes for a frame: {MIN_TILE_CELLS * 8} pixels a side at least")
    oy, ox = (th // 4, tw // 4) if ov is None else pair(ov, "tile_overlap")
    if not (0 <= oy < th and 0 <= ox < tw):
        raise ValueError(f"tile_overlap {(oy * 8, ox * 8)} must lie in [0, tile) per axis, tile is {tuple(tile)}")
    ny, nx = len(tile_starts(h, th, oy)), len(tile_starts(w, tw, ox))
    if ny * nx > ops.COTILE_MAX_TILES:
        raise ValueError(f"tile {tuple(tile)}: {ny} x {nx} tiles, the fused step takes {ops.COTILE_MAX_TILES}")
    return th, tw, oy, ox


def check_loop(cfg, exchange: str = "allgather", world: Optional[int] = None) -> bool:
    """`cfg.loop`; `ValueError` before any work when the job cannot run it: `RULES["loop"]` (ring windows exist only as
    co-denoising: the windowed job's trajectories never meet before the blend), and when `loop_plan` refuses the plan (mode
    "fsdp", a chunk as long as the clip, no overlap, more windows than frames or than the fused step takes).  `world` None: the
    initialised group's, else 1."""
    if not cfg.loop:
        return False
    from .codenoise import loop_plan_of
    check_rules("loop", cfg, exchange)
    try:
        cp = loop_plan_of(cfg, world_size() if world is None else world)
    except PlannerError as err:
        raise ValueError(f"loop: {err}") from None
    if len(cp.ranges) > ops.COFUSE_MAX_WINDOWS:
        raise ValueError(f"loop: {len(cp.ranges)} windows, the fused step takes {ops.COFUSE_MAX_WINDOWS}")
    return True


def _stride(cfg, exchange: str, world: Optional[int]) -> Tuple[int, Optional[StridePlan]]:
    """`check_stride` with the plan it had to build (None with one level)."""
    levels = cfg.context_stride
    if isinstance(levels, bool) or not isinstance(levels, int) or levels < 1:
        raise ValueError(f"context_stride: the number of stride levels must be an integer >= 1, got {levels!r}")
    if levels == 1:
        return 1, None
    from .codenoise import stride_plan_of
    check_rules("context_stride", cfg, exchange)
    try:
        sp = stride_plan_of(cfg, world_size() if world is None else world)
    except PlannerError as err:
        raise ValueError(f"context_stride: {err}") from None
    fused = len(set(sp.windows))
    if fused > ops.COFUSE_MAX_WINDOWS:
        raise ValueError(f"context_stride: {fused} windows, the fused step takes {ops.COFUSE_MAX_WINDOWS}")
    return levels, sp


def check_stride(cfg, exchange: str = "allgather", world: Optional[int] = None) -> int:
    """`cfg.context_stride`, the number of stride levels (1 = off: the job is then plain co-denoising or the windowed job, as
    always); `ValueError` before any work when the job cannot run it: `RULES["context_stride"]` (strided windows exist only as
    co-denoising), and when `stride_plan` refuses the plan or the fused step cannot take its windows.  `world` None: the
    initialised group's, else 1."""
    return _stride(cfg, exchange, world)[0]


def check_prompt_travel(cfg) -> Optional[Tuple[Tuple[int, str], ...]]:
    """`cfg.prompt_travel` as the job's keys, ((frame, text), ...) sorted by frame with `cfg.prompt` at frame 0 unless a key names
    frame 0 (None when off); `ValueError` before any work for a malformed entry, a frame that is no integer inside the clip, a
    frame named twice, a text that is no string, and more than 64 keys (vdx/travel.py).  One key is valid: a constant prompt
    through the per-frame path."""
    if getattr(cfg, "prompt_travel", None) is None:
        return None
    from .travel import keys_of
    return keys_of(cfg)


def check_regions(cfg):
    """`cfg.regions` as the job's `region.RegionPlan` (None when off): the per-level weight tables and launch flags of the masks
    and the regions' texts, computed once, on the host; `ValueError` before any work for a malformed entry, a text that is no
    string, a mask of the wrong dtype or shape, more than 7 regions, an (H, W) or T that does not match the job, and with `tile` or
    `prompt_travel` (vdx/region.py)."""
    if getattr(cfg, "regions", None) is None:
        return None
    from .region import UNET_LEVELS, VAE_SCALE, check_regions as check, region_plan
    return region_plan(check(cfg), cfg.num_frames, cfg.height // VAE_SCALE, cfg.width // VAE_SCALE, UNET_LEVELS)


def check_lora(cfg) -> Optional[Tuple[Tuple[str, float], ...]]:
    """`cfg.lora` as ((path, scale), ...) with float scales (None when off); `ValueError` before anything is loaded for a malformed
    entry, a path that is no string or names no local file, a scale that is no finite number, more than 8 adapters, and a path
    given twice.  The files are read once the pipeline's configs are known (`run_job`, vdx/lora.py `read_lora`)."""
    if getattr(cfg, "lora", None) is None:
        return None
    import math
    entries = cfg.lora
    if not isinstance(entries, (tuple, list)) or not entries:
        raise ValueError(f"lora must be a non-empty sequence of (path, scale) pairs, got {entries!r}")
    if len(entries) > 8:
        raise ValueError(f"lora: {len(entries)} adapters, at most 8 are merged at once")
    out, seen = [], set()
    for e in entries:
        if not isinstance(e, (tuple, list)) or len(e) != 2:
            raise ValueError(f"lora: every entry is a (path, scale) pair, got {e!r}")
        path, scale = e
        if not isinstance(path, (str, os.PathLike)):
            raise ValueError(f"lora: the path must be a string, got {path!r}")
        path = os.fspath(path)
        try:
            scale = float(scale)
        except (TypeError, ValueError):
            raise ValueError(f"lora: the scale of {path!r} must be a number, got {scale!r}") from None
        if isinstance(e[1], bool) or not math.isfinite(scale):
            raise ValueError(f"lora: the scale of {path!r} must be a finite number, got {e[1]!r}")
        if "://" in path or not os.path.isfile(path):
            raise ValueError(f"lora: {path!r} is not a local file (nothing is ever downloaded)")
        real = os.path.realpath(path)
        if real in seen:
            raise ValueError(f"lora: {path!r} is given twice")
        seen.add(real)
        out.append((path, scale))
    return tuple(out)


def job_texts(cfg, travel=None, regions=None) -> list:
    """The texts of a job in the order `run_job` encodes them: the prompt, the negative prompt, the prompt-travel keys' texts, the
    regions' texts (`travel`, `regions`: what `check_prompt_travel` and `check_regions` returned)."""
    texts = [cfg.prompt, cfg.negative_prompt] + [text for _, text in travel or ()]
    if regions is not None:
        texts += list(regions.texts)
    return texts


def check_prompt_syntax(cfg, texts=None) -> str:
    """`cfg.prompt_syntax`, "plain" (off: one tokeniser call, 77 positions, every token at weight 1, as always) or "a1111"
    (vdx/prompt.py: `(text:1.3)` emphasis and 75-token chunks); `ValueError` before anything is loaded for any other value and,
    with `texts` (the job's front end: `job_texts`), for a text that is no string or that makes more chunks than the UNet takes,
    counted with the tokenizer the job's `model_id` will bring (its `tokenizer/` files, else the hash stand-in: no weights are read)."""
    syntax = getattr(cfg, "prompt_syntax", "plain")
    from .prompt import SYNTAXES
    if syntax not in SYNTAXES:
        raise ValueError(f"prompt_syntax must be one of {SYNTAXES}, got {syntax!r}")
    if syntax != "plain" and texts is not None:
        from .compat.diffusers_shim import tokenizer_for
        from .prompt import check_texts
        check_texts(texts, tokenizer_for(cfg.model_id))
    return syntax


# ---- the resolved job ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class JobOptions:
    """What the checks return, for one config, exchange and world size; plain values."""
    exchange: str
    world: int
    free_init_iters: int
    freeu: Optional[dict]
    tome: Optional[dict]
    co_denoise: bool
    tile: Optional[Tuple[int, int, int, int]]        # (th, tw, oy, ox) in latent cells
    loop: bool
    context_stride: int                                # the number of levels
    stride_plan: Optional[StridePlan]                  # with more than one level
    # what only the job's front end checks (`resolve(job=True)`); otherwise the config's values as they stand
    interpolate: int = 1
    pixel_mask: Optional[np.ndarray] = None
    guidance_rescale: float = 0.0
    guidance: dict = field(default_factory=dict)       # the keys the result and the records gain: negative_prompt, guidance_rescale
    prompt_travel: Optional[Tuple[Tuple[int, str], ...]] = None     # the keys, sorted, the prompt at frame 0 among them
    regions: Optional[object] = None                                # regional prompts: the job's `region.RegionPlan` (host tables)
    lora: Optional[Tuple[Tuple[str, float], ...]] = None            # LoRA adapters: the job's (path, scale) pairs
    lora_found: Optional[tuple] = None                              # what `read_lora` found in them (`run_job` fills it in): the record
    prompt_syntax: str = "plain"                                    # "plain" | "a1111" (vdx/prompt.py)
    prompt_found: Optional[dict] = None                             # the chunked texts' record (`run_job` fills it in once they are encoded)
    cfg_mimic: Optional[dict] = None                                # dynamic thresholding: {"scale", "percentile"} (csrc/dynthresh.hip)
    noise: Optional[dict] = None                                    # the portable generator: {"generator", "seed"} (vdx/noise.py); None: torch's stream
    sampler_noise: Optional[dict] = None                            # a stochastic sampler: {"eta", "algorithm"} (vdx/scheduler.py); None: deterministic


def resolve(cfg, exchange: str = "allgather", world: Optional[int] = None, *, job: bool = False) -> JobOptions:
    """The validated options of `cfg`.  `job` (`run_job`): every check, in `run_job`'s order, the ones that need files (the mask)
    included.  Without it (`DistributedVideoDiffuser.__call__`): the checks of a call, in its order; what only the front end or
    the constructor checks (`interpolate`, `guidance_rescale`) is taken as it stands.  `world` None: the initialised group's
    size, else 1."""
    if world is None:
        world = world_size()
    if job:
        from .inpaint import check_mask
        from .interp import check_factor
        factor = check_factor(cfg.interpolate)
        iters, freeu, tome = check_free_init(cfg, exchange), check_freeu(cfg), check_tome(cfg)
        co, tile = check_co_denoise(cfg, exchange), check_tile(cfg, exchange)
        if tome is not None:                    # the UNet's frame is a tile where tiling is on, else the whole latent frame
            from .tome import check_grid
            check_grid(*((tile[0], tile[1]) if tile is not None else (cfg.height // 8, cfg.width // 8)), tome)
        loop = check_loop(cfg, exchange, world)
        levels, sp = _stride(cfg, exchange, world)
        pixel_mask = check_mask(cfg, exchange)
        phi = check_guidance_rescale(cfg)
        if not isinstance(cfg.negative_prompt, str):
            raise ValueError(f"negative_prompt must be a string, got {cfg.negative_prompt!r}")
        guidance = {"negative_prompt": cfg.negative_prompt} if cfg.negative_prompt else {}
        travel = check_prompt_travel(cfg)
        regions = check_regions(cfg)
        lora = check_lora(cfg)
        syntax = check_prompt_syntax(cfg, job_texts(cfg, travel, regions))
        mimic = check_cfg_mimic(cfg)
        noise = check_noise(cfg)
        sde = check_eta(cfg)
    else:
        co, tile, loop = check_co_denoise(cfg, exchange), check_tile(cfg, exchange), check_loop(cfg, exchange, world)
        levels, sp = _stride(cfg, exchange, world)
        iters, freeu, tome = check_free_init(cfg, exchange), check_freeu(cfg), check_tome(cfg)
        if exchange not in ("allgather", "halo"):
            raise ValueError(f"unknown exchange {exchange!r}")
        factor, pixel_mask, phi, guidance = cfg.interpolate, None, float(cfg.guidance_rescale), {}
        travel = check_prompt_travel(cfg)
        regions = check_regions(cfg)
        lora = check_lora(cfg)
        syntax = check_prompt_syntax(cfg)
        mimic = check_cfg_mimic(cfg)
        noise = check_noise(cfg)
        sde = check_eta(cfg)
    if phi != 0:
        guidance["guidance_rescale"] = phi
    return JobOptions(exchange=exchange, world=world, free_init_iters=iters, freeu=freeu, tome=tome, co_denoise=co, tile=tile,
                      loop=loop, context_stride=levels, stride_plan=sp, interpolate=factor, pixel_mask=pixel_mask,
                      guidance_rescale=phi, guidance=guidance, prompt_travel=travel, regions=regions, lora=lora, prompt_syntax=syntax,
                      cfg_mimic=mimic, noise=noise, sampler_noise=sde)


# ---- the options' entries in `info`, the result dict and the JSON records -----------------------------------------------------
def info_options(opts: JobOptions, rounds) -> dict:
    """The entries `DistributedVideoDiffuser.__call__` adds to `info` after its rounds, in order; `rounds`: the records of
    `co_denoise_round`, one per round (none without `co_denoise`).  Counts and bytes per step are the first round's (every
    round has the same windows), steps and seconds are sums."""
    out = {"guidance_rescale": opts.guidance_rescale} if opts.guidance_rescale != 0 else {}
    if opts.co_denoise:
        first = rounds[0]
        out["co_denoise"] = {"windows": first["windows"], "steps": sum(r["steps"] for r in rounds),
                             "exchange_s": sum(r["exchange_s"] for r in rounds), "bytes_per_step": first["bytes_per_step"]}
        if opts.tile is not None:
            out["tile"] = first["tile"]
        if opts.loop:
            out["loop"] = first["loop"]
        if opts.context_stride > 1:
            out["context_stride"] = out["co_denoise"]["context_stride"] = first["context_stride"]
    out.update(travel_record(opts))
    out.update(region_record(opts))
    out.update(lora_record(opts))
    out.update(prompt_record(opts))
    out.update(mimic_record(opts))
    out.update(noise_record(opts))
    out.update(sampler_noise_record(opts))
    return out


# the option entries of `run_job`'s result dict (after "free_init") and of `main`'s JSON records, in their order
RECORD_KEYS = ("freeu", "tome", "co_denoise", "tile", "loop", "context_stride", "mask", "negative_prompt", "guidance_rescale")


def travel_record(src) -> dict:
    """`{"prompt_travel": {"keys": [[frame, text], ...]}}` beside `record_options`' entries, only when the option is set (else
    {}): from the resolved options, or copied from a dict (`info`, the result) that holds the entry."""
    if isinstance(src, dict):
        return {"prompt_travel": src["prompt_travel"]} if "prompt_travel" in src else {}
    if src.prompt_travel is None:
        return {}
    from .travel import record
    return {"prompt_travel": record(src.prompt_travel)}


def region_record(src) -> dict:
    """`{"regions": {"count", "texts", "coverage"}}` beside `record_options`' entries, only when the option is set (else {}):
    from the resolved options, or copied from a dict (`info`, the result) that holds the entry."""
    if isinstance(src, dict):
        return {"regions": src["regions"]} if "regions" in src else {}
    if src.regions is None:
        return {}
    from .region import record
    return record(src.regions)


def lora_record(src) -> dict:
    """`{"lora": [{"name", "scale", "rank", "unet_modules", "text_modules"}, ...]}` beside `record_options`' entries, only when the
    option is set and its files have been read (else {}): from the resolved options, or copied from a dict (`info`, the result)
    that holds the entry."""
    if isinstance(src, dict):
        return {"lora": src["lora"]} if "lora" in src else {}
    if src.lora_found is None:
        return {}
    return {"lora": [dict(r) for r in src.lora_found]}


def prompt_record(src) -> dict:
    """`{"prompt_syntax": {"syntax", "chunks", "tokens", "weighted"}}` beside `record_options`' entries, only when the option is set
    and the texts have been chunked (else {}): from the resolved options, or copied from a dict (`info`, the result) that holds the
    entry.  `chunks`: the job's k (every text has 77 k positions); `tokens`: per text, in `job_texts`' order."""
    if isinstance(src, dict):
        return {"prompt_syntax": src["prompt_syntax"]} if "prompt_syntax" in src else {}
    if src.prompt_found is None:
        return {}
    return {"prompt_syntax": dict(src.prompt_found)}


def mimic_record(src) -> dict:
    """`{"cfg_mimic": {"scale", "percentile"}}` beside `record_options`' entries, only when the option is set (else {}): from the
    resolved options, or copied from a dict (`info`, the result) that holds the entry."""
    if isinstance(src, dict):
        return {"cfg_mimic": src["cfg_mimic"]} if "cfg_mimic" in src else {}
    if src.cfg_mimic is None:
        return {}
    return {"cfg_mimic": dict(src.cfg_mimic)}


def noise_record(src) -> dict:
    """`{"noise": {"generator": "philox4x32-10/v1", "seed"}}` beside `record_options`' entries, only when the portable generator is
    selected (else {}): from the resolved options, or copied from a dict (`info`, the result) that holds the entry."""
    if isinstance(src, dict):
        return {"noise": src["noise"]} if "noise" in src else {}
    if src.noise is None:
        return {}
    return {"noise": dict(src.noise)}


def sampler_noise_record(src) -> dict:
    """`{"sampler_noise": {"eta", "algorithm"}}` beside `record_options`' entries, only when the job's sampler is stochastic (else
    {}): from the resolved options, or copied from a dict (`info`, the result) that holds the entry."""
    if isinstance(src, dict):
        return {"sampler_noise": src["sampler_noise"]} if "sampler_noise" in src else {}
    if src.sampler_noise is None:
        return {}
    return {"sampler_noise": dict(src.sampler_noise)}


def record_options(res: dict) -> dict:
    """The entries of `RECORD_KEYS` that `res` holds, in that order."""
    return {k: res[k] for k in RECORD_KEYS if k in res}
