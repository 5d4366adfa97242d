"""`DDIMScheduler` with the diffusers call surface the reference uses
(`fsdp_chunked_coherent.py:95,115,132,133,142,182`): `set_timesteps(n, device=)`, `.timesteps`,
`.scale_model_input(x, t)`, `.step(eps, t, x).prev_sample`, `.init_noise_sigma`.

Schedule tables (betas, cumulative alphas, timesteps) are host logic; the sample update runs in
the fused HIP kernel (`vdx_ddim_step_f16` / `vdx_cfg_ddim_step_f16`) — there is no CPU step.
Config = Zeroscope `scheduler_config.json`: 1000 train steps,
scaled-linear betas 0.00085..0.012, steps_offset 1, set_alpha_to_one False, epsilon, eta 0,
leading spacing, no clipping.

`DPMSolverMultistepScheduler` (DPM-Solver++ 2M, the sampler Zeroscope's published recipe swaps in) has the same call
surface and is opt-in; DDIM stays the default everywhere.  Both have a stochastic form, opt-in too (`DDIMScheduler(eta=)`,
`SDEDPMSolverMultistepScheduler`, diffusers' `algorithm_type="sde-dpmsolver++"`): the same kernels plus the seeded generator's draw (`seed_noise`; csrc/step_noise.h).  Both share `_SchedulerBase`: the sync-free timestep lookup and
`add_noise`.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops

# The fused steps: (noise source, guidance) -> (the statistics op or None, the step's (DDIM, DPM-Solver++) pair), as the names of
# `ops` functions, looked up at the call.  The sources: "one" buffer eps2 = [u; c], else the whole clip's noise fused from "windows",
# "tiles", "ring" windows or "strided" ones.  A missing key is a combination that has no kernel.
_STEPS = {
    ("one", "plain"): (None, ("cfg_ddim_step", "cfg_dpm_step")),
    ("one", "rescale"): ("cfg_rescale_stats", ("cfg_rescale_ddim_step", "cfg_rescale_dpm_step")),
    ("one", "mimic"): ("cfg_mimic_stats", ("cfg_mimic_ddim_step", "cfg_mimic_dpm_step")),
    ("windows", "plain"): (None, ("cofuse_cfg_ddim_step", "cofuse_cfg_dpm_step")),
    ("windows", "rescale"): ("cofuse_cfg_rescale_stats", ("cofuse_cfg_rescale_ddim_step", "cofuse_cfg_rescale_dpm_step")),
    ("windows", "mimic"): ("cofuse_cfg_mimic_stats", ("cofuse_cfg_mimic_ddim_step", "cofuse_cfg_mimic_dpm_step")),
    ("tiles", "plain"): (None, ("cotile_cfg_ddim_step", "cotile_cfg_dpm_step")),
    ("ring", "plain"): (None, ("coloop_cfg_ddim_step", "coloop_cfg_dpm_step")),
    ("strided", "plain"): (None, ("costride_cfg_ddim_step", "costride_cfg_dpm_step")),
    # the stochastic forms (DDIM with eta > 0, SDE-DPM-Solver++): the plain step plus the seeded generator's draw, in the same kernel
    ("one", "noise"): (None, ("cfg_ddim_eta_step", "cfg_sde_dpm_step")),
    ("windows", "noise"): (None, ("cofuse_cfg_ddim_eta_step", "cofuse_cfg_sde_dpm_step")),
}


class _SchedulerBase:
    """What the schedulers share: the call-surface constants, the sync-free timestep lookup, `add_noise`, and a `reset()`
    that single-step schedulers have nothing to do in."""
    init_noise_sigma = 1.0
    order = 1
    timesteps = None
    _host_timesteps = None
    rescale_stats = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def reset(self):
        """Forget what earlier `step` calls left behind (multistep history, step index).  Nothing for DDIM."""

    def _host_timestep(self, timestep) -> int:
        """The step's timestep as a host integer, by VALUE (diffusers semantics) and — for the tensors the reference
        hands in — without reading device memory.  The reference passes `step` the 0-d device tensors it iterates
        over (`for t in scheduler.timesteps`, :132,142); `int(t)` on those is a device sync per step.  Such an element
        is a view of `self.timesteps`' storage, so its index is its address: (data_ptr - base) / itemsize, checked
        against the storage's extent.  Any other device tensor (a clone, arithmetic on a timestep, a foreign schedule)
        is read with `int(t)` — one sync, never a guess.  Python numbers and host tensors are used as given."""
        if torch.is_tensor(timestep) and timestep.is_cuda:
            ts = self.timesteps
            if ts is not None and ts.is_cuda and timestep.numel() == 1 and timestep.dtype == ts.dtype \
                    and timestep.device == ts.device \
                    and timestep.untyped_storage().data_ptr() == ts.untyped_storage().data_ptr():
                off = timestep.data_ptr() - ts.data_ptr()
                idx, rem = divmod(off, ts.element_size())
                if rem == 0 and 0 <= idx < ts.numel():
                    return self._host_timesteps[idx]
            return int(timestep)
        return int(timestep)

    def _rescale(self, guidance_rescale, device):
        """CFG rescale (csrc/rescale.hip): `ops.rescale_factors(guidance_rescale)` and this scheduler's 3 halves on `device` that
        every rescaled step leaves [sd_c, sd_g, r] in (`rescale_stats`: read it after the loop, never inside)."""
        st = self.rescale_stats
        if st is None or st.device != device:
            st = self.rescale_stats = torch.zeros(8, dtype=torch.float16, device=device)
        return ops.rescale_factors(guidance_rescale), st

    def _mimic(self, cfg_mimic, percentile, sample):
        """Dynamic thresholding (csrc/dynthresh.hip): `ops.mimic_factors` of the sample's channel size, kept per (scale, percentile,
        size): the float64 rank is formed once."""
        if sample.dim() != 5:
            raise ValueError("cfg_mimic needs a (1,C,T,H,W) sample: the statistics are per channel")
        key = (cfg_mimic, percentile, sample.shape[2] * sample.shape[3] * sample.shape[4])
        if self._mimic_factors is None or self._mimic_factors[0] != key:
            self._mimic_factors = (key, ops.mimic_factors(*key))
        return self._mimic_factors[1]

    _mimic_factors = None
    _dpm = None         # False / True: which of an `ops` step's two forms, (DDIM, DPM-Solver++), this scheduler launches
    _noise_seed = None  # (seed, round) of `seed_noise`: what a stochastic step draws from

    def seed_noise(self, seed, round: int = 0):
        """What this scheduler's stochastic steps draw from: the portable generator (vdx/noise.py) under `seed`, step i of the
        schedule on `stream_of_step(round, i)`.  `round`: the sampling round (the FreeInit iteration less one).  A deterministic
        scheduler (eta 0, "dpmsolver++") never reads it.  None: forget the seed."""
        from . import noise as _noise
        if seed is None:
            self._noise_seed = None
            return
        _noise.stream_of_step(round, 0)
        self._noise_seed = (_noise.check_seed(seed), round)

    def _draw(self, c_n: float, i: int):
        """A stochastic step's `noise` argument of the `ops` steps, (c_n, seed, stream), for step `i` of the full schedule."""
        from . import noise as _noise
        if self._noise_seed is None:
            raise ValueError("a stochastic step (eta > 0, \"sde-dpmsolver++\") draws from the seeded generator: call "
                             "seed_noise(seed, round) first (the torch stream has no per-step form)")
        seed, rnd = self._noise_seed
        return (c_n, seed, _noise.stream_of_step(rnd, i))

    def _begin(self, timestep, sample):
        """The one hook of the `step_cfg*` methods -> (this step's coefficients, the `ops` step's history keywords, what to call
        once the kernel was enqueued, a stochastic step's `_draw` or None).  It changes nothing that a launch which raises would
        have to undo."""
        raise NotImplementedError

    def _fused_step(self, source, head, timestep, sample, guidance_scale, guidance_rescale=0.0, cfg_mimic=None, cfg_mimic_percentile=1.0,
                    frames=None):
        """One fused step of `_STEPS[source, guide]` on `head`, the ops' leading arguments (the noise, then the latent).  Plain: one
        launch.  `guidance_rescale` != 0 (csrc/rescale.hip): the statistics op, then the rescaled step, two launches.  `cfg_mimic`
        (csrc/dynthresh.hip): four launches, the statistics in `ops`' per-stream workspace.  Never a host read.  A stochastic
        step (`_begin` gave a draw): `_STEPS[source, "noise"]`, still one launch; `frames` = (s, T), the one-buffer sample's place
        in the clip."""
        if cfg_mimic is not None and guidance_rescale != 0.0:
            raise ValueError("cfg_mimic and guidance_rescale exclude each other: both rewrite the guided noise, and no order is defined")
        guide = "mimic" if cfg_mimic is not None else "rescale" if guidance_rescale != 0.0 else "plain"
        stats_name, step_names = _STEPS[source, guide]
        step, stats_op = getattr(ops, step_names[self._dpm]), stats_name and getattr(ops, stats_name)
        coeffs, history, commit, draw = self._begin(timestep, sample)
        if draw is not None:
            if guide != "plain" or (source, "noise") not in _STEPS:
                raise ValueError(f"a stochastic step (eta > 0, sde-dpmsolver++) has no noise form yet for the {source!r} / {guide!r} step")
            step = getattr(ops, _STEPS[source, "noise"][1][self._dpm])
            res = step(*head, guidance_scale, coeffs, draw, **({"frames": frames} if source == "one" else {}), **history)
            commit()
            return res[0] if self._dpm else res
        noise = head[:1] if source == "one" else head             # what the statistics read: eps2, or (z for its shape, the windows ...)
        if guide == "mimic":
            ws = stats_op(*noise, guidance_scale, self._mimic(cfg_mimic, cfg_mimic_percentile, sample))
            res = step(*head, guidance_scale, coeffs, ws, **history)
        elif guide == "rescale":
            rescale, stats = self._rescale(guidance_rescale, sample.device)
            part = stats_op(*noise, guidance_scale)
            res = step(*head, guidance_scale, rescale, coeffs, part, stats_out=stats, **history)
        else:
            res = step(*head, guidance_scale, coeffs, **history)
        commit()
        return res[0] if self._dpm else res                       # the DPM-Solver++ ops return (the new latent, x0)

    def step_cfg(self, noise2, timestep, sample, guidance_scale: float, guidance_rescale: float = 0.0, cfg_mimic=None,
                 cfg_mimic_percentile: float = 1.0, frames=None):
        """Fused `u + gs*(c-u)` + step (fsdp_chunked_coherent.py:141-142) in one kernel (`vdx_cfg_ddim_step_f16` /
        `vdx_cfg_dpm_step_f16`).  `guidance_rescale` != 0 (Lin et al. 2023, diffusers' `rescale_noise_cfg`; csrc/rescale.hip): the
        guided noise is rescaled towards the standard deviation of the conditional one over this sample, in two launches (the
        statistics, then the step) and without a host read.  `cfg_mimic` (a mimic scale; dynamic thresholding, csrc/dynthresh.hip):
        every channel of the guided noise, less its mean, is clamped at the `cfg_mimic_percentile` quantile of its magnitude and
        squeezed into the range the same prediction has at the mimic scale, in four launches and without a host read.  Not both.
        `frames` = (s, T) (read by a stochastic step only): the sample is the frames [s, s + L) of a clip of T frames, and draws
        the clip's noise at those frames; None: the sample is the clip."""
        if self._dpm or guidance_rescale != 0.0 or cfg_mimic is not None:   # the plain DDIM op refuses a non-contiguous sample itself
            sample = sample.contiguous()
        return self._fused_step("one", (noise2, sample), timestep, sample, guidance_scale, guidance_rescale, cfg_mimic, cfg_mimic_percentile,
                                frames)

    def step_cfg_windows(self, windows, table, wn, timestep, sample, guidance_scale: float, guidance_rescale: float = 0.0,
                         cfg_mimic=None, cfg_mimic_percentile: float = 1.0, frames=None):
        """Co-denoising (vdx/codenoise.py): `step_cfg` of the whole clip's latent `sample` on the noise fused from the
        windows' raw UNet outputs in `windows` (`table`, `wn`: `ops.cofuse_cfg_ddim_step` / `ops.cofuse_cfg_dpm_step`), one
        kernel; with `guidance_rescale` != 0 two, with `cfg_mimic` four, the statistics being those of the fused noise over the
        whole clip.  `frames`: None only, the sample is the clip (a stochastic step draws the clip's noise)."""
        if frames is not None:
            raise ValueError("step_cfg_windows: the sample is the whole clip, frames must be None")
        sample = sample.contiguous()
        return self._fused_step("windows", (sample, windows, table, wn), timestep, sample, guidance_scale, guidance_rescale, cfg_mimic,
                                cfg_mimic_percentile)

    def step_cfg_tiles(self, windows, table, wn, tiles, timestep, sample, guidance_scale: float):
        """Spatially tiled co-denoising (vdx/codenoise.py `tile_plan`): `step_cfg_windows` with every time window's block holding
        its row x column tiles' outputs (`tiles`: an `ops.TileGrid`; `ops.cotile_cfg_ddim_step` / `ops.cotile_cfg_dpm_step`), one
        kernel.  There is no `guidance_rescale` form: its statistics pass has no tiled fuse."""
        sample = sample.contiguous()
        return self._fused_step("tiles", (sample, windows, table, wn, tiles), timestep, sample, guidance_scale)

    def step_cfg_loop(self, windows, table, wn, timestep, sample, guidance_scale: float):
        """Seamless looping (vdx/codenoise.py `loop_plan`): `step_cfg_windows` with every window on a ring, a `table` row
        (offset, s, L) meaning the frames (s + f) mod T (`ops.coloop_cfg_ddim_step` / `ops.coloop_cfg_dpm_step`), one kernel.
        No `guidance_rescale` form."""
        sample = sample.contiguous()
        return self._fused_step("ring", (sample, windows, table, wn), timestep, sample, guidance_scale)

    def step_cfg_strided(self, windows, table, wn, timestep, sample, guidance_scale: float):
        """Strided context windows (vdx/codenoise.py `stride_plan`): `step_cfg_windows` with a `table` row (offset, s, L, d)
        meaning the frames s + f * d (`ops.costride_cfg_ddim_step` / `ops.costride_cfg_dpm_step`), one kernel.
        No `guidance_rescale` form."""
        sample = sample.contiguous()
        return self._fused_step("strided", (sample, windows, table, wn), timestep, sample, guidance_scale)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers `DDIMScheduler.add_noise` for one timestep: alphas_cumprod is cast to the sample dtype (fp16) FIRST,
        then sqrt(a_t) and sqrt(1 - a_t) are fp16 tensor ops (evaluated here with torch on the sample's device, as diffusers
        does), then x_t = sqrt(a_t)*x0 + sqrt(1-a_t)*noise in the HIP kernel with fp16 rounding after each op.  Unpinned
        boundary (diffusers is not installed: DESIGN §2)."""
        sa, s1 = self.add_noise_coefficients(timesteps, original_samples)
        return ops.add_noise(original_samples.contiguous(), noise.contiguous(), sa, s1)

    def add_noise_coefficients(self, timesteps, like):
        """`add_noise`'s two scalars for one timestep, (sqrt(a_t), sqrt(1 - a_t)), evaluated as it always evaluated them: in
        `like`'s dtype on `like`'s device.  The masked job (vdx/inpaint.py) computes them once per step of its schedule."""
        t = self._host_timestep(timesteps) if torch.is_tensor(timesteps) else int(timesteps)
        if not 0 <= t < len(self.alphas_cumprod):
            raise ValueError(f"add_noise: timestep {t} is outside the {len(self.alphas_cumprod)} training steps")
        ac = self.alphas_cumprod.to(device=like.device, dtype=like.dtype)
        return float(ac[t] ** 0.5), float((1 - ac[t]) ** 0.5)


class DDIMScheduler(_SchedulerBase):
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                 beta_schedule="scaled_linear", steps_offset=1, set_alpha_to_one=False,
                 clip_sample=False, prediction_type="epsilon", timestep_spacing="leading", eta: float = 0.0):
        self.eta = self._check_eta(eta)
        if beta_schedule != "scaled_linear" or clip_sample or prediction_type != "epsilon" \
                or timestep_spacing != "leading":
            raise NotImplementedError("only the Zeroscope DDIM configuration is implemented")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start,
                                      beta_end=beta_end, beta_schedule=beta_schedule,
                                      steps_offset=steps_offset, set_alpha_to_one=set_alpha_to_one,
                                      clip_sample=clip_sample, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = None
        self._host_timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        n_train = self.config.num_train_timesteps
        if num_inference_steps > n_train:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = n_train // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        ts += self.config.steps_offset
        self._host_timesteps = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device)

    @staticmethod
    def _check_eta(eta) -> float:
        import math
        if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not math.isfinite(eta) or not 0 <= eta <= 1:
            raise ValueError(f"eta must be a finite number in [0, 1], got {eta!r}")
        return float(eta)

    def coefficients(self, t: int):
        """(sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev)) evaluated in fp32 like diffusers."""
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return (float((1 - a_t) ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))

    def eta_coefficients(self, t: int, eta: float):
        """eta > 0 (diffusers `DDIMScheduler.step`, fp32 0-d tensors in the grouping written): var = ((1-a_prev)/(1-a_t)) *
        (1 - a_t/a_prev), std = eta * var**0.5 -> ((sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1 - a_prev - std**2)), std): the
        step's four coefficients, the direction's in the place of sqrt(1-a_prev), and the noise's factor c_n."""
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
        std = eta * var ** 0.5
        direction = (1 - a_prev - std ** 2) ** 0.5
        assert std.dtype == torch.float32 and direction.dtype == torch.float32
        return (float((1 - a_t) ** 0.5), float(a_t ** 0.5), float(a_prev ** 0.5), float(direction)), float(std)

    def step(self, model_output, timestep, sample, eta=None, variance_noise=None, generator=None, **_unused):
        """`eta` None: the scheduler's own (`DDIMScheduler(eta=)`, 0 by default).  eta > 0 draws from the seeded generator
        (`seed_noise`) on the sample as the logical tensor."""
        if variance_noise is not None or generator is not None:
            raise NotImplementedError("variance_noise= / generator= are not taken: a stochastic step draws from the seeded generator "
                                      "philox4x32-10/v1 inside its kernel (seed_noise(seed, round))")
        eta = self.eta if eta is None else self._check_eta(eta)
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        t = self._host_timestep(timestep)
        if eta == 0.0:
            prev = ops.ddim_step(model_output.contiguous(), sample.contiguous(), self.coefficients(t))
        else:
            coeffs, std = self.eta_coefficients(t, eta)
            prev = ops.ddim_eta_step(model_output.contiguous(), sample.contiguous(), coeffs, self._draw(std, self._index_of(t)))
        return SimpleNamespace(prev_sample=prev)

    def _index_of(self, t: int) -> int:
        if t not in self._host_timesteps:
            raise ValueError(f"timestep {t} is not in the schedule set for {self.num_inference_steps} steps")
        return self._host_timesteps.index(t)

    _dpm = False

    def _begin(self, timestep, sample):
        t = self._host_timestep(timestep)
        if self.eta == 0.0:
            return self.coefficients(t), {}, lambda: None, None
        coeffs, std = self.eta_coefficients(t, self.eta)
        return coeffs, {}, lambda: None, self._draw(std, self._index_of(t))


class DPMSolverMultistepScheduler(_SchedulerBase):
    """DPM-Solver++ 2M (Lu et al., 2022; diffusers `DPMSolverMultistepScheduler`, which Zeroscope's published recipe swaps in
    with `from_config(pipe.scheduler.config)`), with `DDIMScheduler`'s call surface.  Opt-in: DDIM stays the default.

    Implemented: algorithm_type "dpmsolver++" (its stochastic form "sde-dpmsolver++" is the subclass `SDEDPMSolverMultistepScheduler`,
    which `from_config(..., algorithm_type="sde-dpmsolver++")` builds), solver_order 2 (or 1), solver_type "midpoint", epsilon prediction, no
    thresholding, lower_order_final, final_sigmas_type "zero", leading spacing, steps_offset 1, scaled-linear betas; anything
    else raises NotImplementedError.  diffusers is not installed, so — exactly as for DDIM — the schedule and the expression
    below are RESTATED and their parity with diffusers is unpinned; what is pinned, bit for bit, is the HIP kernel against
    this expression (tests/test_dpm_gpu.py against tests/dpm_ref.py).

      ratio = n_train // (n+1);  timesteps = (arange(0, n+1) * ratio).round()[::-1][:-1] + steps_offset        (int64)
      sigmas = interp(timesteps, arange(n_train), sqrt((1-abar)/abar)) ++ [0]                                  (fp32, n+1)
               (n = 999 is the one schedule whose first timestep, 1000, lies past the training range: `interp` clamps its
                sigma to that of timestep 999, as diffusers' does, and the sampler runs; `add_noise` and the miner trace,
                which read alphas_cumprod[t], refuse that timestep with a ValueError)
      for a sigma:  alpha = 1/sqrt(sigma^2+1),  sig = sigma*alpha,  lambda = log(alpha) - log(sig)             (fp32, host)
      step i, sample x, fp16 model output e:  (a0, s0, l0) from sigmas[i], (at, st, lt) from sigmas[i+1], h = lt - l0
        x0 = (x - s0*e) / a0                                               (kept in fp16: the next step's history)
        first order   x' = (st/s0)*x - (at*(exp(-h)-1))*x0                 (no history, solver_order 1, ALWAYS the last step)
        second order  x' = (st/s0)*x - (at*(exp(-h)-1))*x0 - 0.5*(at*(exp(-h)-1))*D1,
                      D1 = (1/r0)*(x0 - x0_prev),  r0 = (l0 - l1)/h,  l1 from sigmas[i-1]
    Every scalar sub-expression is evaluated on the host in fp32 (0-d torch tensors) in the grouping written; every tensor
    operation rounds to fp16, left to right; `/ a0` is `* (1/a0)` (csrc/dpm.hip).  On the last step sigma is 0: st/s0 = 0,
    h = +inf, exp(-h) = 0, and x' is x0.

    The step index is found by VALUE on the first `step` after `set_timesteps` / `reset()` (a video-to-video run starts
    mid-schedule, and its first step is first-order) and then counts up; a timestep that does not continue the schedule is an
    error — call `reset()` between trajectories (`DistributedVideoDiffuser.denoise` does, per chunk).  The x0 history
    ping-pongs two buffers allocated once per `set_timesteps` and shape."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 steps_offset=1, prediction_type="epsilon", timestep_spacing="leading", algorithm_type="dpmsolver++",
                 solver_order=2, solver_type="midpoint", thresholding=False, lower_order_final=True,
                 final_sigmas_type="zero"):
        if beta_schedule != "scaled_linear" or prediction_type != "epsilon" or timestep_spacing != "leading" \
                or algorithm_type != self._ALGORITHM or solver_order not in (1, 2) or solver_type != "midpoint" \
                or thresholding or not lower_order_final or final_sigmas_type != "zero" or steps_offset != 1:
            raise NotImplementedError("only the Zeroscope DPM-Solver++ (2M, midpoint) configuration is implemented (its stochastic form, "
                                      "\"sde-dpmsolver++\": SDEDPMSolverMultistepScheduler, or from_config(..., algorithm_type=\"sde-dpmsolver++\"))")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, steps_offset=steps_offset,
                                      prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                                      algorithm_type=algorithm_type, solver_order=solver_order, solver_type=solver_type,
                                      thresholding=thresholding, lower_order_final=lower_order_final,
                                      final_sigmas_type=final_sigmas_type)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.num_inference_steps = None
        self.timesteps = None
        self._host_timesteps = None
        self.sigmas = None
        self._x0 = None
        self.reset()

    _ALGORITHM = "dpmsolver++"      # the one algorithm_type this class runs; `SDEDPMSolverMultistepScheduler`: "sde-dpmsolver++"
    _CONFIG_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "steps_offset", "prediction_type",
                    "timestep_spacing", "algorithm_type", "solver_order", "solver_type", "thresholding", "lower_order_final",
                    "final_sigmas_type")

    @classmethod
    def from_config(cls, config, **overrides):
        """`DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`: the keys both schedulers know are taken from
        `config` (a `DDIMScheduler.config`, this class's own, or a dict); DDIM-only keys are ignored.  The resulting
        `algorithm_type` chooses the class: "sde-dpmsolver++" gives an `SDEDPMSolverMultistepScheduler`, "dpmsolver++" this one."""
        get = config.get if isinstance(config, dict) else lambda k, d=None: getattr(config, k, d)
        kw = {k: get(k) for k in cls._CONFIG_KEYS if get(k, None) is not None}
        kw.update(overrides)
        by_algorithm = {c._ALGORITHM: c for c in (DPMSolverMultistepScheduler, SDEDPMSolverMultistepScheduler)}
        return by_algorithm.get(kw.get("algorithm_type", cls._ALGORITHM), cls)(**kw)

    def reset(self):
        self._step_index = None
        self._have_prev = False
        self._cur = 0

    def set_timesteps(self, num_inference_steps: int, device=None):
        n_train = self.config.num_train_timesteps
        if not 0 < num_inference_steps < n_train:
            raise ValueError("num_inference_steps must be in [1, num_train_timesteps)")
        self.num_inference_steps = n = num_inference_steps
        ratio = n_train // (n + 1)
        ts = (np.arange(0, n + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64)
        ts += self.config.steps_offset
        sigma_all = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sig = np.interp(ts, np.arange(0, n_train), sigma_all)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self._host_timesteps = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(ts).to(device)
        self._coef = {}
        self._x0 = None
        self.reset()

    @staticmethod
    def _alpha_sigma_lambda(sigma):
        alpha = 1.0 / torch.sqrt(sigma * sigma + 1.0)
        sig = sigma * alpha
        return alpha, sig, torch.log(alpha) - torch.log(sig)

    def coefficients(self, i: int, second_order: bool):
        """Step i's host scalars for the kernel: (s0, 1/a0, st/s0, c_d0, c_d1, 1/r0) with c_d0 = -(at*(exp(-h)-1)) and
        c_d1 = -(0.5*(at*(exp(-h)-1))); first order: c_d1 = 1/r0 = 0.  The last step's are (.., .., 0, 1, ..): x' = x0."""
        key = (i, bool(second_order))
        if key not in self._coef:
            a0, s0, l0 = self._alpha_sigma_lambda(self.sigmas[i])
            at, st, lt = self._alpha_sigma_lambda(self.sigmas[i + 1])
            h = lt - l0
            k = at * (torch.exp(-h) - 1.0)
            c = [s0, 1.0 / a0, st / s0, -k, torch.zeros(()), torch.zeros(())]
            if second_order:
                _, _, l1 = self._alpha_sigma_lambda(self.sigmas[i - 1])
                r0 = (l0 - l1) / h
                c[4], c[5] = -(0.5 * k), 1.0 / r0
            assert all(v.dtype == torch.float32 for v in c)
            self._coef[key] = tuple(float(v) for v in c)
        return self._coef[key]

    @property
    def stochastic(self) -> bool:
        return self.config.algorithm_type == "sde-dpmsolver++"

    def sde_coefficients(self, i: int, second_order: bool):
        """SDE-DPM-Solver++ (2M, midpoint; diffusers `algorithm_type="sde-dpmsolver++"`), with (a0, s0, l0), (at, st, lt), h and r0
        as `coefficients` forms them: c_x = (st/s0)*exp(-h), k = at*(1 - exp(-2h)), c_d0 = k, c_d1 = 0.5*k, c_n = st*sqrt(1 -
        exp(-2h)) -> ((s0, 1/a0, c_x, c_d0, c_d1, 1/r0), c_n); first order: c_d1 = 1/r0 = 0.  The last step's (sigma 0) are
        (.., .., 0, 1, ..) and c_n = 0: x' = x0, and the scheduler launches the deterministic kernel there, with no draw."""
        key = ("sde", i, bool(second_order))
        if key not in self._coef:
            a0, s0, l0 = self._alpha_sigma_lambda(self.sigmas[i])
            at, st, lt = self._alpha_sigma_lambda(self.sigmas[i + 1])
            h = lt - l0
            k = at * (1.0 - torch.exp(-2.0 * h))
            c = [s0, 1.0 / a0, (st / s0) * torch.exp(-h), k, torch.zeros(()), torch.zeros(()), st * torch.sqrt(1.0 - torch.exp(-2.0 * h))]
            if second_order:
                _, _, l1 = self._alpha_sigma_lambda(self.sigmas[i - 1])
                r0 = (l0 - l1) / h
                c[4], c[5] = 0.5 * k, 1.0 / r0
            assert all(v.dtype == torch.float32 for v in c)
            c = tuple(float(v) for v in c)
            self._coef[key] = (c[:6], c[6])
        return self._coef[key]

    def _step_coefficients(self, i: int, second_order: bool):
        """-> (the step's six coefficients, its draw or None): the deterministic ones, or the SDE's; the SDE's last step is
        deterministic (c_n = 0, x' = x0) and runs the existing kernel."""
        if not self.stochastic or i == self.num_inference_steps - 1:
            return self.coefficients(i, second_order), None
        coeffs, c_n = self.sde_coefficients(i, second_order)
        return coeffs, self._draw(c_n, i)

    def _plan(self, timestep, sample):
        """-> (step index, x0_prev or None, x0_out) for this step.  Changes nothing a failed launch would have to undo: the
        index moves and the history buffers flip in `_commit`, after the kernel was enqueued."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        t = self._host_timestep(timestep)
        n = self.num_inference_steps
        if self._step_index is None:
            if t not in self._host_timesteps:
                raise ValueError(f"timestep {t} is not in the schedule set for {n} steps")
            i = self._host_timesteps.index(t)
        else:
            i = self._step_index
        if i >= n or self._host_timesteps[i] != t:
            raise ValueError(f"timestep {t} does not continue the schedule (step index {i} of {n}): call reset() before a new "
                             "trajectory")
        key = (tuple(sample.shape), sample.device)
        if self._x0 is None or self._x0[0] != key:
            if self._have_prev:
                raise ValueError("the sample's shape or device changed in mid-trajectory: call reset() first")
            self._x0 = (key, [torch.empty_like(sample, memory_format=torch.contiguous_format) for _ in range(2)])
        bufs = self._x0[1]
        second = self._have_prev and self.config.solver_order == 2 and i != n - 1
        return i, (bufs[1 - self._cur] if second else None), bufs[self._cur]

    def _commit(self, i: int):
        self._cur ^= 1
        self._have_prev = True
        self._step_index = i + 1

    def step(self, model_output, timestep, sample, **_unused):
        sample = sample.contiguous()
        i, prev, x0_out = self._plan(timestep, sample)
        coeffs, draw = self._step_coefficients(i, prev is not None)
        if draw is None:
            new, _ = ops.dpm_step(model_output.contiguous(), sample, coeffs, x0_prev=prev, x0_out=x0_out)
        else:
            new, _ = ops.sde_dpm_step(model_output.contiguous(), sample, coeffs, draw, x0_prev=prev, x0_out=x0_out)
        self._commit(i)
        return SimpleNamespace(prev_sample=new)

    _dpm = True

    def _begin(self, timestep, sample):
        """ONE x0 history of the sample's shape (with co-denoising the whole clip's; `reset()` once per round), planned here and
        committed by the returned callable after the kernel was enqueued."""
        i, prev, x0_out = self._plan(timestep, sample)
        coeffs, draw = self._step_coefficients(i, prev is not None)
        return coeffs, {"x0_prev": prev, "x0_out": x0_out}, lambda: self._commit(i), draw


class SDEDPMSolverMultistepScheduler(DPMSolverMultistepScheduler):
    """SDE-DPM-Solver++ 2M (diffusers `DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")`, A1111's "DPM++ 2M SDE"): the
    same schedule, history and kernels with `sde_coefficients` and, at the end of every step but the last, the seeded generator's
    draw (`seed_noise`; csrc/step_noise.h).  A class of its own, so that `DPMSolverMultistepScheduler(...)` keeps refusing every
    algorithm_type but its own; `DPMSolverMultistepScheduler.from_config(config, algorithm_type="sde-dpmsolver++")` builds this one."""
    _ALGORITHM = "sde-dpmsolver++"

    def __init__(self, *args, algorithm_type="sde-dpmsolver++", **kw):
        super().__init__(*args, algorithm_type=algorithm_type, **kw)
