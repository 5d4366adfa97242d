"""The stochastic samplers, restated in torch on the CPU (vdx/scheduler.py `DDIMScheduler(eta=)`,
`SDEDPMSolverMultistepScheduler`; csrc/step_noise.h): every scalar a host fp32 0-d tensor in the grouping written, every tensor
operation rounded to fp16, left to right.  The noise w is tests/noise_ref.py's: the portable generator's fp16 N(0, 1) of the
whole clip (1,C,T,h,w) under (seed, stream), of which a sample that is the frames [s, s + L) takes its box.

  DDIM, eta in (0, 1]   var = ((1-a_prev)/(1-a_t)) * (1 - a_t/a_prev), std = eta * var**0.5, dir = (1 - a_prev - std**2)**0.5
                        x0 = (x - sqrt(1-a_t) e) * (1/sqrt(a_t));  x' = sqrt(a_prev) x0 + dir e;  x' = x' + std w
  SDE-DPM-Solver++ 2M   c_x = (st/s0) exp(-h), k = at (1 - exp(-2h)), c_n = st sqrt(1 - exp(-2h))
                        x' = c_x x + k x0 [+ (0.5 k) ((1/r0) (x0 - x0_prev))];  x' = x' + c_n w      (the last step: x' = x0, no draw)
  stream of step i      2^33 + round 2^16 + i, i the index in the full schedule
"""
import numpy as np
import torch

import dpm_ref as D
import noise_ref as N

STREAM_SAMPLER = 2 ** 33
r16 = D.r16


def stream_of_step(rnd: int, i: int) -> int:
    return STREAM_SAMPLER + rnd * 2 ** 16 + i


def clip_noise(shape, seed: int, stream: int, frames=None):
    """fp16 w of the sample: the whole clip's `shape` = (1,C,T,h,w), or with `frames` = (s, L) its frames [s, s + L)."""
    box = None
    if frames is not None:
        s, L = frames
        box = ((0, 0, s, 0, 0), (1, shape[1], L, shape[3], shape[4]))
    return torch.from_numpy(N.normal(shape, seed, stream, box=box))


def add_noise_term(new, c_n: float, w):
    """x' = fp16(x' + fp16(c_n * w))."""
    return r16(new.float() + r16(c_n * w.float())).half()


# ---- DDIM -------------------------------------------------------------------------------------------------------------------
def ddim_timesteps(n):
    return (np.arange(0, n) * (D.N_TRAIN // n)).round()[::-1].copy().astype(np.int64) + D.STEPS_OFFSET


def ddim_scalars(t: int, n: int, eta: float):
    """-> (sqrt(1-a_t), 1/sqrt(a_t) as the kernel forms it, sqrt(a_prev), dir, std) as Python floats holding fp32 values."""
    ac = D.alphas_cumprod()
    prev_t = t - D.N_TRAIN // n
    a_t = ac[t]
    a_prev = ac[prev_t] if prev_t >= 0 else ac[0]
    var = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
    std = eta * var ** 0.5
    direction = (1 - a_prev - std ** 2) ** 0.5
    assert std.dtype == torch.float32 and direction.dtype == torch.float32
    inv_sa = float(np.float32(1.0) / np.float32(float(a_t ** 0.5)))
    return dict(s1=float((1 - a_t) ** 0.5), sa=float(a_t ** 0.5), inv_sa=inv_sa, sp=float(a_prev ** 0.5), dir=float(direction),
                std=float(std))


def ddim_step(e, x, k, w=None):
    """One DDIM update from `ddim_scalars`; `w` None (eta 0): the deterministic step, nothing added."""
    e, x = e.float(), x.float()
    x0 = r16(r16(x - r16(k["s1"] * e)) * k["inv_sa"])
    new = r16(r16(k["sp"] * x0) + r16(k["dir"] * e)).half()
    return new if w is None else add_noise_term(new, k["std"], w)


# ---- SDE-DPM-Solver++ -------------------------------------------------------------------------------------------------------
def sde_scalars(sig, i, second):
    a0, s0, l0 = D.asl(sig[i])
    at, st, lt = D.asl(sig[i + 1])
    h = lt - l0
    k = at * (1.0 - torch.exp(-2.0 * h))
    out = dict(s0=s0, inv_a0=1.0 / a0, cx=(st / s0) * torch.exp(-h), k=k, cn=st * torch.sqrt(1.0 - torch.exp(-2.0 * h)))
    if second:
        _, _, l1 = D.asl(sig[i - 1])
        r0 = (l0 - l1) / h
        out.update(half_k=0.5 * k, inv_r0=1.0 / r0)
    assert all(v.dtype == torch.float32 for v in out.values())
    return {name: float(v) for name, v in out.items()}


def sde_coeffs(k):
    """`sde_scalars` -> the kernel's six coefficients and c_n (include/vdx.h)."""
    return (k["s0"], k["inv_a0"], k["cx"], k["k"], k.get("half_k", 0.0), k.get("inv_r0", 0.0)), k["cn"]


def sde_step(e, x, x0_prev, k, w):
    """-> (x' fp16, x0 fp16); `x0_prev` None: first order; `w` None: no draw (the last step)."""
    e, x = e.float(), x.float()
    x0 = r16(r16(x - r16(k["s0"] * e)) * k["inv_a0"])
    new = r16(r16(k["cx"] * x) + r16(k["k"] * x0))
    if x0_prev is not None:
        d1 = r16(k["inv_r0"] * r16(x0 - x0_prev.float()))
        new = r16(new + r16(k["half_k"] * d1))
    new = new.half()
    return (new if w is None else add_noise_term(new, k["cn"], w)), x0.half()


# ---- trajectories: model(x, t) -> eps2 (2, ...) fp16, CFG at scale gs ---------------------------------------------------------
def ddim_sample(model, x, n, eta, gs, seed, rnd=0, t_start=0):
    ts = ddim_timesteps(n)
    for i in range(t_start, n):
        t = int(ts[i])
        w = clip_noise(tuple(x.shape), seed, stream_of_step(rnd, i)) if eta > 0 else None
        x = ddim_step(D.cfg_combine(model(x, t), gs), x, ddim_scalars(t, n, eta), w)
    return x


def sde_sample(model, x, n, gs, seed, rnd=0, order=2, t_start=0):
    """-> (the final sample, the last step's x0)."""
    ts, sig = D.timesteps(n), D.sigmas(n)
    x0_prev = x0 = None
    for i in range(t_start, n):
        last = i == n - 1
        second = order == 2 and x0_prev is not None and not last
        e = D.cfg_combine(model(x, int(ts[i])), gs)
        if last:
            x, x0 = D.step(e, x, None, D.scalars(sig, i, False))
        else:
            x, x0 = sde_step(e, x, x0_prev if second else None, sde_scalars(sig, i, second), clip_noise(tuple(x.shape), seed, stream_of_step(rnd, i)))
        x0_prev = x0
    return x, x0
