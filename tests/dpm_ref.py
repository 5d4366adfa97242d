"""Torch restatement of the DPM-Solver++ (2M, midpoint) sampler that vdx/scheduler.py `DPMSolverMultistepScheduler` and
csrc/dpm.hip implement: the yardstick of tests/test_dpm_host.py and tests/test_dpm_gpu.py.  Written from the published
definition (Lu et al. 2022, "DPM-Solver++", Algorithm 2 in the data-prediction form; the configuration of diffusers'
`DPMSolverMultistepScheduler` that Zeroscope's recipe uses); it does not import the product scheduler.  diffusers is not
installed, so parity with it is unpinned — as for the other restated dependencies (tests/lpips_ref.py).

  ratio = 1000 // (n+1);  timesteps = (arange(0, n+1) * ratio).round()[::-1][:-1] + 1                  (int64)
  sigmas = interp(timesteps, arange(1000), sqrt((1-abar)/abar)) ++ [0]                                 (fp32, n+1)
  alpha = 1/sqrt(sigma^2+1),  sig = sigma*alpha,  lambda = log(alpha) - log(sig)                       (fp32 host scalars)
  x0 = (x - s0*e) / a0
  first order   x' = (st/s0)*x - (at*(exp(-h)-1))*x0                      no history, order 1, always the last step
  second order  x' = (st/s0)*x - (at*(exp(-h)-1))*x0 - 0.5*(at*(exp(-h)-1))*D1,  D1 = (1/r0)*(x0 - x0_prev), r0 = (l0-l1)/h

Rounding: scalar sub-expressions in fp32 on the host (0-d torch tensors), in the grouping written; every tensor operation
is an fp32 operation on fp16 values rounded to fp16 (what torch does for fp16 tensors against fp32 0-d coefficients on a
GPU), left to right; `/ a0` is `* (1/a0)` (torch-GPU divides by a host scalar that way).  Written with explicit
`.float()` / `.half()`, the tensor part gives the same bits on the CPU and on a GPU.
"""
import numpy as np
import torch

N_TRAIN, BETA_START, BETA_END, STEPS_OFFSET = 1000, 0.00085, 0.012, 1


def alphas_cumprod():
    betas = torch.linspace(BETA_START ** 0.5, BETA_END ** 0.5, N_TRAIN, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def timesteps(n):
    ratio = N_TRAIN // (n + 1)
    return (np.arange(0, n + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + STEPS_OFFSET


def sigmas(n):
    ac = alphas_cumprod()
    sigma_all = (((1 - ac) / ac) ** 0.5).numpy()
    s = np.interp(timesteps(n), np.arange(0, N_TRAIN), sigma_all)
    return torch.from_numpy(np.concatenate([s, [0.0]]).astype(np.float32))


def asl(sigma):
    """(alpha, sig, lambda) of a 0-d fp32 sigma."""
    alpha = 1.0 / torch.sqrt(sigma * sigma + 1.0)
    sig = sigma * alpha
    return alpha, sig, torch.log(alpha) - torch.log(sig)


def scalars(sig, i, second):
    """Host scalars of step i as Python floats holding fp32 values: s0, 1/a0, st/s0, k = at*(exp(-h)-1), 0.5*k, 1/r0."""
    a0, s0, l0 = asl(sig[i])
    at, st, lt = asl(sig[i + 1])
    h = lt - l0
    k = at * (torch.exp(-h) - 1.0)
    out = dict(s0=s0, inv_a0=1.0 / a0, cx=st / s0, k=k)
    if second:
        _, _, l1 = asl(sig[i - 1])
        r0 = (l0 - l1) / h
        out.update(half_k=0.5 * k, inv_r0=1.0 / r0)
    assert all(v.dtype == torch.float32 for v in out.values())
    return {name: float(v) for name, v in out.items()}


def r16(x):
    return x.half().float()


def cfg_combine(eps2, gs):
    """u + gs*(c-u) on fp16 tensors, fp16 after each op -> fp16."""
    u, c = eps2.float().chunk(2)
    return r16(u + r16(gs * r16(c - u))).half()


def step(e, x, x0_prev, k):
    """One update from the scalars `k` (`scalars`): -> (x' fp16, x0 fp16).  `x0_prev=None`: first order."""
    e, x = e.float(), x.float()
    x0 = r16(r16(x - r16(k["s0"] * e)) * k["inv_a0"])
    new = r16(r16(k["cx"] * x) - r16(k["k"] * x0))
    if x0_prev is not None:
        d1 = r16(k["inv_r0"] * r16(x0 - x0_prev.float()))
        new = r16(new - r16(k["half_k"] * d1))
    return new.half(), x0.half()


def sample(model, x, n, order=2, t_start=0):
    """Run steps t_start..n-1 of an n-step schedule from `x` (fp16, any device) with `model(x, t) -> eps` fp16.  Returns the
    final sample and the list of (x', x0) per step.  The first step run has no history, the last one is first order."""
    ts, sig = timesteps(n), sigmas(n)
    x0_prev, trace = None, []
    for i in range(t_start, n):
        second = order == 2 and x0_prev is not None and i != n - 1
        x, x0 = step(model(x, int(ts[i])), x, x0_prev if second else None, scalars(sig, i, second))
        trace.append((x, x0))
        x0_prev = x0
    return x, trace


# ---- the toy problem with a closed-form answer: data ~ N(0, s^2), s = 2 ------------------------------------------------------
TOY_S = 2.0


def toy_eps(x, t, ac=None):
    """eps*(x, t) = sqrt(1-abar_t) * x / (abar_t*s^2 + 1-abar_t): the exact noise prediction for Gaussian data; one fp32
    host scalar times the fp16 tensor, rounded to fp16."""
    ac = alphas_cumprod() if ac is None else ac
    a = ac[t]
    k = float(torch.sqrt(1 - a) / (a * TOY_S ** 2 + (1 - a)))
    return (x.float() * k).half()


def toy_exact(x_T, t_first):
    """The probability-flow ODE's solution at t = 0 (abar = 1) from x_T at t_first (fp64)."""
    a = alphas_cumprod()[t_first].double()
    return x_T.double() * torch.sqrt(TOY_S ** 2 / (a * TOY_S ** 2 + 1 - a))


def toy_start(device="cpu"):
    g = torch.Generator().manual_seed(0)
    return torch.randn(1, 4, 3, 8, 16, generator=g).half().to(device)


def rel_err(x, exact):
    return float((x.double().cpu() - exact.cpu()).norm() / exact.cpu().norm())
