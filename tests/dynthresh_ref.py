"""Torch-CPU restatement of dynamic thresholding of the guided noise with a mimic scale as csrc/dynthresh.hip computes it: the
yardstick of tests/test_dynthresh_host.py and tests/test_dynthresh_gpu.py.  Restated, not pinned externally: no implementation of
the "Dynamic Thresholding (CFG Scale Fix)" extension is installed, so these lines ARE the specification.  It does not import the
product's kernels.  Over ONE sample eps2 = [u; c] fp16 of shape (2, C, T, h, w), M = T h w, per channel:

    g   = cfg_combine(u, c, gs)        l = cfg_combine(u, c, ms)               tests/dpm_ref.py `cfg_combine`, twice
    mg  = fp16(sum g / M),  ml = fp16(sum l / M)                               float64 sums, one division, ONE rounding to fp16
    d   = fp16(g - mg)                 e = fp16(l - ml)
    ref_lo = max |e| as the integer bits(e) & 0x7fff                            (a NaN pattern is above infinity's and wins)
    a   = the channel's bits(d) & 0x7fff, sorted ascending (`torch.sort` on integers)
    pos = q (M - 1) in float64,  k = floor(pos),  f = fp32(pos - k),  lo = a[k],  hi = a[min(k + 1, M - 1)]
    ref_hi = lo's bits when f == 0, else fp16(lo + fp32(f * fp32(hi - lo)))
    s   = whichever of ref_lo, ref_hi has the larger bit pattern
    dc  = d > s ? s : (d < -s ? -s : d)                                         float compares: a NaN d stays NaN
    g'  = fp16(fp16(fp16(dc / s) * ref_lo) + mg)

and g' goes where g went (DDIM: tests/codenoise_ref.py `ddim_chain`; DPM-Solver++: tests/dpm_ref.py `step`).  Every stage takes
the stage before it as an argument (`means=`, `scal=`), so a test can feed it the kernel's own output and no sum order leaks into a
comparison of bits.  A fraction that rounds to fp32 1.0 is the next rank exactly (k + 1, f = 0), as `ops.mimic_factors` has it.
"""
import math

import numpy as np
import torch

import codenoise_ref
import dpm_ref

r16 = dpm_ref.r16


def f32(v):
    """A Python double rounded once to fp32, as a Python float."""
    return float(np.float32(v))


def to_f16(x64):
    """float64 -> fp16 in ONE rounding (numpy converts directly; torch goes through fp32) -> numpy float16 array."""
    with np.errstate(all="ignore"):
        return np.asarray(x64, dtype=np.float64).astype(np.float16)


def factors(ms, q, M):
    """(fp32 ms, k, f) of the rank q (M - 1), formed in float64."""
    pos = float(q) * float(M - 1)
    k = min(int(math.floor(pos)), M - 1)
    f = f32(pos - k)
    if not f < 1.0:
        k, f = min(k + 1, M - 1), 0.0
    return f32(float(ms)), k, f


def _channels(x):
    """(1 or 2, C, T, h, w) -> (.., C, M)."""
    return x.reshape(x.shape[0], x.shape[1], -1)


def combines(eps2, gs, ms):
    """g, l fp16 (C, M)."""
    return _channels(dpm_ref.cfg_combine(eps2, gs))[0], _channels(dpm_ref.cfg_combine(eps2, f32(ms)))[0]


def sums64(eps2, gs, ms):
    """-> (S float64 (C, 2) = [sum g, sum l], the sums of the terms' magnitudes (C, 2): the error bound's scale)."""
    g, l = combines(eps2, gs, ms)
    S = torch.stack([g.double().sum(1), l.double().sum(1)], dim=1)
    A = torch.stack([g.double().abs().sum(1), l.double().abs().sum(1)], dim=1)
    return S.numpy(), A.numpy()


def means_of(S, M):
    """float64 sums (C, 2) -> (mg, ml) numpy float16 (C, 2): one division, ONE rounding."""
    with np.errstate(all="ignore"):
        return to_f16(np.asarray(S, dtype=np.float64) / np.float64(M))


def _bits(h):
    """fp16 tensor -> int32 tensor of bits & 0x7fff."""
    return h.contiguous().view(torch.int16).to(torch.int32) & 0x7fff


def deviations(eps2, gs, ms, means):
    """d, e fp16 (C, M) from `means` = numpy float16 (C, 2)."""
    g, l = combines(eps2, gs, ms)
    m = torch.from_numpy(np.asarray(means, dtype=np.float16).astype(np.float32))
    with np.errstate(all="ignore"):
        d = (g.float() - m[:, :1]).half()
        e = (l.float() - m[:, 1:]).half()
    return d, e


def histogram(eps2, gs, ms, means):
    """-> (hist int64 (C, 32768) of bits(d) & 0x7fff, maxbits int64 (C,) of bits(e) & 0x7fff)."""
    d, e = deviations(eps2, gs, ms, means)
    db, eb = _bits(d).long(), _bits(e).long()
    hist = torch.stack([torch.bincount(row, minlength=32768) for row in db])
    return hist, eb.max(dim=1).values


def _half_of_bits(b):
    return np.array([b], dtype=np.uint16).view(np.float16)[0]


def select(eps2, gs, ms, q, means):
    """-> scal numpy uint16 (C, 4): the bits of (mg, ref_lo, ref_hi, s) per channel."""
    d, e = deviations(eps2, gs, ms, means)
    M = d.shape[1]
    _, k, f = factors(ms, q, M)
    a = torch.sort(_bits(d), dim=1).values
    out = np.zeros((d.shape[0], 4), dtype=np.uint16)
    for ch in range(d.shape[0]):
        lo_b, hi_b = int(a[ch, k]), int(a[ch, min(k + 1, M - 1)])
        ref_lo_b = int(_bits(e[ch]).max())
        if f == 0.0:
            ref_hi_b = lo_b
        else:
            with np.errstate(all="ignore"):
                lo, hi = np.float32(_half_of_bits(lo_b)), np.float32(_half_of_bits(hi_b))
                t = np.float32(np.float32(f) * np.float32(hi - lo))
                ref_hi_b = int(np.float32(lo + t).astype(np.float16).view(np.uint16))
        out[ch] = (int(np.asarray(means, dtype=np.float16)[ch, 0].view(np.uint16)), ref_lo_b, ref_hi_b,
                   ref_hi_b if ref_hi_b > ref_lo_b else ref_lo_b)
    return out


def threshold_with_scal(eps2, gs, scal):
    """g' fp16 (1, C, T, h, w) from eps2 and `scal` = uint16 (C, 4) bits of (mg, ref_lo, ref_hi, s)."""
    sc = torch.from_numpy(np.asarray(scal, dtype=np.uint16).view(np.float16).astype(np.float32))
    g = _channels(dpm_ref.cfg_combine(eps2, gs))[0].float()
    mg, ref_lo, s = sc[:, 0:1], sc[:, 1:2], sc[:, 3:4]
    d = r16(g - mg)
    dc = torch.where(d > s, s.expand_as(d), torch.where(d < -s, (-s).expand_as(d), d))
    out = r16(r16(r16(dc / s) * ref_lo) + mg).half()
    return out.reshape((1,) + tuple(eps2.shape[1:]))


def stats(eps2, gs, ms, q):
    """The restatement's own statistics, end to end -> scal uint16 (C, 4)."""
    M = eps2[0, 0].numel()
    return select(eps2, gs, ms, q, means_of(sums64(eps2, gs, ms)[0], M))


def ddim_step(eps2, x, gs, ms, q, coeffs, scal=None):
    """The thresholded fused CFG + DDIM step -> x' fp16.  `scal`: the scalars to use instead of the restatement's own."""
    g2 = threshold_with_scal(eps2, gs, stats(eps2, gs, ms, q) if scal is None else scal)
    return codenoise_ref.ddim_chain(g2, x, coeffs)


def dpm_step(eps2, x, x0_prev, gs, ms, q, k, scal=None):
    """The thresholded fused CFG + DPM-Solver++ step from tests/dpm_ref.py's scalars `k` -> (x' fp16, x0 fp16)."""
    g2 = threshold_with_scal(eps2, gs, stats(eps2, gs, ms, q) if scal is None else scal)
    return dpm_ref.step(g2, x, x0_prev, k)


def mean_margin(eps2, gs, ms):
    """For every channel and both means: (the distance of the float64 mean from the nearest fp16 rounding boundary, the bound of a
    fixed-order float64 sum of M terms divided by M) -> two float64 arrays (C, 2).  A seed is usable end to end when the first
    exceeds the second everywhere: then any summation order rounds to the same fp16 mean."""
    M = eps2[0, 0].numel()
    S, A = sums64(eps2, gs, ms)
    mean = S / M
    h = to_f16(mean)
    with np.errstate(all="ignore"):
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h64 = h.astype(np.float64)
    dist = np.minimum(np.abs(mean - (h64 + up) / 2), np.abs(mean - (h64 + dn) / 2))
    return dist, M * 2.0 ** -53 * A / M
