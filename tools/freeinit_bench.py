#!/usr/bin/env python3
"""Time FreeInit's re-initialisation at the headline latent (1, 4, 24, 72, 128), medians of 20 after a warm-up:

  * the mix alone (`vdx.freeinit.freq_mix`: five launches of csrc/freeinit.hip);
  * `vdx.freeinit.reinit` as a whole (cast, add_noise, the fresh noise on the GPU, the mix);
  * the same expression as a chain of torch GPU ops: `torch.fft` (fftn, fftshift, ifftn) when it runs on this box, dense
    complex DFT matrices per axis (three einsums forward, three back) otherwise; its result is compared with the kernels'.

Measured numbers only; no ratio is claimed in advance.

    python tools/freeinit_bench.py [--out profiles/freeinit_bench.json] [--iters 20]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vdx  # noqa: E402,F401
from vdx import freeinit, ops  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402

VOL = (1, 4, 24, 72, 128)
DIMS = (-3, -2, -1)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "iters": iters}


def fft_chain(z, eta, filt):
    zf = torch.fft.fftshift(torch.fft.fftn(z.float(), dim=DIMS), dim=DIMS)
    ef = torch.fft.fftshift(torch.fft.fftn(eta, dim=DIMS), dim=DIMS)
    return torch.fft.ifftn(torch.fft.ifftshift(zf * filt + ef * (1 - filt), dim=DIMS), dim=DIMS).real.half()


def dense_chain(mats):
    def run(z, eta, filt):
        (ft, it), (fh, ih), (fw, iw) = mats
        d = (z.float() - eta).to(torch.complex64)
        f = torch.einsum("kt,bcthw->bckhw", ft, torch.einsum("kh,bcthw->bctkw", fh, torch.einsum("kw,bcthw->bcthk", fw, d)))
        f = f * torch.fft.ifftshift(filt, dim=DIMS)
        r = torch.einsum("kt,bcthw->bckhw", it, torch.einsum("kh,bcthw->bctkw", ih, torch.einsum("kw,bcthw->bcthk", iw, f)))
        return (eta + r.real / (VOL[2] * VOL[3] * VOL[4])).half()
    return run


def dft_matrices(n, dev):
    j = torch.arange(n, dtype=torch.float64)
    ang = 2 * math.pi * torch.outer(j, j).remainder(n) / n
    f = torch.complex(torch.cos(ang), -torch.sin(ang)).to(torch.complex64).to(dev)
    return f, f.conj().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    z0 = torch.randn(VOL, generator=g).to(dev)
    base = torch.randn(VOL, generator=g).half().to(dev)
    eta = torch.randn(VOL, generator=g).to(dev)
    filt = freeinit.lowpass_filter(VOL[2:]).to(dev)
    sched = DDIMScheduler()
    z_T = sched.add_noise(z0.half(), base, 999)
    rec = {"job": f"FreeInit re-initialisation of a {VOL} latent (butterworth, order 4, d_s = d_t = 0.25)",
           "device": torch.cuda.get_device_name(0), "source_sha": vdx._lib.source_sha(),
           "direct_dft_flop": 8 * 2 * math.prod(VOL) * (VOL[2] + VOL[3] + VOL[4])}
    got = ops.freeinit_mix(z_T, eta, filt)
    rec["mix"] = timed(lambda: ops.freeinit_mix(z_T, eta, filt), a.iters)
    rec["reinit"] = timed(lambda: freeinit.reinit(z0, base, sched, 1, filt), a.iters)
    try:
        ref = fft_chain(z_T, eta, filt)
        torch.cuda.synchronize()
        chain, name = fft_chain, "torch.fft: fftn, fftshift, mix, ifftshift, ifftn, real, half"
    except Exception as e:                                                 # noqa: BLE001 (rocFFT missing or failing on this box)
        rec["torch_fft_error"] = f"{type(e).__name__}: {e}"[:300]
        chain = dense_chain([dft_matrices(n, dev) for n in VOL[2:]])
        name = "dense complex64 DFT matrices per axis (einsum), difference form"
        ref = chain(z_T, eta, filt)
    rec["torch_chain"] = dict(timed(lambda: chain(z_T, eta, filt), a.iters), ops=name)
    d = (got.float() - ref.float()).abs()
    rec["agreement"] = {"max_abs_difference": float(d.max()), "share_of_elements_that_differ": float((got != ref).float().mean())}
    rec["torch_over_mix"] = round(rec["torch_chain"]["median_ms"] / rec["mix"]["median_ms"], 2)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
