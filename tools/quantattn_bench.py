#!/usr/bin/env python3
"""Time and measure the INT8 attention (csrc/flash_i8.hip), medians of 20 taken in alternating rounds in one process after a
warm-up of every shape:

  * at levels 0-2 of a 24 x 72 x 128 clip under CFG (48 images; 9216 / 2304 / 576 tokens with 5 / 10 / 20 heads) the pre-pass
    `ops.attn_quant_i8`, the main kernel alone (on a workspace already filled) and `ops.flash_attn_i8` (their sum, as the UNet
    calls it), beside `ops.flash_attn(..., v_rows=True)` on the same rows;
  * the whole CFG step (cfg_input, UNet, CFG + DDIM) at the headline latent (1, 4, 24, 72, 128) on seeded synthetic Zeroscope
    weights with the option off, on (level 0), off again, the difference beside the spread of the two off readings;
  * with --parity FILE: for the shapes of tests/test_quantattn_gpu.py the error of `flash_attn_i8` and of `flash_attn` against
    float64 attention on the UNQUANTISED inputs, and the share of int8 values that differ from the torch-CPU restatement.

Measured numbers only.

    python tools/quantattn_bench.py [--out profiles/quantattn_bench.json] [--parity profiles/quantattn_parity.txt] [--iters 20] [--no_step]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from vdx import ops  # noqa: E402
from kvdown_bench import alternating, once  # noqa: E402,F401

#         (level, n_img, S, heads)
KERNELS = [(0, 48, 72 * 128, 5), (1, 48, 36 * 64, 10), (2, 48, 18 * 32, 20)]


def kernel_rows(dev, iters):
    rows = []
    for level, n_img, S, heads in KERNELS:
        C, M = heads * 64, n_img * S
        qkv = torch.randn(M, 3 * C, generator=torch.Generator().manual_seed(0)).half().to(dev)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        out = torch.empty(M, C, dtype=torch.float16, device=dev)
        ws = ops.attn_quant_i8_workspace(n_img, S, heads, dev)
        ops.attn_quant_i8(q, k, n_img=n_img, S=S, heads=heads, scale=0.125, workspace=ws)

        def prepass():
            ops.attn_quant_i8(q, k, n_img=n_img, S=S, heads=heads, scale=0.125, workspace=ws)

        def main_kernel():
            ops._launch("vdx_flash_attn_i8_f16", ws.data_ptr(), ws.numel(), v.data_ptr(), v.stride(0), out.data_ptr(), out.stride(0), n_img, S, heads)

        def both():
            ops.flash_attn_i8(q, k, v, n_img=n_img, S=S, heads=heads, scale=0.125, out=out, workspace=ws)

        def fp16():
            ops.flash_attn(q, k, v, n_seq=n_img, sq=S, skv=S, skv_pad=S, heads=heads, seq_per_kv=1, scale=0.125, v_rows=True, out=out)

        row = {"level": level, "n_img": n_img, "S": S, "heads": heads, "workspace_bytes": ws.numel()}
        row.update(alternating({"attn_quant_i8": prepass, "flash_attn_i8_main": main_kernel, "flash_attn_i8": both, "flash_attn_fp16": fp16}, iters))
        flops = 4.0 * n_img * heads * S * S * 64
        for name in ("flash_attn_i8_main", "flash_attn_fp16"):
            row[name]["tflops"] = round(flops / row[name]["median_ms"] / 1e9, 1)
        row["i8_sum_over_fp16"] = round(row["flash_attn_i8"]["median_ms"] / row["flash_attn_fp16"]["median_ms"], 4)
        row["i8_main_over_fp16"] = round(row["flash_attn_i8_main"]["median_ms"] / row["flash_attn_fp16"]["median_ms"], 4)
        rows.append(row)
        del qkv, out, ws
    return rows


def step_times(dev, iters):
    import statistics
    from vdx.scheduler import DDIMScheduler
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig.zeroscope()
    unet = UNet3DConditionModel(cfg).load_diffusers_state_dict(synthetic_state_dict(cfg, 1234, dev), device=dev)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, 4, 24, 72, 128, generator=g).half().to(dev)
    emb = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).half().to(dev)
    sched = DDIMScheduler()
    sched.set_timesteps(50, device=dev)
    t = sched._host_timesteps[10]

    def step():
        noise = unet(ops.cfg_input(lat, None, 0.0), t, encoder_hidden_states=emb).sample
        return sched.step_cfg(noise, t, lat, 7.5)

    def reading():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        ms = [once(step) for _ in range(iters)]
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "iters": iters,
                "steps_per_s": round(1000.0 / statistics.median(ms), 4)}
    out = {"latent": [1, 4, 24, 72, 128], "weights": "synthetic Zeroscope, seed 1234", "timestep": int(t), "max_downsample": 1}
    out["quant_attn_off"] = reading()
    unet.enable_quant_attn(1)
    out["quant_attn_on"] = reading()
    unet.disable_quant_attn()
    out["quant_attn_off_again"] = reading()
    a, b, on = out["quant_attn_off"]["median_ms"], out["quant_attn_off_again"]["median_ms"], out["quant_attn_on"]["median_ms"]
    out["gap_between_off_readings_ms"] = round(abs(a - b), 4)
    out["on_minus_faster_off_ms"] = round(on - min(a, b), 4)
    out["faster_than_both_by_more_than_their_gap"] = bool(min(a, b) - on > abs(a - b))
    return out


def parity_lines(dev):
    import quantattn_ref as R
    from test_quantattn_gpu import SCALE, SHAPES, case
    lines = ["flash_attn_i8 and flash_attn (fp16) against float64 attention on the UNQUANTISED inputs (seeded N(0, 1) q, k, v, scale 1/8);",
             "share: int8 values of the pre-pass that differ from the torch-CPU restatement (tests/quantattn_ref.py), q8 / k8",
             "(n_img, S, heads)   i8 max-abs  i8 rel-L2   fp16 max-abs  fp16 rel-L2   share q8   share k8"]
    for shape in SHAPES:
        n_img, S, heads = shape
        C, qkv = heads * 64, case(shape)
        x = qkv.to(dev)
        q, k, v = x[:, :C], x[:, C:2 * C], x[:, 2 * C:]
        ws = ops.attn_quant_i8_workspace(n_img, S, heads, dev)
        i8 = ops.flash_attn_i8(q, k, v, n_img=n_img, S=S, heads=heads, scale=SCALE, workspace=ws).cpu().double()
        got = [t.cpu() for t in ops._quant_i8_views(ws, n_img, S, heads)]
        f16 = ops.flash_attn(q, k, v, n_seq=n_img, sq=S, skv=S, skv_pad=S, heads=heads, seq_per_kv=1, scale=SCALE, v_rows=True).cpu().double()
        ref = R.attention64_plain(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], n_img, S, heads, SCALE)
        want = R.quantiser(qkv[:, :C], qkv[:, C:2 * C], n_img, S, heads, SCALE)
        share = [float((got[i] != want[i]).float().mean()) for i in (0, 1)]
        err = [((o - ref).abs().max().item(), ((o - ref).norm() / ref.norm()).item()) for o in (i8, f16)]
        lines.append(f"{str(shape):<19} {err[0][0]:.3e}   {err[0][1]:.3e}   {err[1][0]:.3e}     {err[1][1]:.3e}     {share[0]:.2e}   {share[1]:.2e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no_step", action="store_true")
    ap.add_argument("--no_kernels", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.parity:
        text = "\n".join(parity_lines(dev))
        print(text)
        with open(a.parity, "w") as f:
            f.write(text + "\n")
    rec = {"job": "int8 score product: pre-pass, main kernel and their sum beside fp16 flash attention", "device": torch.cuda.get_device_name(0),
           "source_sha": vdx._lib.source_sha()}
    if not a.no_kernels:
        rec["kernels"] = kernel_rows(dev, a.iters)
    if not a.no_step:
        rec["cfg_step"] = step_times(dev, a.iters)
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
