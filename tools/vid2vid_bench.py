"""Time the video-to-video front end on one GPU: Image.resize (BICUBIC) of a first-stage clip from 576x320 to 1024x576 plus
the VAE encode of its frames (Stable-Diffusion VAE widths, synthetic weights) -> one JSON line, and
profiles/vid2vid_encode.json with --out.  FLOPs = 2 * MACs of the encoder's convolutions and attention GEMMs (formula below;
GroupNorm / SiLU / softmax / resize not counted).
    python tools/vid2vid_bench.py --frames 24 --repeats 3 --out profiles/vid2vid_encode.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def encoder_flops(H, W, ch=(128, 256, 512, 512), layers=2):
    """2 * MACs per frame: conv_in (27 -> ch0), per level `layers` ResNets (two 3x3 convs + a 1x1 shortcut on width changes),
    the (0,1,0,1) stride-2 downsample conv, the mid block (2 ResNets + single-head attention: q, k, v, out projections,
    q.k^T and P.V over h*w tokens), conv_out (ch[-1] -> 8, quant_conv folded in)."""
    macs = H * W * 27 * ch[0]
    h, w, prev = H, W, ch[0]
    for i, c in enumerate(ch):
        for j in range(layers):
            ci = prev if j == 0 else c
            macs += h * w * 9 * (ci * c + c * c) + (h * w * ci * c if ci != c else 0)
        prev = c
        if i != len(ch) - 1:
            h, w = h // 2, w // 2
            macs += h * w * 9 * c * c
    C, S = ch[-1], h * w
    macs += 2 * S * 9 * 2 * C * C                    # two mid ResNets
    macs += 4 * S * C * C + 2 * S * S * C            # projections, scores, P.V
    macs += S * 9 * C * 8
    return 2 * macs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import vdx  # noqa: F401
    from vdx import _lib, ops
    from vdx.vae import AutoencoderKL, VaeConfig
    from vdx.weights import synthetic_vae_encoder_state_dict
    dev = torch.device("cuda:0")
    vae = AutoencoderKL(VaeConfig.sd()).load_diffusers_encoder_state_dict(synthetic_vae_encoder_state_dict(VaeConfig.sd(), 8),
                                                                          device=dev)
    T, H, W = a.frames, 576, 1024
    clip = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (T, 320, 576, 3), dtype=np.uint8)).to(dev)
    noise = torch.randn((T, 4, H // 8, W // 8), generator=torch.Generator(device=dev).manual_seed(1), device=dev,
                        dtype=torch.float16)

    def run():
        fr = ops.resize_u8(clip, H, W)
        return fr, vae.encode_frames_u8(fr, noise=noise)
    run()                                             # warm-up: plan cache, allocator
    torch.cuda.synchronize()
    times, rs = [], []
    for _ in range(a.repeats):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        fr = ops.resize_u8(clip, H, W)
        e1.record()
        lat = vae.encode_frames_u8(fr, noise=noise)
        e2.record()
        torch.cuda.synchronize()
        rs.append(e0.elapsed_time(e1))
        times.append(e0.elapsed_time(e2))
    flops = T * encoder_flops(H, W)
    best = min(times)
    rec = {"what": f"resize 576x320 -> 1024x576 (bicubic) + VAE encode of {T} frames, SD widths, synthetic weights",
           "frames": T, "ms": round(best, 2), "ms_all": [round(t, 2) for t in times], "resize_ms": round(min(rs), 3),
           "flops": flops, "tflops_per_s": round(flops / (best * 1e-3) / 1e12, 1), "batch": 8,
           "latent_shape": list(lat.shape), "finite": bool(torch.isfinite(lat).all()), "source_sha": _lib.source_sha(),
           "device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d %H:%M:%S")}
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
