#!/usr/bin/env python3
"""Time the CLIP quality score (vdx/clip_score.py; InferNet/template/validator/scoring.py:87-147) of one video: 24 uint8
frames at 576x1024 already on the GPU and one prompt -> Q, with HIP events around `CLIPScorer.score` (front end, both
towers, the cosine score; the host copy of the per-frame values included).  Next to it, the same job through stock
PyTorch-ROCm: `transformers.CLIPModel` in fp16 on the GPU with torch's antialiased bilinear resize and the ImageNet
normalization (the reference's arithmetic, torch's kernels).  Prints one JSON line; `--out FILE` also writes it.

    python tools/clip_score_bench.py [--frames 24] [--iters 20] [--hip-only] [--out profiles/clip_score_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vdx  # noqa: E402,F401
from vdx.clip_score import CLIPScorer  # noqa: E402


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
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hip-only", action="store_true", help="skip the stock-PyTorch leg (kernel traces of the HIP path)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (a.frames, 576, 1024, 3), generator=g, dtype=torch.uint8).to(dev)
    ids = torch.cat([torch.tensor([49406]), torch.randint(1000, 49000, (10,), generator=g), torch.tensor([49407])]).view(1, -1)
    scorer = CLIPScorer.synthetic(seed=0, device=dev)
    res = {"job": f"CLIP ViT-B/32 score, {a.frames} frames 576x1024 uint8 on the GPU, 12-token prompt", "device": torch.cuda.get_device_name(0)}
    res["hip"] = timed(lambda: scorer.score(frames, ids), a.iters)
    res["hip"]["score"] = scorer.score(frames, ids)[0]
    if not a.hip_only:
        import transformers
        torch.manual_seed(0)
        model = transformers.CLIPModel(transformers.CLIPConfig()).half().to(dev).eval()
        mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
        std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
        ids_d = ids.to(dev)

        @torch.no_grad()
        def stock():
            x = frames.permute(0, 3, 1, 2).float()
            x = torch.nn.functional.interpolate(x, size=(224, 224), mode="bilinear", antialias=True, align_corners=False)
            x = ((x.round().clamp(0, 255) / 255 - mean) / std).half()
            i = torch.nn.functional.normalize(model.get_image_features(pixel_values=x).pooler_output.float(), dim=-1)
            t = torch.nn.functional.normalize(model.get_text_features(input_ids=ids_d).pooler_output.float(), dim=-1)
            return float((i @ t.T).mean())
        res["stock_torch_fp16"] = timed(stock, a.iters)
        res["stock_torch_fp16"]["score"] = stock()
        res["speedup_vs_stock"] = res["stock_torch_fp16"]["median_ms"] / res["hip"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
