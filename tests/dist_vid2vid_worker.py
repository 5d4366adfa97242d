"""Worker of tests/test_vid2vid_gpu.py (not a test): one rank of a real multi-process video-to-video run.  All ranks
compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every rank loads and
encodes the whole clip itself (`vdx.pipeline.encode_init_video`: no collective), builds its own start latent and ctx,
and the ranks then check over gloo that they hold the same bits; rank 0 saves them and the blended result.

    torchrun --nproc-per-node W tests/dist_vid2vid_worker.py OUT.pt CLIP.npy T CHUNK OVERLAP STEPS STRENGTH"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, encode_init_video  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402
from vdx.vae import AutoencoderKL, VaeConfig  # noqa: E402

VAE_WIDTHS = (64, 64, 128, 128)


def config(clip, T, chunk, ov, steps, strength):
    return DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=128, width=128, mode="hybrid_ctx",
                          device="cuda", noise_device="cpu", init_video=clip, strength=strength)


def main():
    out, clip = sys.argv[1], sys.argv[2]
    T, chunk, ov, steps = (int(a) for a in sys.argv[3:7])
    strength = float(sys.argv[7])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = config(clip, T, chunk, ov, steps, strength)
    x0, _ = encode_init_video(cfg, AutoencoderKL(VaeConfig(block_out_channels=VAE_WIDTHS)), dev)
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1], init_latents=x0)
    mine = {"x0": x0.cpu(), "start": d._start.cpu(), "ctx": d.ctx.cpu()}
    for k, v in mine.items():
        every = [torch.empty_like(v) for _ in range(world)]
        dist.all_gather(every, v)
        for r, t in enumerate(every):
            assert torch.equal(t, v), (k, rank, r)
    full, info = d(exchange="allgather")
    if rank == 0:
        torch.save(dict(mine, lat=full.cpu(), ranges=[tuple(r) for r in info["ranges"]], overlap=info["overlap"],
                        steps_run=info["steps_run"], gathers=getattr(m.W, "gathers", None)), out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
