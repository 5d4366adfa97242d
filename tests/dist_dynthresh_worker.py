"""Worker of tests/test_dist_dynthresh_gpu.py (not a test): one rank of a real multi-process co-denoised job with dynamic
thresholding.  All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of tests/dist_pipeline_worker.py).  Every
rank steps its own copy of the whole clip's latent from the same gathered noise buffer, so every rank forms the same channel
statistics with no collective of its own; the ranks then check over gloo that their latents carry the same bits; rank 0 saves its
latent.

    torchrun --nproc-per-node W tests/dist_dynthresh_worker.py OUT.pt T CHUNK OVERLAP STEPS SCHEDULER GS MIMIC PERCENTILE"""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import vdx  # noqa: E402,F401
from dist_pipeline_worker import build  # noqa: E402
from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, make_scheduler  # noqa: E402
from vdx.scheduler import DDIMScheduler  # noqa: E402


def main():
    out = sys.argv[1]
    T, chunk, ov, steps = (int(a) for a in sys.argv[2:6])
    sampler, gs, ms, q = sys.argv[6], float(sys.argv[7]), float(sys.argv[8]), float(sys.argv[9])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler=sampler, co_denoise=True, guidance_scale=gs, cfg_mimic=ms,
                         cfg_mimic_percentile=q)
    d = DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1])
    lat, info = d(exchange="allgather")
    mine = lat.cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    if rank == 0:
        torch.save({"lat": mine, "ranges": [tuple(r) for r in info["ranges"]], "world_size": info["world_size"],
                    "cfg_mimic": info["cfg_mimic"]}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
