"""Worker of tests/test_dist_coloop_gpu.py (not a test): one rank of a real multi-process LOOPING co-denoised job (ring windows,
vdx/codenoise.py `loop_plan`).  All ranks compute on cuda:0 and talk over gloo (the share-GPU rehearsal of
tests/dist_pipeline_worker.py).  Every rank runs its ring windows, the packed noise buffers are gathered once per step, and every
rank steps its own copy of the whole clip's latent; the ranks then check over gloo that their latents carry the same bits; rank 0
saves its latent and `info`.

    torchrun --nproc-per-node W tests/dist_coloop_worker.py OUT.pt T CHUNK OVERLAP STEPS SCHEDULER"""
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
    sampler = sys.argv[6]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    m, emb = build(dev, rank, world)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=256, width=256, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", scheduler=sampler, co_denoise=True, loop=True)
    d = DistributedVideoDiffuser(cfg, m, make_scheduler(sampler, DDIMScheduler()), emb[1:], emb[:1])
    lat, info = d(exchange="allgather")
    mine = lat.cpu()
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    for r, t in enumerate(every):
        assert torch.equal(t.view(torch.int32), mine.view(torch.int32)), (rank, r)
    if rank == 0:
        keep = ("ranges", "chunk_size", "overlap", "world_size", "network_bytes", "payload_bytes", "payload_bytes_actual",
                "steps_run", "co_denoise", "loop")
        torch.save({"lat": mine, "info": {k: info[k] for k in keep}, "gathers": getattr(m.W, "gathers", None)}, out)
    dist.barrier()
    dist.destroy_process_group()
    print("rank", rank, "ok", flush=True)


if __name__ == "__main__":
    main()
