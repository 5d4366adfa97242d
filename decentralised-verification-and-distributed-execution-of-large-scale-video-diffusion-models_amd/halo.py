"""The halo exchange of `DistributedVideoDiffuser.__call__(exchange="halo")` (vdx/pipeline.py): who owns which frames and who
sends what (`HaloPlan`: host logic, integers only), the point-to-point transfers (`exchange_halos`) and the blend of the frames
a rank owns (`blend_owned`), in the reference's accumulation order (`fsdp_chunked_coherent.py:204-217`)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch
import torch.distributed as dist

from . import ops
from .planner import ChunkPlan


def ramp_weights(length: int, ov: int) -> torch.Tensor:
    """Per-frame blend weights of one chunk (:206-213), built with the same torch calls."""
    w = torch.ones(length)
    if ov > 0:
        ramp = torch.linspace(0, 1, ov)
        k = min(ov, length)
        w[:k] = ramp[:k]
        w[-k:] = torch.flip(ramp[:k], [0])
    return w


@dataclass(frozen=True)
class HaloTransfer:
    chunk: int          # window index (position in ChunkPlan.ranges) the frames come from
    src: int            # rank that denoised it
    dst: int            # rank that owns the frames
    s: int              # video frames [s, e)
    e: int


@dataclass(frozen=True)
class HaloSegment:
    s: int              # video frames [s, e): all covered by the same set of windows
    e: int
    chunks: Tuple[int, ...]     # covering window indices in the REFERENCE's accumulation order


class HaloPlan:
    """Frame ownership and transfers for a ChunkPlan.

    Windows come out of the planner with increasing start frames; the tail may repeat the last window
    (padding, :174-177) and `--mode fsdp` repeats the only window once per rank.  Distinct windows u = 0.. own the
    frames [start_u, start_{u+1}) (the last one up to T); the owner rank is the rank of the FIRST window with that
    range.  Every window (repeats included) that covers frames it does not own on its own rank sends them to the
    owner.  The reference accumulates `full[s:e] += lat * w` window by window in rank-major order (:208-216); frames
    are independent in that update, so replaying, per owned frame segment, the covering windows in that same order
    reproduces the reference's bits."""

    def __init__(self, cp: ChunkPlan, total: int):
        self.cp, self.total = cp, total
        W = cp.world
        n = len(cp.ranges)
        self.rank_of = [i % W for i in range(n)]
        self.slot_of = [i // W for i in range(n)]                       # position in the rank's own list
        # reference accumulation order: rank-major, then the rank's own order (:208-209)
        self.ref_order = sorted(range(n), key=lambda i: (self.rank_of[i], self.slot_of[i]))
        pos = {c: k for k, c in enumerate(self.ref_order)}
        uniq: List[int] = []
        for i, r in enumerate(cp.ranges):
            if not uniq or r != cp.ranges[uniq[-1]]:
                if uniq and r[0] <= cp.ranges[uniq[-1]][0]:
                    raise ValueError(f"window starts must increase: {cp.ranges}")
                uniq.append(i)
        self.owner_chunks = uniq
        self.owned: dict = {}                                            # rank -> [(s, e)] frames it owns
        self.segments: dict = {}                                         # rank -> [HaloSegment]
        self.transfers: List[HaloTransfer] = []
        for k, i in enumerate(uniq):
            s0 = cp.ranges[i][0]
            e0 = cp.ranges[uniq[k + 1]][0] if k + 1 < len(uniq) else total
            if k == 0:
                s0 = 0
            if e0 <= s0:
                continue
            owner = self.rank_of[i]
            self.owned.setdefault(owner, []).append((s0, e0))
            cover = [j for j, (s, e) in enumerate(cp.ranges) if s < e0 and e > s0]
            cuts = sorted({s0, e0} | {x for j in cover for x in cp.ranges[j] if s0 < x < e0})
            for a, b in zip(cuts[:-1], cuts[1:]):
                cs_ = tuple(sorted((j for j in cover if cp.ranges[j][0] <= a and cp.ranges[j][1] >= b), key=pos.get))
                self.segments.setdefault(owner, []).append(HaloSegment(a, b, cs_))
            for j in cover:
                if self.rank_of[j] != owner:
                    self.transfers.append(HaloTransfer(j, self.rank_of[j], owner, max(cp.ranges[j][0], s0),
                                                       min(cp.ranges[j][1], e0)))
        self.transfers.sort(key=lambda t: (t.chunk, t.s))
        for r in range(W):
            self.owned.setdefault(r, [])
            self.segments.setdefault(r, [])

    def bytes_sent(self, rank: int, frame_bytes: int) -> int:
        return sum((t.e - t.s) * frame_bytes for t in self.transfers if t.src == rank)


def exchange_halos(mine: List[torch.Tensor], hp: HaloPlan, rank: int, side_stream=None, comm=None):
    """Send the frames other ranks own, receive the frames this rank owns from the windows other ranks denoised.
    Returns ({(chunk, s, e): tensor (1,C,e-s,H,W)}, event or None): the received pieces are valid on the current
    stream after `event.wait()` (GPU) or immediately (CPU).  `comm` (a `vdx.comm.Comm`): the transfers go through the
    C-ABI entry point `vdx_halo_exchange` (RCCL send/recv), one grouped send + receive per neighbour.  (Executed with
    more than one rank on no machine this build had: a one-GPU box cannot host two RCCL ranks.)"""
    cp = hp.cp
    ref = mine[0]
    _, C, _, H, W = ref.shape
    got, p2p, keep, per_peer = {}, [], [], {}                 # per_peer: neighbour -> (pieces to send, receive buffers)
    for t in hp.transfers:
        if t.src == rank:
            s0 = cp.ranges[t.chunk][0]
            piece = mine[hp.slot_of[t.chunk]][:, :, t.s - s0:t.e - s0].contiguous()
            keep.append(piece)
            p2p.append(dist.P2POp(dist.isend, piece, t.dst))
            per_peer.setdefault(t.dst, ([], []))[0].append(piece)
        elif t.dst == rank:
            buf = ref.new_empty((1, C, t.e - t.s, H, W))
            got[(t.chunk, t.s, t.e)] = buf
            p2p.append(dist.P2POp(dist.irecv, buf, t.src))
            per_peer.setdefault(t.src, ([], []))[1].append(buf)
    if not p2p:
        return got, None
    if not ref.is_cuda:
        for r in dist.batch_isend_irecv(p2p):
            r.wait()
        return got, None
    if comm is None and dist.get_backend() == "gloo":
        # rehearsal of a multi-rank job whose ranks share one GPU: gloo has no device transport for send / recv, so
        # the pieces are staged through host memory (the product's transport is RCCL, below)
        host = {id(op.tensor): op.tensor.cpu() for op in p2p}
        for r in dist.batch_isend_irecv([dist.P2POp(op.op, host[id(op.tensor)], op.peer) for op in p2p]):
            r.wait()
        for buf in got.values():
            buf.copy_(host[id(buf)])
        return got, None
    # the side-stream hand-off, the same for both transports: the side stream is the current one while the transfers are
    # issued (torch.distributed issues on the current stream; `comm.halo` is handed its stream and does not look)
    side = side_stream or torch.cuda.Stream(device=ref.device, priority=-1)   # own hardware queue: vdx/shard.py on `_side`
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(ref.device))     # pieces / buffers exist once the current stream gets here
    with torch.cuda.stream(side):
        side.wait_event(ready)
        if comm is None:
            for r in dist.batch_isend_irecv(p2p):
                r.wait()
        else:
            # one grouped send + receive per neighbour and call (include/vdx.h), neighbours in ascending order: with every
            # rank walking its pairs in that order the pairs are met in one global (lexicographic) order — no cycle of waits
            for peer in sorted(per_peer):
                snds, rcvs = per_peer[peer]
                for k in range(max(len(snds), len(rcvs))):
                    comm.halo(snds[k] if k < len(snds) else None, peer if k < len(snds) else -1,
                              rcvs[k] if k < len(rcvs) else None, peer if k < len(rcvs) else -1, side)
        done = torch.cuda.Event()
        done.record(side)
    for t_ in keep + list(got.values()):
        t_.record_stream(side)
    return got, done


def blend_owned(mine: List[torch.Tensor], hp: HaloPlan, got: dict, done, like: torch.Tensor, rank: int):
    """Blend the frames this rank owns (reference :204-217 restricted to them).  Segments whose covering windows
    are all local are accumulated while the halo transfers are still in flight; the others after `done`.
    Returns [(s, e, fp32 latent (1,C,e-s,H,W))] for the owned ranges, in frame order."""
    cp, ov = hp.cp, hp.cp.overlap
    out = []
    for (o_s, o_e) in hp.owned[rank]:
        n = o_e - o_s
        full = like.new_zeros((1, like.shape[1], n, like.shape[3], like.shape[4]))
        weight = torch.zeros(n, dtype=torch.float32, device=like.device)
        segs = [g for g in hp.segments[rank] if o_s <= g.s and g.e <= o_e]
        local = lambda g: all(hp.rank_of[c] == rank for c in g.chunks)    # noqa: E731
        waited = done is None
        for g in sorted(segs, key=lambda g: (not local(g), g.s)):
            if not local(g) and not waited:
                torch.cuda.current_stream(like.device).wait_event(done)
                waited = True
            for c in g.chunks:
                cs_, ce_ = cp.ranges[c]
                if hp.rank_of[c] == rank:
                    piece = mine[hp.slot_of[c]][:, :, g.s - cs_:g.e - cs_]
                else:
                    key = next(k for k in got if k[0] == c and k[1] <= g.s and g.e <= k[2])
                    piece = got[key][:, :, g.s - key[1]:g.e - key[1]]
                w = ramp_weights(ce_ - cs_, ov)[g.s - cs_:g.e - cs_]
                ops.blend_accumulate(full, weight, piece.contiguous(), w.contiguous().to(like.device),
                                     g.s - o_s, g.e - o_s)
        out.append((o_s, o_e, ops.blend_finalize(full, weight)))
    return out
