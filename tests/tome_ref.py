"""Token merging around a spatial self-attention, restated on the CPU with torch: `tomesd`'s
bipartite_soft_matching_random2d with two orders fixed (ties and layout), steps 1-6 of the definition the kernels in
csrc/tome.hip are pinned to.  The match is in float64; select, merge and unmerge are exact restatements (integers and fp32 steps)."""
import torch


def tomesd_partition(h, w, sx, sy, rand_idx=None):
    """`tomesd`'s own construction, literally: the idx_buffer scatter, the argsort, the split at num_dst.
    -> (a_idx, b_idx) = (sources, destinations) as int64 token indices in the argsort's order."""
    hsy, wsx = h // sy, w // sx
    if rand_idx is None:
        rand_idx = torch.zeros(hsy, wsx, 1, dtype=torch.int64)
    idx_buffer_view = torch.zeros(hsy, wsx, sy * sx, dtype=torch.int64)
    idx_buffer_view.scatter_(dim=2, index=rand_idx, src=-torch.ones_like(rand_idx, dtype=rand_idx.dtype))
    idx_buffer_view = idx_buffer_view.view(hsy, wsx, sy, sx).transpose(1, 2).reshape(hsy * sy, wsx * sx)
    if (hsy * sy) < h or (wsx * sx) < w:
        idx_buffer = torch.zeros(h, w, dtype=torch.int64)
        idx_buffer[:(hsy * sy), :(wsx * sx)] = idx_buffer_view
    else:
        idx_buffer = idx_buffer_view
    rand_idx = idx_buffer.reshape(1, -1, 1).argsort(dim=1)
    num_dst = hsy * wsx
    return rand_idx[0, num_dst:, 0], rand_idx[0, :num_dst, 0]


def scores(t, src_idx, dst_idx, n_img, S):
    """t fp16 [n_img * S][C] -> float64 [n_img][n_src][n_dst] cosine similarities (a zero row: 0 * inf = NaN, as it comes)."""
    x = t.double().view(n_img, S, -1)
    with torch.no_grad():
        inv = 1.0 / x.pow(2).sum(-1).sqrt()
        a, b = x[:, src_idx.long()], x[:, dst_idx.long()]
        return (a @ b.transpose(1, 2)) * inv[:, src_idx.long(), None] * inv[:, None, dst_idx.long()]


def match(t, src_idx, dst_idx, n_img, S):
    """-> (score float64 [n_img][n_src][n_dst], node_max float64 [n_img][n_src], node_idx int64): the maximum over j with a NaN
    never winning (-inf where nothing wins) and the lowest j that reaches it (0 where nothing wins)."""
    sc = scores(t, src_idx, dst_idx, n_img, S)
    clean = torch.where(torch.isnan(sc), torch.full_like(sc, float("-inf")), sc)
    node_max = clean.max(-1).values
    j = torch.arange(sc.shape[-1]).expand_as(sc)
    hit = (clean == node_max[..., None]) & (clean > float("-inf"))
    node_idx = torch.where(hit, j, torch.full_like(j, sc.shape[-1])).min(-1).values
    node_idx = torch.where(node_idx == sc.shape[-1], torch.zeros_like(node_idx), node_idx)
    return sc, node_max, node_idx


def orderable(node_max):
    """fp32 -> int64 key whose order is the value's: NaN lowest, then -inf .. +inf; -0 and +0 share a key."""
    v = node_max.float()
    b = v.view(torch.int32).long() & 0xffffffff
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where(b >= 0x80000000, 0xffffffff - b, b | 0x80000000)
    return torch.where(torch.isnan(v), torch.zeros_like(key), key)


def select(node_max, node_idx, src_idx, dst_idx, S, r):
    """One image.  node_max fp32 [n_src], node_idx int [n_src] -> (slot int32 [S], off int32 [n_dst + 1], items int32 [r])."""
    n_src, n_dst = src_idx.numel(), dst_idx.numel()
    key = orderable(node_max)
    order = sorted(range(n_src), key=lambda i: (-int(key[i]), i))
    merged = torch.zeros(n_src, dtype=torch.bool)
    merged[order[:r]] = True
    n_unm = n_src - r
    slot = torch.zeros(S, dtype=torch.int32)
    lists = [[] for _ in range(n_dst)]
    pos = 0
    for i in range(n_src):
        if merged[i]:
            j = min(max(int(node_idx[i]), 0), n_dst - 1)
            slot[int(src_idx[i])] = n_unm + j
            lists[j].append(i)
        else:
            slot[int(src_idx[i])] = pos
            pos += 1
    for j in range(n_dst):
        slot[int(dst_idx[j])] = n_unm + j
    off = torch.zeros(n_dst + 1, dtype=torch.int32)
    off[1:] = torch.tensor([len(x) for x in lists], dtype=torch.int32).cumsum(0)
    items = torch.tensor([i for x in lists for i in x], dtype=torch.int32)
    return slot, off, items


def merge(y, src_idx, dst_idx, slot, off, items, S, r):
    """One image.  y fp16 [S][C] -> fp16 [S - r][C]: unmerged rows copied; destination j is
    fp16((fp32(y[dst j]) + sum fp32(y[src i])) / fp32(1 + count)), the sum in ascending i, each add rounded to fp32."""
    n_src, n_dst = src_idx.numel(), dst_idx.numel()
    n_unm = n_src - r
    out = torch.zeros((S - r, y.shape[1]), dtype=torch.float16)
    for i in range(n_src):
        q = int(slot[int(src_idx[i])])
        if q < n_unm:
            out[q] = y[int(src_idx[i])]
    for j in range(n_dst):
        acc = y[int(dst_idx[j])].float()
        b, e = int(off[j]), int(off[j + 1])
        for m in range(b, e):
            acc = acc + y[int(src_idx[int(items[m])])].float()
        out[n_unm + j] = (acc / torch.tensor(float(1 + e - b), dtype=torch.float32)).half()
    return out


def unmerge_add(a, slot, t):
    """One image.  fp16(fp32(a[slot[p]]) + fp32(t[p]))."""
    return (a[slot.long()].float() + t.float()).half()


def select_merge_all(node_max, node_idx, y, src_idx, dst_idx, n_img, S, r):
    """Every image: -> (slot [n_img][S], off, items, merged rows [n_img * (S - r)][C])."""
    outs = [select(node_max[n], node_idx[n], src_idx, dst_idx, S, r) for n in range(n_img)]
    slot, off, items = (torch.stack([o[k] for o in outs]) for k in range(3))
    ys = y.view(n_img, S, -1)
    rows = torch.cat([merge(ys[n], src_idx, dst_idx, slot[n], off[n], items[n], S, r) for n in range(n_img)])
    return slot, off, items, rows
