"""Cross-frame attention, the float64 definition: per (sample, frame) gather the R reference frames' K and V rows, then
softmax(q k^T / 8) v."""
import torch


def attention(qkv, n_samples, F, S, heads, refs):
    """qkv: fp16 [n_samples F S][3 heads 64] (q | k | v); refs: [F][R] frame indices -> float64 [n_samples F S][heads 64]."""
    C = heads * 64
    x = qkv.double().view(n_samples, F, S, 3, heads, 64)
    out = torch.zeros(n_samples, F, S, heads, 64, dtype=torch.float64)
    for b in range(n_samples):
        for f in range(F):
            q = x[b, f, :, 0].transpose(0, 1)                                               # [heads][S][64]
            k = torch.cat([x[b, int(r), :, 1] for r in refs[f]]).transpose(0, 1)            # [heads][R S][64]
            v = torch.cat([x[b, int(r), :, 2] for r in refs[f]]).transpose(0, 1)
            out[b, f] = (torch.softmax(q @ k.transpose(1, 2) / 8, -1) @ v).transpose(0, 1)
    return out.reshape(n_samples * F * S, C)
