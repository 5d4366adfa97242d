"""Restatements for the INT8 attention's tests (include/vdx.h `vdx_attn_quant_i8`): the quantiser in torch-CPU fp32, operation
for operation and in the kernel's summation order, and the attention in float64 from given quantised operands."""
import numpy as np
import torch

BLOCK = 64


def key_mean(K):
    """fp32 [64] mean of the rows of K [S][64]: rows g, g + 32, ... added in ascending order into 32 partial sums, those added
    in ascending g, one division by S."""
    S, C = K.shape
    x = torch.cat([K.float(), torch.zeros((-S) % 32, C)]).view(-1, 32, C)      # adding +0.0 leaves a partial sum as it is
    acc = torch.zeros(32, C)
    for rows in x:
        acc = acc + rows
    tot = torch.zeros(C)
    for g in range(32):
        tot = tot + acc[g]
    return tot / torch.tensor(float(S), dtype=torch.float32)


def quantise_blocks(X):
    """X fp32 [S][64] -> (int8 [S_pad][64] with zero tail rows, delta fp32 [S_pad / 64])."""
    S, C = X.shape
    nb = (S + BLOCK - 1) // BLOCK
    xp = torch.zeros(nb * BLOCK, C)
    xp[:S] = X
    blocks = xp.view(nb, BLOCK * C)
    amax = blocks.abs().amax(1)
    delta = torch.where(amax == 0, torch.ones_like(amax), amax / 127.0)
    x8 = torch.clamp(torch.round(blocks / delta[:, None]), -127, 127).to(torch.int8)      # torch.round: half to even
    return x8.view(nb * BLOCK, C), delta


def quantiser(q, k, n_img, S, heads, scale):
    """q, k fp16 [n_img*S][heads*64] -> (q8, k8 int8 [n_img][heads][S_pad][64], dq, dk fp32 [n_img][heads][S_pad/64])."""
    c = float(np.float32(scale) * np.float32(1.44269504088896341))
    out = [[], [], [], []]
    for n in range(n_img):
        for h in range(heads):
            Q, K = (t[n * S:(n + 1) * S, h * 64:(h + 1) * 64].float() for t in (q, k))
            for i, (x8, d) in enumerate((quantise_blocks(Q * c), quantise_blocks(K - key_mean(K)))):
                out[i].append(x8)
                out[2 + i].append(d)
    nb = (S + BLOCK - 1) // BLOCK
    return (torch.stack(out[0]).view(n_img, heads, nb * BLOCK, 64), torch.stack(out[1]).view(n_img, heads, nb * BLOCK, 64),
            torch.stack(out[2]).view(n_img, heads, nb), torch.stack(out[3]).view(n_img, heads, nb))


def attention64(q8, k8, dq, dk, v, S):
    """float64 [n_img*S][heads*64]: per (image, head) the base-2 softmax of fp32(q8 k8^T) (dq dk) over the S keys, times V
    (v fp16 [n_img*S][heads*64]); the product of the two block scales is taken in fp32, as the kernel takes it."""
    n_img, heads = q8.shape[:2]
    dd = (dq[..., :, None] * dk[..., None, :]).double().repeat_interleave(BLOCK, 2).repeat_interleave(BLOCK, 3)[..., :S, :S]
    s = (q8[:, :, :S].double() @ k8[:, :, :S].double().transpose(2, 3)) * dd
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    V = v.double().view(n_img, S, heads, 64).transpose(1, 2)
    return ((p @ V) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(n_img * S, heads * 64)


def attention64_plain(q, k, v, n_img, S, heads, scale):
    """float64 softmax(q k^T scale) v on the unquantised fp16 inputs: what the quantisation error is measured against."""
    Q, K, V = (t.double().view(n_img, S, heads, 64).transpose(1, 2) for t in (q, k, v))
    return (torch.softmax(Q @ K.transpose(2, 3) * scale, -1) @ V).transpose(1, 2).reshape(n_img * S, heads * 64)
