"""Weight re-layout from the diffusers state-dict shapes to the kernel layouts (include/vdx.h).

Pure tensor reshapes/permutations done once at load time (on whatever device the weights are on).
"""
from __future__ import annotations

import torch


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def pad_rows(w: torch.Tensor, mult: int = 64) -> torch.Tensor:
    """Zero-pad the output-channel dimension (dim 0) to a multiple of `mult`."""
    n = w.shape[0]
    npad = round_up(n, mult)
    if npad == n:
        return w.contiguous()
    out = w.new_zeros((npad,) + tuple(w.shape[1:]))
    out[:n] = w
    return out


def _taps_slice_major(w_taps: torch.Tensor) -> torch.Tensor:
    """[Cout][T][Cin] -> [Cout][T*Cin] in the kernels' K order (64-channel slice, tap, channel):
    K = (c // 64) * T * 64 + tap * 64 + c % 64.  All taps of one channel slice are consumed back to
    back, which keeps the shifted re-reads of the source pixels in L2 (gemm.hip)."""
    co, t, ci = w_taps.shape
    assert ci % 64 == 0, "gathered convolutions need Cin % 64 == 0"
    return w_taps.reshape(co, t, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, t * ci).contiguous()


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [Cout][Cin][3][3] -> [Cout][9*Cin], tap = ky*3+kx, K order of `_taps_slice_major`."""
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3
    return _taps_slice_major(w.permute(0, 2, 3, 1).reshape(co, 9, ci))


def pack_upconv_phase(w: torch.Tensor, dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """Conv2d weight [N][C][3][3] of a conv that follows a nearest-x2 upsample -> the PHASE table [4*N][4*C] (`dtype`).

    Output pixel (2i+a, 2j+b) of conv3x3(nearest_x2(x)) sees only the 2x2 source pixels (i+a-1+ty, j+b-1+tx), ty, tx in
    {0, 1} (zero outside the image: the padding of the upsampled image falls on the padding of the source), so the nine taps
    collapse onto four whose weights are sums of the original ones:
        a = 0: ty 0 <- ky 0, ty 1 <- ky 1 + ky 2        a = 1: ty 0 <- ky 0 + ky 1, ty 1 <- ky 2        (columns likewise)
    Rows p*N .. p*N+N-1 are phase p = 2a + b; inside a row tap = 2*ty + tx in the K order of `_taps_slice_major`.
    For the fp16 table the sums are formed in fp32 from the fp16-rounded weights and rounded once."""
    n, c, kh, kw = w.shape
    assert kh == 3 and kw == 3
    acc = torch.float32 if dtype == torch.float16 else dtype
    w = (w.to(torch.float16) if dtype == torch.float16 else w).to(acc)
    # mix[a][ty][ky]: which original rows land on tap ty at parity a
    mix = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=acc, device=w.device)
    ph = torch.einsum("ayk,bxl,nckl->abnyxc", mix, mix, w)                      # [a][b][N][ty][tx][C]
    return _taps_slice_major(ph.reshape(4 * n, 4, c)).to(dtype).contiguous()


def pack_conv_in(w: torch.Tensor) -> torch.Tensor:
    """conv_in weight [Cout][Cin][3][3] -> [Cout][Kpad]: K = (ky*3+kx)*Cin + c zero-padded to a
    multiple of 64 (matches the im2col rows of vdx_im2col_in_f16)."""
    p = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)          # plain (tap, channel) order: plain GEMM
    k = p.shape[1]
    out = p.new_zeros((p.shape[0], round_up(k, 64)))
    out[:, :k] = p
    return out


def pack_conv1x1(w: torch.Tensor) -> torch.Tensor:
    """Conv2d 1x1 weight [Cout][Cin][1][1] (or Linear [Cout][Cin]) -> [Cout][Cin]."""
    return w.reshape(w.shape[0], -1).contiguous()


def pack_tconv3(w: torch.Tensor) -> torch.Tensor:
    """Conv3d weight [Cout][Cin][3][1][1] -> [Cout][3*Cin], tap = kt, K order of `_taps_slice_major`."""
    co, ci = w.shape[:2]
    return _taps_slice_major(w.reshape(co, ci, 3).permute(0, 2, 1))


def pack_geglu(w: torch.Tensor, b: torch.Tensor):
    """GEGLU proj Linear(C, 8C): rows [0,4C) = value, [4C,8C) = gate.  Interleave in groups of 4
    rows (value 4t..4t+3, gate 4t..4t+3) so that the GEMM epilogue finds value and gate of the
    same output column in one lane (gemm.hip GEGLU epilogue)."""
    n2, k = w.shape
    half = n2 // 2
    assert half % 4 == 0
    wv = w[:half].reshape(half // 4, 1, 4, k)
    wg = w[half:].reshape(half // 4, 1, 4, k)
    wp = torch.cat([wv, wg], dim=1).reshape(n2, k).contiguous()
    bv = b[:half].reshape(half // 4, 1, 4)
    bg = b[half:].reshape(half // 4, 1, 4)
    bp = torch.cat([bv, bg], dim=1).reshape(n2).contiguous()
    return wp, bp


def nchw_to_rows(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) -> rows [N*H*W][C] (test/helper use)."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def rows_to_nchw(r: torch.Tensor, n: int, h: int, w: int) -> torch.Tensor:
    return r.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------
# K7 (csrc/tattn_fused.hip): weight STAGE IMAGES of the fused temporal-attention sub-block.
# A stage is what one LDS-DMA burst copies verbatim into one ring slot: [tiles][16 rows][4 slots][8 k]
# (64-byte rows: the 32 k values of one MFMA k-step); slot s of row n holds k-chunk s ^ g(n >> 2),
# g = [0, 2, 3, 1], which makes every 16-lane group of the fragment's ds_read_b128 hit 16 distinct
# 16-byte slots of the 256-byte bank row.
# ---------------------------------------------------------------------------------------------
K7_GEOMETRY = {320: dict(nch=1, cg=10), 512: dict(nch=2, cg=8)}      # inner -> column halves, P3 tiles per column group
_K7_G = (0, 2, 3, 1)


def _k7_slot_swizzle(x: torch.Tensor) -> torch.Tensor:
    """x[..., 16 rows, 4 k-chunks, 8] -> same shape with slot s of row n = chunk s ^ g(n >> 2)."""
    n = torch.arange(16, device=x.device)
    g = torch.tensor(_K7_G, device=x.device)[n >> 2]
    idx = torch.arange(4, device=x.device)[None, :] ^ g[:, None]              # [16][4]: source chunk of slot s
    idx = idx[..., None].expand(16, 4, 8)
    return torch.gather(x, -2, idx.expand(x.shape))


def pack_k7_qkv(wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor) -> torch.Tensor:
    """to_q / to_k / to_v weights [inner][inner] -> stages [head group][k step] of [nch][12 tiles][16][4][8]:
    tiles 0-3 = the head's q rows (16 per tile), 4-7 = k, 8-11 = v."""
    inner = wq.shape[0]
    nch = K7_GEOMETRY[inner]["nch"]
    heads, ks = inner // 64, inner // 32
    w = torch.stack([m.reshape(heads, 64, inner) for m in (wq, wk, wv)], dim=1)     # [heads][3][64][inner]
    w = w.reshape(heads // nch, nch, 12, 16, ks, 4, 8)                               # [hg][ch][tile][n][ks][chunk][8]
    w = w.permute(0, 4, 1, 2, 3, 5, 6)                                               # [hg][ks][ch][tile][n][chunk][8]
    return _k7_slot_swizzle(w).contiguous().reshape(-1)


def pack_k7_out(wo: torch.Tensor) -> torch.Tensor:
    """to_out.0 weight [inner][inner] -> stages [column group][k step] of [nch][cg tiles][16][4][8], zero padded to
    the q|k|v stage size.  Row n of tile (2a + j) of a wave's column group carries output column
    32a + 8*(n >> 2) + 4j + (n & 3): after the MFMA a lane owns 8 consecutive columns (16-byte stores)."""
    inner = wo.shape[0]
    nch, cg = K7_GEOMETRY[inner]["nch"], K7_GEOMETRY[inner]["cg"]
    ks, wcols = inner // 32, inner // nch
    ncg = wcols // (16 * cg)
    dev = wo.device
    tile = torch.arange(cg, device=dev)[:, None]
    n = torch.arange(16, device=dev)[None, :]
    col_in_group = 32 * (tile // 2) + 8 * (n >> 2) + 4 * (tile % 2) + (n & 3)      # [cg][16]
    chv = torch.arange(nch, device=dev)[None, :, None, None]
    cgv = torch.arange(ncg, device=dev)[:, None, None, None]
    col = chv * wcols + cgv * 16 * cg + col_in_group[None, None]                   # [ncg][nch][cg][16]
    w = wo[col.reshape(-1)].reshape(ncg, nch, cg, 16, ks, 4, 8)
    w = _k7_slot_swizzle(w.permute(0, 4, 1, 2, 3, 5, 6)).contiguous()              # [ncg][ks][nch][cg][16][4][8]
    stage = nch * 192 * 32                                                           # elements of a q|k|v stage
    out = wo.new_zeros((ncg, ks, stage))
    out[:, :, :nch * cg * 512] = w.reshape(ncg, ks, -1)
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------
# K7, second design (csrc/tattn2.hip): ONE packed blob per attention sub-block.
#   [heads][15 units]  q|k|v stream: per head q0 k0 q1 k1 .. q4 k4 v0 .. v4, a unit = 64 weight rows x 64 k as 8 tiles
#                      (tile 4*kk + j: rows 16j .. 16j+15, MFMA k step 2m + kk), tile format as above;
#   [2 full column groups][heads][2 units] + [last 64 columns][heads][1 unit]  output projection, contracted head by
#                      head; its k index is PERMUTED so that the P.V accumulators of the kernel are its B operand
#                      as they stand: element j8 of lane quad q4 of k step (h, kk) is channel
#                      64h + 32kk + 16*(j8 >> 2) + 4*q4 + (j8 & 3);
#   fp32 [inner] q bias, fp32 [inner] output bias.
# LayerNorm's affine and the softmax scale are folded in here: W_q' = c.W_q.diag(gamma) (c = scale.log2 e),
# W_k' = W_k.diag(gamma), W_v' = W_v.diag(gamma); q bias = c.W_q.beta; the k bias adds a per-query constant to the
# scores (softmax-invariant) and is dropped; the v bias passes through the softmax (rows of P sum to 1) into the
# output bias: b_o' = b_o + W_o.(W_v.beta).
# ---------------------------------------------------------------------------------------------
K7B_WIDTHS = (320,)


def _k7b_units(w: torch.Tensor, heads: int, km: int) -> torch.Tensor:
    """[heads*64][inner] -> [heads][km][8 tiles][16][4][8] (tile = 4*kk + j)."""
    x = w.reshape(heads, 4, 16, km, 2, 4, 8)              # [h][j][n][m][kk][chunk][8]
    x = x.permute(0, 3, 4, 1, 2, 5, 6)                     # [h][m][kk][j][n][chunk][8]
    return x.reshape(heads, km, 8, 16, 4, 8)


def pack_k7b(wq, wk, wv, wo, gamma, beta, bo, scale: float) -> torch.Tensor:
    """-> fp16 tensor holding the blob (the two fp32 vectors at its end are stored as raw bits)."""
    inner = wq.shape[0]
    assert inner in K7B_WIDTHS and inner % 128 == 64
    heads, km = inner // 64, inner // 64
    dev = wq.device
    f = lambda x: x.to(device=dev, dtype=torch.float32)    # noqa: E731
    wq, wk, wv, wo, gamma, beta, bo = (f(x) for x in (wq, wk, wv, wo, gamma, beta, bo))
    c = float(scale) * 1.4426950408889634
    q16 = (wq * gamma[None, :] * c).half()
    k16 = (wk * gamma[None, :]).half()
    v16 = (wv * gamma[None, :]).half()
    bq = c * (wq @ beta)
    bo2 = bo + wo @ (wv @ beta)
    uq, uk, uv = (_k7b_units(x, heads, km) for x in (q16, k16, v16))
    qk = torch.stack([uq, uk], dim=2).reshape(heads, 2 * km, 8, 16, 4, 8)
    qkv = _k7_slot_swizzle(torch.cat([qk, uv], dim=1)).reshape(-1)             # [h][15][8][16][4][8]
    # output projection
    wo16 = wo.half()
    ar = lambda n: torch.arange(n, device=dev)             # noqa: E731
    chunk, j8 = ar(4)[:, None], ar(8)[None, :]
    kperm = 16 * (j8 >> 2) + 4 * chunk + (j8 & 3)                               # [4][8] channel inside a 32-wide k step
    n = ar(16)

    def cols(base, ntile):
        jt = ar(ntile)[:, None]
        return base + 32 * (jt // 2) + 8 * (n[None, :] >> 2) + 4 * (jt % 2) + (n[None, :] & 3)     # [ntile][16]

    parts = []
    for cg in range(inner // 128):
        col = cols(128 * cg, 8)                                                 # [8][16]
        u = torch.empty((heads, 2, 8, 16, 4, 8), dtype=torch.float16, device=dev)
        for h in range(heads):
            for kk in range(2):
                ch = 64 * h + 32 * kk + kperm                                   # [4][8]
                u[h, kk] = wo16[col[:, :, None, None], ch[None, None]]
        parts.append(_k7_slot_swizzle(u).reshape(-1))
    col = cols(128 * (inner // 128), 4)                                         # [4][16]
    u = torch.empty((heads, 2, 4, 16, 4, 8), dtype=torch.float16, device=dev)
    for h in range(heads):
        for kk in range(2):
            ch = 64 * h + 32 * kk + kperm
            u[h, kk] = wo16[col[:, :, None, None], ch[None, None]]
    parts.append(_k7_slot_swizzle(u).reshape(-1))                               # [h][tile 4*kk + jt][16][4][8]
    vec = torch.cat([bq, bo2]).contiguous().view(torch.float16)
    return torch.cat([qkv] + parts + [vec]).contiguous()


def pack_k8_proj(wp, bp) -> torch.Tensor:
    """The transformer's proj_out [inner][inner] + bias as the TAIL of K8 (csrc/ff_fused.hip, PO): 25 units in tattn2's
    output-projection format with the natural k order, fp32 b_p."""
    inner = wp.shape[0]
    assert inner in K8_WIDTHS and tuple(wp.shape) == (inner, inner)
    dev = wp.device
    parts = _k7b_pack_wo(wp.to(device=dev, dtype=torch.float32).half(), inner // 64, inner, natural=True)
    vec = bp.to(device=dev, dtype=torch.float32).contiguous().view(torch.float16)
    return torch.cat(parts + [vec]).contiguous()


# ---------------------------------------------------------------------------------------------
# K5 (csrc/xattn.hip): the cross-attention sub-block in one kernel.  The static blob is K7B's with the k / v parts
# taken out: [heads][5 units] q stream (W_q' = c.W_q.diag(gamma), c = scale.log2 e), the output projection exactly as
# K7B packs it (k index permuted to the order in which P.V leaves the accumulators), fp32 q bias c.W_q.beta, fp32 b_o.
# The text keys / values are packed ONCE PER PROMPT (`pack_k5_kv`, torch ops on the device) into MFMA-fragment order:
# per (batch item, head) 3 units of 8 KB = K fragments [kt 5][j 4][lane 64][4 halfs] (lane (n16, q4) holds
# K[16kt + n16][64h + 16j + 4q4 + e]), V fragments [kt 5][dt 4][lane][4] (V[16kt + 4q4 + e][64h + 16dt + n16]), zero pad.
# ---------------------------------------------------------------------------------------------
K5_WIDTHS = (320,)
K5_KEY_SLOTS = 80


def _k7b_pack_wo(wo16: torch.Tensor, heads: int, inner: int, natural: bool = False):
    """tattn2's output-projection units.  `natural`: the k index in its natural order (lane quad q holds channels 8q .. 8q+7 of a
    32-wide k step: the B operand is a tile pair of fp16-rounded accumulators, K8's tail) instead of the order in which P.V leaves
    the accumulators (K7 / K5)."""
    dev = wo16.device
    ar = lambda n: torch.arange(n, device=dev)             # noqa: E731
    chunk, j8 = ar(4)[:, None], ar(8)[None, :]
    kperm = (8 * chunk + j8) if natural else (16 * (j8 >> 2) + 4 * chunk + (j8 & 3))      # [4][8] channel inside a 32-wide k step
    n = ar(16)

    def cols(base, ntile):
        jt = ar(ntile)[:, None]
        return base + 32 * (jt // 2) + 8 * (n[None, :] >> 2) + 4 * (jt % 2) + (n[None, :] & 3)     # [ntile][16]

    parts = []
    for cg in range(inner // 128):
        col = cols(128 * cg, 8)
        u = torch.empty((heads, 2, 8, 16, 4, 8), dtype=torch.float16, device=dev)
        for h in range(heads):
            for kk in range(2):
                ch = 64 * h + 32 * kk + kperm
                u[h, kk] = wo16[col[:, :, None, None], ch[None, None]]
        parts.append(_k7_slot_swizzle(u).reshape(-1))
    col = cols(128 * (inner // 128), 4)
    u = torch.empty((heads, 2, 4, 16, 4, 8), dtype=torch.float16, device=dev)
    for h in range(heads):
        for kk in range(2):
            ch = 64 * h + 32 * kk + kperm
            u[h, kk] = wo16[col[:, :, None, None], ch[None, None]]
    parts.append(_k7_slot_swizzle(u).reshape(-1))
    return parts


def pack_k5(wq, wo, gamma, beta, bo, scale: float) -> torch.Tensor:
    """to_q [inner][inner], to_out.0 [inner][inner] + bias, norm2's gamma / beta -> fp16 tensor holding the static blob."""
    inner = wq.shape[0]
    assert inner in K5_WIDTHS and inner % 128 == 64 and tuple(wq.shape) == (inner, inner) and tuple(wo.shape) == (inner, inner)
    heads, km = inner // 64, inner // 64
    dev = wq.device
    f = lambda x: x.to(device=dev, dtype=torch.float32)    # noqa: E731
    wq, wo, gamma, beta, bo = (f(x) for x in (wq, wo, gamma, beta, bo))
    c = float(scale) * 1.4426950408889634
    q16 = (wq * gamma[None, :] * c).half()
    bq = c * (wq @ beta)
    uq = _k7_slot_swizzle(_k7b_units(q16, heads, km)).reshape(-1)              # [h][5][8][16][4][8]
    vec = torch.cat([bq, bo]).contiguous().view(torch.float16)
    return torch.cat([uq] + _k7b_pack_wo(wo.half(), heads, inner) + [vec]).contiguous()


def pack_k5_kv(k_rows: torch.Tensor, vt: torch.Tensor, n_items: int, text_pad: int) -> torch.Tensor:
    """k_rows [n_items*text_pad][inner] (text keys, rows past the text are ignored by the kernel's mask), vt [inner][n_items*
    text_pad] (text values, transposed: what the un-fused path keeps) -> [n_items][heads][3 * 4096] fp16 fragment blobs."""
    inner = k_rows.shape[1]
    heads, ks = inner // 64, K5_KEY_SLOTS
    assert inner in K5_WIDTHS and text_pad >= ks and k_rows.shape[0] == n_items * text_pad and tuple(vt.shape) == (inner, n_items * text_pad)
    K = k_rows.reshape(n_items, text_pad, inner)[:, :ks]                                             # [item][key][c]
    V = vt.reshape(inner, n_items, text_pad).permute(1, 2, 0)[:, :ks]                                # [item][key][c]
    kf = K.reshape(n_items, 5, 16, heads, 4, 4, 4).permute(0, 3, 1, 4, 5, 2, 6)                      # [item][h][kt][j][q4][n16][e]
    vf = V.reshape(n_items, 5, 4, 4, heads, 4, 16).permute(0, 4, 1, 5, 2, 6, 3)                      # [item][h][kt][dt][q4][n16][e]
    out = torch.zeros((n_items, heads, 3 * 4096), dtype=torch.float16, device=k_rows.device)
    out[:, :, :5120] = kf.reshape(n_items, heads, 5120)
    out[:, :, 5120:10240] = vf.reshape(n_items, heads, 5120)
    return out.contiguous()


# ---------------------------------------------------------------------------------------------
# K8 (csrc/ff_fused.hip): the feed-forward sub-block in one kernel.  LayerNorm's affine is folded into the first
# projection: W1' = W1.diag(gamma), b1' = b1 + W1.beta (the initial accumulators of val / gate).  The hidden width is
# cut into chunks of 64; a chunk's blob is 15 units of 8 KB in K7B's unit format: (val, gate) for each of the five K-64
# steps, then the chunk's k slice of W2 — 2 + 2 units for the two 128-column groups, 1 for the last 64 columns — with
# the k index permuted to the order in which val * gelu(gate) leaves the accumulators (as K7B's W_o).
# ---------------------------------------------------------------------------------------------
K8_WIDTHS = (320,)


def pack_k8(w1, b1, w2, b2, gamma, beta) -> torch.Tensor:
    """w1 [8*inner][inner] (rows: val | gate, diffusers GEGLU.proj), b1 [8*inner], w2 [inner][4*inner], b2 [inner]
    -> fp16 tensor holding the blob (the fp32 vectors at its end are stored as raw bits)."""
    inner = w2.shape[0]
    assert inner in K8_WIDTHS and inner % 128 == 64
    hid, km = 4 * inner, inner // 64
    chunks = hid // 64
    dev = w1.device
    f = lambda x: x.to(device=dev, dtype=torch.float32)    # noqa: E731
    w1, b1, w2, b2, gamma, beta = (f(x) for x in (w1, b1, w2, b2, gamma, beta))
    val16 = (w1[:hid] * gamma[None, :]).half()
    gate16 = (w1[hid:] * gamma[None, :]).half()
    b1f = b1 + w1 @ beta
    uv, ug = _k7b_units(val16, chunks, km), _k7b_units(gate16, chunks, km)     # [chunk][km][8][16][4][8]
    a_units = torch.stack([uv, ug], dim=2).reshape(chunks, 2 * km, 8, 16, 4, 8)
    w2h = w2.half()
    ar = lambda n: torch.arange(n, device=dev)             # noqa: E731
    q, j8 = ar(4)[:, None], ar(8)[None, :]
    kperm = 16 * (j8 >> 2) + 4 * q + (j8 & 3)                                   # [4][8] hidden index inside a 32-wide k step
    n = ar(16)

    def cols(base, ntile):
        jt = ar(ntile)[:, None]
        return base + 32 * (jt // 2) + 8 * (n[None, :] >> 2) + 4 * (jt % 2) + (n[None, :] & 3)     # [ntile][16]

    hcol = 64 * ar(chunks)[:, None, None, None] + 32 * ar(2)[None, :, None, None] + kperm[None, None]      # [chunk][kk][4][8]
    b_units = []
    for cg in range(inner // 128):
        col = cols(128 * cg, 8)                                                 # [8][16]
        u = w2h[col[None, None, :, :, None, None], hcol[:, :, None, None]]      # [chunk][kk][8][16][4][8]
        b_units.append(u)
    col = cols(128 * (inner // 128), 4)                                         # [4][16]
    u = w2h[col[None, None, :, :, None, None], hcol[:, :, None, None]]          # [chunk][kk][4][16][4][8]
    b_units.append(u.reshape(chunks, 1, 8, 16, 4, 8))                           # tile 4*kk + jt
    units = torch.cat([a_units] + b_units, dim=1)                               # [chunk][15][8][16][4][8]
    blob = _k7_slot_swizzle(units).reshape(-1)
    bias = torch.cat([torch.stack([b1f[:hid].reshape(chunks, 64), b1f[hid:].reshape(chunks, 64)], dim=1).reshape(-1), b2])
    return torch.cat([blob, bias.contiguous().view(torch.float16)]).contiguous()
