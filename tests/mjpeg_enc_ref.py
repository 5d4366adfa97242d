"""A slow restatement in Python / numpy of the three stages of csrc/mjpeg_enc.hip (the GPU Motion-JPEG writer): colour
conversion + downsampling, forward DCT + quantisation, entropy coding.  It is libjpeg's baseline encoder as Pillow drives it
(quality 92, 4:2:0 or grey, standard Huffman tables) in integers, so the CPU suite can pin the definition byte for byte
against Pillow without a GPU (tests/test_video_enc_host.py) and the GPU suite can compare every stage of the kernels with it
(tests/test_video_enc_gpu.py).

The edge rules, as libjpeg has them:
  * columns: the last column is replicated at full resolution up to the padded width before the downsample;
  * rows: a row pair cut by the bottom edge (odd H) is completed by replicating the last row at full resolution, then
    downsampled; the rows below are replicas of the last DOWNSAMPLED row (chroma) or of the last row (luma).  The two differ
    whenever H is even and not a multiple of 16: the last chroma row then mixes rows H-2 and H-1, and its replicas do too;
  * luma blocks wholly outside ceil(extent / 8) blocks are dummy blocks: AC zero, DC that of the previous block of the MCU.
"""
import numpy as np

from vdx import video

import mjpeg_enc
import mjpeg_ref

ZIGZAG = np.asarray(video._ZIGZAG)


def _fix(x):
    return int(x * 65536 + 0.5)


def planes(frames, layout):
    """uint8 frames [F][H][W][3] (layout 2) or [F][H][W] (layout 0) -> list over components of uint8 [F][bh*8][bw*8]."""
    frames = np.asarray(frames)
    F, H, W = frames.shape[:3]
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    PH, PW = bh[0] * 8, bw[0] * 8
    rows, cols = np.minimum(np.arange(PH), H - 1), np.minimum(np.arange(PW), W - 1)
    if layout == 0:
        return [frames[:, rows][:, :, cols]]
    x = frames.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    off = (128 << 16) + 32767
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + off) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + off) >> 16
    out = [y[:, rows][:, :, cols].astype(np.uint8)]
    CH = (H + 1) // 2
    for c in (cb, cr):
        full = c[:, np.minimum(np.arange(2 * CH), H - 1)][:, :, cols]               # complete the last row pair, pad the columns
        bias = 1 + (np.arange(PW // 2) & 1)                                         # 1, 2, 1, 2, ... along the output columns
        down = (full[:, 0::2, 0::2] + full[:, 0::2, 1::2] + full[:, 1::2, 0::2] + full[:, 1::2, 1::2] + bias) >> 2
        out.append(down[:, np.minimum(np.arange(PH // 2), CH - 1)].astype(np.uint8))  # replicate the last downsampled row
    return out


def _fdct8(x, first):
    """The 1-D slow-integer forward DCT along the last axis (int64), pass 1 (`first`) or pass 2 of libjpeg's jfdctint."""
    d = [x[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    shift = 13 - 2 if first else 13 + 2
    desc = lambda v, n: (v + (1 << (n - 1))) >> n                                  # noqa: E731
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o[0], o[4] = desc(tmp10 + tmp11, 2), desc(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    o[2], o[6] = desc(z1 + tmp13 * 6270, shift), desc(z1 + tmp12 * -15137, shift)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = desc(tmp4 + z1 + z3, shift), desc(tmp5 + z2 + z4, shift), desc(tmp6 + z2 + z3, shift), \
        desc(tmp7 + z1 + z4, shift)
    return np.stack(o, -1)


def quantise(v, q):
    """sign(v) * ((|v| + (8q >> 1)) // (8q)): the DCT leaves its output scaled by 8."""
    d = 8 * q
    return np.sign(v) * ((np.abs(v) + (d >> 1)) // d)


def source_block(by, bx, rbh, rbw):
    """The block of component 0 whose DC a block at (by, bx) carries: itself when real, else the last real block before it in
    its MCU's order (0,0) (0,1) (1,0) (1,1).  rbh x rbw real blocks; only 2x2 MCUs have dummies."""
    if by >= rbh:                                   # a dummy row follows both blocks of the MCU's first row
        return by - 1, ((bx | 1) if (bx | 1) < rbw else (bx | 1) - 1)
    if bx >= rbw:
        return by, bx - 1
    return by, bx


def coefficients(pl, quant, W, H, layout):
    """component planes, quant int [2][64] (luma, chroma; natural order) -> int16 [F][blocks per frame][64] in the decoder's
    workspace layout (mjpeg_ref._geometry)."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    F = pl[0].shape[0]
    out = np.zeros((F, boff[-1], 64), np.int16)
    for c in range(ncomp):
        x = pl[c].astype(np.int64).reshape(F, bh[c], 8, bw[c], 8).transpose(0, 1, 3, 2, 4) - 128
        x = _fdct8(x, True)                                                         # rows
        x = np.swapaxes(_fdct8(np.swapaxes(x, -1, -2), False), -1, -2)              # columns
        co = quantise(x.reshape(F, bh[c], bw[c], 64), np.asarray(quant[min(c, 1)], np.int64))
        if c == 0 and layout == 2:
            rbh, rbw = -(-H // 8), -(-W // 8)
            real = co.copy()
            for by in range(bh[0]):
                for bx in range(bw[0]):
                    sy, sx = source_block(by, bx, rbh, rbw)
                    if (sy, sx) != (by, bx):
                        co[:, by, bx] = 0
                        co[:, by, bx, 0] = real[:, sy, sx, 0]
        out[:, boff[c]:boff[c + 1]] = co.reshape(F, -1, 64)
    return out


class Counters:
    """What the entropy stage met: filled by `entropy`, asserted by the tests about their own inputs."""
    def __init__(self):
        self.stuffed = self.zrl = self.max_dc_size = self.segments_whole_bytes = self.segments_padded = 0


_CODES = None


def _codes():
    global _CODES
    if _CODES is None:
        std = mjpeg_enc.standard_tables()
        assert std == video.STANDARD_HUFFMAN
        _CODES = {key: mjpeg_enc.codes_of(p) for key, p in std.items()}
    return _CODES


def mcu_order(W, H, layout):
    """-> int array [nmcu * blocks per MCU]: the workspace block index of every block in the order the scan codes them."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    order = []
    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        for c in range(ncomp):
            for by in range(hs[c]):
                for bx in range(hs[c]):
                    order.append(boff[c] + (my * hs[c] + by) * bw[c] + mx * hs[c] + bx)
    return np.asarray(order)


def entropy(coef, W, H, layout, dri=0, counters=None):
    """int16 coefficients [bpf][64] of ONE frame -> the scan's bytes (stuffed, restart markers between the segments, no EOI),
    and the bit length of every block in scan order."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    codes = _codes()
    order = mcu_order(W, H, layout)
    bpm = len(order) // (mcux * mcuy)
    step = (dri or mcux * mcuy) * bpm
    comp_of = np.searchsorted(np.asarray(boff[1:]), order, side="right")
    out, lengths = b"", []
    for si, s0 in enumerate(range(0, len(order), step)):
        acc = nbits = 0
        pred = [0] * ncomp
        for i in range(s0, min(s0 + step, len(order))):
            c = int(comp_of[i])
            dc, ac = codes[(0, min(c, 1))], codes[(1, min(c, 1))]
            before = nbits
            for op in mjpeg_enc.block_ops(coef[order[i]], pred[c]):
                if op[0] == "dc":
                    size, v = abs(op[1]).bit_length(), op[1]
                    sym = dc[size]
                    pred[c] += v
                    if counters is not None:
                        counters.max_dc_size = max(counters.max_dc_size, size)
                elif op[0] == "ac":
                    size, v = abs(op[2]).bit_length(), op[2]
                    sym = ac[(op[1] << 4) | size]
                else:
                    size, v = 0, 0
                    sym = ac[0xF0 if op[0] == "zrl" else 0x00]
                    if counters is not None and op[0] == "zrl":
                        counters.zrl += 1
                acc = (acc << sym[1]) | sym[0]
                nbits += sym[1]
                if size:
                    acc = (acc << size) | (v if v >= 0 else v + (1 << size) - 1)
                    nbits += size
            lengths.append(nbits - before)
        fill = -nbits % 8
        raw = ((acc << fill) | ((1 << fill) - 1)).to_bytes((nbits + fill) // 8, "big")
        if counters is not None:
            counters.stuffed += raw.count(b"\xff")
            counters.segments_whole_bytes += fill == 0
            counters.segments_padded += fill != 0
        if si:
            out += bytes([0xFF, 0xD0 + (si - 1) % 8])
        out += raw.replace(b"\xff", b"\xff\x00")
    return out, lengths


def encode(frames, quality=92, restart_rows=0, counters=None, stages=None):
    """uint8 frames [F][H][W][3] or [F][H][W] -> list of JPEG byte strings; `stages` (a dict) receives the planes and the
    coefficients."""
    frames = np.asarray(frames)
    layout = 2 if frames.ndim == 4 else 0
    sampling = "4:2:0" if layout else "L"
    F, H, W = frames.shape[:3]
    ncomp, mcux = mjpeg_ref._geometry(W, H, layout)[:2]
    head = video.jpeg_header(W, H, sampling, quality, restart_rows)
    pl = planes(frames, layout)
    coef = coefficients(pl, video.quant_tables(quality), W, H, layout)
    if stages is not None:
        stages["planes"], stages["coef"] = pl, coef
    return [head + entropy(coef[f], W, H, layout, restart_rows * mcux, counters)[0] + b"\xff\xd9" for f in range(F)]


# ---------------------------------------------------------------------------------------------
# The inputs tests/test_video_enc_host.py (against Pillow) and tests/test_video_enc_gpu.py (the kernels) share
# ---------------------------------------------------------------------------------------------
KINDS = ("noise", "gradient", "saturated", "constant")
SIZES = ((16, 16), (8, 8), (1, 1), (50, 38), (47, 33), (31, 17), (128, 72))          # W x H
MODES = ("RGB", "L")
RESTART_ROWS = (0, 1, 2)


def content(kind, W, H, mode, seed=0):
    g = np.random.default_rng(seed + 7 * W + H)
    shape = (H, W) if mode == "L" else (H, W, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":                                   # long codes, FF bytes to stuff
        a = g.integers(0, 256, shape)
    elif kind == "gradient":                              # EOB-heavy, long zero runs before a late coefficient (ZRL)
        a = (xx * 255 // max(W - 1, 1) + yy * 3) % 256
        a = a + (g.integers(0, 40, (H, W)) == 0) * 9      # sparse specks: isolated high-frequency coefficients
        a = a if mode == "L" else np.stack([a, a[::-1], (xx + yy) * 255 // max(W + H - 2, 1)], -1)
    elif kind == "saturated":                             # 8x8 checkerboard of 0 / 255: DC differences of size 10; some noise
        a = ((xx // 8 + yy // 8) % 2) * 255
        a = a if mode == "L" else np.stack([a, a, a], -1)
        a = np.where(g.integers(0, 6, shape) == 0, g.integers(0, 2, shape) * 255, a)
    else:
        a = np.full(shape, 77)
    return np.asarray(a, np.int64).clip(0, 255).astype(np.uint8)


def cases():
    """-> [(id, uint8 frame [H][W][3] or [H][W])]"""
    return [(f"{kind}-{W}x{H}-{mode}", content(kind, W, H, mode)) for kind in KINDS for (W, H) in SIZES for mode in MODES]


def pillow_encode(img, restart_rows=0, quality=92):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=quality, **({"restart_marker_rows": restart_rows} if restart_rows else {}))
    return buf.getvalue()
