"""A slow restatement in Python / numpy of the three stages of csrc/mjpeg_enc.hip (the GPU Motion-JPEG writer): colour
conversion + downsampling, forward DCT + quantisation, entropy coding.  It is libjpeg's baseline encoder as Pillow drives it
(any quality, 4:2:0 or grey, standard Huffman tables) in integers, so the CPU suite can pin the definition byte for byte
against Pillow without a GPU (tests/test_video_enc_host.py) and the GPU suite can compare every stage of the kernels with it
(tests/test_video_enc_gpu.py from images; tests/test_video_enc_stages_gpu.py stage by stage, from the inputs at the end of this
file that no image produces).

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


def segments(coef, W, H, layout, dri=0, counters=None):
    """int16 coefficients [bpf][64] of ONE frame -> the restart intervals' bytes before stuffing (padded to a byte with
    1-bits), the bit length of every block in scan order, and the blocks per restart interval."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    codes = _codes()
    order = mcu_order(W, H, layout)
    bpm = len(order) // (mcux * mcuy)
    step = (dri if 0 < dri < mcux * mcuy else mcux * mcuy) * bpm
    comp_of = np.searchsorted(np.asarray(boff[1:]), order, side="right")
    raws, lengths = [], []
    for s0 in range(0, len(order), step):
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
        raws.append(raw)
    return raws, lengths, step


def entropy(coef, W, H, layout, dri=0, counters=None):
    """int16 coefficients [bpf][64] of ONE frame -> the scan's bytes (stuffed, restart markers between the segments, no EOI),
    and the bit length of every block in scan order."""
    raws, lengths, _ = segments(coef, W, H, layout, dri, counters)
    out = b""
    for si, raw in enumerate(raws):
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


# ---------------------------------------------------------------------------------------------
# Inputs at the edges of every stage.  Each one states, on the restatement alone, the property it exists for
# (tests/test_video_enc_host.py runs those assertions); tests/test_video_enc_stages_gpu.py puts them before the kernels.
# ---------------------------------------------------------------------------------------------
QUALITIES = (1, 10, 30, 50, 75, 95, 100)
SWEEP_SIZES = ((47, 33), (16, 16), (1, 1))
BASIS_GRID = (10, 13)                                     # blocks per row, block rows of the basis image: 80 x 104 samples
SLOT_BYTES = video.ENC_SLOT_BYTES


def basis_blocks():
    """-> uint8 [130][8][8]: for every basis function (u, v) of the 8x8 DCT the block that is 255 where the function is >= 0
    and 0 elsewhere (it maximises that coefficient), followed by its inverse; then all-0 and all-255.  Blocks 0 and 1 are
    all-255 and all-0, blocks 128 and 129 all-0 and all-255: neighbours in scan order, DC differences of -2040 and +2040."""
    n = np.arange(8)
    cos = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16)                    # [frequency][position]
    out = []
    for v in range(8):
        for u in range(8):
            b = np.where(cos[v][:, None] * cos[u][None, :] >= -1e-12, 255, 0)
            out += [b, 255 - b]
    out += [np.zeros((8, 8), np.int64), np.full((8, 8), 255)]
    return np.stack(out).astype(np.uint8)


def basis_image(mode):
    """The basis blocks row-major on a grid of 10 x 13 blocks -> uint8 [104][80] ("L"), or [104][80][3] ("RGB": the image, its
    inverse, the image flipped top to bottom; 6.5 MCU rows, so the 4:2:0 frame has a dummy luma block row)."""
    bx, by = BASIS_GRID
    img = basis_blocks().reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
    return img if mode == "L" else np.ascontiguousarray(np.stack([img, 255 - img, img[::-1]], -1))


def basis_planes(W, H, layout, F):
    """Component planes of F frames of W x H (as `planes` shapes them) whose every block, dummy ones included, is a basis block:
    component c of frame f holds the blocks from 43 c + f * (its blocks per frame) on, cyclically."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    blocks = basis_blocks()
    out = []
    for c in range(ncomp):
        n = bw[c] * bh[c]
        idx = (43 * c + np.arange(F * n)) % len(blocks)
        out.append(np.ascontiguousarray(blocks[idx].reshape(F, bh[c], bw[c], 8, 8).transpose(0, 1, 3, 2, 4).reshape(F, bh[c] * 8, bw[c] * 8)))
    return out


def check_basis(coef, counters):
    """What the basis image (grey, quality 100: every divisor 1) must reach: the extremes stage 2's comment names."""
    ac = np.abs(coef[..., 1:].astype(np.int64)).max()
    dc = coef[..., 0]
    assert ac == 1020, f"largest |AC| is {ac}"
    assert (int(dc.min()), int(dc.max())) == (-1024, 1016), (dc.min(), dc.max())
    assert counters.max_dc_size == 11, counters.max_dc_size


def _scan_blocks(W, H, layout, scan):
    """blocks in scan order [bpf][64] -> the workspace's order."""
    order = mcu_order(W, H, layout)
    coef = np.zeros((len(order), 64), np.int16)
    coef[order] = scan
    return coef


def _dense(n, signs, layout=0):
    """n blocks in scan order: every AC 1023 * signs[k] (zigzag k); the DC of each component goes +1023, -1024, +1023, ...
    along the scan, so every difference after a segment's first is +-2047."""
    zz = np.empty((n, 64), np.int64)
    zz[:, 1:] = 1023 * np.asarray(signs)[1:]
    seen = [0, 0, 0]
    for i in range(n):
        c = (0, 0, 0, 0, 1, 2)[i % 6] if layout == 2 else 0
        zz[i, 0] = (1023, -1024)[seen[c] % 2]
        seen[c] += 1
    out = np.empty_like(zz)
    out[:, ZIGZAG] = zz
    return out


_SETS = None


def coef_sets():
    """-> {name: (layout, W, H, int16 coefficients [bpf][64] in the workspace's order, dri)}: valid baseline streams
    (|DC difference| <= 2047, |AC| <= 1023) that no encoder reaches from 8-bit samples.  `check_coef_set` states what each is
    for."""
    global _SETS
    if _SETS is not None:
        return _SETS
    out = {}
    alternating = np.where(np.arange(64) % 2 == 1, 1, -1)
    for tag, layout, W, H in (("L", 0, 48, 16), ("420", 2, 32, 16)):
        n = mjpeg_ref._geometry(W, H, layout)[6][-1]
        for dri in (0, 1):
            out[f"max-bits-{tag}-dri{dri}"] = (layout, W, H, _scan_blocks(W, H, layout, _dense(n, alternating, layout)), dri)
    # every AC +1023: 21 one-bits out of every 26.  8 x 24 blocks, a restart interval per row of 8: slot edges inside a segment
    for nrows in range(1, 64):
        W, H = 64, 8 * nrows
        cand = (0, W, H, _scan_blocks(W, H, 0, _dense(8 * nrows, np.ones(64, np.int64))), 8)
        at = {i % SLOT_BYTES for raw in segments(cand[3], W, H, 0, 8)[0] for i in range(len(raw)) if raw[i] == 0xFF}
        if SLOT_BYTES - 1 in at and 0 in at and nrows >= 2:
            break
    out["all-ones"] = cand
    B = mjpeg_enc._block
    runs = [B(5 + r, **{f"z{r + 1}": (-1) ** r * (r + 2)}) for r in (15, 16, 17, 31, 32, 33, 47, 48)]   # the run before z<r + 1>
    edge = [B(-40, z63=-3),                                # three ZRL + a run of 14 landing on k = 63
            B(7, z1=2, z62=-1, z63=1),                     # k = 63 right after k = 62: no run, no EOB
            B(7),                                          # a lone DC whose difference is 0
            B(-300),                                       # a lone DC
            B(9, z1=1, z18=-1, z35=1, z52=-1),             # a run of 16 three times in one block
            B(0, z16=1, z33=-2, z63=3)]                    # runs of 15, 16 and 29
    out["zrl-L"] = (0, 8 * 14, 8, np.stack(runs + edge).astype(np.int16), 0)
    # 4:2:0 32 x 16: 8 luma blocks, then the chroma blocks (their ZRL has another code): rotate so that chroma gets the edges
    twelve = (edge + runs)[:12]
    out["zrl-420"] = (2, 32, 16, np.stack(twelve[4:] + twelve[:4]).astype(np.int16), 0)
    for mod8 in range(8):
        out[f"mod8-{mod8}"] = (0, 16, 8, mjpeg_enc.sized(mod8)[0].astype(np.int16), 0)
    out["zeros-300"] = (0, 8 * 300, 8, np.zeros((300, 64), np.int16), 0)
    g = np.random.default_rng(11)
    small = g.integers(-3, 4, (11, 64)) * (g.random((11, 64)) < 0.3)
    small[:, 0] = g.integers(-60, 61, 11)
    out["rst-wrap"] = (0, 8, 8 * 11, small.astype(np.int16), 1)
    some = g.integers(-9, 10, (12, 64)) * (g.random((12, 64)) < 0.2)
    some[:, 0] = g.integers(-100, 101, 12)
    for extra in (0, 5):                                   # nmcu = 2
        out[f"one-segment-dri{2 + extra}"] = (2, 32, 16, some.astype(np.int16), 2 + extra)
    _SETS = out
    return out


def slots_of(raws, step, nblocks):
    """The segments' unstuffed bytes, the blocks per segment and per frame -> per block of the frame, in scan order, the bytes
    slot j of its segment takes in the file: bytes [208 j, 208 (j + 1)) of the segment, 2 for every FF among them, and the
    RSTn marker in front of the first slot of every segment but the first."""
    out = []
    for si, raw in enumerate(raws):
        a = np.frombuffer(raw, np.uint8)
        for j in range(min(step, nblocks - si * step)):
            part = a[SLOT_BYTES * j:SLOT_BYTES * (j + 1)]
            out.append(len(part) + int((part == 0xFF).sum()) + (2 if si and j == 0 else 0))
    return out


def check_coef_set(name, entry):
    """The property `name` exists for, asserted on the restatement alone."""
    layout, W, H, coef, dri = entry
    ncomp, mcux, mcuy = mjpeg_ref._geometry(W, H, layout)[:3]
    nmcu, bpm = mcux * mcuy, (6 if layout == 2 else 1)
    c = Counters()
    raws, lengths, step = segments(coef, W, H, layout, dri, c)
    scan = entropy(coef, W, H, layout, dri)[0]
    lengths = np.asarray(lengths)
    zz = coef.astype(np.int64)[mcu_order(W, H, layout)][:, ZIGZAG]
    assert np.abs(zz[:, 1:]).max() <= 1023
    assert len(raws) == (-(-nmcu // dri) if 0 < dri < nmcu else 1) and step * len(raws) >= len(lengths)
    for raw, s0 in zip(raws, range(0, len(lengths), step)):                          # the slot bound of csrc/mjpeg_enc.hip
        assert len(raw) <= SLOT_BYTES * len(lengths[s0:s0 + step])
    if name.startswith("max-bits") or name == "all-ones":
        assert lengths.max() == 1658 and c.max_dc_size == 11
        first = np.arange(len(lengths)) % step < (1 if layout == 0 else bpm)         # the blocks whose prediction may be 0
        luma = np.arange(len(lengths)) % bpm < (4 if layout == 2 else 1)
        assert (lengths[luma & ~first] == 1658).all(), "every luma block after a segment's first costs 1658 bits"
        # the chroma tables code run 0 / size 10 in 12 bits and DC size 11 in 11: 22 + 63 * 22
        assert (lengths[~luma & ~first] == 1408).all()
        assert set(lengths[luma & first]) <= {1656, 1658} and set(lengths[~luma & first]) <= {1406, 1408}     # DC +1023: size 10
        assert name.endswith("dri0") or len(raws) > 1
    if name == "all-ones":
        unstuffed = sum(len(r) for r in raws)
        assert c.stuffed >= unstuffed / 2, (c.stuffed, unstuffed)
        at = {i % SLOT_BYTES for raw in raws for i in range(len(raw)) if raw[i] == 0xFF}
        assert SLOT_BYTES - 1 in at and 0 in at, "an FF as the last byte of a slot and as the first of the next"
        assert max(slots_of(raws, step, len(lengths))) > 1.5 * SLOT_BYTES
    if name.startswith("zrl"):
        ops = [mjpeg_enc.block_ops(b, 0) for b in coef]
        zrls = {sum(o == ("zrl",) for o in op) for op in ops}
        assert {0, 1, 2, 3} <= zrls and c.zrl >= 14
        runs = {(sum(o == ("zrl",) for o in op[:i]), o[1]) for op in ops for i, o in enumerate(op) if o[0] == "ac"}
        assert name != "zrl-L" or {(0, 15), (1, 0), (1, 1), (1, 15), (2, 0), (2, 1), (2, 15), (3, 0), (3, 14)} <= runs
        assert any(op[-1][0] == "ac" and op[-2][0] == "ac" and op[-1][1] == 0 for op in ops), "k = 63 after k = 62, no EOB"
        assert any(len(op) == 2 and op[1] == ("eob",) for op in ops), "a lone DC"
    if name.startswith("mod8"):
        assert len(raws) == 1 and lengths.sum() % 8 == int(name[-1])
        assert (c.segments_whole_bytes, c.segments_padded) == ((1, 0) if name[-1] == "0" else (0, 1))
        fill = -int(lengths.sum()) % 8
        assert raws[0][-1] & ((1 << fill) - 1) == (1 << fill) - 1
    if name == "zeros-300":
        assert (lengths == 6).all() and len(lengths) == 300 and len(raws) == 1 and c.stuffed == 0
    if name == "rst-wrap":
        assert len(raws) == 11
        assert [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0] == \
            [0xD0 + i % 8 for i in range(10)], "RST0 ... RST7, RST0, RST1"
    if name.startswith("one-segment"):
        assert dri >= nmcu and len(raws) == 1 and scan == entropy(coef, W, H, layout, 0)[0]
        assert all(scan[i + 1] == 0 for i in range(len(scan) - 1) if scan[i] == 0xFF), "no marker in the scan"


def coef_stream(entry):
    """A set of `coef_sets` -> (header, scan, jpeg): the header the hand writer tests/mjpeg_enc.py puts before these blocks
    (every divisor 1, the standard tables, DRI as given), the restatement's scan, and header + scan + EOI."""
    layout, W, H, coef, dri = entry
    sampling = {0: "L", 2: "4:2:0"}[layout]
    hand = mjpeg_enc.write(sampling, W, H, list(coef.astype(np.int64)), 1 + np.zeros((1 if layout == 0 else 3, 64), np.int64), dri=dri).jpeg
    header = hand[:video.parse_jpeg(hand).scan[0]]
    scan = entropy(coef, W, H, layout, dri)[0]
    return header, scan, header + scan + b"\xff\xd9", hand


def in_reader_domain(entry):
    """Whether the reader (csrc/mjpeg.hip) decodes these coefficients at divisor 1, or refuses them as outside 8-bit samples."""
    layout, W, H, coef, dri = entry
    ext = mjpeg_ref.extents(coef[None], np.ones((1, 3, 64), np.uint16), W, H, layout)
    return not bool(mjpeg_ref.flagged(ext)[0])
