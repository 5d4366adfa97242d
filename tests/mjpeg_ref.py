"""A slow restatement in Python / numpy of the three stages of csrc/mjpeg.hip, fed by the very upload `vdx.video.plan`
builds (entropy bytes, segment table, Huffman lookups, quantisation tables).  It lets the CPU suite pin the host half
of the decoder (marker walk, lookups, segment table) and the integer definition of every stage against Pillow without a
GPU; tests/test_video_host.py runs it on images of a few MCUs."""
import numpy as np

from vdx import video

NATURAL = video._ZIGZAG


def _geometry(W, H, layout):
    hmax = 2 if layout == 2 else 1
    ncomp = 1 if layout == 0 else 3
    mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * hmax))
    hs = [hmax if c == 0 else 1 for c in range(ncomp)]
    bw = [mcux * s for s in hs]
    bh = [mcuy * s for s in hs]
    boff = [0]
    for c in range(ncomp):
        boff.append(boff[-1] + bw[c] * bh[c])
    return ncomp, mcux, mcuy, hs, bw, bh, boff


class _Bits:
    def __init__(self, data, pos, end):
        self.d, self.pos, self.end, self.buf, self.bits, self.pad = data, pos, end, 0, 0, 0

    def refill(self):
        while self.bits <= 56:
            v = 0
            if self.pos < self.end:
                v = int(self.d[self.pos])
                self.pos += 1
                if v == 0xFF:
                    if self.pos < self.end and self.d[self.pos] == 0:
                        self.pos += 1
                    else:
                        self.pos, v = self.end, 0
                        self.pad += 8
            else:
                self.pad += 8
            self.buf |= v << (56 - self.bits)
            self.bits += 8

    def skip(self, n):
        self.buf = (self.buf << n) & ((1 << 64) - 1)
        self.bits -= n

    def symbol(self, t):
        peek = self.buf >> 48
        fi = peek >> 7
        e = (int(t[fi >> 1]) >> ((fi & 1) * 16)) & 0xFFFF
        if e:
            self.skip(e >> 8)
            return e & 255
        for ln in range(10, 17):
            code = peek >> (16 - ln)
            if code <= int(np.int32(t[256 + ln])):
                i = (int(t[273 + ln]) + code) & 255
                self.skip(ln)
                return (int(t[290 + (i >> 2)]) >> ((i & 3) * 8)) & 255
        return -1

    def receive_extend(self, s):
        v = self.buf >> (64 - s)
        self.skip(s)
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy(blob, off, info):
    """-> (int16 coefficients [F][blocks per frame][64], error words [nseg]) as vdx_mjpeg_entropy leaves them."""
    F, W, H, layout = info["n_frames"], info["width"], info["height"], video.LAYOUTS[info["sampling"]]
    ncomp, mcux, mcuy, hs, bw, bh, boff = _geometry(W, H, layout)
    part = lambda name, dt, n: blob[off[name][0]:off[name][0] + n * np.dtype(dt).itemsize].view(dt)   # noqa: E731
    nseg = info["n_segments"]
    data = blob[:off["data"][1]]
    seg_off, segs = part("seg_off", np.int32, F + 1), part("segs", np.int32, nseg * 4).reshape(nseg, 4)
    huff, sel = part("huff", np.uint32, F * 4 * 384).reshape(F, 4, 384), part("sel", np.int32, F * 3).reshape(F, 3)
    coef = np.zeros((F, boff[-1], 64), np.int16)
    err = np.zeros(nseg, np.uint32)
    for f in range(F):
        for s in range(seg_off[f], seg_off[f + 1]):
            b = _Bits(data, int(segs[s, 0]), int(segs[s, 1]))
            pred = [0, 0, 0]
            code = 0
            for m in range(int(segs[s, 2]), int(segs[s, 2] + segs[s, 3])):
                my, mx = divmod(m, mcux)
                for c in range(ncomp):
                    dct, act = huff[f, sel[f, c] & 1], huff[f, 2 + ((sel[f, c] >> 4) & 1)]
                    for by in range(hs[c]):
                        for bx in range(hs[c]):
                            blk = coef[f, boff[c] + (my * hs[c] + by) * bw[c] + mx * hs[c] + bx]
                            if b.bits < 32:
                                b.refill()
                            sym = b.symbol(dct)
                            if sym < 0:
                                code = 3
                            elif sym > 15:
                                code = 4
                            else:
                                if sym:
                                    pred[c] += b.receive_extend(sym)
                                if b.pad > b.bits:
                                    code = 1
                            k = 1
                            if code == 0:
                                blk[0] = np.int16(((pred[c] + 32768) & 65535) - 32768)
                            while code == 0 and k < 64:
                                if b.bits < 32:
                                    b.refill()
                                sym = b.symbol(act)
                                if sym < 0:
                                    code = 3
                                    break
                                r, sz = sym >> 4, sym & 15
                                if sz == 0:
                                    if b.pad > b.bits:
                                        code = 1
                                        break
                                    if r != 15:
                                        break
                                    k += 16
                                    continue
                                k += r
                                val = b.receive_extend(sz)
                                if b.pad > b.bits:
                                    code = 1
                                    break
                                if k > 63:
                                    code = 2
                                    break
                                blk[NATURAL[k]] = val
                                k += 1
                            if code:
                                break
                        if code:
                            break
                    if code:
                        break
                if code:
                    err[s] = code | ((m - int(segs[s, 2])) << 8)
                    break
    return coef, err


def _idct8(x, shift):
    """The 1-D slow-integer inverse DCT along the last axis, in the integer type of x (int64: nothing wraps; int32: wraps)."""
    i = [x[..., k] for k in range(8)]
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    rnd = 1 << (shift - 1)
    o = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(v + rnd) >> shift for v in o], -1)


# The domain of "bit-equal to Pillow": csrc/mjpeg.hip MJ_DOMAIN_PRODUCT / MJ_DOMAIN_PASS1 and the range of the decoder's
# range-limit table.  A frame with a value outside is flagged by the kernel and refused by read_frames.
DOMAIN_PRODUCT = 32767
DOMAIN_PASS1 = 32767
DOMAIN_SAMPLE = (-512, 511)


def _stages(coef, quant, c, boff, int32):
    """Component c of every frame -> (dequantised products, pass-1 values, samples before the range limit), each
    [F][blocks][8][8].  int32=True computes in numpy int32, which wraps exactly as the kernel's -fwrapv int32 does, so the two
    are comparable on ANY int16 x uint16 input; int64 never wraps on such input."""
    dt = np.int32 if int32 else np.int64
    x = coef[:, boff[c]:boff[c + 1]].astype(dt) * quant[:, c].astype(dt)[:, None, :]
    prod = x.reshape(x.shape[0], -1, 8, 8)
    p1 = np.swapaxes(_idct8(np.swapaxes(prod, -1, -2), 11), -1, -2)          # pass 1: columns
    pre = _idct8(p1, 18)                                                     # pass 2: rows
    assert prod.dtype == p1.dtype == pre.dtype == dt
    return prod, p1, pre


def idct(coef, quant, W, H, layout, int32=False):
    """coefficients [F][bpf][64], quant [F][3][64] -> list over components of uint8 planes [F][bh*8][bw*8]."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = _geometry(W, H, layout)
    planes = []
    for c in range(ncomp):
        x = _stages(coef, quant, c, boff, int32)[2]
        x = ((x & 1023) ^ 512) - 512
        x = np.clip(x + 128, 0, 255).astype(np.uint8)
        F = x.shape[0]
        planes.append(x.reshape(F, bh[c], bw[c], 8, 8).transpose(0, 1, 3, 2, 4).reshape(F, bh[c] * 8, bw[c] * 8))
    return planes


def extents(coef, quant, W, H, layout, int32=False):
    """-> int64 [F][3][2]: per frame the (min, max) of the dequantised products, of the pass-1 values and of the samples
    before the range limit, over all components."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = _geometry(W, H, layout)
    F = coef.shape[0]
    out = np.zeros((F, 3, 2), np.int64)
    for c in range(ncomp):
        for i, v in enumerate(_stages(coef, quant, c, boff, int32)):
            v = v.reshape(F, -1).astype(np.int64)
            lo, hi = v.min(1), v.max(1)
            out[:, i, 0] = lo if c == 0 else np.minimum(out[:, i, 0], lo)
            out[:, i, 1] = hi if c == 0 else np.maximum(out[:, i, 1], hi)
    return out


def flagged(ext, product=None, pass1=None):
    """extents -> bool [F]: outside the domain, the word vdx_mjpeg_idct leaves per frame."""
    product = DOMAIN_PRODUCT if product is None else product
    pass1 = DOMAIN_PASS1 if pass1 is None else pass1
    return ((ext[:, 0, 0] < -product - 1) | (ext[:, 0, 1] > product) | (ext[:, 1, 0] < -pass1 - 1) | (ext[:, 1, 1] > pass1) |
            (ext[:, 2, 0] < DOMAIN_SAMPLE[0]) | (ext[:, 2, 1] > DOMAIN_SAMPLE[1]))


def _fancy_h2v2(p, W, H):
    CW, CH = (W + 1) // 2, (H + 1) // 2
    p = p[:, :CH, :CW].astype(np.int64)
    up, down = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    rows = np.empty((p.shape[0], 2 * CH, CW), np.int64)
    rows[:, 0::2], rows[:, 1::2] = 3 * p + up, 3 * p + down
    last, nxt = np.concatenate([rows[..., :1], rows[..., :-1]], -1), np.concatenate([rows[..., 1:], rows[..., -1:]], -1)
    out = np.empty((p.shape[0], 2 * CH, 2 * CW), np.int64)
    out[..., 0::2], out[..., 1::2] = (3 * rows + last + 8) >> 4, (3 * rows + nxt + 7) >> 4
    return out[:, :H, :W]


def color(planes, W, H, layout):
    y = planes[0][:, :H, :W].astype(np.int64)
    if layout == 0:
        return y.astype(np.uint8)
    if layout == 2:
        cb, cr = _fancy_h2v2(planes[1], W, H), _fancy_h2v2(planes[2], W, H)
    else:
        cb, cr = planes[1][:, :H, :W].astype(np.int64), planes[2][:, :H, :W].astype(np.int64)
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(jpegs, with_extents=False):
    """List of JPEG byte strings -> (uint8 frames, error words[, extents]): the whole decoder on the CPU."""
    blob, off, info, _ = video.plan(jpegs)
    F, W, H, layout = info["n_frames"], info["width"], info["height"], video.LAYOUTS[info["sampling"]]
    coef, err = entropy(blob, off, info)
    quant = blob[off["quant"][0]:off["quant"][0] + F * 3 * 64 * 2].view(np.uint16).reshape(F, 3, 64)
    frames = color(idct(coef, quant, W, H, layout), W, H, layout)
    return (frames, err, extents(coef, quant, W, H, layout)) if with_extents else (frames, err)
