"""A slow restatement in Python / numpy of the animated-GIF writer (vdx/gif.py, csrc/gif.hip): the histogram, a second median cut
written independently of `vdx.gif.median_cut`, the LUT, the dither and index map, the strip LZW, the sub-block framing, the
whole file, and an LZW decoder of its own.  Nothing here imports the package: tests/test_gif_host.py holds it against Pillow,
tests/test_gif_gpu.py holds the kernels against it bit for bit."""
import struct

import numpy as np

BINS = 32768
CLEAR, EOI, FIRST, CODES = 256, 257, 258, 4096


# ---- stage 1: histogram ------------------------------------------------------------------------------------------------------
def bins_of(rgb):
    """uint8 (..., 3) -> the 5-5-5 bin of every pixel"""
    v = np.asarray(rgb).astype(np.int64) >> 3
    return (v[..., 0] << 10) | (v[..., 1] << 5) | v[..., 2]


def hist(frames):
    return np.bincount(bins_of(frames).reshape(-1), minlength=BINS).astype(np.int64)


# ---- stage 2: the second median cut ------------------------------------------------------------------------------------------
def median_cut(h):
    """The rule of `vdx.gif.median_cut`'s docstring, restated with plain Python lists of (r, g, b, count)."""
    h = [int(v) for v in np.asarray(h).reshape(-1)]
    assert len(h) == BINS
    boxes = [[(i >> 10, (i >> 5) & 31, i & 31, n) for i, n in enumerate(h) if n]]
    assert boxes[0]
    while len(boxes) < 256:
        pick = None
        for i, box in enumerate(boxes):
            if len(box) > 1:
                n = sum(e[3] for e in box)
                if pick is None or n > pick[1]:
                    pick = (i, n)
        if pick is None:
            break
        i, total = pick
        box = boxes[i]
        extent = [max(e[a] for e in box) - min(e[a] for e in box) for a in range(3)]
        axis = 1                                                            # G, then R, then B
        if extent[0] > extent[axis]:
            axis = 0
        if extent[2] > extent[axis]:
            axis = 2
        top = max(e[axis] for e in box)
        below, cut = 0, None
        for v in range(32):
            below += sum(e[3] for e in box if e[axis] == v)
            if 2 * below >= total:
                cut = v
                break
        if cut >= top:
            cut = top - 1
        boxes[i] = [e for e in box if e[axis] <= cut]
        boxes.append([e for e in box if e[axis] > cut])
        assert boxes[i] and boxes[-1]
    pal = []
    for box in boxes:
        n = sum(e[3] for e in box)
        pal.append([(2 * sum(((e[a] << 3) | 4) * e[3] for e in box) + n) // (2 * n) for a in range(3)])
    return np.array(pal, np.uint8)


# ---- stage 3: LUT ------------------------------------------------------------------------------------------------------------
def lut(palette):
    """uint8 [32768]: the nearest entry to every bin centre, the lowest index on a tie (np.argmin returns the first minimum)"""
    b = np.arange(BINS)
    centre = np.stack([((b >> 10) << 3) | 4, (((b >> 5) & 31) << 3) | 4, ((b & 31) << 3) | 4], axis=1).astype(np.int64)
    d = ((centre[:, None, :] - np.asarray(palette).astype(np.int64)[None, :, :]) ** 2).sum(axis=2)
    return np.argmin(d, axis=1).astype(np.uint8)


# ---- stage 4: dither and index map ---------------------------------------------------------------------------------------------
def bayer8():
    """The standard 8x8 Bayer matrix 0..63 by the recursion M(2n) = [[4M, 4M + 2], [4M + 3, 4M + 1]]"""
    m = np.zeros((1, 1), np.int64)
    for _ in range(3):
        m = np.block([[4 * m, 4 * m + 2], [4 * m + 3, 4 * m + 1]])
    return m


def dither_offsets(H, W):
    d = ((bayer8() * 8 + 4) >> 6) - 4
    assert d.min() == -4 and d.max() == 3
    return d[np.arange(H)[:, None] & 7, np.arange(W)[None, :] & 7]


def index_map(frames, table, dither="bayer"):
    """uint8 (T, H, W, 3) -> uint8 (T, H, W) through `table` = lut(palette)"""
    f = np.asarray(frames).astype(np.int64)
    if dither == "bayer":
        f = np.clip(f + dither_offsets(f.shape[1], f.shape[2])[None, :, :, None], 0, 255)
    else:
        assert dither == "none"
    return np.asarray(table)[bins_of(f)]


# ---- stage 5: LZW over strips --------------------------------------------------------------------------------------------------
def strip_codes(pixels, first, last):
    """One strip's (code, width) list: [CLEAR if first] codes ... then EOI if last else CLEAR, from an empty table at width 9."""
    out = []
    width, nxt, table = 9, FIRST, {}
    if first:
        out.append((CLEAR, width))
    px = [int(v) for v in pixels]
    p = px[0]
    for c in px[1:]:
        k = (p << 8) | c
        q = table.get(k)
        if q is not None:
            p = q
            continue
        out.append((p, width))
        if nxt < CODES:
            table[k] = nxt
            nxt += 1
            if nxt > (1 << width) and width < 12:
                width += 1
        else:
            out.append((CLEAR, width))
            table, nxt, width = {}, FIRST, 9
        p = c
    out.append((p, width))
    if nxt < CODES:                                                         # the decoder adds an entry after this code too
        nxt += 1
        if nxt > (1 << width) and width < 12:
            width += 1
    out.append((EOI if last else CLEAR, width))
    return out


def closing_width(pixels):
    """The width a strip's closing code is written at"""
    return strip_codes(pixels, True, True)[-1][1]


def pack_bits(codes):
    """(code, width) pairs LSB first -> (bytes, bits)"""
    acc = n = total = 0
    b = bytearray()
    for c, w in codes:
        acc |= c << n
        n += w
        total += w
        while n >= 8:
            b.append(acc & 255)
            acc >>= 8
            n -= 8
    if n:
        b.append(acc & 255)
    return bytes(b), total


def strips_of(H, strip_rows):
    rows = min(strip_rows, H)
    return [(r, min(r + rows, H)) for r in range(0, H, rows)]


def frame_stream(idx, strip_rows):
    """One frame's uint8 (H, W) indices -> (the stream's bytes, [bits of every strip], [(bytes, bits) of every strip alone])"""
    spans = strips_of(idx.shape[0], strip_rows)
    codes, bits, alone = [], [], []
    for i, (a, b) in enumerate(spans):
        c = strip_codes(idx[a:b].reshape(-1), i == 0, i == len(spans) - 1)
        codes += c
        alone.append(pack_bits(c))
        bits.append(alone[-1][1])
    return pack_bits(codes)[0], bits, alone


def slot_words(strip_rows, H, W):
    """The slot bound of include/vdx.h: at most n data codes, one CLEAR per 3838 of them, the opening and the closing code."""
    n = min(strip_rows, H) * W
    return (12 * (n + n // 3838 + 3) + 31) // 32


# ---- stage 6: sub-blocks and the file --------------------------------------------------------------------------------------------
def sub_blocks(data):
    out = bytearray()
    for i in range(0, len(data), 255):
        out.append(len(data[i:i + 255]))
        out += data[i:i + 255]
    out.append(0)
    assert len(out) == len(data) + -(-len(data) // 255) + 1
    return bytes(out)


def delay_cs(fps):
    return int(np.floor(100.0 / fps + 0.5))


def gif_file(idx, palette, strip_rows, delay, loop=0):
    """uint8 (T, H, W) indices and a uint8 (n, 3) palette -> the bytes of the GIF89a file"""
    T, H, W = idx.shape
    n = len(palette)
    size = 2
    while size < n:
        size *= 2
    table = np.zeros((size, 3), np.uint8)
    table[:n] = palette
    o = bytearray(b"GIF89a" + struct.pack("<HHBBB", W, H, 0x80 | 0x70 | (size.bit_length() - 2), 0, 0) + table.tobytes())
    o += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    for t in range(T):
        o += b"\x21\xF9\x04" + bytes([1 << 2]) + struct.pack("<H", delay) + b"\x00\x00"
        o += b"\x2C" + struct.pack("<HHHHB", 0, 0, W, H, 0) + b"\x08"
        o += sub_blocks(frame_stream(idx[t], strip_rows)[0])
    o.append(0x3B)
    return bytes(o)


def encode(frames, fps, loop=0, dither="bayer", strip_rows=None, palette=None):
    """The whole of `vdx.gif.encode_gif` -> (bytes, palette, indices)"""
    frames = np.asarray(frames)
    W = frames.shape[2]
    if strip_rows is None:
        strip_rows = max(1, -(-8192 // W))
    pal = median_cut(hist(frames)) if palette is None else np.asarray(palette)
    idx = index_map(frames, lut(pal), dither)
    return gif_file(idx, pal, strip_rows, delay_cs(fps), loop), pal, idx


# ---- a decoder of its own ----------------------------------------------------------------------------------------------------
def lzw_decode(data, npixels):
    """GIF LZW, minimum code size 8, as a decoder reads it: variable width from 9, CLEAR resets, the table stops at 4096."""
    out = []
    table = None
    acc = n = pos = 0
    width, prev = 9, None
    while True:
        while n < width:
            assert pos < len(data), "the stream ended before EOI"
            acc |= data[pos] << n
            pos += 1
            n += 8
        code = acc & ((1 << width) - 1)
        acc >>= width
        n -= width
        if code == CLEAR:
            table = [bytes([i]) for i in range(256)] + [b"", b""]
            width, prev = 9, None
            continue
        if code == EOI:
            break
        assert table is not None, "data before the first CLEAR"
        if prev is None:
            entry = table[code]
        else:
            assert code <= len(table), "a code beyond the next free one"
            entry = table[code] if code < len(table) else prev + prev[:1]
            if len(table) < CODES:
                table.append(prev + entry[:1])
        out.append(entry)
        prev = entry
        if len(table) == (1 << width) and width < 12:
            width += 1
    got = b"".join(out)
    assert len(got) == npixels, (len(got), npixels)
    assert pos == len(data), "bytes after EOI"
    return np.frombuffer(got, np.uint8)


def decode_file(blob):
    """-> dict(W, H, palette (real + padding), loop, delays [cs], frames uint8 (T, H, W) of indices) of a file `gif_file` wrote"""
    assert blob[:6] == b"GIF89a"
    W, H, flags, _bg, _aspect = struct.unpack("<HHBBB", blob[6:13])
    assert flags & 0x80
    size = 2 << (flags & 7)
    palette = np.frombuffer(blob[13:13 + 3 * size], np.uint8).reshape(size, 3)
    pos = 13 + 3 * size
    assert blob[pos:pos + 16] == b"\x21\xFF\x0BNETSCAPE2.0\x03\x01"
    loop = struct.unpack("<H", blob[pos + 16:pos + 18])[0]
    assert blob[pos + 18] == 0
    pos += 19
    frames, delays = [], []
    while blob[pos] != 0x3B:
        assert blob[pos:pos + 4] == b"\x21\xF9\x04\x04"
        delays.append(struct.unpack("<H", blob[pos + 4:pos + 6])[0])
        pos += 8
        assert blob[pos] == 0x2C and struct.unpack("<HHHHB", blob[pos + 1:pos + 10]) == (0, 0, W, H, 0) and blob[pos + 10] == 8
        pos += 11
        data = bytearray()
        while blob[pos]:
            data += blob[pos + 1:pos + 1 + blob[pos]]
            pos += 1 + blob[pos]
        pos += 1
        frames.append(lzw_decode(bytes(data), W * H).reshape(H, W))
    assert pos == len(blob) - 1
    return {"W": W, "H": H, "palette": palette, "loop": loop, "delays": delays, "frames": np.stack(frames)}


# ---- the figures profiles/gif_parity.txt records (tools/gif_parity.py) -----------------------------------------------------------
def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def gradient_clip(T=3, H=96, W=128):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([(x * 255 // (W - 1) + 4 * t) % 256, y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], axis=-1)
                     for t in range(T)]).astype(np.uint8)


def uniform_676():
    r, g, b = np.meshgrid(np.linspace(0, 255, 6), np.linspace(0, 255, 7), np.linspace(0, 255, 6), indexing="ij")
    return np.stack([r, g, b], axis=-1).reshape(-1, 3).round().astype(np.uint8)


def parity_figures(cut):
    """`cut`: the median cut under test.  -> (its PSNR on a gradient clip through the nearest mapping, a uniform 6x7x6 palette's,
    the line that records both beside Pillow's own per-frame median cut)"""
    from PIL import Image
    f = gradient_clip()
    pal = cut(hist(f))
    ours = psnr(pal[index_map(f, lut(pal), "none")], f)
    uni = uniform_676()
    uniform = psnr(uni[index_map(f, lut(uni), "none")], f)
    pil = np.stack([np.asarray(Image.fromarray(x).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB"))
                    for x in f])
    line = (f"gradient clip 3x96x128, nearest mapping without dither: PSNR median_cut(256, one cut per clip, 15 bits) {ours:.2f} dB, "
            f"uniform 6x7x6 {uniform:.2f} dB, Pillow quantize(256, MEDIANCUT, dither=NONE, one cut per frame, 24 bits) {psnr(pil, f):.2f} dB")
    return ours, uniform, [line]


def strip_cost_figures(cut):
    """File size at the default strips against one strip per frame at 576 x 1024, from the restatement: the cost of independent
    strips.  Recorded, not asserted (seconds of pure Python per frame)."""
    H, W = 576, 1024
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    smooth = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x + y) * 255 // (H + W - 2)], axis=-1).astype(np.uint8)[None]
    noisy = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    lines = []
    for name, f, dither in (("smooth", smooth, "none"), ("noisy", noisy, "none"), ("dithered", smooth, "bayer")):
        pal = cut(hist(f))
        idx = index_map(f, lut(pal), dither)
        a = len(gif_file(idx, pal, 8, 13))
        b = len(gif_file(idx, pal, H, 13))
        lines.append(f"{name} 576x1024, dither {dither}: {a} bytes at strip_rows=8, {b} bytes at one strip per frame, ratio {a / b:.4f}")
    return lines
