"""An animated GIF89a of a clip, written on the GPU (csrc/gif.hip; no reference counterpart).

`encode_gif` takes uint8 RGB frames in any of `vdx.frames`' forms and returns the file's bytes: one global colour table for the
whole clip (a histogram over 5-5-5 bins on the device, `median_cut` of it on the host), an ordered 8x8 dither, LZW over
independent strips of rows and the data sub-blocks on the device; the host writes only the headers, after one copy of the
per-frame lengths and one of the packed bytes.  Integers only: the bytes are pinned to the numpy restatement tests/gif_ref.py
and decode in Pillow to `palette[index]`.

Not built: frame differencing and transparency, per-frame local palettes, Floyd-Steinberg dithering, reading GIFs, and byte
equality with Pillow's own writer (it crops frames to changed boxes and cuts its palette per image in 24 bits).
"""
from __future__ import annotations

import contextlib
import math
import os
import struct
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import frames as _frames
from . import ops
from ._lib import VdxError

BINS = 32768
MAX_COLORS = 256
STRIP_PIXELS = 8192                   # the default strip: the fewest rows that hold this many pixels


def delay_cs(fps: float) -> int:
    """The frame delay in centiseconds GIF can say for `fps`: floor(100 / fps + 0.5); 8 fps is 13 cs (GIF has no 12.5).  `VdxError`
    for an fps that is not a positive finite number, and for a delay below 2 cs, which players replace by 10 cs."""
    try:
        f = float(fps)
    except (TypeError, ValueError):
        raise VdxError(f"gif: fps={fps!r} is not a number") from None
    if not math.isfinite(f) or f <= 0:
        raise VdxError(f"gif: fps={fps!r} must be positive and finite")
    d = int(math.floor(100.0 / f + 0.5))
    if d < 2:
        raise VdxError(f"gif: fps={fps!r} gives a delay of {d} cs; players replace a delay below 2 cs by 10 cs")
    if d > 65535:
        raise VdxError(f"gif: fps={fps!r} gives a delay of {d} cs, above the 65535 a GIF holds")
    return d


def default_strip_rows(W: int) -> int:
    return max(1, -(-STRIP_PIXELS // W))


def _weighted_counts(v: np.ndarray, w: np.ndarray) -> np.ndarray:
    """int64 [32]: the sum of the counts `w` at every coordinate `v`.  np.bincount sums in float64, which is exact here: the counts
    are uint32 values and a clip has fewer than 2^32 pixels, so every partial sum is an integer below 2^53."""
    return np.bincount(v, weights=w, minlength=32).astype(np.int64)


def median_cut(hist) -> np.ndarray:
    """The clip's colour table from its 5-5-5 histogram (`hist[r5 << 10 | g5 << 5 | b5]` pixels) -> uint8 (n <= 256, 3).

    The rule, in integers:  start with one box holding all occupied bins.  Repeatedly take the box with the largest pixel count
    among the boxes that hold more than one occupied bin (a tie: the lowest box index) and split it along its longest axis,
    the extent max - min of its occupied bins in bin units (a tie: G before R before B).  With c(v) the box's pixels at
    coordinates <= v on that axis and N its pixels, the cut is the smallest v with 2 c(v) >= N, lowered to max - 1 where it is
    the maximum: bins at <= v stay in the box (it keeps its index), the others become a new box with the next index; both are
    non-empty.  Stop at 256 boxes or when no box can be split.  Entry i is box i's count-weighted mean of its bins' centres
    (v << 3 | 4) per channel, rounded half up: (2 S + N) // (2 N).  A clip with at most 256 occupied bins gets exactly its
    bins' centres."""
    h = np.asarray(hist).reshape(-1).astype(np.int64)
    if h.size != BINS:
        raise VdxError(f"median_cut: a histogram of {h.size} bins ({BINS} expected)")
    h = h & 0xFFFFFFFF                                                      # the device's uint32 counts may arrive as int32
    occ = np.flatnonzero(h)
    if occ.size == 0:
        raise VdxError("median_cut: an empty histogram")
    cnt = h[occ]
    coord = np.stack([occ >> 10, (occ >> 5) & 31, occ & 31], axis=1)       # R, G, B in bin units
    boxes = [np.arange(occ.size)]
    pixels = np.zeros(MAX_COLORS, np.int64)                                 # every box's pixel count, carried along the splits
    pixels[0] = cnt.sum()
    bins = np.zeros(MAX_COLORS, np.int64)                                   # and its occupied bins
    bins[0] = occ.size
    while len(boxes) < MAX_COLORS:
        n = len(boxes)
        best = int(np.argmax(np.where(bins[:n] > 1, pixels[:n], -1)))       # the first maximum: the lowest box index on a tie
        if bins[best] <= 1:
            break
        b = boxes[best]
        c = coord[b]
        ext = c.max(axis=0) - c.min(axis=0)
        axis = next(a for a in (1, 0, 2) if ext[a] == ext.max())          # G, R, B on ties
        v = c[:, axis]
        cum = np.cumsum(_weighted_counts(v, cnt[b]))
        cut = int(np.argmax(2 * cum >= pixels[best]))
        cut = min(cut, int(v.max()) - 1)
        low = v <= cut
        boxes[best] = b[low]
        boxes.append(b[~low])
        pixels[n] = pixels[best] - cum[cut]
        pixels[best] = cum[cut]
        bins[best], bins[n] = boxes[best].size, boxes[n].size
    pal = np.zeros((len(boxes), 3), np.uint8)
    centre = (coord << 3) | 4
    for i, b in enumerate(boxes):
        n = int(cnt[b].sum())
        s = (centre[b] * cnt[b][:, None]).sum(axis=0)
        pal[i] = (2 * s + n) // (2 * n)
    return pal


def _check_loop_dither(who: str, loop, dither) -> None:
    if isinstance(loop, bool) or not isinstance(loop, (int, np.integer)) or not 0 <= loop <= 65535:
        raise VdxError(f"{who}: loop={loop!r} is outside 0..65535")
    if dither not in ops.GIF_DITHERS:
        raise VdxError(f"{who}: dither {dither!r} is not one of {sorted(ops.GIF_DITHERS)}")


def check_job_args(fps, dither, loop) -> None:
    """What a job can refuse about its GIF before it has frames: the delay `fps` gives, the dither, the repeat count."""
    delay_cs(fps)
    _check_loop_dither("out_gif", loop, dither)


def _check_palette(palette) -> np.ndarray:
    p = palette.detach().cpu().numpy() if isinstance(palette, torch.Tensor) else np.asarray(palette)
    if p.dtype != np.uint8:
        raise VdxError(f"encode_gif: palette must be uint8, got {p.dtype}")
    if p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= MAX_COLORS:
        raise VdxError(f"encode_gif: palette of shape {tuple(p.shape)}: (n, 3) with n in 1..{MAX_COLORS} rows expected")
    return np.ascontiguousarray(p)


def file_bytes(W: int, H: int, palette: np.ndarray, blocks, delay: int, loop: int) -> bytes:
    """The GIF89a file around every frame's data sub-blocks: header, logical screen descriptor, the global colour table padded
    with zeros to a power of two (at least 2 entries), the NETSCAPE2.0 loop extension; per frame a graphic control extension
    (disposal 1, the delay) and an image descriptor (the full frame, no local table), the minimum code size 8; the trailer."""
    n = int(palette.shape[0])
    bits = max(1, (n - 1).bit_length())
    table = np.zeros((1 << bits, 3), np.uint8)
    table[:n] = palette
    out = bytearray(b"GIF89a" + struct.pack("<HHBBB", W, H, 0xF0 | (bits - 1), 0, 0) + table.tobytes())
    out += b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    for blk in blocks:
        out += b"\x21\xF9\x04\x04" + struct.pack("<H", delay) + b"\x00\x00"
        out += b"\x2C" + struct.pack("<HHHHB", 0, 0, W, H, 0) + b"\x08"
        out += blk
    out += b"\x3B"
    return bytes(out)


def encode_gif(frames, fps: float, loop: int = 0, dither: str = "bayer", strip_rows: Optional[int] = None, palette=None,
               device=None, _events: Optional[list] = None) -> Tuple[bytes, dict]:
    """uint8 RGB frames (T, H, W, 3), in any of `vdx.frames`' forms -> (the bytes of an animated GIF89a, info).  `loop`: the
    NETSCAPE2.0 repeat count, 0 for ever.  `dither`: "bayer" (ordered 8x8, half a bin) or "none".  `strip_rows`: rows per
    independent LZW strip, by default the fewest that hold 8192 pixels; >= H is one strip per frame.  `palette`: uint8 (n <= 256, 3)
    to use instead of the clip's own (no histogram, no median cut).  info: frames, colors, bytes, delay_cs, fps (the effective
    100 / delay_cs), dither, strip_rows, loop.  Every refusal is a `VdxError` raised before anything is launched."""
    delay = delay_cs(fps)
    T, H, W = _frames.check(frames, "encode_gif")
    if T < 1:
        raise VdxError(f"encode_gif: T={T}: a GIF needs at least one frame")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise VdxError(f"encode_gif: H={H}, W={W} are outside the 1..65535 a GIF's screen descriptor holds")
    if T * H * W >= 1 << 32:
        raise VdxError(f"encode_gif: {T * H * W} pixels do not fit the uint32 histogram (2^32 or more)")
    _check_loop_dither("encode_gif", loop, dither)
    if strip_rows is None:
        strip_rows = default_strip_rows(W)
    if isinstance(strip_rows, bool) or not isinstance(strip_rows, (int, np.integer)) or strip_rows < 1:
        raise VdxError(f"encode_gif: strip_rows={strip_rows!r} must be an integer >= 1")
    strip_rows = min(int(strip_rows), H)
    pal = None if palette is None else _check_palette(palette)
    dev = _frames.device_for(frames, device)
    if dev.type != "cuda":
        raise VdxError("encode_gif: the encoder runs on the GPU (there is no CPU path)")
    ws_bytes = ops.gif_lzw_workspace(T, H, W, strip_rows)

    @contextlib.contextmanager
    def stage(name):
        """with `_events`: HIP events on the stream around the stage's launches, appended as (name, start, end)"""
        if _events is None:
            yield
            return
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        yield
        ev1.record()
        _events.append((name, ev0, ev1))

    with torch.cuda.device(dev):
        clip = _frames.on_device(frames, dev)
        if pal is None:
            with stage("hist"):
                hist = ops.gif_hist(clip)
            pal = median_cut(hist.cpu().numpy())
        with stage("lut"):
            lut = ops.gif_lut(torch.from_numpy(pal).to(dev))
        with stage("index"):
            idx = ops.gif_index(clip, lut, dither)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with stage("lzw"):
            lengths = ops.gif_lzw(idx, strip_rows, ws)
        sizes = lengths.cpu().numpy().astype(np.int64)                      # copy 1: the per-frame lengths
        total = int(sizes.sum())
        if sizes.min() < 3 or total >= 1 << 40:
            raise VdxError("encode_gif: the device returned impossible frame lengths")
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        with stage("pack"):
            ops.gif_pack(ws, T, H, W, strip_rows, out)
        data = out.cpu().numpy().tobytes()                                  # copy 2: the packed bytes
    ends = np.cumsum(sizes)
    blob = file_bytes(W, H, pal, (data[int(e - n):int(e)] for e, n in zip(ends, sizes)), delay, int(loop))
    info = {"frames": T, "colors": int(pal.shape[0]), "bytes": len(blob), "delay_cs": delay, "fps": 100.0 / delay, "dither": dither,
            "strip_rows": strip_rows, "loop": int(loop)}
    return blob, info


def write_gif(path: Union[str, os.PathLike], frames, fps: float, **kw) -> dict:
    """`encode_gif(frames, fps, **kw)` written to `path` -> its info."""
    blob, info = encode_gif(frames, fps, **kw)
    with open(os.fspath(path), "wb") as f:
        f.write(blob)
    return info
