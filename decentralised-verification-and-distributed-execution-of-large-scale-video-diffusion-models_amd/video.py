"""Read the job's video file back into frames on the GPU: the read side of `cv2.VideoCapture(video_path)`, with which every
validator entry point of the reference starts (InferNet/template/validator/scoring.py:16, :110, :230, :272, :314).

    read_frames(src, device="cuda") -> (uint8 frames (F, H, W, 3) RGB or (F, H, W) grey on the device, info)

`src` is a path, the file's bytes, or a list of JPEG byte strings.  The container is the one `vdx/compat/cv2_shim.py`
(:199-289) writes: ISO base media, `ftyp`, `mdat`, `moov`, one video track whose `stsd` holds an `mp4v` entry with an `esds`
of object type 0x6C (JPEG), `stsz` / `stco` / `stsc` / `stts`; a bare JPEG is a clip of one frame.  Anything else (`avc1`, real
MPEG-4 part 2: the reference miner's own files) raises `VdxError`: this is a Motion-JPEG reader and no more.

The host walks the JPEG markers (numpy, no per-byte Python loop over entropy data), builds the Huffman lookups from the
stream's own DHT segments, reads DQT / SOF0 / DRI / SOS, finds the restart markers and cuts the scan into segments; the device
(csrc/mjpeg.hip) decodes the Huffman codes one lane per segment, runs the slow-integer IDCT and the fancy chroma upsampling +
YCbCr -> RGB.  Baseline sequential 8-bit JPEG with one interleaved scan: 4:2:0, 4:4:4 or grey; every other kind is refused by
name on the host.

The result is pinned bit for bit to Pillow's (libjpeg-turbo's) decode of the same bytes (tests/test_video_gpu.py) for every
frame whose coefficients lie in the range that 8-bit samples produce: every dequantised product and every value after the
IDCT's first pass within int16, every sample before the range limit within [-512, 511] (csrc/mjpeg.hip MJ_DOMAIN_*;
profiles/mjpeg_domain.txt).  Outside that range libjpeg's C code wraps the sample to 10 bits, libjpeg-turbo saturates and
wraps in 16-bit lanes, and other decoders do something else again: one stream, several images.  No encoder that started from
pixels writes such a frame, a peer who chooses the bytes can, so the IDCT stage flags it and `read_frames` refuses it by
name instead of returning one of the possible images.

One upload (entropy bytes and all tables in one buffer) and one synchronisation (the per-segment error words and the
per-frame domain words, one buffer) per call.

The write side is the second half of the module: `encode_frames` / `write_frames` turn uint8 frames on the GPU into the bytes
`cv2_shim.VideoWriter` writes for them (csrc/mjpeg_enc.hip), pinned byte for byte to Pillow's encoder
(tests/test_video_enc_host.py, tests/test_video_enc_gpu.py); the host builds the header and the container only.
"""
from __future__ import annotations

import os
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import VdxError

HUFF_WORDS = 384                     # csrc/mjpeg.hip MJ_HUFF_WORDS and the offsets inside a table
_FAST_BITS, _MAXCODE, _VALOFF, _SYMS = 9, 256, 273, 290
LAYOUTS = {"L": 0, "4:4:4": 1, "4:2:0": 2}
ERRORS = {1: "the entropy data ends inside a symbol", 2: "a coefficient index runs past 63", 3: "no Huffman code matches",
          4: "a DC size above 15", 5: "a segment outside the clip"}

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])            # natural index of the k-th coefficient in zigzag (file) order

_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic-coded progressive (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)",
              0xCD: "arithmetic-coded differential (SOF13)", 0xCE: "arithmetic-coded differential progressive (SOF14)",
              0xCF: "arithmetic-coded differential lossless (SOF15)"}


class JpegInfo(NamedTuple):
    """What the host learns from one JPEG.  `quant`: {table id: 64 values in natural (row-major) order}; `segments`: int64
    [n][4] = byte begin, byte end (offsets into the JPEG), first MCU, MCU count; `scan` = (first entropy byte, offset of the
    marker that ends the scan)."""
    width: int
    height: int
    sampling: str
    restart_interval: int
    quant: Dict[int, List[int]]
    comp_quant: Tuple[int, ...]
    comp_tables: Tuple[Tuple[int, int], ...]
    huffman: Dict[Tuple[int, int], bytes]
    segments: np.ndarray
    scan: Tuple[int, int]


def _huffman_lookup(payload: bytes) -> np.ndarray:
    """16 counts + symbols of one DHT table -> the 384 words csrc/mjpeg.hip stages in LDS (include/vdx.h vdx_mjpeg_entropy)."""
    counts = np.frombuffer(payload[:16], np.uint8).astype(np.int64)
    syms = np.frombuffer(payload[16:], np.uint8)
    fast = np.zeros(1 << _FAST_BITS, np.uint16)
    maxcode = np.full(17, -1, np.int32)
    valoff = np.zeros(17, np.int32)
    code = k = 0
    for ln in range(1, 17):
        n = int(counts[ln - 1])
        if code + n > (1 << ln):
            raise VdxError(f"JPEG: a DHT table assigns more codes of {ln} bits than exist")
        if n:
            valoff[ln] = k - code
            maxcode[ln] = code + n - 1
            if ln <= _FAST_BITS:
                span = 1 << (_FAST_BITS - ln)
                entry = (ln << 8) | syms[k:k + n].astype(np.uint16)
                fast[code * span:(code + n) * span] = np.repeat(entry, span)
        code = (code + n) << 1
        k += n
    words = np.zeros(HUFF_WORDS, np.uint32)
    words[:_MAXCODE] = fast.astype("<u2").view("<u4")                 # entry 2i in the low half of word i
    words[_MAXCODE:_MAXCODE + 17] = maxcode.view(np.uint32)
    words[_VALOFF:_VALOFF + 17] = valoff.view(np.uint32)
    padded = np.zeros(256, np.uint8)
    padded[:len(syms)] = syms
    words[_SYMS:_SYMS + 64] = padded.view("<u4")
    return words


_LOOKUPS: Dict[bytes, np.ndarray] = {}


def _lookup(payload: bytes) -> np.ndarray:
    t = _LOOKUPS.get(payload)
    if t is None:
        if len(_LOOKUPS) > 256:
            _LOOKUPS.clear()
        t = _LOOKUPS[payload] = _huffman_lookup(payload)
    return t


def parse_jpeg(jpeg: bytes) -> JpegInfo:
    """Walk the markers of one baseline JPEG; refuse by name whatever the decoder does not take."""
    n = len(jpeg)
    if n < 4 or jpeg[:2] != b"\xff\xd8":
        raise VdxError("JPEG: no SOI marker at the start")
    pos = 2
    quant: Dict[int, List[int]] = {}
    huffman: Dict[Tuple[int, int], bytes] = {}
    frame = None
    dri = 0
    while True:
        if pos + 4 > n:
            raise VdxError("JPEG: truncated before the scan (no SOS)")
        if jpeg[pos] != 0xFF:
            raise VdxError(f"JPEG: expected a marker at byte {pos}")
        m = jpeg[pos + 1]
        if m == 0xFF:                                   # fill byte
            pos += 1
            continue
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            pos += 2
            continue
        if m == 0xD9:
            raise VdxError("JPEG: EOI before any scan")
        ln = struct.unpack_from(">H", jpeg, pos + 2)[0]
        body, end = pos + 4, pos + 2 + ln
        if ln < 2 or end > n:
            raise VdxError(f"JPEG: segment FF{m:02X} at byte {pos} runs past the end of the data")
        if m == 0xDB:                                   # DQT
            p = body
            while p < end:
                pq, tq = jpeg[p] >> 4, jpeg[p] & 15
                if pq != 0:
                    raise VdxError("JPEG: 16-bit quantisation tables (12-bit JPEG) are not supported, 8-bit baseline only")
                if tq > 3 or p + 65 > end:
                    raise VdxError("JPEG: malformed DQT segment")
                nat = np.zeros(64, np.int64)
                nat[_ZIGZAG] = np.frombuffer(jpeg[p + 1:p + 65], np.uint8)
                quant[tq] = nat.tolist()
                p += 65
        elif m == 0xC4:                                 # DHT
            p = body
            while p < end:
                if p + 17 > end:
                    raise VdxError("JPEG: malformed DHT segment")
                tc, th = jpeg[p] >> 4, jpeg[p] & 15
                cnt = sum(jpeg[p + 1:p + 17])
                if tc > 1 or th > 1 or cnt > 256 or p + 17 + cnt > end:
                    raise VdxError(f"JPEG: DHT table class {tc} id {th} with {cnt} symbols: baseline takes class 0/1, id 0/1")
                huffman[(tc, th)] = bytes(jpeg[p + 1:p + 17 + cnt])
                p += 17 + cnt
        elif m == 0xC0:                                 # SOF0
            if frame is not None:
                raise VdxError("JPEG: more than one frame header")
            if ln < 8:
                raise VdxError("JPEG: malformed SOF0 segment")
            prec, h, w, nc = struct.unpack_from(">BHHB", jpeg, body)
            if prec != 8:
                raise VdxError(f"JPEG: {prec}-bit samples, 8-bit baseline only")
            if w == 0 or h == 0 or ln != 8 + 3 * nc:
                raise VdxError("JPEG: malformed SOF0 segment")
            comps = [(jpeg[body + 6 + 3 * i], jpeg[body + 7 + 3 * i] >> 4, jpeg[body + 7 + 3 * i] & 15, jpeg[body + 8 + 3 * i])
                     for i in range(nc)]
            frame = (w, h, comps)
        elif m in _SOF_NAMES:
            raise VdxError(f"JPEG: {_SOF_NAMES[m]} is not supported, baseline sequential (SOF0) only")
        elif m == 0xCC:
            raise VdxError("JPEG: arithmetic coding (DAC) is not supported, baseline Huffman only")
        elif m == 0xDD:                                 # DRI
            if ln != 4:
                raise VdxError("JPEG: malformed DRI segment")
            dri = struct.unpack_from(">H", jpeg, body)[0]
        elif m == 0xDA:                                 # SOS
            break
        pos = end
    if frame is None:
        raise VdxError("JPEG: scan without a frame header (SOF0)")
    w, h, comps = frame
    samp = [(c[1], c[2]) for c in comps]
    if len(comps) == 1:
        sampling = "L"
    elif len(comps) == 3 and samp == [(1, 1)] * 3:
        sampling = "4:4:4"
    elif len(comps) == 3 and samp == [(2, 2), (1, 1), (1, 1)]:
        sampling = "4:2:0"
    elif len(comps) == 3 and samp == [(2, 1), (1, 1), (1, 1)]:
        raise VdxError("JPEG: 4:2:2 chroma subsampling is not supported (4:2:0, 4:4:4 or grey)")
    elif len(comps) == 4:
        raise VdxError("JPEG: 4 components (CMYK / YCCK) are not supported")
    else:
        raise VdxError(f"JPEG: {len(comps)} components with sampling factors {samp} are not supported (4:2:0, 4:4:4 or grey)")
    ns = jpeg[body]
    if ln != 6 + 2 * ns:
        raise VdxError("JPEG: malformed SOS segment")
    if ns != len(comps):
        raise VdxError(f"JPEG: a scan of {ns} of {len(comps)} components (several scans) is not supported")
    tables = []
    for i in range(ns):
        cid, tt = jpeg[body + 1 + 2 * i], jpeg[body + 2 + 2 * i]
        if cid != comps[i][0]:
            raise VdxError("JPEG: scan components out of frame order")
        td, ta = tt >> 4, tt & 15
        if (0, td) not in huffman or (1, ta) not in huffman:
            raise VdxError(f"JPEG: the scan uses Huffman tables DC {td} / AC {ta} that no DHT defined")
        tables.append((td, ta))
    ss, se, ahl = jpeg[body + 1 + 2 * ns:body + 4 + 2 * ns]
    if (ss, se, ahl) != (0, 63, 0):
        raise VdxError("JPEG: spectral selection / successive approximation in a baseline scan")
    for c in comps:
        if c[3] not in quant:
            raise VdxError(f"JPEG: component {c[0]} uses quantisation table {c[3]} that no DQT defined")
    for key in set((0, t[0]) for t in tables) | set((1, t[1]) for t in tables):
        _lookup(huffman[key])                           # validates the code lengths
    # the scan: every FF that is not stuffed (FF 00) starts a marker
    start = end
    a = np.frombuffer(jpeg, np.uint8, offset=start)
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, np.int64)
    mk = ff[a[ff + 1] != 0]
    codes = a[mk + 1]
    stop = np.flatnonzero((codes < 0xD0) | (codes > 0xD7))
    if len(stop) == 0:
        raise VdxError("JPEG: truncated inside the scan (no EOI)")
    if codes[stop[0]] == 0xFF:
        raise VdxError("JPEG: fill bytes (FF FF) inside the scan are not supported")
    if codes[stop[0]] != 0xD9:
        raise VdxError(f"JPEG: marker FF{codes[stop[0]]:02X} after the scan (several scans are not supported)")
    rst = mk[:stop[0]]
    scan_end = int(mk[stop[0]])
    hmax = 2 if sampling == "4:2:0" else 1
    nmcu = -(-w // (8 * hmax)) * -(-h // (8 * hmax))
    if dri == 0:
        if len(rst):
            raise VdxError("JPEG: restart markers in a scan without DRI")
        nseg = 1
    else:
        nseg = -(-nmcu // dri)
        if len(rst) != nseg - 1:
            raise VdxError(f"JPEG: {len(rst)} restart markers where {nmcu} MCUs in intervals of {dri} need {nseg - 1}")
        if np.any(codes[:stop[0]] != 0xD0 + (np.arange(len(rst)) & 7)):
            raise VdxError("JPEG: restart markers out of sequence (RSTn must count modulo 8)")
    seg = np.zeros((nseg, 4), np.int64)
    seg[:, 0] = np.concatenate([[0], rst + 2]) + start
    seg[:, 1] = np.concatenate([rst, [scan_end]]) + start
    step = dri if dri else nmcu
    seg[:, 2] = np.arange(nseg) * step
    seg[:, 3] = np.minimum(step, nmcu - seg[:, 2])
    return JpegInfo(w, h, sampling, dri, quant, tuple(c[3] for c in comps), tuple(tables), huffman, seg, (start, scan_end + start))


# ---------------------------------------------------------------------------------------------
# ISO base media: the layout cv2_shim.VideoWriter produces
# ---------------------------------------------------------------------------------------------
def _boxes(data: bytes, lo: int, hi: int, where: str):
    """(type, payload begin, payload end) of the boxes in data[lo:hi]; a box that runs past `hi` raises."""
    out = []
    while lo < hi:
        if lo + 8 > hi:
            raise VdxError(f"mp4: truncated inside {where} (a box header runs past the end)")
        size, kind = struct.unpack_from(">I4s", data, lo)
        hdr = 8
        if size == 1:
            if lo + 16 > hi:
                raise VdxError(f"mp4: truncated inside {where}")
            size, hdr = struct.unpack_from(">Q", data, lo + 8)[0], 16
        elif size == 0:
            size = hi - lo
        if size < hdr or lo + size > hi:
            raise VdxError(f"mp4: truncated inside {where}: box '{kind.decode('latin-1')}' of {size} bytes, {hi - lo} left")
        out.append((kind, lo + hdr, lo + size))
        lo += size
    return out


def _child(data, boxes, kind: bytes, where: str):
    for k, lo, hi in boxes:
        if k == kind:
            return lo, hi
    raise VdxError(f"mp4: no '{kind.decode()}' box in {where}")


def _descriptor(data: bytes, p: int, hi: int):
    """(tag, payload begin, payload end) of one MPEG-4 descriptor (1-byte tag, 7-bit groups of length)."""
    if p + 2 > hi:
        raise VdxError("mp4: truncated esds descriptor")
    tag, ln = data[p], 0
    p += 1
    for _ in range(4):
        if p >= hi:
            raise VdxError("mp4: truncated esds descriptor")
        b = data[p]
        p += 1
        ln = (ln << 7) | (b & 0x7F)
        if not b & 0x80:
            break
    if p + ln > hi:
        raise VdxError("mp4: truncated esds descriptor")
    return tag, p, p + ln


def demux(data: bytes) -> Tuple[List[bytes], dict]:
    """The file's bytes -> (the JPEG byte string of every sample, {"fps", "width", "height", "n_frames"}).  A bare JPEG is
    one sample (fps 0.0).  Refuses every sample entry but `mp4v` with object type 0x6C."""
    if data[:2] == b"\xff\xd8":
        return [bytes(data)], {"fps": 0.0, "width": None, "height": None, "n_frames": 1}
    if len(data) < 12 or data[4:8] != b"ftyp":
        raise VdxError("not an ISO base-media (.mp4) file and not a JPEG: no 'ftyp' box or SOI marker at the start")
    top = _boxes(data, 0, len(data), "the file")
    moov = _child(data, top, b"moov", "the file (truncated before the index?)")
    stbl = None
    timescale = 0
    for k, lo, hi in _boxes(data, *moov, "moov"):
        if k != b"trak":
            continue
        mdia = _child(data, _boxes(data, lo, hi, "trak"), b"mdia", "trak")
        mb = _boxes(data, *mdia, "mdia")
        hdlr = _child(data, mb, b"hdlr", "mdia")
        if data[hdlr[0] + 8:hdlr[0] + 12] != b"vide":
            continue
        mdhd = _child(data, mb, b"mdhd", "mdia")
        ver = data[mdhd[0]]
        timescale = struct.unpack_from(">I", data, mdhd[0] + (20 if ver == 1 else 12))[0]
        minf = _child(data, mb, b"minf", "mdia")
        stbl = _child(data, _boxes(data, *minf, "minf"), b"stbl", "minf")
        break
    if stbl is None:
        raise VdxError("mp4: no video track")
    sb = _boxes(data, *stbl, "stbl")
    lo, hi = _child(data, sb, b"stsd", "stbl")
    if struct.unpack_from(">I", data, lo + 4)[0] != 1:
        raise VdxError("mp4: expected one sample description")
    (ekind, elo, ehi), = _boxes(data, lo + 8, hi, "stsd")[:1]
    if ekind != b"mp4v":
        raise VdxError(f"mp4: sample entry '{ekind.decode('latin-1')}' is not Motion-JPEG (this reader takes 'mp4v' with object "
                       "type 0x6C only; H.264 / MPEG-4 part 2 files are not decoded here)")
    width, height = struct.unpack_from(">HH", data, elo + 24)
    esds = _child(data, _boxes(data, elo + 78, ehi, "mp4v"), b"esds", "the mp4v entry")
    tag, p, e = _descriptor(data, esds[0] + 4, esds[1])
    if tag != 0x03:
        raise VdxError("mp4: esds without an ES descriptor")
    flags = data[p + 2]
    p += 3 + (2 if flags & 0x80 else 0) + (2 if flags & 0x20 else 0)
    if flags & 0x40:
        p += 1 + data[p]
    tag, p, e = _descriptor(data, p, e)
    if tag != 0x04 or p >= e:
        raise VdxError("mp4: esds without a decoder configuration")
    if data[p] != 0x6C:
        raise VdxError(f"mp4: object type 0x{data[p]:02X} is not Motion-JPEG (0x6C); MPEG-4 part 2 and other codecs are not decoded here")
    lo, hi = _child(data, sb, b"stsz", "stbl")
    fixed, n = struct.unpack_from(">II", data, lo + 4)
    if fixed == 0 and lo + 12 + 4 * n > hi:
        raise VdxError("mp4: truncated stsz")
    sizes = [fixed] * n if fixed else list(struct.unpack_from(f">{n}I", data, lo + 12))
    lo, hi = _child(data, sb, b"stco", "stbl")
    nchunk = struct.unpack_from(">I", data, lo + 4)[0]
    if lo + 8 + 4 * nchunk > hi:
        raise VdxError("mp4: truncated stco")
    chunks = struct.unpack_from(f">{nchunk}I", data, lo + 8)
    lo, hi = _child(data, sb, b"stsc", "stbl")
    nrun = struct.unpack_from(">I", data, lo + 4)[0]
    if lo + 8 + 12 * nrun > hi:
        raise VdxError("mp4: truncated stsc")
    runs = [struct.unpack_from(">III", data, lo + 8 + 12 * i) for i in range(nrun)]
    lo, hi = _child(data, sb, b"stts", "stbl")
    nstts = struct.unpack_from(">I", data, lo + 4)[0]
    delta = struct.unpack_from(">II", data, lo + 8)[1] if nstts and lo + 16 <= hi else 0
    samples, s = [], 0
    for ci, off in enumerate(chunks):                   # samples of a chunk lie back to back
        per = 0
        for first, cnt, _ in runs:
            if first <= ci + 1:
                per = cnt
        for _ in range(per):
            if s >= n:
                break
            if off + sizes[s] > len(data):
                raise VdxError(f"mp4: sample {s} runs past the end of the file")
            samples.append(bytes(data[off:off + sizes[s]]))
            off += sizes[s]
            s += 1
    if s != n:
        raise VdxError(f"mp4: the chunk table covers {s} of {n} samples")
    fps = float(timescale) / delta if delta else 0.0
    return samples, {"fps": fps, "width": width, "height": height, "n_frames": n}


# ---------------------------------------------------------------------------------------------
def _samples(src) -> Tuple[List[bytes], dict]:
    if isinstance(src, (list, tuple)):
        jpegs = [bytes(j) for j in src]
        return jpegs, {"fps": 0.0, "width": None, "height": None, "n_frames": len(jpegs)}
    if isinstance(src, (bytes, bytearray, memoryview)):
        return demux(bytes(src))
    try:
        with open(os.fspath(src), "rb") as f:
            data = f.read()
    except OSError as e:
        raise VdxError(f"read_frames: cannot read {src!r}: {e}") from None
    return demux(data)


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def plan(jpegs: Sequence[bytes]):
    """Parse every frame and lay out the single upload: -> (blob uint8, offsets {name: (begin, count)}, info, infos).
    The blob holds, 256-byte aligned: the scans of all frames back to back (restart markers included, padded to 4 bytes),
    seg_off int32 [F+1], segs int32 [nseg][4] (byte ranges now relative to the blob's data), huff uint32 [F][4][384],
    sel int32 [F][3], quant uint16 [F][3][64]."""
    if len(jpegs) == 0:
        raise VdxError("read_frames: no frames")
    infos = []
    for i, j in enumerate(jpegs):
        try:
            infos.append(parse_jpeg(j))
        except VdxError as e:
            raise VdxError(f"frame {i}: {e}") from None
    first = infos[0]
    for i, it in enumerate(infos):
        if (it.width, it.height, it.sampling) != (first.width, first.height, first.sampling):
            raise VdxError(f"frame {i} is {it.width}x{it.height} {it.sampling}, frame 0 is {first.width}x{first.height} "
                           f"{first.sampling}: all frames of a clip must share size and sampling")
    F = len(infos)
    scans, segs, seg_off, base = [], [], [0], 0
    for j, it in zip(jpegs, infos):
        a, b = it.scan
        scans.append(np.frombuffer(j, np.uint8, count=b - a, offset=a))
        s = it.segments.copy()
        s[:, :2] += base - a
        segs.append(s)
        seg_off.append(seg_off[-1] + len(s))
        base += b - a
    nbytes = _align(base, 4)
    if nbytes >= 1 << 31:
        raise VdxError("read_frames: the clip's entropy data exceeds 2 GiB")
    segs = np.concatenate(segs).astype(np.int32)
    huff = np.zeros((F, 4, HUFF_WORDS), np.uint32)
    sel = np.zeros((F, 3), np.int32)
    quant = np.ones((F, 3, 64), np.uint16)
    for f, it in enumerate(infos):
        for (tc, th), payload in it.huffman.items():
            huff[f, tc * 2 + th] = _lookup(payload)
        for c, (td, ta) in enumerate(it.comp_tables):
            sel[f, c] = td | (ta << 4)
            quant[f, c] = it.quant[it.comp_quant[c]]
    parts = {"data": np.concatenate(scans), "seg_off": np.asarray(seg_off, np.int32), "segs": segs, "huff": huff, "sel": sel,
             "quant": quant}
    offsets, total = {}, 0
    for name, arr in parts.items():
        offsets[name] = (total, arr.size)
        total = _align(total + (nbytes if name == "data" else arr.nbytes))
    blob = np.zeros(total, np.uint8)
    for name, arr in parts.items():
        blob[offsets[name][0]:offsets[name][0] + arr.nbytes] = arr.reshape(-1).view(np.uint8)
    offsets["data"] = (0, nbytes)
    info = {"n_frames": F, "width": first.width, "height": first.height, "sampling": first.sampling,
            "restart_interval": first.restart_interval, "n_segments": int(seg_off[-1]),
            "max_segments_per_frame": int(max(len(it.segments) for it in infos))}
    return blob, offsets, info, infos


def read_frames(src: Union[str, os.PathLike, bytes, Sequence[bytes]], device="cuda", _events: Optional[list] = None):
    """Decode a Motion-JPEG .mp4 (path or bytes), a bare JPEG, or a list of JPEG byte strings on the GPU ->
    (uint8 frames on `device`: (F, H, W, 3) RGB, or (F, H, W) for grey streams; info).  `info`: n_frames, width, height, fps,
    sampling ("4:2:0", "4:4:4", "L"), restart_interval (MCUs, 0 without DRI), n_segments.  Raises `VdxError` for whatever is
    not Motion-JPEG / baseline JPEG, and, naming the frame, for entropy data the device found corrupt and for coefficients
    outside the range of 8-bit samples (decoders disagree on those: the module's docstring)."""
    jpegs, meta = _samples(src)
    blob, off, info, _ = plan(jpegs)
    if meta["width"] is not None and (meta["width"], meta["height"]) != (info["width"], info["height"]):
        raise VdxError(f"mp4: the sample entry says {meta['width']}x{meta['height']}, the JPEG frames are "
                       f"{info['width']}x{info['height']}")
    info["fps"] = meta["fps"]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise VdxError("read_frames: the decoder runs on the GPU (device must be a cuda device)")
    F, W, H, layout = info["n_frames"], info["width"], info["height"], LAYOUTS[info["sampling"]]
    if layout == 2 and W < 5:                # libjpeg upsamples chroma rows of one or two samples by replication instead
        raise VdxError("read_frames: 4:2:0 frames narrower than 5 pixels are not supported")
    lib = _lib.load()
    ws_bytes = lib.vdx_mjpeg_workspace(F, W, H, layout)
    if ws_bytes == 0:
        raise VdxError(f"read_frames: {F} frames of {W}x{H} are outside what the decoder takes")
    with torch.cuda.device(dev):
        up = torch.from_numpy(blob).to(dev, non_blocking=False)           # the one upload
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        nseg = info["n_segments"]
        err = torch.empty(nseg + F, dtype=torch.int32, device=dev)            # per segment: entropy errors; per frame: domain
        out = torch.empty((F, H, W, 3) if layout else (F, H, W), dtype=torch.uint8, device=dev)
        ptr = {k: up.data_ptr() + v[0] for k, v in off.items()}
        stream = torch.cuda.current_stream().cuda_stream

        def mark():
            if _events is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                _events.append(ev)

        mark()
        _lib.check(lib.vdx_mjpeg_entropy(ptr["data"], off["data"][1], ptr["seg_off"], ptr["segs"], nseg,
                                         info["max_segments_per_frame"], ptr["huff"], ptr["sel"], F, W, H, layout, ws.data_ptr(),
                                         err.data_ptr(), stream), "vdx_mjpeg_entropy")
        mark()
        _lib.check(lib.vdx_mjpeg_idct(ptr["quant"], F, W, H, layout, ws.data_ptr(), err.data_ptr() + 4 * nseg, stream),
                   "vdx_mjpeg_idct")
        mark()
        _lib.check(lib.vdx_mjpeg_color(ws.data_ptr(), F, W, H, layout, out.data_ptr(), stream), "vdx_mjpeg_color")
        mark()
        both = err.cpu().numpy().view(np.uint32)                             # the one synchronisation
    words, outside = both[:nseg], both[nseg:]
    bad = np.flatnonzero(words)
    if len(bad):
        seg_off = blob[off["seg_off"][0]:off["seg_off"][0] + 4 * (F + 1)].view(np.int32)
        s = int(bad[0])
        f = int(np.searchsorted(seg_off, s, side="right") - 1)
        code, mcu = int(words[s]) & 255, int(words[s]) >> 8
        raise VdxError(f"read_frames: frame {f} is corrupt: {ERRORS.get(code, f'error {code}')} (segment {s - int(seg_off[f])}, "
                       f"MCU {mcu} of it; {len(bad)} of {nseg} segments failed)")
    if outside.any():
        f = int(np.flatnonzero(outside)[0])
        raise VdxError(f"read_frames: frame {f} holds coefficients outside the range of 8-bit samples, on which libjpeg, "
                       f"libjpeg-turbo and this decoder disagree ({int(np.count_nonzero(outside))} of {F} frames)")
    return out, info


# ---------------------------------------------------------------------------------------------
# The write side: frames on the device -> the bytes cv2_shim.VideoWriter writes (csrc/mjpeg_enc.hip)
# ---------------------------------------------------------------------------------------------
# ITU-T T.81 Annex K: the example quantisation tables (natural order) and the typical Huffman tables (16 counts + symbols).
_QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
               80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
               95, 98, 112, 100, 103, 99]
_QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] + \
    [99] * 36
_AC_LUMA_SYMS = (
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
    "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
    "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_SYMS = (
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
STANDARD_HUFFMAN = {
    (0, 0): bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]) + bytes(range(12)),
    (0, 1): bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]) + bytes(range(12)),
    (1, 0): bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]) + bytes.fromhex(_AC_LUMA_SYMS),
    (1, 1): bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]) + bytes.fromhex(_AC_CHROMA_SYMS),
}
ENC_TABLE_WORDS = 272                 # csrc/mjpeg_enc.hip MJE_TABLE_WORDS: 16 DC + 256 AC words of (length << 16 | code)
ENC_SLOT_BYTES = 208                  # csrc/mjpeg_enc.hip MJE_SLOT_BYTES: the most one block's codes can take


def quant_tables(quality: int = 92) -> np.ndarray:
    """The Annex K tables scaled as libjpeg's jpeg_set_quality does (baseline: clamped to 1..255) -> int64 [2][64], natural
    order: luma, chroma."""
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = np.array([_QUANT_LUMA, _QUANT_CHROMA], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255)


def _marker(m: int, body: bytes) -> bytes:
    return bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body


def _mcu_grid(W: int, H: int, sampling: str) -> Tuple[int, int]:
    step = 16 if sampling == "4:2:0" else 8
    return -(-W // step), -(-H // step)


def jpeg_header(W: int, H: int, sampling: str, quality: int = 92, restart_rows: int = 0) -> bytes:
    """Everything Pillow (libjpeg) writes before the entropy data of a baseline frame with the standard Huffman tables:
    SOI, JFIF APP0, DQT per table, SOF0, DHT per table, DRI when `restart_rows` > 0, SOS.  `sampling`: "4:2:0" or "L"."""
    if sampling not in ("4:2:0", "L"):
        raise VdxError(f"jpeg_header: sampling {sampling!r} is not written here (\"4:2:0\" or \"L\")")
    if not (0 < W <= 65535 and 0 < H <= 65535):
        raise VdxError(f"jpeg_header: {W}x{H} is outside what a JPEG frame header holds")
    ncomp = 1 if sampling == "L" else 3
    q = quant_tables(quality)
    out = b"\xff\xd8" + _marker(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if ncomp == 3 else 1):
        out += _marker(0xDB, bytes([t]) + bytes(int(v) for v in q[t][_ZIGZAG]))
    comps = [(1, 0x22 if ncomp == 3 else 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)][:ncomp]
    out += _marker(0xC0, struct.pack(">BHHB", 8, H, W, ncomp) + b"".join(bytes(c) for c in comps))
    for t in range(2 if ncomp == 3 else 1):
        out += _marker(0xC4, bytes([t]) + STANDARD_HUFFMAN[(0, t)]) + _marker(0xC4, bytes([0x10 | t]) + STANDARD_HUFFMAN[(1, t)])
    if restart_rows > 0:
        dri = restart_rows * _mcu_grid(W, H, sampling)[0]
        if dri > 65535:
            raise VdxError(f"jpeg_header: a restart interval of {dri} MCUs does not fit the DRI segment")
        out += _marker(0xDD, struct.pack(">H", dri))
    out += _marker(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, 0x11 if c else 0]) for c in range(ncomp)) + bytes([0, 63, 0]))
    return out


def encoder_tables() -> np.ndarray:
    """The standard tables as the encoder kernels index them -> uint32 [2][272]: per table id 16 DC words (by size) and 256
    AC words (by run << 4 | size), each `length << 16 | code`; 0 for a symbol the table does not hold."""
    out = np.zeros((2, ENC_TABLE_WORDS), np.uint32)
    for (tc, th), payload in STANDARD_HUFFMAN.items():
        code = k = 0
        for ln in range(1, 17):
            for _ in range(payload[ln - 1]):
                out[th, (16 if tc else 0) + payload[16 + k]] = (ln << 16) | code
                code += 1
                k += 1
            code <<= 1
    return out


ENC_STAGES = ("coef", "planes", "bits", "segbits", "slots", "raw")      # vdx_mjpeg_enc_offsets


def encode_frames(frames: torch.Tensor, quality: int = 92, restart_rows: int = 0, sampling: Optional[str] = None,
                  _events: Optional[list] = None, _stages: Optional[dict] = None) -> List[bytes]:
    """Encode uint8 frames that are on the GPU as baseline JPEG there -> one byte string per frame, byte for byte what
    `Image.save(format="JPEG", quality=quality)` (Pillow on libjpeg) writes for the same frame: (F, H, W, 3) RGB as 4:2:0,
    (F, H, W) as grey; `restart_rows` > 0 as Pillow's `restart_marker_rows`.  One copy of the per-frame lengths and one of the
    packed bytes come back from the device.  Raises `VdxError` for anything else."""
    if not isinstance(frames, torch.Tensor):
        raise VdxError("encode_frames: frames must be a torch tensor on the GPU")
    if frames.device.type != "cuda":
        raise VdxError("encode_frames: the encoder runs on the GPU (frames must be on a cuda device)")
    if frames.dtype != torch.uint8:
        raise VdxError(f"encode_frames: frames must be uint8, not {frames.dtype}")
    if frames.dim() == 4 and frames.shape[3] == 3:
        layout, want = 2, "4:2:0"
    elif frames.dim() == 3:
        layout, want = 0, "L"
    else:
        raise VdxError(f"encode_frames: frames of shape {tuple(frames.shape)}: (F, H, W, 3) RGB or (F, H, W) grey expected")
    if sampling is not None and sampling != want:
        raise VdxError(f"encode_frames: sampling {sampling!r} is not written for frames of shape {tuple(frames.shape)} "
                       f"(only {want!r})")
    F, H, W = (int(v) for v in frames.shape[:3])
    if F * H * W == 0:
        raise VdxError(f"encode_frames: empty frames {tuple(frames.shape)}")
    if restart_rows < 0:
        raise VdxError(f"encode_frames: restart_rows={restart_rows}")
    header = jpeg_header(W, H, want, quality, restart_rows)
    dri = restart_rows * _mcu_grid(W, H, want)[0]
    lib = _lib.load()
    ws_bytes = lib.vdx_mjpeg_enc_workspace(F, W, H, layout)
    if ws_bytes == 0:
        raise VdxError(f"encode_frames: {F} frames of {W}x{H} are outside what the encoder takes")
    # the one upload: header | quantisation tables uint16 [2][64] | code tables uint32 [2][272]
    hb = _align(len(header))
    consts = np.zeros(hb + 256 + 2 * ENC_TABLE_WORDS * 4, np.uint8)
    consts[:len(header)] = np.frombuffer(header, np.uint8)
    consts[hb:hb + 256] = quant_tables(quality).astype(np.uint16).reshape(-1).view(np.uint8)
    consts[hb + 256:] = encoder_tables().reshape(-1).view(np.uint8)
    dev = frames.device
    with torch.cuda.device(dev):
        frames = frames.contiguous()
        up = torch.from_numpy(consts).to(dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        lengths = torch.empty(F, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def mark():
            if _events is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                _events.append(ev)

        mark()
        _lib.check(lib.vdx_mjpeg_enc_color(frames.data_ptr(), F, W, H, layout, ws.data_ptr(), stream), "vdx_mjpeg_enc_color")
        mark()
        _lib.check(lib.vdx_mjpeg_enc_fdct(up.data_ptr() + hb, F, W, H, layout, ws.data_ptr(), stream), "vdx_mjpeg_enc_fdct")
        mark()
        _lib.check(lib.vdx_mjpeg_enc_entropy(up.data_ptr() + hb + 256, F, W, H, layout, dri, len(header), ws.data_ptr(),
                                             lengths.data_ptr(), stream), "vdx_mjpeg_enc_entropy")
        mark()
        sizes = lengths.cpu().numpy().astype(np.int64)                      # copy 1: the per-frame lengths
        total = int(sizes.sum())
        if sizes.min() < len(header) + 2 or total >= 1 << 40:
            raise VdxError("encode_frames: the device returned impossible frame lengths")
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        mark()
        _lib.check(lib.vdx_mjpeg_enc_pack(up.data_ptr(), len(header), F, W, H, layout, dri, ws.data_ptr(), lengths.data_ptr(),
                                          out.data_ptr(), total, stream), "vdx_mjpeg_enc_pack")
        mark()
        data = out.cpu().numpy().tobytes()                                  # copy 2: the packed bytes
        if _stages is not None:
            import ctypes
            offs = (ctypes.c_size_t * 6)()
            _lib.check(lib.vdx_mjpeg_enc_offsets(F, W, H, layout, offs), "vdx_mjpeg_enc_offsets")
            ends = list(offs[1:]) + [ws_bytes]
            for name, a, b in zip(ENC_STAGES, offs, ends):
                _stages[name] = ws[a:b].cpu().numpy()
    ends = np.cumsum(sizes)
    return [data[int(e - n):int(e)] for e, n in zip(ends, sizes)]


def write_frames(path: Union[str, os.PathLike], frames: torch.Tensor, fps: float, restart_rows: int = 0) -> None:
    """Write frames that are on the GPU as the Motion-JPEG .mp4 `cv2_shim.VideoWriter` writes for them (RGB frames; the same
    file byte for byte): `encode_frames` on the device, the container through the writer's own box builder."""
    from .compat import cv2_shim
    jpegs = encode_frames(frames, 92, restart_rows)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    with open(os.fspath(path), "wb") as f:
        f.write(cv2_shim.mp4_bytes(jpegs, fps, W, H))
