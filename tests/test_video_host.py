"""The host half of the Motion-JPEG reader (vdx/video.py, vdx/compat/cv2_shim.py VideoCapture): container, marker walk,
Huffman lookups, segment table and every refusal, without a GPU.  tests/mjpeg_ref.py restates the three device stages in
Python from the very upload the host builds, so the integer definition the kernels implement is pinned to Pillow's decode here
too, on images of a few MCUs."""
import io
import struct

import numpy as np
import pytest

import vdx  # noqa: F401
from vdx import metrics, video
from vdx._lib import VdxError
from vdx.compat import cv2_shim

import mjpeg_ref

Image = pytest.importorskip("PIL.Image")

H, W, F = 48, 64, 3


def clip_frames(seed=0, n=F, h=H, w=W):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.clip(np.stack([xx * 3 + 10 * f, yy * 4, xx + yy], -1) + g.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
            for f in range(n)]


def jpeg_of(rgb, **kw):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", **{"quality": 92, **kw})
    return buf.getvalue()


def write_clip(path, frames, fps=8, **kw):
    vw = cv2_shim.VideoWriter(str(path), cv2_shim.VideoWriter_fourcc(*"mp4v"), fps, (frames[0].shape[1], frames[0].shape[0]), **kw)
    for f in frames:
        vw.write(f[..., ::-1])
    vw.release()
    return open(path, "rb").read()


def test_shim_exposes_videocapture_and_its_constants():
    assert callable(cv2_shim.VideoCapture)
    assert (cv2_shim.CAP_PROP_FRAME_WIDTH, cv2_shim.CAP_PROP_FRAME_HEIGHT, cv2_shim.CAP_PROP_FPS,
            cv2_shim.CAP_PROP_FRAME_COUNT) == (3, 4, 5, 7)                 # OpenCV's values


@pytest.mark.parametrize("restart_rows", [0, 1])
def test_demux_returns_pillows_bytes_and_the_tables(tmp_path, restart_rows):
    frames = clip_frames()
    kw = {"restart_rows": restart_rows} if restart_rows else {}
    data = write_clip(tmp_path / "c.mp4", frames, fps=8, **kw)
    jpegs, meta = video.demux(data)
    extra = {"restart_marker_rows": 1} if restart_rows else {}
    assert jpegs == [jpeg_of(f, **extra) for f in frames]
    assert meta == {"fps": 8.0, "width": W, "height": H, "n_frames": F}
    per_frame = -(-H // 16) if restart_rows else 1
    for j in jpegs:
        info = video.parse_jpeg(j)
        q = Image.open(io.BytesIO(j)).quantization
        assert {k: list(v) for k, v in q.items()} == info.quant
        assert (info.width, info.height, info.sampling) == (W, H, "4:2:0")
        assert info.restart_interval == (W // 16 if restart_rows else 0)
        seg = info.segments
        assert seg.shape == (per_frame, 4)
        # the byte ranges tile the scan: SOS payload end | segment | RSTn | segment | ... | EOI
        assert seg[0, 0] == info.scan[0] == j.index(b"\xff\xda") + 2 + struct.unpack_from(">H", j, j.index(b"\xff\xda") + 2)[0]
        assert np.array_equal(seg[1:, 0], seg[:-1, 1] + 2)
        assert seg[-1, 1] == info.scan[1] == len(j) - 2 and j[-2:] == b"\xff\xd9"
        for i in range(per_frame - 1):
            assert j[seg[i, 1]:seg[i, 1] + 2] == bytes([0xFF, 0xD0 + i % 8])
        nmcu = (H // 16) * (W // 16)
        assert np.array_equal(seg[:, 2], np.arange(per_frame) * (nmcu // per_frame)) and seg[:, 3].sum() == nmcu
    blob, off, info, _ = video.plan(jpegs)
    assert info["n_segments"] == F * per_frame and info["max_segments_per_frame"] == per_frame
    assert (info["n_frames"], info["width"], info["height"], info["sampling"]) == (F, W, H, "4:2:0")


def test_writer_default_bytes_are_unchanged(tmp_path):
    frames = clip_frames(1)
    a = write_clip(tmp_path / "a.mp4", frames)
    b = write_clip(tmp_path / "b.mp4", frames, restart_rows=0)
    assert a == b
    metrics.write_video(frames, str(tmp_path / "c.mp4"), 8)
    metrics.write_video(frames, str(tmp_path / "d.mp4"), 8, restart_rows=0)
    assert open(tmp_path / "c.mp4", "rb").read() == open(tmp_path / "d.mp4", "rb").read()
    if metrics._cv2() is cv2_shim:
        assert a == open(tmp_path / "c.mp4", "rb").read()
    metrics.write_video(frames, str(tmp_path / "e.mp4"), 8, restart_rows=1)
    assert video.demux(open(tmp_path / "e.mp4", "rb").read())[0] == [jpeg_of(f, restart_marker_rows=1) for f in frames]


def test_refusals_are_decided_on_the_host(tmp_path, monkeypatch):
    """Every one of these raises before anything is enqueued: loading the library would be the first step of a launch."""
    from vdx import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refusal reached the device"))
    frames = clip_frames(2)
    with pytest.raises(VdxError, match="progressive"):
        video.read_frames([jpeg_of(frames[0], progressive=True)])
    with pytest.raises(VdxError, match="4:2:2"):
        video.read_frames([jpeg_of(frames[0], subsampling=1)])
    with pytest.raises(VdxError, match="CMYK"):
        buf = io.BytesIO()
        Image.fromarray(np.dstack([frames[0], frames[0][..., 0]]), mode="CMYK").save(buf, format="JPEG")
        video.read_frames(buf.getvalue())
    good = write_clip(tmp_path / "g.mp4", frames)
    moov = good.rindex(b"moov") - 4
    with pytest.raises(VdxError, match="truncated inside"):
        video.read_frames(good[:moov + 200])
    with pytest.raises(VdxError, match="truncated inside the file: box 'mdat'"):      # cut inside the last frame's scan
        video.read_frames(good[:moov - 300])
    j = jpeg_of(frames[0])
    with pytest.raises(VdxError, match="truncated inside the scan"):
        video.read_frames(j[:len(j) - 200])
    with pytest.raises(VdxError, match="truncated inside the scan"):
        video.read_frames([jpeg_of(frames[1]), j[:len(j) - 200]])
    assert b"mp4v" in good
    with pytest.raises(VdxError, match="not Motion-JPEG"):
        video.read_frames(good.replace(b"mp4v", b"avc1"))
    esds = good.rindex(b"esds")
    i = good.index(bytes([0x04, 13, 0x6C]), esds) + 2
    with pytest.raises(VdxError, match="not Motion-JPEG"):            # object type 0x20: real MPEG-4 part 2
        video.read_frames(good[:i] + b"\x20" + good[i + 1:])
    with pytest.raises(VdxError, match="share size and sampling"):
        video.read_frames([j, jpeg_of(frames[0], subsampling=0)])
    rst = jpeg_of(frames[0], restart_marker_rows=1)
    k = rst.index(b"\xff\xd1")
    with pytest.raises(VdxError, match="out of sequence"):
        video.read_frames(rst[:k] + b"\xff\xd2" + rst[k + 2:])
    with pytest.raises(VdxError, match="cannot read"):
        video.read_frames(str(tmp_path / "missing.mp4"))


def test_videocapture_is_not_opened_for_missing_or_foreign_files(tmp_path):
    assert not cv2_shim.VideoCapture(str(tmp_path / "missing.mp4")).isOpened()
    good = write_clip(tmp_path / "g.mp4", clip_frames(3), fps=12)
    (tmp_path / "h264.mp4").write_bytes(good.replace(b"mp4v", b"avc1"))
    (tmp_path / "junk.mp4").write_bytes(b"\0" * 64)
    assert not cv2_shim.VideoCapture(str(tmp_path / "h264.mp4")).isOpened()
    assert not cv2_shim.VideoCapture(str(tmp_path / "junk.mp4")).isOpened()
    cap = cv2_shim.VideoCapture(str(tmp_path / "g.mp4"))
    assert cap.isOpened()
    assert [cap.get(p) for p in (cv2_shim.CAP_PROP_FRAME_COUNT, cv2_shim.CAP_PROP_FRAME_WIDTH, cv2_shim.CAP_PROP_FRAME_HEIGHT,
                                 cv2_shim.CAP_PROP_FPS)] == [3.0, float(W), float(H), 12.0]
    cap.release()
    assert not cap.isOpened() and cap.read() == (False, None)


CASES = [(16, 16, "RGB", {}), (38, 50, "RGB", {"optimize": True}), (38, 50, "RGB", {"subsampling": 0, "quality": 100}),
         (38, 50, "L", {"quality": 30}), (24, 80, "RGB", {"restart_marker_blocks": 3}), (32, 32, "RGB", {"restart_marker_rows": 1})]


@pytest.mark.parametrize("h,w,mode,kw", CASES)
def test_the_integer_definition_equals_pillows_decode(h, w, mode, kw):
    """The upload the host builds, decoded by the Python restatement of the kernels, is Pillow's image bit for bit: the
    lookups built from the stream's DHT, the segment table, and the arithmetic csrc/mjpeg.hip implements."""
    a = np.random.default_rng(h * w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: h // 2, : w // 3] = 0
    a[h // 2:, w // 2:] = 255
    if mode == "L":
        a = a[..., 0]
    j = jpeg_of(a, **kw)
    got, err = mjpeg_ref.decode([j, j])
    want = np.asarray(Image.open(io.BytesIO(j)).convert(mode))
    assert not err.any()
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)


# ---------------------------------------------------------------------------------------------
# The hand writer (tests/mjpeg_enc.py) and the domain of "bit-equal to Pillow"
# ---------------------------------------------------------------------------------------------
import mjpeg_enc  # noqa: E402


def pillow(jpeg, mode):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert(mode))


def test_hand_written_streams_open_in_pillow_and_carry_what_they_claim():
    """Every valid output of the writer opens in Pillow; the restatement reads back the very coefficients (low 16 bits) and,
    inside the domain, Pillow's pixels.  The special forms are really in the bytes."""
    streams = mjpeg_enc.valid_streams()
    assert set(streams) == {"zrl", "k63-ff00", "dc11", "dc-wrap", "huff16"}
    for name, (sampling, W, H, blocks, quant, wr, in_domain) in streams.items():
        mode = "L" if sampling == "L" else "RGB"
        want = pillow(wr.jpeg, mode)
        assert want.shape[:2] == (H, W)
        info = video.parse_jpeg(wr.jpeg)
        assert (info.width, info.height, info.sampling) == (W, H, sampling)
        blob, off, pinfo, _ = video.plan([wr.jpeg])
        coef, err = mjpeg_ref.entropy(blob, off, pinfo)
        assert not err.any(), name
        assert np.array_equal(coef[0], blocks.astype(np.int16)), name
        got, _, ext = mjpeg_ref.decode([wr.jpeg], with_extents=True)
        assert bool(mjpeg_ref.flagged(ext)[0]) == (not in_domain), name
        if in_domain:
            assert np.array_equal(got[0], want), name
    s = streams["k63-ff00"]
    seg = video.parse_jpeg(s[5].jpeg).segments
    assert len(seg) == 2 and all(s[5].jpeg[e - 2:e] == b"\xff\x00" for e in seg[:, 1])       # FF 00 ends both segments
    assert not np.array_equal(streams["dc-wrap"][3], streams["dc-wrap"][3].astype(np.int16))  # the DC sum left int16
    assert max(abs(int(b[0]) - int(a[0])) for a, b in zip(streams["dc11"][3][:3], streams["dc11"][3][1:4])) >= 1024   # size 11
    codes = mjpeg_enc.codes_of(video.parse_jpeg(streams["huff16"][5].jpeg).huffman[(1, 0)])
    assert {n for _, n in codes.values()} == set(range(10, 17))
    for mod8 in (0, 1):
        blocks, wr = mjpeg_enc.sized(mod8)
        assert wr.seg_bits[0] % 8 == mod8 and pillow(wr.jpeg, "L").shape == (8, 16)
        assert not mjpeg_ref.decode([wr.jpeg])[1].any()


def test_refused_streams_give_their_error_word_in_the_restatement():
    for name, (jpeg, code, mcu) in mjpeg_enc.error_streams().items():
        assert mjpeg_ref.decode([jpeg])[1].tolist() == [code | (mcu << 8)], name


def test_domain_bounds_are_the_kernels():
    import os
    import re
    src = open(os.path.join(os.path.dirname(video.__file__), "csrc", "mjpeg.hip")).read()
    assert int(re.search(r"#define MJ_DOMAIN_PRODUCT (\d+)", src).group(1)) == mjpeg_ref.DOMAIN_PRODUCT
    assert int(re.search(r"#define MJ_DOMAIN_PASS1 (\d+)", src).group(1)) == mjpeg_ref.DOMAIN_PASS1


def test_int32_mode_equals_int64_where_nothing_wraps_and_wraps_elsewhere():
    g = np.random.default_rng(0)
    quant = g.integers(1, 17, (4, 3, 64)).astype(np.uint16)
    small = g.integers(-8, 9, (4, 6, 64)).astype(np.int16)
    for a, b in zip(mjpeg_ref.idct(small, quant, 16, 16, 2), mjpeg_ref.idct(small, quant, 16, 16, 2, int32=True)):
        assert np.array_equal(a, b)
    assert np.array_equal(mjpeg_ref.extents(small, quant, 16, 16, 2), mjpeg_ref.extents(small, quant, 16, 16, 2, int32=True))
    big = g.integers(-32768, 32768, (4, 6, 64)).astype(np.int16)
    wide = g.integers(0, 65536, (4, 3, 64)).astype(np.uint16)
    e64, e32 = mjpeg_ref.extents(big, wide, 16, 16, 2), mjpeg_ref.extents(big, wide, 16, 16, 2, int32=True)
    assert np.array_equal(e64[:, 0], e32[:, 0]) and np.abs(e64[:, 1]).max() > 2 ** 31 > np.abs(e32[:, 1]).max()


def test_every_stream_inside_the_domain_decodes_as_pillow_does():
    """The domain of the Pillow claim: a stream with every dequantised product and pass-1 value inside int16 and every sample
    before the range limit inside [-512, 511] decodes to Pillow's pixels, with no exception among streams whose amplitude
    sweeps across that boundary (profiles/mjpeg_domain.txt records a run).  A condition, not a tolerance."""
    res = mjpeg_enc.domain_search(seed=0)
    print({k: v for k, v in res.items() if k != "counterexamples"})
    assert res["blocks"] >= 20000
    assert res["unflagged"] >= 3000 and res["flagged_differ"] >= 3000        # the sweep straddles the boundary
    assert res["nearest"][0] <= 8                                          # and comes within a few grey levels of it from outside
    assert res["unflagged_differ"] == 0, res["counterexamples"][:3]


def _content(kind, h, w, mode, seed=0):
    g = np.random.default_rng(seed)
    shape = (h, w) if mode == "L" else (h, w, 3)
    if kind == "noise":
        a = g.integers(0, 256, shape)
    elif kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        a = xx * 255 // max(w - 1, 1) if mode == "L" else np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1),
                                                                    (xx + yy) * 255 // (w + h - 2)], -1)
    elif kind == "const":
        a = np.full(shape, 77)
    else:
        a = g.integers(0, 256, shape)
        a[: h // 2, : w // 3] = 0
        a[h // 3:, w // 2:] = 255
    return np.asarray(a, np.int64).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("kind", ["noise", "ramp", "const", "sat"])
def test_no_stream_pillow_encoded_from_pixels_is_refused(kind):
    """No false refusals: the contents of the GPU cases at quality 1 .. 100, both samplings and grey, stay inside the domain
    (a flag here would mean the bound is wrong, not the image)."""
    worst = np.zeros((3, 2), np.int64)
    for quality in (1, 5, 30, 75, 92, 100):
        for mode, kw in (("RGB", {}), ("RGB", {"subsampling": 0}), ("L", {})):
            j = jpeg_of(_content(kind, 38, 50, mode, seed=quality), quality=quality, **kw)
            blob, off, info, _ = video.plan([j])
            coef = _fast_coefficients(j)
            quant = blob[off["quant"][0]:off["quant"][0] + 3 * 64 * 2].view(np.uint16).reshape(1, 3, 64)
            ext = mjpeg_ref.extents(coef[None], quant, 50, 38, video.LAYOUTS[info["sampling"]])
            worst[:, 0], worst[:, 1] = np.minimum(worst[:, 0], ext[0, :, 0]), np.maximum(worst[:, 1], ext[0, :, 1])
            assert not mjpeg_ref.flagged(ext)[0], (kind, quality, mode, kw, ext.tolist())
    print(kind, "extents (product, pass 1, sample):", worst.tolist())


def _fast_coefficients(jpeg):
    blob, off, info, _ = video.plan([jpeg])
    coef, err = mjpeg_ref.entropy(blob, off, info)
    assert not err.any()
    return coef[0]


def test_dqt_patched_files_differ_from_pillow_only_outside_the_domain():
    """A Pillow-encoded noise image whose quantisation tables alone were rewritten to larger legal values: where the
    restatement (libjpeg's C arithmetic) and Pillow (libjpeg-turbo) return different pixels, the frame is flagged, every one;
    the unmodified files are never flagged."""
    differ = flagged = 0
    for name, original, patched in mjpeg_enc.dqt_family():
        mode = "RGB"
        got, err, ext = mjpeg_ref.decode([original, patched], with_extents=True)
        assert not err.any()
        flag = mjpeg_ref.flagged(ext)
        assert not flag[0] and np.array_equal(got[0], pillow(original, mode)), name
        d = not np.array_equal(got[1], pillow(patched, mode))
        differ, flagged = differ + d, flagged + int(flag[1])
        assert flag[1] or not d, f"{name}: differs from Pillow by up to {np.abs(got[1].astype(int) - pillow(patched, mode)).max()} unflagged"
    print(f"{differ} of 48 patched files differ from Pillow, {flagged} are flagged")
    assert differ >= 1 and flagged < 48
