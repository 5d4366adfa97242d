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
