"""-m gpu: the Motion-JPEG decoder (vdx/video.py, csrc/mjpeg.hip) against Pillow's decode of the same bytes.  Every stage is
integer-defined (slow-integer IDCT, h2v2 fancy upsampling, fixed-point YCbCr -> RGB), so the bound is zero everywhere:
`read_frames` on the device must equal `np.asarray(Image.open(BytesIO(jpeg)).convert(mode))` bit for bit."""
import io
import json

import numpy as np
import pytest
import torch

import lpips_ref as R

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")


def content(kind, h, w, mode, seed=0):
    g = np.random.default_rng(seed)
    shape = (h, w) if mode == "L" else (h, w, 3)
    if kind == "noise":                                   # long codes, ZRL, large coefficients
        a = g.integers(0, 256, shape)
    elif kind == "ramp":                                  # EOB-heavy
        yy, xx = np.mgrid[0:h, 0:w]
        a = xx * 255 // max(w - 1, 1) if mode == "L" else np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1),
                                                                    (xx + yy) * 255 // (w + h - 2)], -1)
    elif kind == "const":                                 # DC only
        a = np.full(shape, 77)
    else:                                                 # "sat": noise with 0 / 255 patches, the clamps
        a = g.integers(0, 256, shape)
        a[: h // 2, : w // 3] = 0
        a[h // 3:, w // 2:] = 255
    return np.asarray(a, np.int64).clip(0, 255).astype(np.uint8)


def jpeg_of(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **{"quality": 92, **kw})
    return buf.getvalue()


def pillow(jpeg, mode="RGB"):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert(mode))


# (H, W, content, mode, encoder keywords): every size, content and encoding of the issue at least once
CASES = [
    (16, 16, "noise", "RGB", {}),
    (16, 16, "const", "RGB", {}),
    (16, 16, "sat", "L", {}),
    (38, 50, "noise", "RGB", {}),
    (38, 50, "ramp", "RGB", {"quality": 30}),
    (38, 50, "sat", "RGB", {"quality": 100}),
    (38, 50, "noise", "RGB", {"optimize": True}),
    (38, 50, "sat", "RGB", {"subsampling": 0}),
    (38, 50, "noise", "L", {}),
    (38, 50, "noise", "RGB", {"restart_marker_rows": 1}),
    (38, 50, "noise", "RGB", {"restart_marker_blocks": 3, "subsampling": 0, "quality": 100}),
    (48, 64, "noise", "RGB", {}),
    (48, 64, "ramp", "RGB", {}),
    (48, 64, "const", "RGB", {"subsampling": 0}),
    (48, 64, "sat", "RGB", {"quality": 30, "optimize": True}),
    (48, 64, "noise", "RGB", {"restart_marker_rows": 1}),
    (48, 64, "ramp", "L", {"restart_marker_rows": 1, "optimize": True}),
    (32, 1024, "noise", "RGB", {}),
    (32, 1024, "sat", "RGB", {"restart_marker_blocks": 3}),       # 43 intervals: they end mid-row and wrap RST7 -> RST0
    (32, 1024, "ramp", "RGB", {"restart_marker_rows": 1, "quality": 100}),
    (32, 1024, "noise", "L", {"restart_marker_blocks": 3, "quality": 30}),
]


@pytest.mark.parametrize("h,w,kind,mode,kw", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}-" + "-".join(f"{k}{v}" for k, v in c[4].items())
                                                         for c in CASES])
def test_read_frames_is_bit_equal_to_pillow(gpu, h, w, kind, mode, kw):
    from vdx import video
    jpegs = [jpeg_of(content(kind, h, w, mode, seed=s), **kw) for s in (1, 2)]
    frames, info = video.read_frames(jpegs, device=gpu)
    want = np.stack([pillow(j, mode) for j in jpegs])
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == want.shape and frames.device.type == "cuda"
    sampling = "L" if mode == "L" else ("4:4:4" if kw.get("subsampling") == 0 else "4:2:0")
    assert (info["n_frames"], info["width"], info["height"], info["sampling"]) == (2, w, h, sampling)
    if "restart_marker_blocks" in kw:
        assert info["restart_interval"] == 3 and info["n_segments"] // 2 >= 9
    got = frames.cpu().numpy()
    diff = np.abs(got.astype(np.int32) - want)
    print(f"max |diff| {diff.max()}, differing samples {np.count_nonzero(diff)} of {diff.size}")
    assert np.array_equal(got, want)


def _write(path, frames, **kw):
    from vdx.compat import cv2_shim
    vw = cv2_shim.VideoWriter(str(path), cv2_shim.VideoWriter_fourcc(*"mp4v"), 8, (frames[0].shape[1], frames[0].shape[0]), **kw)
    for f in frames:
        vw.write(f[..., ::-1])
    vw.release()


def test_videocapture_reads_what_videowriter_wrote(gpu, tmp_path):
    """VideoWriter -> VideoCapture.read() is Pillow's decode with the channels reversed, then (False, None); the clip in one
    call equals its frames decoded one at a time, and two runs agree bit for bit."""
    from vdx import video
    from vdx.compat import cv2_shim
    clip = R.frames_like_video(5, 40, 72, seed=3)
    path = tmp_path / "c.mp4"
    _write(path, clip)
    jpegs, meta = video.demux(path.read_bytes())
    want = np.stack([pillow(j) for j in jpegs])
    cap = cv2_shim.VideoCapture(str(path))
    assert cap.isOpened() and cap.get(cv2_shim.CAP_PROP_FRAME_COUNT) == 5.0 and cap.get(cv2_shim.CAP_PROP_FPS) == 8.0
    for i in range(5):
        ok, bgr = cap.read()
        assert ok and bgr.dtype == np.uint8 and np.array_equal(bgr, want[i][..., ::-1])
    assert cap.read() == (False, None) and cap.read() == (False, None)
    cap.release()
    whole, info = video.read_frames(str(path), device=gpu)
    assert info["fps"] == 8.0 and info["n_frames"] == 5 and info["restart_interval"] == 0
    again = video.read_frames(path.read_bytes(), device=gpu)[0]
    assert torch.equal(whole, again)
    single = torch.cat([video.read_frames([j], device=gpu)[0] for j in jpegs])
    assert torch.equal(whole, single)
    assert np.array_equal(whole.cpu().numpy(), want)


def test_untrusted_entropy_bytes_raise_or_decode_and_leave_the_process_sound(gpu, tmp_path):
    """Random bytes in one restart interval (markers kept), and a stream that ends in the middle of a code: `read_frames` names
    the frame in a VdxError or returns an image, and the untouched clip then still decodes bit-equal."""
    from vdx import video
    from vdx._lib import VdxError
    clip = R.frames_like_video(3, 48, 64, seed=5)
    path = tmp_path / "c.mp4"
    _write(path, clip, restart_rows=1)
    jpegs, _ = video.demux(path.read_bytes())
    want = np.stack([pillow(j) for j in jpegs])
    seg = video.parse_jpeg(jpegs[1]).segments
    assert len(seg) == 3
    outcomes = []
    for seed in (0, 3, 5):                                 # 0 happens to decode; 3 and 5 run a coefficient index past 63
        noise = np.random.default_rng(seed).integers(0, 255, int(seg[1, 1] - seg[1, 0]), dtype=np.uint8)      # never FF: no new marker
        bad = jpegs[1][:seg[1, 0]] + noise.tobytes() + jpegs[1][seg[1, 1]:]
        assert len(video.parse_jpeg(bad).segments) == 3
        variants = [bad]
        if seed == 0:                                      # the last interval stops inside a code: cut its tail, keep EOI
            variants.append(jpegs[1][:seg[2, 0] + (seg[2, 1] - seg[2, 0]) // 2] + b"\xff\xd9")
        for v in variants:
            try:
                out = video.read_frames([jpegs[0], v, jpegs[2]], device=gpu)[0]
                assert tuple(out.shape) == want.shape
                assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[2].cpu().numpy(), want[2])
                outcomes.append("image")
            except VdxError as e:
                assert "frame 1" in str(e)
                outcomes.append("error")
    print("outcomes:", outcomes)
    assert outcomes[1] == "error"                          # half a restart interval cannot hold its MCUs
    assert np.array_equal(video.read_frames(jpegs, device=gpu)[0].cpu().numpy(), want)


def test_file_scores_are_decode_plus_the_frame_scores(gpu, tmp_path):
    """compute_md_vqs_file / verify_video_authenticity_file / CLIPScorer.score_file on the mp4 equal the frame-taking methods on
    Pillow's decode of its samples, exactly: decode + the existing path, nothing else."""
    from vdx import video
    from vdx.compat.diffusers_shim import HashTokenizer
    from vdx.mdvqs import MDVQS, verify_video_authenticity, verify_video_authenticity_file
    clip = R.frames_like_video(8, 64, 64, seed=11)
    path = tmp_path / "c.mp4"
    _write(path, clip, restart_rows=1)
    want = np.stack([pillow(j) for j in video.demux(path.read_bytes())[0]])
    m = MDVQS.synthetic(seed=0, device=gpu, flow="gpu")
    tok = HashTokenizer()
    assert m.compute_md_vqs_file(str(path), "a rocket", tokenizer=tok) == m.compute_md_vqs(want, "a rocket", tokenizer=tok)
    assert verify_video_authenticity_file(str(path), device=gpu) == verify_video_authenticity(want, device=gpu)
    s_file, per_file = m.clip.score_file(path.read_bytes(), "a rocket", tokenizer=tok)
    s_mem, per_mem = m.clip.score(want, "a rocket", tokenizer=tok)
    assert s_file == s_mem and torch.equal(per_file, per_mem)


BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--noise_device", "cpu"]
KEYS = {"pf", "vq", "tc", "total", "weights", "lpips_per_pair", "authentic", "authenticity", "synthetic_weights", "n_frames"}


def test_pipeline_scores_the_written_file(gpu, tmp_path):
    """--mdvqs_json --score_from_file --video_restart_rows 1: the record says "source": "file" and its authenticity block is
    the gate of Pillow's decode of out.mp4; without the flags the record has the keys it always had."""
    from vdx import video
    from vdx.mdvqs import verify_video_authenticity
    from vdx.pipeline import main
    mp4, js = tmp_path / "out.mp4", tmp_path / "m.json"
    base = BASE + ["--out_csv", str(tmp_path / "r.csv"), "--out_video", str(mp4), "--mdvqs_json", str(js)]
    assert main(base + ["--score_from_file", "--video_restart_rows", "1"]) == 0
    rec = json.load(open(js))
    assert set(rec) == KEYS | {"source"} and rec["source"] == "file" and rec["n_frames"] == 8
    jpegs, meta = video.demux(mp4.read_bytes())
    assert len(jpegs) == 8 and video.parse_jpeg(jpegs[0]).restart_interval == 256 // 16
    ok, stats = verify_video_authenticity(np.stack([pillow(j) for j in jpegs]), device=gpu)
    assert rec["authentic"] == ok and rec["authenticity"] == stats
    assert main(base) == 0
    assert set(json.load(open(js))) == KEYS
    assert video.parse_jpeg(video.demux(mp4.read_bytes())[0][0]).restart_interval == 0
