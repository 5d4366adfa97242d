"""-m gpu: the Motion-JPEG writer (vdx/video.py `encode_frames` / `write_frames`, csrc/mjpeg_enc.hip) against Pillow's bytes for
the same frames and, stage by stage, against the numpy restatement tests/mjpeg_enc_ref.py (which tests/test_video_enc_host.py
pins to Pillow on the CPU).  Everything is integer-defined: the bound is zero, equality of bytes."""
import io

import numpy as np
import pytest
import torch

import mjpeg_enc_ref as E
import mjpeg_ref

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

CASES = E.cases()


def pillow(jpeg, mode="RGB"):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert(mode))


def _sections(stages, F, W, H, layout):
    """What the first two stages left in the workspace -> (component planes as the restatement shapes them, coefficients)."""
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    bpf = boff[-1]
    flat = stages["planes"][:F * bpf * 64].reshape(F, bpf * 64)
    planes = [flat[:, boff[c] * 64:boff[c + 1] * 64].reshape(F, bh[c] * 8, bw[c] * 8) for c in range(ncomp)]
    coef = stages["coef"][:F * bpf * 128].view(np.int16).reshape(F, bpf, 64)
    return planes, coef


@pytest.mark.parametrize("name,img", CASES, ids=[c[0] for c in CASES])
def test_every_stage_is_the_restatements_and_the_bytes_are_pillows(gpu, name, img):
    from vdx import video
    layout = 2 if img.ndim == 3 else 0
    H, W = img.shape[:2]
    frames = torch.from_numpy(img[None]).to(gpu)
    want, got = {}, {}
    jpeg = video.encode_frames(frames, restart_rows=1, _stages=got)[0]
    ref = E.encode(img[None], 92, 1, stages=want)[0]
    planes, coef = _sections(got, 1, W, H, layout)
    for c, (a, b) in enumerate(zip(planes, want["planes"])):
        assert np.array_equal(a, b), f"stage 1, component {c}: {int((a != b).sum())} samples differ"
    assert np.array_equal(coef, want["coef"]), f"stage 2: {int((coef != want['coef']).sum())} coefficients differ"
    lengths = E.entropy(want["coef"][0], W, H, layout, mjpeg_ref._geometry(W, H, layout)[1])[1]
    bits = got["bits"][:4 * len(lengths)].view(np.uint32)
    step = mjpeg_ref._geometry(W, H, layout)[1] * (6 if layout else 1)
    offsets = np.concatenate([np.cumsum([0] + lengths[s:s + step][:-1]) for s in range(0, len(lengths), step)])
    assert np.array_equal(bits, offsets), "stage 3: bit offsets of the blocks"
    assert jpeg == ref, "stage 3 / 4: bytes differ from the restatement's"
    assert jpeg == E.pillow_encode(img, 1)
    for rr in (0, 2):
        assert video.encode_frames(frames, restart_rows=rr)[0] == E.pillow_encode(img, rr), f"restart_rows={rr}"


@pytest.mark.parametrize("W,H", [(24, 20), (16, 4), (20, 24), (16, 8), (27, 27), (5, 12)])
def test_bottom_and_right_edges(gpu, W, H):
    """A dummy luma row and replicas of the last downsampled chroma row (H = 4, 8, 20, 24), a dummy column (W = 20, 5), neither."""
    from vdx import video
    for mode in E.MODES:
        img = E.content("noise", W, H, mode, seed=3)
        for rr in (0, 1):
            assert video.encode_frames(torch.from_numpy(img[None]).to(gpu), restart_rows=rr)[0] == E.pillow_encode(img, rr), (mode, rr)


def test_headline_size_many_thread_blocks_and_scan_chunks(gpu):
    """576 x 1024: 13824 blocks per frame (54 chunks of the per-frame scan; a segment of 384 blocks with restart_rows=1), two
    frames, against Pillow."""
    from vdx import video
    g = np.random.default_rng(5)
    yy, xx = np.mgrid[0:576, 0:1024]
    smooth = np.stack([xx // 4, yy // 3, (xx + yy) // 7], -1) % 256
    noisy = np.where(g.integers(0, 4, (576, 1024, 1)) == 0, g.integers(0, 256, (576, 1024, 3)), smooth)
    clip = np.stack([smooth, noisy]).astype(np.uint8)
    frames = torch.from_numpy(clip).to(gpu)
    for rr in (0, 1):
        got = video.encode_frames(frames, restart_rows=rr)
        assert got == [E.pillow_encode(f, rr) for f in clip], f"restart_rows={rr}"
    grey = torch.from_numpy(np.ascontiguousarray(clip[..., 1])).to(gpu)
    assert video.encode_frames(grey) == [E.pillow_encode(f) for f in clip[..., 1]]


def test_a_batch_is_its_frames_and_runs_repeat(gpu):
    from vdx import video
    clip = np.stack([E.content(k, 50, 38, "RGB", seed=i) for i, k in enumerate(("noise", "gradient", "saturated", "constant", "noise"))])
    frames = torch.from_numpy(clip).to(gpu)
    for rr in (0, 1):
        batch = video.encode_frames(frames, restart_rows=rr)
        assert batch == [video.encode_frames(frames[i:i + 1], restart_rows=rr)[0] for i in range(5)]
        assert batch == video.encode_frames(frames, restart_rows=rr)
        assert batch == [E.pillow_encode(f, rr) for f in clip]
    assert video.encode_frames(frames.permute(0, 2, 1, 3))[0] == E.pillow_encode(np.ascontiguousarray(clip[0].transpose(1, 0, 2)))


def test_write_then_read_is_pillows_decode_of_pillows_encode(gpu, tmp_path):
    from vdx import video
    from vdx.compat import cv2_shim
    clip = np.stack([E.content(k, 50, 38, "RGB", seed=i) for i, k in enumerate(("noise", "gradient", "saturated"))])
    for rr in (0, 1):
        path = tmp_path / f"w{rr}.mp4"
        video.write_frames(path, torch.from_numpy(clip).to(gpu), 8, restart_rows=rr)
        got, info = video.read_frames(path, device=gpu)
        assert info["n_frames"] == 3 and info["fps"] == 8.0 and info["restart_interval"] == rr * 4
        assert np.array_equal(got.cpu().numpy(), np.stack([pillow(E.pillow_encode(f, rr)) for f in clip]))
        ref = tmp_path / f"host{rr}.mp4"                    # the file the host writer leaves for the same frames
        vw = cv2_shim.VideoWriter(str(ref), cv2_shim.VideoWriter_fourcc(*"mp4v"), 8, (50, 38), restart_rows=rr)
        for f in clip:
            vw.write(cv2_shim.cvtColor(f, cv2_shim.COLOR_RGB2BGR))
        vw.release()
        assert path.read_bytes() == ref.read_bytes()


def test_write_video_on_a_device_writes_the_host_paths_file(gpu, tmp_path):
    from vdx import metrics
    frames = [E.content(k, 64, 48, "RGB", seed=i) for i, k in enumerate(("noise", "gradient"))]
    for rr in (0, 2):
        a, b = tmp_path / f"a{rr}.mp4", tmp_path / f"b{rr}.mp4"
        metrics.write_video(frames, str(a), 8, restart_rows=rr)
        metrics.write_video(frames, str(b), 8, restart_rows=rr, device=gpu)
        assert a.read_bytes() == b.read_bytes()


BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--noise_device", "cpu"]


def test_pipeline_gpu_video_write_leaves_the_same_file(gpu, tmp_path, monkeypatch):
    """`python -m vdx.pipeline --gpu_video_write --video_restart_rows 1` on the tiny stand-in job: the mp4 is the one the host
    path writes for the very frames the job handed to `write_video`."""
    from vdx import metrics
    from vdx.pipeline import main
    real, seen = metrics.write_video, {}

    def spy(frames, path, fps, **kw):
        seen.update(kw, fps=fps, frames=[np.array(f) for f in frames])
        return real(frames, path, fps, **kw)

    monkeypatch.setattr(metrics, "write_video", spy)
    mp4 = tmp_path / "out.mp4"
    assert main(BASE + ["--out_csv", str(tmp_path / "r.csv"), "--out_video", str(mp4), "--gpu_video_write",
                        "--video_restart_rows", "1"]) == 0
    assert seen["device"] is not None and seen["restart_rows"] == 1 and len(seen["frames"]) == 8
    host = tmp_path / "host.mp4"
    real(seen["frames"], str(host), seen["fps"], restart_rows=1)
    assert mp4.read_bytes() == host.read_bytes()


def test_refusals(gpu):
    from vdx import video
    ok = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=gpu)
    bad = [ok.cpu(), ok.float(), ok.to(torch.int8), ok[0, 0], ok[None], torch.zeros((1, 16, 16, 4), dtype=torch.uint8, device=gpu),
           ok[:0], ok[:, :0], ok[:, :, :0]]
    for t in bad:
        with pytest.raises(video.VdxError):
            video.encode_frames(t)
    with pytest.raises(video.VdxError):
        video.encode_frames(np.zeros((1, 16, 16, 3), np.uint8))
    with pytest.raises(video.VdxError):
        video.encode_frames(ok, sampling="4:4:4")
    with pytest.raises(video.VdxError):
        video.encode_frames(ok[..., 0], sampling="4:2:0")
    with pytest.raises(video.VdxError):
        video.encode_frames(ok, restart_rows=-1)
    assert video.encode_frames(ok, sampling="4:2:0") == [E.pillow_encode(np.zeros((16, 16, 3), np.uint8))]
