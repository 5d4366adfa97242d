"""-m gpu: the Motion-JPEG decoder (vdx/video.py, csrc/mjpeg.hip) against Pillow's decode of the same bytes.  Every stage is
integer-defined (slow-integer IDCT, h2v2 fancy upsampling, fixed-point YCbCr -> RGB), so the bound is zero everywhere:
`read_frames` on the device must equal `np.asarray(Image.open(BytesIO(jpeg)).convert(mode))` bit for bit, for every frame
inside the claim's domain (dequantised products and pass-1 values within int16, samples before the range limit within
[-512, 511]: tests/test_video_host.py measures it); a frame outside it must raise, because decoders disagree there.

The second half calls the three stages one by one through `_lib` on the upload `video.plan` builds and compares what each
leaves in the workspace with its restatement in tests/mjpeg_ref.py, on inputs no encoder from pixels produces
(tests/mjpeg_enc.py writes them)."""
import io
import json

import numpy as np
import pytest
import torch

import lpips_ref as R
import mjpeg_enc
import mjpeg_ref

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


# ---------------------------------------------------------------------------------------------
# The domain of the Pillow claim
# ---------------------------------------------------------------------------------------------
def test_frames_outside_the_domain_raise_and_the_others_are_pillows(gpu):
    """Quantisation tables rewritten to larger legal values (tests/mjpeg_enc.py dqt_family, 48 files): as frame 1 of a clip
    whose frames 0 and 2 are the unmodified file, every file the restatement flags raises naming frame 1 (all that differ
    from Pillow are among them: test_video_host.py), every other one decodes bit-equal to Pillow."""
    from vdx import video
    from vdx._lib import VdxError
    raised = equal = 0
    for name, original, patched in mjpeg_enc.dqt_family():
        flag = mjpeg_ref.flagged(mjpeg_ref.decode([patched], with_extents=True)[2])[0]
        clip = [original, patched, original]
        if flag:
            with pytest.raises(VdxError, match="frame 1 holds coefficients outside the range of 8-bit samples"):
                video.read_frames(clip, device=gpu)
            raised += 1
        else:
            got = video.read_frames(clip, device=gpu)[0].cpu().numpy()
            assert np.array_equal(got, np.stack([pillow(j) for j in clip])), name
            equal += 1
    print(f"{raised} of 48 raise, {equal} decode bit-equal to Pillow")
    assert raised >= 17 and equal >= 1


def test_the_domain_boundary_is_exact_on_the_device(gpu):
    """One DC coefficient, samples before the limit of exactly 511, -512 (inside: Pillow's pixels) and 512, -513 (refused)."""
    from vdx import video
    from vdx._lib import VdxError
    for dc, inside in ((511, True), (-512, True), (512, False), (-513, False)):
        blocks = [mjpeg_enc._block(dc), mjpeg_enc._block(dc, z1=0)]
        j = mjpeg_enc.write("L", 16, 8, blocks, np.full((1, 64), 8)).jpeg                  # 8 * dc / 8
        ext = mjpeg_ref.decode([j], with_extents=True)[2]
        assert (ext[0, 2, 0 if dc < 0 else 1] == dc) and bool(mjpeg_ref.flagged(ext)[0]) != inside
        if inside:
            assert np.array_equal(video.read_frames([j], device=gpu)[0].cpu().numpy()[0], pillow(j, "L"))
        else:
            with pytest.raises(VdxError, match="frame 0 holds coefficients outside"):
                video.read_frames([j], device=gpu)


# ---------------------------------------------------------------------------------------------
# Stage by stage
# ---------------------------------------------------------------------------------------------
class Stages:
    """The upload of `video.plan` on the device, a workspace, and the three entry points called one at a time."""

    def __init__(self, gpu, blob, off, info):
        from vdx import _lib, video
        self.lib, self.check = _lib.load(), _lib.check
        self.F, self.W, self.H, self.layout = info["n_frames"], info["width"], info["height"], video.LAYOUTS[info["sampling"]]
        self.geo = mjpeg_ref._geometry(self.W, self.H, self.layout)
        self.bpf = self.geo[6][-1]
        self.info, self.off, self.nseg = info, off, info["n_segments"]
        self.up = torch.from_numpy(blob).to(gpu)
        self.ptr = {k: self.up.data_ptr() + v[0] for k, v in off.items()}
        nbytes = self.lib.vdx_mjpeg_workspace(self.F, self.W, self.H, self.layout)
        assert nbytes > 0
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=gpu)
        self.planes_at = (self.F * self.bpf * 128 + 255) // 256 * 256
        self.err = torch.full((self.nseg,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        self.flags = torch.full((self.F,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        shape = (self.F, self.H, self.W, 3) if self.layout else (self.F, self.H, self.W)
        self.out = torch.zeros(shape, dtype=torch.uint8, device=gpu)
        self.stream = torch.cuda.current_stream().cuda_stream

    def entropy(self, max_segs=None):
        a = (self.ptr["data"], self.off["data"][1], self.ptr["seg_off"], self.ptr["segs"], self.nseg,
             max_segs or self.info["max_segments_per_frame"], self.ptr["huff"], self.ptr["sel"], self.F, self.W, self.H, self.layout,
             self.ws.data_ptr(), self.err.data_ptr(), self.stream)
        self.check(self.lib.vdx_mjpeg_entropy(*a), "vdx_mjpeg_entropy")
        coef = self.ws[:self.F * self.bpf * 128].cpu().numpy().view(np.int16).reshape(self.F, self.bpf, 64)
        return coef, self.err.cpu().numpy().view(np.uint32)

    def set_coef(self, coef):
        self.ws[:self.F * self.bpf * 128] = torch.from_numpy(np.ascontiguousarray(coef, np.int16).reshape(-1).view(np.uint8)).to(self.ws.device)

    def idct(self, quant_ptr=None):
        self.check(self.lib.vdx_mjpeg_idct(quant_ptr or self.ptr["quant"], self.F, self.W, self.H, self.layout, self.ws.data_ptr(),
                                           self.flags.data_ptr(), self.stream), "vdx_mjpeg_idct")
        raw = self.ws[self.planes_at:self.planes_at + self.F * self.bpf * 64].cpu().numpy().reshape(self.F, self.bpf * 64)
        ncomp, _, _, _, bw, bh, boff = self.geo
        planes = [raw[:, boff[c] * 64:boff[c + 1] * 64].reshape(self.F, bh[c] * 8, bw[c] * 8) for c in range(ncomp)]
        return planes, self.flags.cpu().numpy().view(np.uint32)

    def color(self):
        self.check(self.lib.vdx_mjpeg_color(self.ws.data_ptr(), self.F, self.W, self.H, self.layout, self.out.data_ptr(), self.stream),
                   "vdx_mjpeg_color")
        return self.out.cpu().numpy()


def quant_of(blob, off, F):
    return blob[off["quant"][0]:off["quant"][0] + F * 3 * 64 * 2].view(np.uint16).reshape(F, 3, 64)


def test_entropy_with_part_filled_blocks_of_lanes(gpu):
    """Grey 8x48 frames with a restart marker after every block: 6 segments per frame and enough frames for 4 (or 5) segments per
    thread block, so each frame takes two blocks, the second part filled, and lanes >= spb idle: coefficients and error words
    against the restatement, the whole clip against Pillow."""
    from vdx import video
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    F = 3 * cus // 6 + 2
    spb = min(max(-(-F * 6 // cus), 1), 64)
    print(f"F {F}, segments per frame 6, CUs {cus}, segments per block {spb}")
    assert spb >= 3 and 6 % spb != 0
    jpegs = [jpeg_of(content("noise" if f % 3 else "sat", 8, 48, "L", seed=f), restart_marker_blocks=1, quality=(92, 30, 100)[f % 3])
             for f in range(F)]
    blob, off, info, _ = video.plan(jpegs)
    assert info["n_segments"] == 6 * F and info["max_segments_per_frame"] == 6
    st = Stages(gpu, blob, off, info)
    coef, err = st.entropy()
    want_coef, want_err = mjpeg_ref.entropy(blob, off, info)
    assert np.array_equal(err, want_err) and not err.any()
    assert np.array_equal(coef, want_coef)
    got = video.read_frames(jpegs, device=gpu)[0].cpu().numpy()
    assert np.array_equal(got, np.stack([pillow(j, "L") for j in jpegs]))


def test_entropy_of_a_clip_whose_frames_share_nothing_but_their_size(gpu):
    """Five 24x40 4:2:0 frames cycling through no DRI / DRI 1 / DRI 4, optimised and standard Huffman tables, quality 30 / 92 /
    100: uneven seg_off, max_segs_per_frame above most frames' own count, tables per frame."""
    from vdx import video
    kws = [{}, {"restart_marker_blocks": 1, "optimize": True, "quality": 30}, {"restart_marker_blocks": 4, "quality": 100},
           {"optimize": True, "quality": 100}, {"restart_marker_blocks": 1, "quality": 92}]
    jpegs = [jpeg_of(content("noise" if f % 2 else "sat", 24, 40, "RGB", seed=f), **kw) for f, kw in enumerate(kws)]
    blob, off, info, infos = video.plan(jpegs)
    assert [len(i.segments) for i in infos] == [1, 6, 2, 1, 6] and info["max_segments_per_frame"] == 6
    assert len({i.huffman[(1, 0)] for i in infos}) >= 3 and len({tuple(i.quant[0]) for i in infos}) == 3
    st = Stages(gpu, blob, off, info)
    coef, err = st.entropy()
    want_coef, want_err = mjpeg_ref.entropy(blob, off, info)
    assert np.array_equal(err, want_err) and not err.any() and np.array_equal(coef, want_coef)
    whole = video.read_frames(jpegs, device=gpu)[0]
    assert np.array_equal(whole.cpu().numpy(), np.stack([pillow(j) for j in jpegs]))
    assert torch.equal(whole, torch.cat([video.read_frames([j], device=gpu)[0] for j in jpegs]))


def test_entropy_of_hand_encoded_streams(gpu):
    """ZRL, k = 63 without EOB, FF 00 ending a segment, DC differences of size 11, a DC sum past int16, codes of 10..16 bits:
    the coefficients written are the coefficients read; inside the domain the frame is Pillow's."""
    from vdx import video
    from vdx._lib import VdxError
    for name, (sampling, W, H, blocks, quant, wr, in_domain) in mjpeg_enc.valid_streams().items():
        blob, off, info, _ = video.plan([wr.jpeg, wr.jpeg])
        coef, err = Stages(gpu, blob, off, info).entropy()
        want_coef, want_err = mjpeg_ref.entropy(blob, off, info)
        assert not err.any() and np.array_equal(err, want_err), name
        assert np.array_equal(coef, want_coef) and np.array_equal(coef[1], blocks.astype(np.int16)), name
        if in_domain:
            got = video.read_frames([wr.jpeg], device=gpu)[0].cpu().numpy()[0]
            assert np.array_equal(got, pillow(wr.jpeg, "L" if sampling == "L" else "RGB")), name
        else:
            with pytest.raises(VdxError, match="outside the range of 8-bit samples"):
                video.read_frames([wr.jpeg], device=gpu)


def test_entropy_error_words_by_construction(gpu):
    """Each error code once, with its MCU: the bad frame sits between two good ones, whose coefficients must be untouched; the
    same kind of stream ending exactly on its last bit is no error; a clean clip decodes afterwards."""
    from vdx import video
    from vdx._lib import VdxError
    q = np.ones((1, 64))
    good32 = mjpeg_enc.write("L", 32, 8, [mjpeg_enc._block(10 * i, z1=i + 1, z9=-3) for i in range(4)], q).jpeg
    exact_blocks, exact = mjpeg_enc.sized(0)
    good16 = exact.jpeg
    for name, (bad, code, mcu) in mjpeg_enc.error_streams().items():
        good = good16 if name == "short" else good32
        blob, off, info, _ = video.plan([good, bad, good])
        coef, err = Stages(gpu, blob, off, info).entropy()
        want_coef, want_err = mjpeg_ref.entropy(blob, off, info)
        print(name, [hex(e) for e in err])
        assert err.tolist() == [0, code | (mcu << 8), 0] and np.array_equal(err, want_err), name
        assert np.array_equal(coef[0], want_coef[0]) and np.array_equal(coef[2], want_coef[2]), name
        with pytest.raises(VdxError, match=f"frame 1 is corrupt: {video.ERRORS[code]}.*MCU {mcu} of it"):
            video.read_frames([good, bad, good], device=gpu)
    # the stream whose last symbol ends on the last bit of the last byte: every bit is there, no error
    assert exact.seg_bits[0] % 8 == 0
    blob, off, info, _ = video.plan([exact.jpeg])
    coef, err = Stages(gpu, blob, off, info).entropy()
    assert err.tolist() == [0] and np.array_equal(coef[0], exact_blocks.astype(np.int16))
    # code 5: rows of the segment table that point outside the clip, given to the entry point directly
    blob, off, info, _ = video.plan([good32, good32, good32])
    want_coef, _ = mjpeg_ref.entropy(blob, off, info)
    at = off["segs"][0]
    for col, value in ((0, off["data"][1] + 4), (1, off["data"][1] + 4), (2, 4), (3, 5), (2, -1), (1, -7)):
        edited = blob.copy()
        segs = edited[at:at + 3 * 16].view(np.int32).reshape(3, 4)
        segs[1, col] = value
        coef, err = Stages(gpu, edited, off, info).entropy()
        print("segment row", segs[1].tolist(), [hex(e) for e in err])
        assert err.tolist() == [0, 5, 0], (col, value)
        assert np.array_equal(coef[0], want_coef[0]) and np.array_equal(coef[2], want_coef[2]) and not coef[1].any()
    clean = video.read_frames([good32, good32], device=gpu)[0].cpu().numpy()
    assert np.array_equal(clean[0], pillow(good32, "L")) and np.array_equal(clean[1], clean[0])


def test_idct_on_any_coefficients_equals_the_int32_restatement(gpu):
    """Coefficients written straight into the workspace of 4:2:0 frames of 40x24 (36 blocks each; the block count is no multiple
    of the kernel's 32, so its tail is live): the 64 unit basis blocks at +-1, +-1023, +-32767 with quant 1 and quant 255, 4096
    random int16 blocks under quant tables of 1..255, of any uint16 and of 1 (small blocks, inside the domain).  The planes must
    equal the restatement in wrapping int32 byte for byte, the flag words its extents."""
    from vdx import video
    g = np.random.default_rng(7)
    basis = np.zeros((6, 64, 64), np.int16)
    for a, amp in enumerate((1, -1, 1023, -1023, 32767, -32767)):
        basis[a, np.arange(64), np.arange(64)] = amp
    per = 36
    nb_basis = -(-6 * 64 // per) * per                                       # whole frames per quant value
    rand = g.integers(-32768, 32768, (4096, 64)).astype(np.int16)
    rand[:per * 10] = g.integers(-6, 7, (per * 10, 64))                      # ten frames that stay inside the domain
    F = 2 * nb_basis // per + -(-4096 // per) + 1
    coef = np.zeros((F * per, 64), np.int16)
    coef[:384], coef[nb_basis:nb_basis + 384] = basis.reshape(-1, 64), basis.reshape(-1, 64)
    coef[2 * nb_basis:2 * nb_basis + 4096] = rand
    coef = coef.reshape(F, per, 64)
    assert (F * per) % 32 != 0 and F * per >= 2 * 384 + 4096 + 31
    quant = np.ones((F, 3, 64), np.uint16)
    f0 = nb_basis // per
    quant[f0:2 * f0] = 255
    kinds = np.arange(F - 2 * f0) % 3
    quant[2 * f0:][kinds == 1] = g.integers(1, 256, (int((kinds == 1).sum()), 3, 64))
    quant[2 * f0:][kinds == 2] = g.integers(0, 65536, (int((kinds == 2).sum()), 3, 64))
    quant[2 * f0:2 * f0 + 10] = g.integers(1, 3, (10, 3, 64))
    jpeg = jpeg_of(content("noise", 24, 40, "RGB"))
    blob, off, info, _ = video.plan([jpeg] * F)
    st = Stages(gpu, blob, off, info)
    assert st.bpf == per
    st.set_coef(coef)
    qdev = torch.from_numpy(quant.view(np.int16)).to(gpu)
    planes, flags = st.idct(qdev.data_ptr())
    want = mjpeg_ref.idct(coef, quant, 40, 24, 2, int32=True)
    want_flags = mjpeg_ref.flagged(mjpeg_ref.extents(coef, quant, 40, 24, 2, int32=True))
    print(f"{F} frames, {F * per} blocks, {int(want_flags.sum())} flagged")
    for c in range(3):
        assert np.array_equal(planes[c], want[c]), f"component {c}: {np.count_nonzero(planes[c] != want[c])} bytes differ"
    assert 10 <= want_flags.sum() <= F - 10 and not want_flags[2 * f0:2 * f0 + 10].any() and not want_flags[0]
    assert np.array_equal(flags, want_flags.astype(np.uint32))


def test_colour_conversion_of_every_triple(gpu):
    """One 4:4:4 frame of 4096x4096 whose planes hold every (Y, Cb, Cr) once, written straight into the workspace: all 2^24
    outputs of mj_rgb against the restatement in int64."""
    from vdx import _lib
    lib = _lib.load()
    n = 4096
    nbytes = lib.vdx_mjpeg_workspace(1, n, n, 1)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    bpf = 3 * (n // 8) ** 2
    at = (bpf * 128 + 255) // 256 * 256
    i = torch.arange(n * n, dtype=torch.int32, device=gpu)
    for c in range(3):
        ws[at + c * n * n:at + (c + 1) * n * n] = ((i >> (8 * c)) & 255).to(torch.uint8)
    out = torch.zeros((1, n, n, 3), dtype=torch.uint8, device=gpu)
    _lib.check(lib.vdx_mjpeg_color(ws.data_ptr(), 1, n, n, 1, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "vdx_mjpeg_color")
    got = out.cpu().numpy()
    del ws, out, i
    rows = 512                                                                # the reference in bands: int64 of all 2^24 is large
    for y0 in range(0, n, rows):
        idx = np.arange(y0 * n, (y0 + rows) * n, dtype=np.int32).reshape(1, rows, n)
        planes = [((idx >> (8 * c)) & 255).astype(np.uint8) for c in range(3)]
        want = mjpeg_ref.color(planes, n, rows, 1)
        band = got[:, y0:y0 + rows]
        assert np.array_equal(band, want), f"rows {y0}..: {np.count_nonzero((band != want).any(-1))} triples differ"


SIZES = [(1, 5), (2, 6), (3, 7), (7, 9), (8, 17), (9, 16), (15, 33), (17, 17), (37, 51), (1, 1), (1, 3), (3, 1)]


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_odd_sizes_upsampling_edges_and_both_store_paths(gpu, h, w):
    """Odd W and H, one chroma row, the narrowest 4:2:0 frame, W % 4 of 0..3: read_frames against Pillow for 4:2:0, 4:4:4 and
    grey; 4:2:0 narrower than 5 is refused."""
    from vdx import video
    from vdx._lib import VdxError
    for mode, kw in (("RGB", {}), ("RGB", {"subsampling": 0}), ("L", {})):
        jpegs = [jpeg_of(content("noise", h, w, mode, seed=h * w), **kw), jpeg_of(content("sat", h, w, mode, seed=h + w), quality=100, **kw)]
        if mode == "RGB" and not kw and w < 5:
            with pytest.raises(VdxError, match="narrower than 5"):
                video.read_frames(jpegs, device=gpu)
            continue
        got = video.read_frames(jpegs, device=gpu)[0].cpu().numpy()
        want = np.stack([pillow(j, mode) for j in jpegs])
        assert got.shape == want.shape
        assert np.array_equal(got, want), f"{mode} {kw}: {np.count_nonzero(got != want)} of {want.size} samples differ"
