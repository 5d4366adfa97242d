"""-m gpu: the animated-GIF writer (vdx/gif.py, csrc/gif.hip) against the numpy restatement tests/gif_ref.py, bit for bit: every
stage on its own at its edges, whole files (which Pillow must decode to palette[index]), batches, repeats, files and the job."""
import ctypes
import io

import numpy as np
import pytest
import torch

import gif_ref as R

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

CANARY = 0xA5


def _rng(seed):
    return np.random.default_rng(seed)


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


# ---- stage 1: histogram ------------------------------------------------------------------------------------------------------
def _hist(frames, gpu):
    from vdx import ops
    t = frames if isinstance(frames, torch.Tensor) else _dev(frames, gpu)
    return ops.gif_hist(t).cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def test_hist_one_colour(gpu):
    f = np.empty((2, 37, 53, 3), np.uint8)
    f[:] = (200, 17, 95)
    h = _hist(f, gpu)
    assert np.array_equal(h, R.hist(f)) and h[(25 << 10) | (2 << 5) | 11] == 2 * 37 * 53 and np.count_nonzero(h) == 1


def test_hist_every_bin_once(gpu):
    b = _rng(1).permutation(R.BINS)
    f = np.stack([((b >> 10) << 3) | 4, (((b >> 5) & 31) << 3) | 1, ((b & 31) << 3) | 7], axis=1).astype(np.uint8).reshape(1, 128, 256, 3)
    h = _hist(f, gpu)
    assert np.array_equal(h, np.ones(R.BINS, np.int64)) and np.array_equal(h, R.hist(f))


def test_hist_unaligned_and_pitched(gpu):
    f = _rng(2).integers(0, 256, (3, 33, 47, 3), dtype=np.uint8)
    f[1, :20] = f[1, 0, 0]                                                  # runs of one bin, across rows
    assert np.array_equal(_hist(f, gpu), R.hist(f))
    big = _dev(_rng(3).integers(0, 256, (3, 40, 50, 3), dtype=np.uint8), gpu)
    view = big[:, 3:36, 2:49]                                               # packed pixels, pitched rows and frames
    assert not view.is_contiguous()
    assert np.array_equal(_hist(view, gpu), R.hist(view.cpu().numpy()))


# ---- stage 3: LUT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "full", "duplicates"])
def test_lut(gpu, name):
    from vdx import ops
    rng = _rng(4)
    if name == "one":
        pal = np.array([[9, 200, 31]], np.uint8)
    elif name == "full":
        pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    else:
        pal = np.repeat(rng.integers(0, 256, (40, 3), dtype=np.uint8), 3, axis=0)[rng.permutation(120)]
    got = ops.gif_lut(_dev(pal, gpu)).cpu().numpy()
    want = R.lut(pal)
    assert np.array_equal(got, want)
    if name == "duplicates":                                                # of equal entries only the first is ever named
        first = {tuple(p): i for i, p in reversed(list(enumerate(pal.tolist())))}
        assert all(first[tuple(pal[i])] == i for i in np.unique(got))


# ---- stage 4: index map --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dither", ["bayer", "none"])
def test_index_map(gpu, dither):
    from vdx import ops
    rng = _rng(5)
    f = rng.integers(0, 256, (2, 33, 47, 3), dtype=np.uint8)
    f[0, :8] = rng.integers(0, 8, (8, 47, 3))                               # the clamp at 0 ...
    f[0, 8:16] = rng.integers(248, 256, (8, 47, 3))                         # ... and at 255
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    table = R.lut(pal)
    got = ops.gif_index(_dev(f, gpu), _dev(table, gpu), dither).cpu().numpy()
    assert got.shape == (2, 33, 47) and np.array_equal(got, R.index_map(f, table, dither))
    big = _dev(rng.integers(0, 256, (2, 40, 50, 3), dtype=np.uint8), gpu)
    view = big[:, 3:36, 2:49]
    assert np.array_equal(ops.gif_index(view, _dev(table, gpu), dither).cpu().numpy(), R.index_map(view.cpu().numpy(), table, dither))


# ---- stage 5 and 6: LZW and the sub-blocks, with canaries ------------------------------------------------------------------------
def _words(b, n):
    return np.frombuffer(b + bytes(4 * n - len(b)), "<u4")


def run_lzw(idx, strip_rows, gpu):
    """Stages 5 and 6 on uint8 (T, H, W) indices, every buffer prefilled with the canary byte and longer than asked for; checks
    everything the stages leave against the restatement and returns the strips' slots (the used words) per frame."""
    from vdx import ops
    T, H, W = idx.shape
    need = ops.gif_lzw_workspace(T, H, W, strip_rows)
    lay = ops.gif_lzw_offsets(T, H, W, strip_rows)
    ns, sw = lay["nstrips"], lay["slot_words"]
    assert ns == len(R.strips_of(H, strip_rows)) and sw == R.slot_words(strip_rows, H, W)
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=gpu)
    lengths = torch.full((T + 8,), -7, dtype=torch.int32, device=gpu)
    ops.gif_lzw(_dev(idx, gpu), strip_rows, ws, lengths)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    assert (raw[need:] == CANARY).all(), "stage 5 wrote behind its workspace"
    ln = lengths.cpu().numpy()
    assert (ln[T:] == -7).all()
    sbits = raw[lay["sbits"]:lay["sbits"] + 4 * T * ns].view("<u4").reshape(T, ns)
    soff = raw[lay["soff"]:lay["soff"] + 4 * T * ns].view("<u4").reshape(T, ns)
    fbits = raw[lay["fbits"]:lay["fbits"] + 4 * T].view("<u4")
    slots = raw[lay["slots"]:lay["slots"] + 4 * T * ns * sw].view("<u4").reshape(T, ns, sw)
    stream = raw[lay["stream"]:lay["stream"] + 4 * T * ns * sw].view("<u4").reshape(T, ns * sw)
    used, blocks = [], []
    for t in range(T):
        data, bits, alone = R.frame_stream(idx[t], strip_rows)
        assert sbits[t].tolist() == bits
        assert soff[t].tolist() == np.concatenate([[0], np.cumsum(bits)[:-1]]).tolist() and fbits[t] == sum(bits)
        mine = []
        for s, (b, nb) in enumerate(alone):
            k = -(-nb // 32)
            assert k <= sw
            assert np.array_equal(slots[t, s, :k], _words(b, k)), (t, s)
            assert (slots[t, s, k:] == CANARY * 0x01010101).all(), f"strip {s} of frame {t} wrote past its bits"
            mine.append(slots[t, s, :k].copy())
        used.append(mine)
        k = -(-len(data) // 4)
        assert np.array_equal(stream[t, :k], _words(data, k)) and not stream[t, k:].any()
        blocks.append(R.sub_blocks(data))
        assert np.array_equal(R.lzw_decode(data, H * W).reshape(H, W), idx[t])      # the restatement's own decoder reads it back
        assert ln[t] == len(blocks[-1])
    foff = raw[lay["foff"]:lay["foff"] + 8 * T].view("<u8")
    assert foff.tolist() == np.concatenate([[0], np.cumsum(ln[:T].astype(np.int64))[:-1]]).tolist()
    total = int(ln[:T].sum())
    out = torch.full((total + 256,), CANARY, dtype=torch.uint8, device=gpu)
    ops.gif_pack(ws, T, H, W, strip_rows, out[:total])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == CANARY).all(), "stage 6 wrote behind its output"
    assert got[:total].tobytes() == b"".join(blocks)
    assert (ws.cpu().numpy()[need:] == CANARY).all()
    return used


def _clears(pixels):
    return sum(1 for c, _w in R.strip_codes(pixels, True, True) if c == R.CLEAR)


def lzw_cases():
    rng = _rng(6)
    flat = np.full((2, 40, 64), 7, np.uint8)
    flat[1] = 9
    return {
        "1x1": (rng.integers(0, 256, (1, 1, 1), dtype=np.uint8), 1),
        "47x33-short-last-strip": (rng.integers(0, 256, (2, 33, 47), dtype=np.uint8), 4),
        "one-row-strips": (rng.integers(0, 16, (2, 9, 40), dtype=np.uint8), 1),
        "one-strip": (rng.integers(0, 256, (2, 33, 47), dtype=np.uint8), 33),
        "strip-rows-beyond-H": (rng.integers(0, 4, (1, 5, 7), dtype=np.uint8), 1000),
        "table-fills": (rng.integers(0, 256, (1, 64, 96), dtype=np.uint8), 64),
        "flat": (flat, 40),
        "flat-strips": (flat, 16),
        "three-colours": (rng.integers(0, 3, (2, 130, 70), dtype=np.uint8), 7),
    }


LZW = lzw_cases()


@pytest.mark.parametrize("name", list(LZW))
def test_lzw_and_pack(gpu, name):
    idx, strip_rows = LZW[name]
    if name == "table-fills":
        assert idx[0].size >= 6144 and _clears(idx[0].reshape(-1)) >= 2, "the table never filled"
    if name == "flat":
        assert R.closing_width(idx[0].reshape(-1)) == 9                     # 2560 pixels in some 70 codes: the width never grows
    run_lzw(idx, strip_rows, gpu)


def _crossings():
    """For one seeded row, the smallest n at which the closing code of row[:n] is 10, 11 and 12 bits wide (the entry the decoder
    adds after the last data code crosses 512 / 1024 / 2048), by bisection: the width never shrinks as the strip grows."""
    row = _rng(7).integers(0, 256, 2400, dtype=np.uint8)
    out = []
    for width in (10, 11, 12):
        lo, hi = 1, len(row)
        assert R.closing_width(row[:hi]) >= width
        while lo < hi:
            mid = (lo + hi) // 2
            if R.closing_width(row[:mid]) >= width:
                hi = mid
            else:
                lo = mid + 1
        assert R.closing_width(row[:lo]) == width and R.closing_width(row[:lo - 1]) == width - 1
        out.append(lo)
    return row, out


def test_lzw_closing_code_at_the_width_after_the_bump(gpu):
    row, ns = _crossings()
    for n in ns:
        for m in (n - 1, n, n + 1):
            run_lzw(row[:m].reshape(1, 1, m), 1, gpu)


def test_a_frames_bits_are_the_same_alone_and_in_a_batch(gpu):
    idx = _rng(8).integers(0, 256, (3, 33, 47), dtype=np.uint8)
    batch = run_lzw(idx, 4, gpu)
    for t in range(3):
        alone = run_lzw(idx[t:t + 1], 4, gpu)[0]
        assert len(alone) == len(batch[t]) and all(np.array_equal(a, b) for a, b in zip(alone, batch[t]))


# ---- whole files -----------------------------------------------------------------------------------------------------------------
def _pillow_frames(blob):
    im = Image.open(io.BytesIO(blob))
    out = []
    for t in range(im.n_frames):
        im.seek(t)
        out.append(np.asarray(im.convert("RGB")))
    return np.stack(out), im.info


def _content(T, H, W, seed):
    """A gradient that moves, noise in one corner, flat bands: smooth, busy and flat regions in every frame"""
    rng = _rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    f = np.stack([np.stack([(x * 255 // max(W - 1, 1) + 8 * t) % 256, y * 255 // max(H - 1, 1), (x + y + 16 * t) // 4 % 256], axis=-1)
                  for t in range(T)]).astype(np.uint8)
    f[:, :H // 3, :W // 3] = rng.integers(0, 256, (T, H // 3, W // 3, 3))
    f[:, 2 * H // 3:] = (40, 90, 200)
    return f


FILES = {"47x33": ((3, 33, 47), {"strip_rows": 4}), "47x33-none": ((3, 33, 47), {"dither": "none", "strip_rows": 1}),
         "1x1": ((2, 1, 1), {}), "96x64-default": ((2, 64, 96), {"loop": 3}), "576x1024": ((4, 576, 1024), {})}


@pytest.mark.parametrize("name", list(FILES))
def test_encode_gif_is_the_restatement_and_pillow_reads_it(gpu, name):
    from vdx import gif
    (T, H, W), kw = FILES[name]
    f = _content(T, H, W, 9)
    blob, info = gif.encode_gif(_dev(f, gpu), 8, **kw)
    want, pal, idx = R.encode(f, 8, **kw)
    assert blob == want
    assert info == {"frames": T, "colors": len(pal), "bytes": len(blob), "delay_cs": 13, "fps": 100 / 13, "dither": kw.get("dither", "bayer"),
                    "strip_rows": min(kw.get("strip_rows", max(1, -(-8192 // W))), H), "loop": kw.get("loop", 0)}
    got, pinfo = _pillow_frames(blob)
    assert got.shape == (T, H, W, 3) and np.array_equal(got, pal[idx])
    assert pinfo["duration"] == 130 and pinfo.get("loop") == kw.get("loop", 0)
    if name == "576x1024":                                                  # 288 workgroups of LZW, and two runs
        assert info["strip_rows"] == 8 and len(pal) == 256
        again, _ = gif.encode_gif(_dev(f, gpu), 8, **kw)
        assert again == blob


def test_more_strips_than_one_scan_chunk(gpu):
    """600 strips of one row: the per-frame scan walks three chunks of 256"""
    idx = _rng(10).integers(0, 256, (2, 600, 5), dtype=np.uint8)
    run_lzw(idx, 1, gpu)


def test_palette_given_and_two_runs(gpu):
    from vdx import gif
    f = _content(3, 33, 47, 11)
    pal = _rng(12).integers(0, 256, (100, 3), dtype=np.uint8)
    a, info = gif.encode_gif(_dev(f, gpu), 12.5, palette=pal, strip_rows=4)
    b, _ = gif.encode_gif(list(f), 12.5, palette=torch.from_numpy(pal), strip_rows=4, device=gpu)      # host frames: uploaded
    want, _, idx = R.encode(f, 12.5, palette=pal, strip_rows=4)
    assert a == b == want and info["colors"] == 100 and info["delay_cs"] == 8
    got, _ = _pillow_frames(a)
    assert np.array_equal(got, pal[idx])
    one, _ = gif.encode_gif(_dev(f[1:2], gpu), 12.5, palette=pal, strip_rows=4)
    assert R.decode_file(one)["frames"][0].tolist() == R.decode_file(a)["frames"][1].tolist()


def test_write_gif_writes_encode_gifs_bytes(gpu, tmp_path):
    from vdx import gif
    f = _dev(_content(2, 20, 30, 13), gpu)
    info = gif.write_gif(tmp_path / "a.gif", f, 10, loop=2, dither="none")
    blob, info2 = gif.encode_gif(f, 10, loop=2, dither="none")
    assert (tmp_path / "a.gif").read_bytes() == blob and info == info2 and info["delay_cs"] == 10


def test_refusals_that_need_a_device(gpu):
    from vdx import gif, ops
    from vdx._lib import VdxError
    ok = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError, match="GPU"):
        gif.encode_gif(ok, 8, device="cpu")
    for bad in (ok.cpu(), ok.float(), ok[..., :2], ok[0]):
        with pytest.raises(VdxError):
            ops.gif_hist(bad)
        with pytest.raises(VdxError):
            ops.gif_index(bad, torch.zeros(R.BINS, dtype=torch.uint8, device=gpu))
    with pytest.raises(VdxError):
        ops.gif_index(ok, torch.zeros(100, dtype=torch.uint8, device=gpu))
    with pytest.raises(VdxError):
        ops.gif_lut(torch.zeros((257, 3), dtype=torch.uint8, device=gpu))
    with pytest.raises(VdxError):
        ops.gif_lut(torch.zeros((0, 3), dtype=torch.uint8, device=gpu))
    idx = torch.zeros((1, 16, 16), dtype=torch.uint8, device=gpu)
    with pytest.raises(VdxError):
        ops.gif_lzw(idx, 0, torch.zeros(1 << 16, dtype=torch.uint8, device=gpu))
    with pytest.raises(VdxError):
        ops.gif_lzw(idx, 4, torch.zeros(16, dtype=torch.uint8, device=gpu))        # a workspace too small
    with pytest.raises(VdxError, match="outside what the encoder takes"):
        ops.gif_lzw_workspace(1, 65535, 65535, 65535)                              # the frame's bit offsets would pass 2^32
    lib = __import__("vdx._lib", fromlist=["load"]).load()
    assert lib.vdx_gif_hist_u8(ctypes.c_void_p(ok.data_ptr()), 1 << 40, 1 << 20, 65535, 65535, 2, ctypes.c_void_p(idx.data_ptr()), None) != 0
    assert b"2^32" in lib.vdx_last_error()


# ---- the job -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--interpolate", "2", "--co_denoise", "--loop"]], ids=["plain", "interpolated-loop"])
def test_run_job_out_gif(gpu, tmp_path, monkeypatch, extra):
    """The tiny stand-in job with and without `out_gif`: the GIF is the restatement's file for the frames the job handed to the
    writer and decodes to their restated indices; the result carries "gif"; the mp4 and the CSV row are what they are without."""
    from vdx import gif, metrics
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import build_arg_parser, config_from_args, gif_record, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    base = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "128", "--chunk_size", "6",
            "--overlap", "2", "--noise_device", "cpu"]
    cfg = config_from_args(build_arg_parser().parse_args(base + extra))
    real, seen = gif.write_gif, {}

    def spy(path, frames, fps, **kw):
        assert isinstance(frames, torch.Tensor) == bool(extra), "interpolated frames stay on the device"
        seen.update(frames=np.stack([np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f) for f in frames]), fps=fps, kw=kw)
        return real(path, frames, fps, **kw)

    monkeypatch.setattr(gif, "write_gif", spy)
    res0 = run_job(cfg, out_video=str(tmp_path / "a.mp4"), pipe=pipe)
    assert not seen
    res1 = run_job(cfg, out_video=str(tmp_path / "b.mp4"), pipe=pipe, out_gif=str(tmp_path / "b.gif"), gif_dither="none", gif_loop=5)
    T = 16 if extra else 8
    assert seen["frames"].shape == (T, 128, 128, 3) and seen["fps"] == cfg.fps * (2 if extra else 1)
    want, pal, idx = R.encode(seen["frames"], seen["fps"], loop=5, dither="none")
    blob = (tmp_path / "b.gif").read_bytes()
    assert blob == want
    got, pinfo = _pillow_frames(blob)
    assert np.array_equal(got, pal[idx]) and pinfo["loop"] == 5 and pinfo["duration"] == 10 * R.delay_cs(seen["fps"])
    assert set(res1) == set(res0) | {"gif"}
    assert res1["gif"] == {"frames": T, "colors": len(pal), "bytes": len(blob), "delay_cs": R.delay_cs(seen["fps"]), "dither": "none",
                           "strip_rows": 64}
    assert gif_record(res1) == {"gif": res1["gif"]} and gif_record(res0) == {}
    assert (tmp_path / "a.mp4").read_bytes() == (tmp_path / "b.mp4").read_bytes()
    timing = {"peak_vram_mb", "end_vram_mb", "net_gather_s", "net_reduce_s", "denoise_s", "encode_s"}
    assert {k: v for k, v in res0.items() if k not in timing} == {k: v for k, v in res1.items() if k not in timing | {"gif"}}
    for name, res in (("a", res0), ("b", res1)):                           # the row, its clock readings held equal
        row = metrics.result_row({**res, **{k: 0 for k in timing}}, mode=cfg.mode, num_frames=8, elapsed_s=1.0)
        metrics.append_csv(str(tmp_path / f"{name}.csv"), {**row, "timestamp": "t", "host": "h"})
    assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes()
    only = run_job(cfg, out_video=None, pipe=pipe, out_gif=str(tmp_path / "c.gif"), gif_dither="none", gif_loop=5)       # without an mp4
    assert (tmp_path / "c.gif").read_bytes() == blob and only["frames_written"] is None and only["gif"] == res1["gif"]
