"""-m gpu: every stage of the Motion-JPEG writer (csrc/mjpeg_enc.hip) on its own, at its edges and at every quality.  The entry
points `video.encode_frames` calls are driven one at a time on a workspace with a canary behind it, so that a stage can be fed
what the stage before it never produces from 8-bit samples: the coefficient sets and basis blocks of tests/mjpeg_enc_ref.py,
whose reach tests/test_video_enc_host.py establishes on the CPU.  Every expected value is the restatement's or Pillow's, and
everything is integer-defined: the bound is zero."""
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import mjpeg_enc_ref as E
import mjpeg_ref

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")

SETS = E.coef_sets()
CANARY, FILL, OUT_CANARY = 256, 0xA5, 0xC3


def pillow(jpeg, mode="RGB"):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert(mode))


class EncStages:
    """A workspace of `vdx_mjpeg_enc_workspace` bytes with 256 canary bytes behind it, and the four entry points called one at a
    time.  The workspace starts as 0xA5 throughout: a stage that relies on memory it did not write shows."""

    def __init__(self, gpu, F, W, H, layout):
        from vdx import _lib, video
        self.lib, self.check, self.video = _lib.load(), _lib.check, video
        self.gpu, self.F, self.W, self.H, self.layout = gpu, F, W, H, layout
        self.geo = mjpeg_ref._geometry(W, H, layout)
        self.ncomp, self.nmcu, self.bpf = self.geo[0], self.geo[1] * self.geo[2], self.geo[6][-1]
        self.nbytes = self.lib.vdx_mjpeg_enc_workspace(F, W, H, layout)
        assert self.nbytes > 0
        offs = (ctypes.c_size_t * 6)()
        self.check(self.lib.vdx_mjpeg_enc_offsets(F, W, H, layout, offs), "vdx_mjpeg_enc_offsets")
        self.at = dict(zip(video.ENC_STAGES, offs))
        assert list(offs) == sorted(offs) and offs[5] + F * self.bpf * E.SLOT_BYTES <= self.nbytes
        self.buf = torch.full((self.nbytes + CANARY,), FILL, dtype=torch.uint8, device=gpu)
        assert self.buf.data_ptr() % 16 == 0
        self.tables = torch.from_numpy(video.encoder_tables()).to(gpu)
        self.lengths = torch.full((F,), -1, dtype=torch.int32, device=gpu)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.args = (F, W, H, layout)

    def _section(self, name, nbytes):
        return self.buf[self.at[name]:self.at[name] + nbytes]

    def _upload(self, name, arr):
        flat = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self._section(name, flat.size).copy_(torch.from_numpy(flat).to(self.gpu))

    # ---- uploads in the restatement's shapes
    def set_planes(self, planes):
        F, boff = self.F, self.geo[6]
        flat = np.concatenate([np.asarray(p, np.uint8).reshape(F, -1) for p in planes], 1)
        assert flat.shape == (F, self.bpf * 64) and all(p.shape[1] * p.shape[2] == (boff[c + 1] - boff[c]) * 64 for c, p in enumerate(planes))
        self._upload("planes", flat)

    def set_coef(self, coef):
        coef = np.asarray(coef, np.int16)
        assert coef.shape == (self.F, self.bpf, 64)
        self._upload("coef", coef)

    # ---- the stages
    def color(self, frames):
        assert frames.is_contiguous() and frames.dtype == torch.uint8 and tuple(frames.shape[:3]) == (self.F, self.H, self.W)
        self.check(self.lib.vdx_mjpeg_enc_color(frames.data_ptr(), *self.args, self.buf.data_ptr(), self.stream), "vdx_mjpeg_enc_color")
        return self.planes()

    def fdct(self, quant_u16):
        q = torch.from_numpy(np.ascontiguousarray(quant_u16, np.uint16).reshape(2, 64).view(np.int16)).to(self.gpu)
        self.check(self.lib.vdx_mjpeg_enc_fdct(q.data_ptr(), *self.args, self.buf.data_ptr(), self.stream), "vdx_mjpeg_enc_fdct")
        return self.coef()

    def entropy(self, dri, header_bytes):
        self.check(self.lib.vdx_mjpeg_enc_entropy(self.tables.data_ptr(), *self.args, dri, header_bytes, self.buf.data_ptr(),
                                                  self.lengths.data_ptr(), self.stream), "vdx_mjpeg_enc_entropy")
        return self.lengths.cpu().numpy()

    def pack(self, header, dri, out_bytes=None):
        """-> the first `out_bytes` bytes (default: all) of a buffer with 64 canary bytes behind the packed frames; what lies
        behind `out_bytes` is kept in `self.behind`."""
        total = int(self.lengths.cpu().numpy().astype(np.int64).sum())
        out_bytes = total if out_bytes is None else out_bytes
        head = torch.from_numpy(np.frombuffer(header, np.uint8).copy()).to(self.gpu)
        out = torch.full((total + 64,), OUT_CANARY, dtype=torch.uint8, device=self.gpu)
        self.check(self.lib.vdx_mjpeg_enc_pack(head.data_ptr(), len(header), *self.args, dri, self.buf.data_ptr(), self.lengths.data_ptr(),
                                               out.data_ptr(), out_bytes, self.stream), "vdx_mjpeg_enc_pack")
        data = out.cpu().numpy()
        self.behind = data[out_bytes:]
        return data[:out_bytes].tobytes()

    # ---- readers
    def _read(self, name, nbytes):
        return self._section(name, nbytes).cpu().numpy()

    def planes(self):
        ncomp, _, _, _, bw, bh, boff = self.geo
        flat = self._read("planes", self.F * self.bpf * 64).reshape(self.F, self.bpf * 64)
        return [flat[:, boff[c] * 64:boff[c + 1] * 64].reshape(self.F, bh[c] * 8, bw[c] * 8) for c in range(ncomp)]

    def coef(self):
        return self._read("coef", self.F * self.bpf * 128).view(np.int16).reshape(self.F, self.bpf, 64)

    def bits(self):
        return self._read("bits", self.F * self.bpf * 4).view(np.uint32).reshape(self.F, self.bpf)

    def segbits(self):
        return self._read("segbits", self.F * self.nmcu * 4).view(np.uint32).reshape(self.F, self.nmcu)

    def slots(self):
        return self._read("slots", self.F * self.bpf * 4).view(np.uint32).reshape(self.F, self.bpf)

    def raw(self):
        """-> uint8 [F][bpf * 208]: the words hold the stream MSB first."""
        words = self._read("raw", self.F * self.bpf * E.SLOT_BYTES).view(np.uint32)
        return words.byteswap().view(np.uint8).reshape(self.F, self.bpf * E.SLOT_BYTES)

    def check_canary(self):
        tail = self.buf[self.nbytes:].cpu().numpy()
        assert tail.size == CANARY and (tail == FILL).all(), f"{int((tail != FILL).sum())} bytes behind the workspace were written"

    # ---- the reader's entropy stage on frames this writer produced
    def read_back(self, jpegs):
        blob, off, info, _ = self.video.plan(jpegs)
        up = torch.from_numpy(blob).to(self.gpu)
        ptr = {k: up.data_ptr() + v[0] for k, v in off.items()}
        F, nseg = info["n_frames"], info["n_segments"]
        ws = torch.zeros(self.lib.vdx_mjpeg_workspace(F, self.W, self.H, self.layout), dtype=torch.uint8, device=self.gpu)
        err = torch.full((nseg,), 0x5A5A5A5A, dtype=torch.int32, device=self.gpu)
        self.check(self.lib.vdx_mjpeg_entropy(ptr["data"], off["data"][1], ptr["seg_off"], ptr["segs"], nseg, info["max_segments_per_frame"],
                                              ptr["huff"], ptr["sel"], F, self.W, self.H, self.layout, ws.data_ptr(), err.data_ptr(),
                                              self.stream), "vdx_mjpeg_entropy")
        return ws[:F * self.bpf * 128].cpu().numpy().view(np.int16).reshape(F, self.bpf, 64), err.cpu().numpy()


def _stage_sections(stages, F, W, H, layout):
    ncomp, mcux, mcuy, hs, bw, bh, boff = mjpeg_ref._geometry(W, H, layout)
    bpf = boff[-1]
    flat = stages["planes"][:F * bpf * 64].reshape(F, bpf * 64)
    planes = [flat[:, boff[c] * 64:boff[c + 1] * 64].reshape(F, bh[c] * 8, bw[c] * 8) for c in range(ncomp)]
    return planes, stages["coef"][:F * bpf * 128].view(np.int16).reshape(F, bpf, 64)


# ---------------------------------------------------------------------------------------------
# 1, 2, 7: the whole encoder, at every quality, on narrow and short frames, on many frames
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_every_quality_is_pillows(gpu, quality):
    from vdx import video
    for kind in E.KINDS:
        for W, H in E.SWEEP_SIZES:
            for mode in E.MODES:
                img = E.content(kind, W, H, mode)
                frames = torch.from_numpy(img[None]).to(gpu)
                for rr in (0, 1):
                    got, want = {}, {}
                    jpeg = video.encode_frames(frames, quality=quality, restart_rows=rr, _stages=got)[0]
                    assert jpeg == E.pillow_encode(img, rr, quality), (kind, W, H, mode, rr)
                    if quality in (1, 100):
                        assert E.encode(img[None], quality, rr, stages=want)[0] == jpeg
                        planes, coef = _stage_sections(got, 1, W, H, 2 if mode == "RGB" else 0)
                        for c, (a, b) in enumerate(zip(planes, want["planes"])):
                            assert np.array_equal(a, b), f"stage 1, component {c}: {(kind, W, H, mode, rr)}"
                        assert np.array_equal(coef, want["coef"]), f"stage 2: {(kind, W, H, mode, rr)}"


def test_narrow_and_short_frames(gpu):
    """Every W in 1 .. 33 at H in (1, 9, 16) and every H in 1 .. 33 at W in (1, 9, 16): the colour kernel's pair of luma samples
    and the grey kernel's four with their clamps, a cut row pair, dummy block rows and columns."""
    from vdx import video
    sizes = sorted({(W, H) for W in range(1, 34) for H in (1, 9, 16)} | {(W, H) for H in range(1, 34) for W in (1, 9, 16)})
    assert len(sizes) == 189
    bad = []
    for W, H in sizes:
        for mode in E.MODES:
            img = E.content("noise", W, H, mode, seed=5)
            if video.encode_frames(torch.from_numpy(img[None]).to(gpu), restart_rows=1)[0] != E.pillow_encode(img, 1):
                bad.append((W, H, mode))
    assert not bad, bad


def test_many_short_frames(gpu):
    """300 frames of 16 x 16: the packing kernel's sum over the frames before its own, up to f = 299."""
    from vdx import video
    clip = np.stack([E.content(E.KINDS[i % 4], 16, 16, "RGB", seed=i) for i in range(300)])
    frames = torch.from_numpy(clip).to(gpu)
    for rr in (0, 1):
        want = [E.pillow_encode(f, rr) for f in clip]
        got = video.encode_frames(frames, restart_rows=rr)
        assert len(got) == 300 and [len(j) for j in got] == [len(j) for j in want]
        assert sum(len(j) for j in got) == len(b"".join(want))
        assert len({len(j) for j in want}) >= 8, "the frames' lengths vary: no offset is a multiple of one length"
        assert got == want, [i for i in range(300) if got[i] != want[i]][:8]


# ---------------------------------------------------------------------------------------------
# 3: stage 1 on every input
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _every_triple():
    """-> uint32 [2^24]: every RGB triple (r << 16 | g << 8 | b) once, in a seeded order."""
    return np.random.default_rng(2024).permutation(1 << 24).astype(np.uint32)


def _fix(x):
    return int(round(x * 65536))


@pytest.mark.parametrize("strip", range(4))
def test_colour_conversion_of_every_triple(gpu, strip):
    """A 4096 x 4096 frame that holds each of the 2^24 triples once, in four strips of 1024 rows (the cost is the reference's, on
    the CPU).  The expected planes are computed here in int64 from the decimal constants of the JFIF conversion and must also
    be the restatement's."""
    W, H = 4096, 1024
    t = _every_triple()[strip * W * H:(strip + 1) * W * H].reshape(H, W)
    frame = np.stack([t >> 16, (t >> 8) & 255, t & 255], -1).astype(np.uint8)
    if strip == 0:
        assert np.array_equal(np.sort(_every_triple()), np.arange(1 << 24, dtype=np.uint32))
    r, g, b = (frame[..., k].astype(np.int64) for k in range(3))
    y = (_fix(0.299) * r + _fix(0.587) * g + _fix(0.114) * b + 32768) >> 16
    off = (128 << 16) + 32767
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + off) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + off) >> 16
    assert _fix(0.299) + _fix(0.587) + _fix(0.114) == 65536
    bias = 1 + (np.arange(W // 2) & 1)                                              # 1, 2, 1, 2, ...
    down = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (cb, cr)]
    want = [a.astype(np.uint8)[None] for a in [y] + down]
    assert all(0 <= a.min() and a.max() <= 255 for a in [y] + down)
    ref = E.planes(frame[None], 2)
    for c in range(3):
        assert np.array_equal(want[c], ref[c]), f"the restatement's component {c} is not the formula's"
    st = EncStages(gpu, 1, W, H, 2)
    got = st.color(torch.from_numpy(frame[None]).to(gpu))
    for c in range(3):
        assert got[c].shape == want[c].shape and np.array_equal(got[c], want[c]), f"component {c}: {int((got[c] != want[c]).sum())} differ"
    st.check_canary()


def test_grey_pack_of_every_value_at_every_column_phase(gpu):
    """The grey kernel packs four samples per thread and clamps each column: every value at every x mod 4, at a width that is no
    multiple of 4 or 8, over a bottom edge that replicates rows, in two frames."""
    W, H = 1027, 5
    yy, xx = np.mgrid[0:H, 0:W]
    a = ((xx // 4 + 67 * (xx % 4) + 31 * yy) % 256).astype(np.uint8)
    for phase in range(4):
        assert len(np.unique(a[0, phase::4])) == 256
    clip = np.stack([a, 255 - a[::-1, ::-1]])
    st = EncStages(gpu, 2, W, H, 0)
    got = st.color(torch.from_numpy(clip).to(gpu))
    want = E.planes(clip, 0)
    assert got[0].shape == (2, 8, 1032) and np.array_equal(got[0], want[0])
    assert np.array_equal(want[0][:, :H, :W], clip) and (want[0][:, :, W:] == want[0][:, :, W - 1:W]).all()
    st.check_canary()
    for W in (1, 2, 3, 5, 6, 7):                                                    # fewer samples than a thread packs
        clip = E.content("noise", W, 3, "L", seed=W)[None]
        st = EncStages(gpu, 1, W, 3, 0)
        assert np.array_equal(st.color(torch.from_numpy(clip).to(gpu))[0], E.planes(clip, 0)[0]), W
        st.check_canary()


# ---------------------------------------------------------------------------------------------
# 4: stage 2 at the extremes
# ---------------------------------------------------------------------------------------------
def _tables():
    from vdx import video
    return {"quality 100": video.quant_tables(100), "all 1": np.ones((2, 64), np.int64), "all 255": np.full((2, 64), 255),
            "quality 50": video.quant_tables(50), "quality 1": video.quant_tables(1)}


def test_fdct_of_the_basis_blocks(gpu):
    """The 0 / 255 sign pattern of every basis function, grey: the largest coefficients 8-bit samples give, with the smallest
    and the largest divisor.  The restatement computes in int64: a wrapped int32 on the device would differ."""
    img = E.basis_image("L")
    H, W = img.shape
    pl = E.planes(img[None], 0)
    st = EncStages(gpu, 1, W, H, 0)
    for name, q in _tables().items():
        st.set_planes(pl)
        want = E.coefficients(pl, q, W, H, 0)
        got = st.fdct(q)
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} coefficients differ"
        if name == "all 1":
            assert np.abs(want[..., 1:].astype(np.int64)).max() == 1020 and (want[..., 0].min(), want[..., 0].max()) == (-1024, 1016)
    st.check_canary()


def test_fdct_of_the_basis_blocks_in_420_with_dummy_blocks(gpu):
    """24 x 40 in 4:2:0: the luma plane is 4 x 6 blocks of which 3 x 5 are real.  Every block of every component is a basis
    block; a dummy block keeps the DC of the block `source_block` names and no AC."""
    W, H, F = 24, 40, 22
    pl = E.basis_planes(W, H, 2, F)
    st = EncStages(gpu, F, W, H, 2)
    ncomp, mcux, mcuy, hs, bw, bh, boff = st.geo
    for name, q in _tables().items():
        st.set_planes(pl)
        want = E.coefficients(pl, q, W, H, 2)
        got = st.fdct(q)
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} coefficients differ"
        dummies = 0
        for by in range(bh[0]):
            for bx in range(bw[0]):
                sy, sx = E.source_block(by, bx, 5, 3)
                if (sy, sx) != (by, bx):
                    dummies += 1
                    assert not got[:, by * bw[0] + bx, 1:].any() and np.array_equal(got[:, by * bw[0] + bx, 0], got[:, sy * bw[0] + sx, 0])
        assert dummies == 9
        if name == "all 1":                                                         # chroma blocks are never dummies
            assert (np.abs(got[:, boff[1]:].astype(np.int64)).max(-1) > 0).all() and np.abs(got[:, boff[1]:, 1:].astype(np.int64)).max() == 1020
    st.check_canary()


def test_the_basis_image_is_pillows_at_quality_100(gpu):
    """End to end: DC differences of size 11 and |AC| = 1020 from samples."""
    from vdx import video
    for mode in E.MODES:
        img = E.basis_image(mode)
        for rr in (0, 1):
            assert video.encode_frames(torch.from_numpy(img[None]).to(gpu), quality=100, restart_rows=rr)[0] == E.pillow_encode(img, rr, 100)


# ---------------------------------------------------------------------------------------------
# 5: stages 3 and 4 on coefficients
# ---------------------------------------------------------------------------------------------
def _expected(entry, header):
    """-> per frame: bit offsets of the blocks within their segment, bits per segment, slot offsets, raw bytes, file bytes."""
    layout, W, H, coef, dri = entry
    raws, lengths, step = E.segments(coef, W, H, layout, dri)
    n = len(lengths)
    bits = np.concatenate([np.cumsum([0] + lengths[s:s + step][:-1]) for s in range(0, n, step)])
    segbits = np.asarray([sum(lengths[s:s + step]) for s in range(0, n, step)])
    slots = np.asarray(E.slots_of(raws, step, n))
    raw = np.zeros(n * E.SLOT_BYTES, np.uint8)
    for si, r in enumerate(raws):
        raw[si * step * E.SLOT_BYTES:si * step * E.SLOT_BYTES + len(r)] = np.frombuffer(r, np.uint8)
    return bits, segbits, slots, raw, header + E.entropy(coef, W, H, layout, dri)[0] + b"\xff\xd9"


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("name", sorted(SETS))
def test_entropy_and_pack_of_coefficient_sets(gpu, name, F):
    from vdx import video
    entry = SETS[name]
    layout, W, H, coef, dri = entry
    header, _, jpeg, _ = E.coef_stream(entry)
    bits, segbits, slots, raw, want = _expected(entry, header)
    assert want == jpeg
    st = EncStages(gpu, F, W, H, layout)
    st.set_coef(np.stack([coef] * F))
    lengths = st.entropy(dri, len(header))
    for f in range(F):
        assert np.array_equal(st.bits()[f], bits), f"frame {f}: bit offsets of the blocks"
        assert np.array_equal(st.segbits()[f, :len(segbits)], segbits), f"frame {f}: bits of the segments"
        got_slots = st.slots()[f]
        assert np.array_equal(got_slots, np.cumsum(slots) - slots), f"frame {f}: offsets of the slots"
        counts = np.diff(np.append(got_slots.astype(np.int64), int(lengths[f]) - len(header) - 2))
        assert np.array_equal(counts, slots), f"frame {f}: stuffed bytes of the slots"
        assert np.array_equal(st.raw()[f], raw), f"frame {f}: the unstuffed stream"
    assert lengths.tolist() == [len(jpeg)] * F
    packed = st.pack(header, dri)
    assert (st.behind == OUT_CANARY).all()
    assert packed == jpeg * F
    st.check_canary()
    # the reader finds the coefficients that went in, and decodes what lies in its domain as Pillow does
    back, err = st.read_back([jpeg] * F)
    assert not err.any() and np.array_equal(back, np.stack([coef] * F))
    if E.in_reader_domain(entry):
        frames = video.read_frames([packed[i * len(jpeg):(i + 1) * len(jpeg)] for i in range(F)], device=gpu)[0].cpu().numpy()
        assert np.array_equal(frames, np.stack([pillow(jpeg, "RGB" if layout else "L")] * F))
    else:
        assert name.startswith(("max-bits", "all-ones"))
        with pytest.raises(video.VdxError, match="outside the range of 8-bit samples"):
            video.read_frames([jpeg], device=gpu)


# ---------------------------------------------------------------------------------------------
# 6: the guards
# ---------------------------------------------------------------------------------------------
def test_pack_stores_nothing_at_or_behind_out_bytes(gpu):
    for name in ("all-ones", "rst-wrap", "zrl-420"):
        layout, W, H, coef, dri = SETS[name]
        header, _, jpeg, _ = E.coef_stream(SETS[name])
        st = EncStages(gpu, 2, W, H, layout)
        st.set_coef(np.stack([coef] * 2))
        assert st.entropy(dri, len(header)).tolist() == [len(jpeg)] * 2
        total = 2 * len(jpeg)
        got = st.pack(header, dri, out_bytes=total - 7)
        assert got == (jpeg * 2)[:total - 7]
        assert st.behind.size == 64 + 7 and (st.behind == OUT_CANARY).all()
        st.check_canary()


def test_what_the_encoder_refuses(gpu):
    """The sizes `mje_args` turns away: the workspace query answers 0 (it is host code: sizes only), every entry point fails,
    and `encode_frames` raises before it allocates (the frames here are views of a few bytes)."""
    from vdx import _lib, video
    lib = _lib.load()
    ws = lib.vdx_mjpeg_enc_workspace
    assert ws(1, 16, 16, 0) > 0 and ws(1, 16, 16, 2) > 0 and ws(65535, 8, 8, 0) > 0
    assert ws(1, 16, 16, 1) == 0 and ws(1, 16, 16, 3) == 0 and ws(1, 16, 16, -1) == 0
    assert ws(0, 16, 16, 0) == 0 and ws(-1, 16, 16, 0) == 0 and ws(65536, 8, 8, 0) == 0
    assert ws(1, 0, 16, 0) == 0 and ws(1, 16, 65536, 0) == 0
    assert 65535 * 512 < 1 << 25 <= 65535 * 513                                     # F * blocks per frame
    assert ws(65535, 8 * 512, 8, 0) > 0 and ws(65535, 8 * 513, 8, 0) == 0
    assert ws(32768, 16 * 171, 16, 2) == 0 and ws(32768, 16 * 170, 16, 2) > 0       # 6 blocks per MCU
    assert 8192 * 157 * 1664 < 1 << 31 <= 8192 * 158 * 1664                         # bits of a frame's slots
    assert ws(1, 65535, 8 * 157, 0) > 0 and ws(1, 65535, 8 * 158, 0) == 0
    offs = (ctypes.c_size_t * 6)()
    buf = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    p, stream = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    for args in ((1, 16, 16, 1), (0, 16, 16, 0), (65536, 8, 8, 0), (65535, 8 * 513, 8, 0), (1, 65535, 8 * 158, 0)):
        assert lib.vdx_mjpeg_enc_offsets(*args, offs) != 0
        assert lib.vdx_mjpeg_enc_color(p, *args, p, stream) != 0
        assert lib.vdx_mjpeg_enc_fdct(p, *args, p, stream) != 0
        assert lib.vdx_mjpeg_enc_entropy(p, *args, 0, 100, p, p, stream) != 0
        assert lib.vdx_mjpeg_enc_pack(p, 100, *args, 0, p, p, p, 4096, stream) != 0
        with pytest.raises(video.VdxError, match="outside what the encoder takes"):
            _lib.check(lib.vdx_mjpeg_enc_offsets(*args, offs), "vdx_mjpeg_enc_offsets")
    torch.cuda.synchronize()
    assert not buf.any()
    one = torch.zeros((1, 1, 1), dtype=torch.uint8, device=gpu)
    for shape in ((65536, 1, 1), (65535, 8, 8 * 513), (1, 8 * 158, 65535)):
        with pytest.raises(video.VdxError, match="outside what the encoder takes"):
            video.encode_frames(one.expand(*shape))
    rgb = torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=gpu)
    with pytest.raises(video.VdxError, match="outside what the encoder takes"):
        video.encode_frames(rgb.expand(32768, 16, 16 * 171, 3))
    with pytest.raises(video.VdxError):
        video.encode_frames(one.expand(1, 16, 16), sampling="4:4:4")                # layout 1 is not written
    with pytest.raises(video.VdxError):
        video.encode_frames(one[:0])                                                # F = 0
