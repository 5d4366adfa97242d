"""Host-side op wrappers: torch device tensors -> pointers/sizes -> libvdx_hip.so.

Every wrapper validates shapes/strides/alignment on the host before a kernel is enqueued
(a bad shape must raise here, never fault on the device).  Kernels run on torch's current
HIP stream.  All tensors are fp16 CUDA(=HIP) tensors whose last dimension is contiguous;
activations are channels-last row matrices [pixels][channels].
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import GemmArgs, VdxError
from .frames import is_packed

PLAIN, CONV3X3, TCONV3 = 0, 1, 2
EPI_GEGLU = 1


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor], name: str, dtype=torch.float16) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise VdxError(f"{name}: expected a GPU tensor (the denoising path has no CPU fallback)")
    if t.dtype != dtype:
        raise VdxError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise VdxError(f"{name}: last dimension must be contiguous")
    if t.data_ptr() % 16 != 0:
        raise VdxError(f"{name}: pointer not 16-byte aligned")
    return t.data_ptr()


def _rows(t: torch.Tensor, name: str):
    if t.dim() != 2:
        raise VdxError(f"{name}: expected a 2-D row matrix, got shape {tuple(t.shape)}")
    return t.shape[0], t.shape[1], t.stride(0)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _launch(symbol: str, *args) -> None:
    """Enqueue `symbol`(*args) on torch's current stream; a failure raises VdxError labelled with `symbol`."""
    _lib.check(getattr(_lib.load(), symbol)(*args, _stream()), symbol)


@contextlib.contextmanager
def _timed(name: Optional[str], flops: float, shape: tuple):
    """bench.py instrumentation around one launch: with PROFILE set and `name` profiled, HIP events on the launch stream
    just before and after the body, appended to PROFILE as (name, algorithmic FLOPs, start, end, shape)."""
    if PROFILE is None or not _profiled(name):
        yield
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    yield
    ev1.record()
    PROFILE.append((name, flops, ev0, ev1, shape))


def _covers(t, rows: int, cols: int, what: str, name: str, rows_per_row: int = 1) -> int:
    """Row stride of the optional row matrix `t` (0 without one), which must cover [rows][cols] of the product when each
    of its rows serves `rows_per_row` product rows (bias2: one time-embedding row per sample)."""
    if t is None:
        return 0
    r, c, ld = _rows(t, name)
    if rows_per_row <= 0 or r * rows_per_row < rows or c < cols:
        raise VdxError(f"{what}: {name} {tuple(t.shape)} does not cover [{rows}][{cols}]")
    return ld


def _out(out, rows: int, cols: int, like: torch.Tensor, what: str):
    """-> (out, ldo): `out`, or a new fp16 [rows][cols] on `like`'s device; a given `out` must cover [rows][cols]."""
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float16, device=like.device)
    return out, _covers(out, rows, cols, what, "out")


def check_u8_frames(frames, what):
    """-> (F, H, W) of a uint8 RGB clip the u8 kernels can read where it lies (vdx/frames.py `is_packed`); `VdxError` otherwise."""
    if not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise VdxError(f"{what}: expected uint8 (F, H, W, 3) frames on the GPU, got {frames.dtype} {tuple(frames.shape)}")
    F, H, W, _ = frames.shape
    if F == 0 or H == 0 or W == 0:
        raise VdxError(f"{what}: empty frames")
    if not is_packed(frames):
        raise VdxError(f"{what}: pixels must be packed RGB with non-overlapping rows and frames")
    return F, H, W


def _u8_args(frames):
    """(pointer, frame pitch, row pitch) of a checked clip, the leading arguments of every u8 entry point; zeros for None."""
    return (frames.data_ptr(), frames.stride(0), frames.stride(1)) if frames is not None else (None, 0, 0)


def _packed(blob, nbytes: int, what: str, packer: str) -> None:
    """A fused block's weight blob must be contiguous fp16 of exactly the kernel's `nbytes` (the layout `packer` builds)."""
    if blob.dtype != torch.float16 or blob.numel() * 2 != nbytes or not blob.is_contiguous():
        raise VdxError(f"{what} does not match the kernel's layout ({packer})")


# --------------------------------------------------------------------------------------------
_KSPLIT_WS: dict = {}   # fp32 partial slabs of the split-K tails
_GN_WS: dict = {}       # GroupNorm statistics (vdx_groupnorm_workspace_part)


def _scratch(pool: dict, device, nbytes: int, dtype: torch.dtype, minimum: int = 0) -> torch.Tensor:
    """A workspace of at least `nbytes` from `pool`: one buffer per (device, stream), grown on demand to
    max(nbytes, minimum) bytes.  A kernel and the launch that reads what it left there are ordered by ONE stream, so two
    streams must not share a buffer."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = pool.get(key)
    if ws is None or ws.numel() * ws.element_size() < nbytes:
        ws = pool[key] = torch.empty(-(-max(nbytes, minimum) // dtype.itemsize), dtype=dtype, device=device)
    return ws


def groupnorm_linear_supported(C: int, N: int, rows_per_sample: int) -> bool:
    """Shapes `groupnorm_linear` folds (the weights-stationary GEMM families with a weight set per sample)."""
    return C in (320, 640) and N % 32 == 0 and rows_per_sample % 64 == 0


def groupnorm_linear(x, gamma, beta, w, bias, *, groups, n_samples, rows_per_sample, eps, partition_samples=0, out=None):
    """Linear(GroupNorm(x)) without the normalised tensor (`norm` -> `proj_in` of the transformer blocks): the statistics
    pass, then one weight matrix + fp32 bias per sample (`vdx_groupnorm_fold_linear_f16`), then the weights-stationary GEMM
    on the raw rows with `wset_rows = rows_per_sample`."""
    r, Cc, ldx = _rows(x, "x")
    M = n_samples * rows_per_sample
    N, K = w.shape
    if r < M or K != Cc or gamma.numel() != Cc or beta.numel() != Cc:
        raise VdxError(f"groupnorm_linear: x [{r}][{Cc}], w [{N}][{K}], gamma {gamma.numel()}: shapes do not match")
    if not groupnorm_linear_supported(Cc, N, rows_per_sample) or not w.is_contiguous():
        raise VdxError(f"groupnorm_linear: C={Cc}, N={N}, rows_per_sample={rows_per_sample} not supported")
    need = _lib.load().vdx_groupnorm_workspace_part(n_samples, rows_per_sample, Cc, groups, partition_samples)
    ws = _scratch(_GN_WS, x.device, need, torch.uint8, 1 << 20)
    w_s = torch.empty((n_samples * N, K), dtype=torch.float16, device=x.device)
    b_s = torch.empty((n_samples, N), dtype=torch.float32, device=x.device)
    _launch("vdx_groupnorm_fold_linear_f16", _p(x, "x"), Cc, ldx, _p(gamma, "gamma"), _p(beta, "beta"), float(eps), groups,
            n_samples, rows_per_sample, ws.data_ptr(), partition_samples, _p(w, "w"), _p(bias, "bias"), N, w_s.data_ptr(),
            b_s.data_ptr())
    return gemm(x, w_s, M=M, wset_rows=rows_per_sample, wset_bias=b_s, out=out)


def gemm(a, w, *, M, mode=PLAIN, a2=None, bias=None, bias2=None, rows_per_bias2=0, residual=None,
         out=None, geglu=False, conv=None, tconv=None, variant=0, row_begin=0, row_end=0, allow_ksplit=False, ksplit=0,
         wset_rows=0, wset_bias=None, pad_mode=0):
    """out[M][N] = epi(gather(a|a2)[M][K] @ w[N][K]^T).  See include/vdx.h `vdx_gemm_args`.
    `pad_mode=1` (conv3x3, stride 2): zero padding (0,1,0,1) — diffusers Downsample2D(padding=0); h_out = h_in // 2.
    `allow_ksplit`: the tail of the product (less than half a round of big tiles) may run as K slices + a fixed-order
    reduction (vdx_gemm_plan_ksplit) — faster on the 16-frame windows, not bit-identical to the unsplit order (the
    callers that rely on row-split bit-identity do not pass it).  `ksplit`: pin it for rows [row_begin, row_end).
    `wset_rows` / `wset_bias`: one weight set per `wset_rows` rows, w = [M / wset_rows][N][K] and an fp32 bias per set
    (a GroupNorm folded into the Linear: `groupnorm_linear`).
    `conv=(..., stride, upsample)` with upsample 3: nearest x2 in phase form — `w` is packing.pack_upconv_phase's
    [4 * N][4 * c1] table; row ranges and the plan's split count its 4 * round_up(M / 4, 256) virtual rows (vdx.h)."""
    ar, c1, lda = _rows(a, "a")
    N, K = w.shape
    phase = mode == CONV3X3 and int(conv[6]) == 3
    if phase:
        if N % 4:
            raise VdxError("gemm: the phase form (upsample 3) takes a [4 * N][4 * c1] table")
        N //= 4
    if wset_rows:
        if M % wset_rows or N % (M // wset_rows) or wset_bias is None or wset_bias.dtype != torch.float32:
            raise VdxError("gemm: wset_rows needs M % wset_rows == 0, w = [sets * N][K] and an fp32 wset_bias [sets][N]")
        N //= M // wset_rows
        if wset_bias.numel() != (M // wset_rows) * N or not wset_bias.is_contiguous():
            raise VdxError("gemm: wset_bias must be contiguous [sets][N]")
    if not w.is_contiguous():
        raise VdxError("w: must be contiguous [N][K]")
    c2 = 0
    g = GemmArgs()
    if a2 is not None:
        a2r, c2, lda2 = _rows(a2, "a2")
        g.lda2 = lda2
    taps = 4 if phase else {PLAIN: 1, CONV3X3: 9, TCONV3: 3}[mode]
    if K != taps * (c1 + c2):
        raise VdxError(f"gemm: K={K} != {taps}*(c1={c1}+c2={c2})")
    n_out = N // 2 if geglu else N
    # rows each operand must provide
    if mode == PLAIN:
        need_rows = M
    elif mode == CONV3X3:
        n_img, h_in, w_in, h_out, w_out, stride, ups = conv
        if M != n_img * h_out * w_out:
            raise VdxError(f"gemm: M={M} != n_img*h_out*w_out={n_img * h_out * w_out}")
        need_rows = n_img * h_in * w_in
        g.h_in, g.w_in, g.h_out, g.w_out, g.stride, g.upsample = h_in, w_in, h_out, w_out, stride, int(ups)
    else:
        frames, hw = tconv
        if M % (frames * hw) != 0:
            raise VdxError(f"gemm: M={M} is not a whole number of (frames={frames} x hw={hw}) clips")
        need_rows = M
        g.frames, g.hw = frames, hw
    if ar < need_rows or (a2 is not None and a2r < need_rows):
        raise VdxError(f"gemm: source has {ar} rows, kernel would read {need_rows}")
    out, ldo = _out(out, M, n_out, a, "gemm")
    if bias is not None and bias.numel() != N:
        raise VdxError(f"gemm: bias has {bias.numel()} elements, N={N}")
    g.ldb2 = _covers(bias2, M, N, "gemm", "bias2", rows_per_bias2)
    g.rows_per_bias2 = rows_per_bias2 if bias2 is not None else 0
    g.ldr = _covers(residual, M, N, "gemm", "residual")
    g.a, g.a2, g.w = _p(a, "a"), _p(a2, "a2"), _p(w, "w")
    g.bias, g.bias2, g.residual, g.out = _p(bias, "bias"), _p(bias2, "bias2"), _p(residual, "residual"), _p(out, "out")
    g.M, g.N, g.K, g.mode, g.c1, g.c2 = M, N, K, mode, c1, c2
    g.lda, g.ldo = lda, ldo
    g.pad_mode = int(pad_mode)
    g.epilogue = (EPI_GEGLU if geglu else 0) | ((variant & 15) << 8)   # variant: kernel override (tests/tuning)
    if wset_rows:
        g.wset_rows, g.wset_bias = wset_rows, wset_bias.data_ptr()
    # One product, up to two launches: whole rounds of 256 big tiles, then the rest on whatever tile suits it
    # (vdx_gemm_plan; the bits do not depend on the split).  A pinned variant or an explicit row range is left alone.
    spans = [(row_begin, row_end, ksplit)]
    if variant == 0 and row_begin == 0 and row_end == 0 and ksplit == 0 and not wset_rows:
        key = (M, N, K, mode, geglu, a2 is not None, bias2 is not None, allow_ksplit, int(g.upsample))      # everything the plan depends on
        if pad_mode:
            key += (int(pad_mode),)
        plan_ = _PLAN_CACHE.get(key)
        if plan_ is None:
            v_, split_, ks_, wsb_ = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_size_t(0)
            lib = _lib.load()           # host-only queries: no stream
            if allow_ksplit:
                _lib.check(lib.vdx_gemm_plan_ksplit(C.byref(g), C.byref(split_), C.byref(ks_), C.byref(wsb_)), "vdx_gemm_plan_ksplit")
            if ks_.value == 0:
                _lib.check(lib.vdx_gemm_plan(C.byref(g), C.byref(v_), C.byref(split_)), "vdx_gemm_plan")
            plan_ = _PLAN_CACHE[key] = (split_.value, ks_.value, wsb_.value)
        split, ks, wsb = plan_
        if split:
            spans = [(0, split, 0), (split, 0, ks)]
    elif ksplit > 1:
        nt = -(-((row_end or M) - row_begin) // 256) * -(-N // 320)
        wsb = nt * ksplit * 327680
    for rb, re_, ks in spans:
        g.row_begin, g.row_end, g.ksplit, g.workspace, g.workspace_bytes = rb, re_, ks, None, 0
        if ks > 1:
            ws_ = _scratch(_KSPLIT_WS, out.device, wsb, torch.float32)
            g.workspace, g.workspace_bytes = ws_.data_ptr(), ws_.numel() * 4
        rows = (re_ or (4 * round_up(M // 4, 256) if phase else M)) - rb
        name = _gemm_name(g) if PROFILE is not None else None     # only asked for when bench.py profiles
        with _timed(name, 2.0 * rows * N * K, (rows, N, K)):
            _launch("vdx_gemm_f16", C.byref(g))
    return out


_PLAN_CACHE = {}
PROFILE = None   # set to a list by bench.py to collect (kernel name, algorithmic FLOPs, start, end)
PROFILE_ONLY = None   # with PROFILE set: only launches whose kernel name contains one of these strings get events (None: all)


def _profiled(name: str) -> bool:
    return PROFILE_ONLY is None or any(s_ in name for s_ in PROFILE_ONLY)


def _gemm_name(g: GemmArgs) -> str:
    """vdx_gemm_kernel_name: the instantiation vdx_gemm_f16(g) would launch, named by the library's own dispatch."""
    buf = C.create_string_buffer(128)
    _lib.check(_lib.load().vdx_gemm_kernel_name(C.byref(g), buf, len(buf)), "vdx_gemm_kernel_name")
    return buf.value.decode()


def gemm_kernel_name(M: int, N: int, K: int, mode: int, geglu: bool, variant: int = 0, single_source: bool = True,
                     residual: bool = False, whole: bool = True, wset: bool = False, conv=None, tconv=None,
                     pad_mode: int = 0, ksplit: int = 0, rows=None, wset_rows: int = 0) -> str:
    """Name of the instantiation vdx_gemm_f16 launches (as rocprofv3 prints it) for M rows (`whole`: the call covers
    the whole product — the weights-stationary kernels take no row ranges).  Host-only (no GPU): a call of this shape
    with placeholder pointers, which the library tests for null and never reads, and the smallest geometry its
    validation accepts (one M x 1 picture, one one-frame clip), which the choice does not depend on.
    A call can also be spelled out as `gemm` takes it: `conv` = (n_img, h_in, w_in, h_out, w_out, stride, upsample) with
    `pad_mode`, `tconv` = (frames, hw), a pinned `ksplit`, `rows` = (row_begin, row_end) of the M rows, `wset_rows`; the
    library then validates that geometry and a call it refuses raises VdxError as `gemm` would."""
    g = GemmArgs()
    g.a = g.w = g.out = 1 << 20
    g.M, g.N, g.K, g.mode, g.ldo = M, N, K, mode, N
    g.c1 = g.lda = K // {PLAIN: 1, CONV3X3: 9, TCONV3: 3}[mode]
    g.epilogue = (EPI_GEGLU if geglu else 0) | ((variant & 15) << 8)
    if mode == CONV3X3:
        g.h_in, g.w_in, g.h_out, g.w_out, g.stride = M, 1, M, 1, 1
        if conv is not None:
            _, g.h_in, g.w_in, g.h_out, g.w_out, g.stride, ups = conv
            g.upsample = int(ups)
        g.pad_mode = int(pad_mode)
    elif mode == TCONV3:
        g.frames, g.hw = tconv if tconv is not None else (1, M)
    elif not single_source:             # a second source: 64 channels of the concat
        g.a2, g.c2, g.lda2, g.c1 = 1 << 20, 64, 64, K - 64
    if residual:
        g.residual, g.ldr = 1 << 20, N
    if wset or wset_rows:
        g.wset_rows, g.wset_bias = wset_rows or M, 1 << 20
    if ksplit:
        g.ksplit = ksplit
    if rows is not None:
        g.row_begin, g.row_end = rows
    if not whole:                       # rows [0, M) of a longer product
        g.row_end = M
        g.M = 2 * M
    return _gemm_name(g)


def conv_in(x, w, bias, out=None):
    """x (B,Cin,F,H,W) fp16 -> rows [B*F*H*W][Cout]; w [Cout][Kpad] = pack_conv3x3 zero-padded in K
    to a multiple of 64.  im2col gather (HBM-light: Cin = 4) + the MFMA GEMM."""
    B, Cin, F, H, W = x.shape
    if not x.is_contiguous():
        raise VdxError("conv_in: x must be contiguous (B,C,F,H,W)")
    Cout, Kpad = w.shape
    if Kpad % 64 != 0 or Kpad < 9 * Cin or not w.is_contiguous():
        raise VdxError("conv_in: w must be contiguous [Cout][Kpad], Kpad a multiple of 64 >= 9*Cin")
    M = B * F * H * W
    cols = torch.empty((M, Kpad), dtype=torch.float16, device=x.device)
    _launch("vdx_im2col_in_f16", _p(x, "x"), _p(cols, "cols"), B, Cin, F, H, W, Kpad)
    return gemm(cols, w, M=M, bias=bias, out=out)


def rows_to_ncfhw(rows, B, C, F, H, W, out=None):
    r, c, ld = _rows(rows, "rows")
    if r < B * F * H * W or c < C:
        raise VdxError("rows_to_ncfhw: rows too small")
    if out is None:
        out = torch.empty((B, C, F, H, W), dtype=torch.float16, device=rows.device)
    if tuple(out.shape) != (B, C, F, H, W) or not out.is_contiguous():
        raise VdxError("rows_to_ncfhw: bad out")
    _launch("vdx_rows_to_ncfhw_f16", _p(rows, "rows"), ld, _p(out, "out"), B, C, F, H, W)
    return out


def silu(x, out=None):
    if not x.is_contiguous():
        raise VdxError("silu: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    _launch("vdx_silu_f16", _p(x, "x"), _p(out, "out"), x.numel())
    return out


def timestep_embedding(t_dev, B, dim, out=None):
    """Sinusoidal embedding of ONE fp32 timestep held in device memory -> fp16 [B][dim] (include/vdx.h)."""
    if t_dev.dtype != torch.float32 or t_dev.numel() != 1:
        raise VdxError("timestep_embedding: t must be one fp32 value on the GPU")
    if out is None:
        out = torch.empty((B, dim), dtype=torch.float16, device=t_dev.device)
    _launch("vdx_timestep_embedding_f16", _p(t_dev, "t", torch.float32), _p(out, "out"), B, dim)
    return out


def gelu(x, out=None):
    if not x.is_contiguous():
        raise VdxError("gelu: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    _launch("vdx_gelu_f16", _p(x, "x"), _p(out, "out"), x.numel())
    return out


def quick_gelu(x, out=None):
    """x * sigmoid(1.702 x): CLIP ViT-B/32's MLP activation (vdx_quick_gelu_f16)."""
    if not x.is_contiguous():
        raise VdxError("quick_gelu: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape or not out.is_contiguous():
        raise VdxError("quick_gelu: out must be contiguous and shaped like x")
    _launch("vdx_quick_gelu_f16", _p(x, "x"), _p(out, "out"), x.numel())
    return out


# --------------------------------------------------------------------------------------------
# CLIP score front end (InferNet/template/validator/scoring.py:81-85, :121-122; include/vdx.h vdx_clip_preprocess_u8)
CLIP_IMAGE = 224
CLIP_BAND = 8                 # output rows per block of vdx_clip_preprocess_u8
CLIP_LDS_MAX = 65536


def _bilinear_filter(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic_filter(x: float) -> float:          # Pillow's bicubic_filter, a = -0.5
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


RESIZE_FILTERS = {"bilinear": (_bilinear_filter, 1.0), "bicubic": (_bicubic_filter, 2.0)}   # name -> (filter, support)


def clip_resize_coeffs(in_size: int, out_size: int = CLIP_IMAGE, filter: str = "bilinear"):
    """Pillow's windows and 22-bit weights for one axis (ImagingResample's precompute_coeffs + normalize_coeffs_8bpc), in
    float64 on the host -> (bounds int32 [out][2] = (first input index, count), coeffs int32 [out][ksize]).  `filter`:
    "bilinear" (support 1, the CLIP front end) or "bicubic" (a = -0.5, support 2: Image.resize's default); the support is
    widened by max(in/out, 1) when reducing; a weight w becomes int(w * 2^22 +- 0.5)."""
    import math
    import numpy as np
    filt, base_support = RESIZE_FILTERS[filter]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = base_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        if filter == "bilinear":                   # (kept as the CLIP front end has always computed it)
            w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        else:
            w = [filt((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = sum(w)
        for x, v in enumerate(w):
            v = v / ww if ww != 0.0 else v
            coeffs[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, n)
    return bounds, coeffs


def clip_band_span(y_bounds, band: int) -> int:
    """Input rows the widest band of `band` output rows reads (its LDS rows in vdx_clip_preprocess_u8)."""
    out = len(y_bounds)
    return max(int(y_bounds[min(b + band, out) - 1].sum() - y_bounds[b, 0]) for b in range(0, out, band))


def pillow_resizes_vertically_first(in_h: int, in_w: int, out_h: int) -> bool:
    """`Image.resize` runs the vertical pass first, as a resize of its own, on an image more than 100 times taller than wide
    whose height shrinks (PIL/Image.py); every other image gets the horizontal pass first.  The intermediate image is uint8
    either way, so the two orders differ in the low bit of many pixels."""
    return in_h > 100 * in_w and out_h < in_h


_CLIP_TABLES: dict = {}   # (in_size, device) -> (bounds, coeffs) int32 device tensors, host-computed once per size


def _clip_table(in_size: int, device):
    key = (in_size, str(device))
    t = _CLIP_TABLES.get(key)
    if t is None:
        b, k = clip_resize_coeffs(in_size)
        t = _CLIP_TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), b)
    return t


def clip_preprocess(frames, out=None, return_u8=False):
    """uint8 RGB frames (F, H, W, 3) on the GPU (rows and frames may be pitched; pixels packed) -> the patch-GEMM rows
    fp16 [F*49][3072] of Resize((224, 224)) + ToTensor + Normalize(ImageNet).  `return_u8`: also the resized uint8
    (F, 224, 224, 3) image -> (rows, u8)."""
    F, H, W = check_u8_frames(frames, "clip_preprocess")
    if pillow_resizes_vertically_first(H, W, CLIP_IMAGE):
        # the kernel's order is horizontal, then vertical: hand it the vertical pass's (F, 224, W, 3) image, which its own
        # vertical pass (224 -> 224: weights 2^22, 0) leaves as it is
        frames, H = resize_u8(frames, CLIP_IMAGE, W, "bilinear"), CLIP_IMAGE
    dev = frames.device
    xb, xk, _ = _clip_table(W, dev)
    yb, yk, yb_host = _clip_table(H, dev)
    band = CLIP_BAND
    while band > 1 and clip_band_span(yb_host, band) * CLIP_IMAGE * 3 > CLIP_LDS_MAX:
        band //= 2
    span = clip_band_span(yb_host, band)
    if span * CLIP_IMAGE * 3 > CLIP_LDS_MAX:
        raise VdxError(f"clip_preprocess: H={H} needs {span} input rows per output row (more than LDS holds)")
    out, ldo = _out(out, F * 49, 3072, frames, "clip_preprocess")
    u8 = torch.empty((F, CLIP_IMAGE, CLIP_IMAGE, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    a = _lib.ClipPreprocessArgs()
    a.frames, a.frame_pitch, a.row_pitch = _u8_args(frames)
    a.out, a.out_u8 = _p(out, "out"), (u8.data_ptr() if u8 is not None else None)
    a.x_bounds, a.x_coeffs, a.y_bounds, a.y_coeffs = xb.data_ptr(), xk.data_ptr(), yb.data_ptr(), yk.data_ptr()
    a.F, a.H, a.W = F, H, W
    a.kx, a.ky, a.band, a.span, a.ldo = xk.shape[1], yk.shape[1], band, span, ldo
    _launch("vdx_clip_preprocess_u8", C.byref(a))
    return (out, u8) if return_u8 else out


def clip_vision_embed(patch, class_emb, pos_emb, gamma, beta, *, F, seq_pad, eps=1e-5, out=None):
    """CLIPVisionEmbeddings + pre_layrnorm: patch-GEMM rows [F*P][D] -> rows [F*seq_pad][D] (class token, P patches,
    zero rows up to seq_pad), P = pos_emb rows - 1."""
    r, D, ldp = _rows(patch, "patch")
    P = pos_emb.shape[0] - 1
    if r < F * P or pos_emb.shape[1] != D or class_emb.numel() != D or gamma.numel() != D or beta.numel() != D:
        raise VdxError(f"clip_vision_embed: patch [{r}][{D}], pos {tuple(pos_emb.shape)}: shapes do not match F={F}")
    if seq_pad <= P or not pos_emb.is_contiguous():
        raise VdxError(f"clip_vision_embed: seq_pad={seq_pad} must exceed {P} patches; pos_emb contiguous")
    out, ldo = _out(out, F * seq_pad, D, patch, "clip_vision_embed")
    _launch("vdx_clip_vision_embed_f16", _p(patch, "patch"), ldp, _p(class_emb, "class_emb"), _p(pos_emb, "pos_emb"),
            _p(gamma, "gamma"), _p(beta, "beta"), float(eps), F, P, seq_pad, D, _p(out, "out"), ldo)
    return out


def clip_cosine_score(img, txt):
    """F.normalize(img[f]) . F.normalize(txt) for F image embeddings fp16 [F][D] and one text embedding fp16 [D]
    -> (mean fp32 [1], per_frame fp32 [F]) on the device, in a fixed reduction order."""
    F, D, ldi = _rows(img, "img")
    if txt.numel() != D or not txt.is_contiguous():
        raise VdxError(f"clip_cosine_score: text embedding has {txt.numel()} values, images {D}")
    if F == 0:
        raise VdxError("clip_cosine_score: no frames")
    per = torch.empty(F, dtype=torch.float32, device=img.device)
    mean = torch.empty(1, dtype=torch.float32, device=img.device)
    _launch("vdx_clip_cosine_score_f16", _p(img, "img"), ldi, _p(txt, "txt"), F, D, _p(per, "per_frame", torch.float32),
            _p(mean, "mean", torch.float32))
    return mean, per


# --------------------------------------------------------------------------------------------
def groupnorm(x, gamma, beta, *, groups, n_samples, rows_per_sample, eps, silu_act, x2=None, out=None, partition_samples=0):
    """GroupNorm (+SiLU) over rows [n_samples*rows_per_sample][C]; x2 = second concat source.
    partition_samples: reduce the statistics with the slab partition of a batch of that many samples (bit-stable
    results for a sample whatever batch it is normalised in; include/vdx.h)."""
    r, c1, ldx = _rows(x, "x")
    c2, ldx2 = 0, 0
    M = n_samples * rows_per_sample
    if r < M:
        raise VdxError(f"groupnorm: x has {r} rows, need {M}")
    if x2 is not None:
        r2, c2, ldx2 = _rows(x2, "x2")
        if r2 < M:
            raise VdxError(f"groupnorm: x2 has {r2} rows, need {M}")
    Cc = c1 + c2
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise VdxError(f"groupnorm: gamma/beta size {gamma.numel()} != C={Cc}")
    out, ldy = _out(out, M, Cc, x, "groupnorm")
    need = _lib.load().vdx_groupnorm_workspace_part(n_samples, rows_per_sample, Cc, groups, partition_samples)
    ws = _scratch(_GN_WS, x.device, need, torch.uint8, 1 << 20)
    _launch("vdx_groupnorm_part_f16", _p(x, "x"), c1, ldx, _p(x2, "x2"), c2, ldx2, _p(gamma, "gamma"), _p(beta, "beta"),
            float(eps), groups, n_samples, rows_per_sample, int(bool(silu_act)), _p(out, "out"), ldy, ws.data_ptr(),
            partition_samples)
    return out


def conv3x3_gn_preferred(c1: int, c2: int, N: int, n_img: int, h: int, w: int) -> bool:
    """K1 supported AND expected to be faster than the apply pass + conv GEMM (level 0 of the XL UNet)."""
    return bool(_lib.load().vdx_conv3x3_gn_preferred(c1, c2, N, n_img, h, w))


def conv3x3_gn_supported(c1: int, c2: int, N: int) -> bool:
    return bool(_lib.load().vdx_conv3x3_gn_supported(c1, c2, N))


def conv3x3_gn(x, gamma, beta, w, *, x2=None, bias=None, bias2=None, rows_per_bias2=0, residual=None, groups, n_img, h, wd, eps,
               partition_samples=0, out=None):
    """Conv2d 3x3 (pad 1, stride 1) of SiLU(GroupNorm4d(cat(x, x2))) — conv1 / conv2 of ResnetBlock2D — without the
    normalised tensor: the statistics pass (`vdx_groupnorm_stats_f16`, one sample per image) leaves a scale / shift pair per
    (image, channel); K1 (`vdx_conv3x3_gn_f16`, csrc/conv_fused.hip) applies them, and the SiLU, to its staged image patch
    in LDS.  x (and x2: the skip tensor of the up blocks): raw rows [n_img*h*wd][c]; w: packed weights [N][9*(c1+c2)]."""
    r, c1, ldx = _rows(x, "x")
    S = h * wd
    M = n_img * S
    c2 = ldx2 = 0
    if x2 is not None:
        r2, c2, ldx2 = _rows(x2, "x2")
        if r2 < M:
            raise VdxError(f"conv3x3_gn: x2 has {r2} rows, need {M}")
    Cc = c1 + c2
    N, K = w.shape
    if r < M or K != 9 * Cc or gamma.numel() != Cc or beta.numel() != Cc or not w.is_contiguous():
        raise VdxError(f"conv3x3_gn: x [{r}][{c1}] (+{c2}), w [{N}][{K}], gamma {gamma.numel()}, M = {M}: shapes do not match")
    if not conv3x3_gn_supported(c1, c2, N):
        raise VdxError(f"conv3x3_gn: c1={c1}, c2={c2}, N={N} not supported")
    if bias is not None and bias.numel() != N:
        raise VdxError(f"conv3x3_gn: bias has {bias.numel()} elements, N={N}")
    ldb2 = _covers(bias2, M, N, "conv3x3_gn", "bias2", rows_per_bias2)
    ldr = _covers(residual, M, N, "conv3x3_gn", "residual")
    out, ldo = _out(out, M, N, x, "conv3x3_gn")
    need = _lib.load().vdx_groupnorm_workspace_part(n_img, S, Cc, groups, partition_samples)
    ws = _scratch(_GN_WS, x.device, need, torch.uint8, 1 << 20)
    off = C.c_size_t(0)
    _launch("vdx_groupnorm_stats_f16", _p(x, "x"), c1, ldx, _p(x2, "x2"), c2, ldx2, _p(gamma, "gamma"), _p(beta, "beta"),
            float(eps), groups, n_img, S, ws.data_ptr(), partition_samples, C.byref(off))
    with _timed("conv3x3_gn_kernel", 2.0 * M * N * K, (M, N, K)):
        _launch("vdx_conv3x3_gn_f16", _p(x, "x"), ldx, _p(x2, "x2"), ldx2, c1, c2, ws.data_ptr() + off.value, _p(w, "w"),
                _p(bias, "bias"), _p(bias2, "bias2"), rows_per_bias2, ldb2, _p(residual, "residual"), ldr, _p(out, "out"), ldo,
                n_img, h, wd, N)
    return out


def tconv_gn_supported(C: int, N: int, F: int) -> bool:
    """Shapes `tconv_gn` (K3, csrc/tconv_fused.hip) takes: C % 64 == 0, N % 320 == 0, F % 8 == 0."""
    return bool(_lib.load().vdx_tconv_gn_supported(C, N, F))


def tconv_gn_preferred(C: int, N: int, B: int, F: int, S: int) -> bool:
    """K3 supported AND expected to be faster than the apply pass + TCONV3 GEMM (level 0 of the XL UNet)."""
    return bool(_lib.load().vdx_tconv_gn_preferred(C, N, B, F, S))


def tconv_gn(x, gamma, beta, w, *, bias=None, residual=None, groups, B, F, S, eps, partition_samples=0, out=None):
    """Conv3d (3,1,1) of SiLU(GroupNorm5d(x)) — one link of TemporalConvLayer's chain — without the normalised tensor:
    the statistics pass (`vdx_groupnorm_stats_f16`, n_samples = B, rows_per_sample = F*S) leaves a scale / shift pair per
    (sample, channel); K3 (`vdx_tconv_gn_f16`) applies them, and the SiLU, to its staged image in LDS.  x: raw rows
    [B*F*S][C]; w: packed temporal weights [N][3*C] (packing.pack_tconv)."""
    r, Cc, ldx = _rows(x, "x")
    M = B * F * S
    N, K = w.shape
    if r < M or K != 3 * Cc or gamma.numel() != Cc or beta.numel() != Cc or not w.is_contiguous():
        raise VdxError(f"tconv_gn: x [{r}][{Cc}], w [{N}][{K}], gamma {gamma.numel()}, M = {M}: shapes do not match")
    if not tconv_gn_supported(Cc, N, F):
        raise VdxError(f"tconv_gn: C={Cc}, N={N}, F={F} not supported")
    if bias is not None and bias.numel() != N:
        raise VdxError(f"tconv_gn: bias has {bias.numel()} elements, N={N}")
    ldr = _covers(residual, M, N, "tconv_gn", "residual")
    out, ldo = _out(out, M, N, x, "tconv_gn")
    need = _lib.load().vdx_groupnorm_workspace_part(B, F * S, Cc, groups, partition_samples)
    ws = _scratch(_GN_WS, x.device, need, torch.uint8, 1 << 20)
    off = C.c_size_t(0)
    _launch("vdx_groupnorm_stats_f16", _p(x, "x"), Cc, ldx, None, 0, 0, _p(gamma, "gamma"), _p(beta, "beta"), float(eps), groups, B,
            F * S, ws.data_ptr(), partition_samples, C.byref(off))
    with _timed(f"tconv_gn_kernel<{16 if F % 16 == 0 else 12 if F % 12 == 0 else 8}>", 2.0 * M * N * K, (M, N, K)):
        _launch("vdx_tconv_gn_f16", _p(x, "x"), ldx, ws.data_ptr() + off.value, _p(w, "w"), _p(bias, "bias"),
                _p(residual, "residual"), ldr, _p(out, "out"), ldo, B, F, S, Cc, N)
    return out


def layernorm(x, gamma, beta, *, M, eps=1e-5, out=None):
    r, Cc, ldx = _rows(x, "x")
    if r < M:
        raise VdxError("layernorm: x too small")
    if gamma.numel() != Cc or beta.numel() != Cc:
        raise VdxError("layernorm: gamma/beta size")
    out, ldy = _out(out, M, Cc, x, "layernorm")
    _launch("vdx_layernorm_f16", _p(x, "x"), ldx, _p(gamma, "gamma"), _p(beta, "beta"), float(eps), M, Cc, _p(out, "out"), ldy)
    return out


def softmax_rows(x, *, rows, cols, scale):
    """In-place softmax(scale * x[r, :cols]) per row (fp32 inside): AutoencoderKL mid-block attention."""
    r, c, ld = _rows(x, "x")
    if r < rows or c < cols:
        raise VdxError("softmax_rows: x too small")
    _launch("vdx_softmax_rows_f16", _p(x, "x"), ld, rows, cols, float(scale))
    return x


def rows_to_u8_frames(rows, n, H, W):
    """Decoder output rows [n*H*W][ld] (RGB first) -> uint8 (n,H,W,3): fsdp_chunked_coherent.py:224-225."""
    r, c, ld = _rows(rows, "rows")
    if r < n * H * W or c < 3:
        raise VdxError("rows_to_u8_frames: rows too small")
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=rows.device)
    _launch("vdx_rows_to_u8_frames", _p(rows, "rows"), ld, n * H * W, out.data_ptr())
    return out


# --------------------------------------------------------------------------------------------
def flash_attn(q, k, vt, *, n_seq, sq, skv, skv_pad, heads, seq_per_kv, scale, out=None, causal=False, v_rows=False):
    """q rows [n_seq*sq][>=heads*64]; k rows [n_kv*skv_pad][>=heads*64]; vt [heads*64][>= n_kv*skv_pad] — or, with
    `v_rows`, V as rows like k (the third column block of a q|k|v projection: `vdx_flash_attn_rows_f16`)."""
    qr, qc, ldq = _rows(q, "q")
    kr, kc, ldk = _rows(k, "k")
    vr, vc, ldvt = _rows(vt, "v" if v_rows else "vt")
    inner = heads * 64
    n_kv = n_seq // seq_per_kv
    if qr < n_seq * sq or qc < inner:
        raise VdxError("flash_attn: q too small")
    if kr < n_kv * skv_pad or kc < inner:
        raise VdxError("flash_attn: k too small")
    if v_rows and (vr < n_kv * skv_pad or vc < inner):
        raise VdxError("flash_attn: v too small")
    if not v_rows and (vr < inner or vc < n_kv * skv_pad):
        raise VdxError("flash_attn: vt too small")
    out, ldo = _out(out, n_seq * sq, inner, q, "flash_attn")
    two = sq >= 512 and skv >= 256                      # flash.hip: 64 queries per wave
    name = f"flash_attn_kernel<{2 if two else 1}, {'true' if causal else 'false'}, {'true' if v_rows else 'false'}>"
    with _timed(name, 4.0 * n_seq * heads * sq * skv * 64, (n_seq * sq, skv, heads * 64)):
        _launch("vdx_flash_attn_rows_f16" if v_rows else "vdx_flash_attn_f16", _p(q, "q"), ldq, _p(k, "k"), ldk, _p(vt, "vt"),
                ldvt, _p(out, "out"), ldo, n_seq, sq, skv, skv_pad, heads, seq_per_kv, float(scale), int(bool(causal)))
    return out


def temporal_attn(qkv, *, B, F, HW, heads, scale, out=None):
    r, c, ld = _rows(qkv, "qkv")
    inner = heads * 64
    M = B * F * HW
    if r < M or c < 3 * inner:
        raise VdxError("temporal_attn: qkv too small")
    out, ldo = _out(out, M, inner, qkv, "temporal_attn")
    _launch("vdx_temporal_attn_f16", _p(qkv, "qkv"), ld, _p(out, "out"), ldo, B, F, HW, heads, float(scale))
    return out


def temporal_attn_block2_supported(inner: int, F: int) -> bool:
    return bool(_lib.load().vdx_temporal_attn_block2_supported(inner, F))


def temporal_attn_block2(t, packed, *, B, F, HW, eps=1e-5, out=None):
    """K7, second design (csrc/tattn2.hip): t + to_out(attention_over_frames(LayerNorm(t))) in one kernel; LayerNorm's
    affine, the softmax scale and the biases are inside `packed` (packing.pack_k7b)."""
    r, inner, ldt = _rows(t, "t")
    M = B * F * HW
    if r < M:
        raise VdxError(f"temporal_attn_block2: t has {r} rows, need {M}")
    if not temporal_attn_block2_supported(inner, F):
        raise VdxError(f"temporal_attn_block2: inner={inner}, F={F} not supported by the fused kernel")
    _packed(packed, _lib.load().vdx_temporal_attn_block2_pack_bytes(inner), "temporal_attn_block2: packed blob", "packing.pack_k7b")
    out, ldo = _out(out, M, inner, t, "temporal_attn_block2")
    if out.data_ptr() == t.data_ptr():
        raise VdxError("temporal_attn_block2: out may not alias t")
    _launch("vdx_temporal_attn_block2_f16", _p(t, "t"), ldt, _p(packed, "packed"), float(eps), _p(out, "out"), ldo, B, F, HW, inner)
    return out


def ff_block_supported(inner: int) -> bool:
    return bool(_lib.load().vdx_ff_block_supported(inner))


def ff_block(t, packed, *, M, eps=1e-5, out=None, proj=None):
    """K8 (csrc/ff_fused.hip): t + ff(LayerNorm(t)) — GEGLU feed-forward of a transformer block — in one kernel;
    LayerNorm's affine and the biases are inside `packed` (packing.pack_k8).
    `proj` = (tail blob of packing.pack_k8_proj, x, xrows): the transformer's proj_out and its residual run behind the
    feed-forward in the same kernel — out[r] = x[r % xrows] + W_p . (t[r] + ff(LayerNorm(t[r]))) + b_p, xrows = M or M / 2."""
    r, inner, ldt = _rows(t, "t")
    if r < M:
        raise VdxError(f"ff_block: t has {r} rows, need {M}")
    if not ff_block_supported(inner):
        raise VdxError(f"ff_block: inner={inner} not supported by the fused kernel")
    _packed(packed, _lib.load().vdx_ff_block_pack_bytes(inner), "ff_block: packed blob", "packing.pack_k8")
    out, ldo = _out(out, M, inner, t, "ff_block")
    if out.data_ptr() == t.data_ptr():
        raise VdxError("ff_block: out may not alias t")
    if proj is None:
        args = ("vdx_ff_block_f16", _p(t, "t"), ldt, _p(packed, "packed"), float(eps), _p(out, "out"), ldo, M, inner)
    else:
        blob, x, xrows = proj
        xr, xc, ldx = _rows(x, "x")
        if xc < inner or xr < xrows or xrows not in (M, M // 2) or (xrows != M and 2 * xrows != M):
            raise VdxError(f"ff_block: x {tuple(x.shape)} / xrows {xrows} do not pair with M = {M} rows")
        _packed(blob, _lib.load().vdx_ff_block_proj_pack_bytes(inner), "ff_block: proj blob", "packing.pack_k8_proj")
        if out.data_ptr() == x.data_ptr():
            raise VdxError("ff_block: out may not alias x")
        args = ("vdx_ff_block_proj_f16", _p(t, "t"), ldt, _p(packed, "packed"), float(eps), _p(x, "x"), ldx, int(xrows),
                _p(blob, "proj"), _p(out, "out"), ldo, M, inner)
    with _timed(f"ff_fused_kernel<{inner}, {'true' if proj is not None else 'false'}>",
                2.0 * M * inner * (12 + (1 if proj is not None else 0)) * inner, (M, inner, 12 * inner)):
        _launch(*args)
    return out


def cross_attn_block_supported(inner: int, kv_len: int) -> bool:
    return bool(_lib.load().vdx_cross_attn_block_supported(inner, kv_len))


def cross_attn_block(t, packed, kv_packed, *, kv_len, n_items, rows_per_item, eps=1e-5, out=None):
    """K5 (csrc/xattn.hip): t + to_out(softmax(q K^T) V), q = LayerNorm(t).W_q^T — the cross-attention sub-block of a spatial
    transformer — in one kernel.  `packed`: packing.pack_k5 (LayerNorm's affine, the scale, the biases inside);
    `kv_packed`: packing.pack_k5_kv of the text keys / values, [n_items][heads][3 units]; rows [n_items*rows_per_item][inner]."""
    r, inner, ldt = _rows(t, "t")
    M = n_items * rows_per_item
    if r < M:
        raise VdxError(f"cross_attn_block: t has {r} rows, need {M}")
    if not cross_attn_block_supported(inner, kv_len):
        raise VdxError(f"cross_attn_block: inner={inner}, kv_len={kv_len} not supported by the fused kernel")
    lib = _lib.load()
    _packed(packed, lib.vdx_cross_attn_block_pack_bytes(inner), "cross_attn_block: packed blob", "packing.pack_k5")
    _packed(kv_packed, n_items * lib.vdx_cross_attn_block_kv_bytes(inner), "cross_attn_block: key / value blob", "packing.pack_k5_kv")
    out, ldo = _out(out, M, inner, t, "cross_attn_block")
    if out.data_ptr() == t.data_ptr():
        raise VdxError("cross_attn_block: out may not alias t")
    with _timed(f"xattn_kernel<{inner}>", 2.0 * M * (2 * inner * inner + 2 * kv_len * inner), (M, inner, 2 * inner + 2 * kv_len)):
        _launch("vdx_cross_attn_block_f16", _p(t, "t"), ldt, _p(packed, "packed"), _p(kv_packed, "kv_packed"), int(kv_len),
                float(eps), _p(out, "out"), ldo, n_items, rows_per_item, inner)
    return out


def temporal_attn_block_supported(inner: int, F: int) -> bool:
    return bool(_lib.load().vdx_temporal_attn_block_supported(inner, F))


def temporal_attn_block(t, gamma, beta, wqkv_packed, wo_packed, bo, *, B, F, HW, scale, eps=1e-5, out=None):
    """K7: t + to_out(attention_over_frames(LayerNorm(t))) in one kernel (include/vdx.h)."""
    r, inner, ldt = _rows(t, "t")
    M = B * F * HW
    if r < M:
        raise VdxError(f"temporal_attn_block: t has {r} rows, need {M}")
    if not temporal_attn_block_supported(inner, F):
        raise VdxError(f"temporal_attn_block: inner={inner}, F={F} not supported by the fused kernel")
    if gamma.numel() != inner or beta.numel() != inner or bo.numel() != inner:
        raise VdxError("temporal_attn_block: gamma/beta/bias size")
    lib = _lib.load()
    _packed(wqkv_packed, lib.vdx_temporal_attn_block_wqkv_bytes(inner), "temporal_attn_block: wqkv blob", "packing.pack_k7_qkv")
    _packed(wo_packed, lib.vdx_temporal_attn_block_wo_bytes(inner), "temporal_attn_block: wo blob", "packing.pack_k7_out")
    out, ldo = _out(out, M, inner, t, "temporal_attn_block")
    if out.data_ptr() == t.data_ptr():
        raise VdxError("temporal_attn_block: out may not alias t")
    _launch("vdx_temporal_attn_block_f16", _p(t, "t"), ldt, _p(gamma, "gamma"), _p(beta, "beta"), float(eps),
            _p(wqkv_packed, "wqkv"), _p(wo_packed, "wo"), _p(bo, "bo"), _p(out, "out"), ldo, B, F, HW, inner, float(scale))
    return out


# --------------------------------------------------------------------------------------------
def cfg_input(lat, ctx, weight, out=None):
    """fsdp_chunked_coherent.py:133-137: cat([lat]*2) (+ weight * ctx.repeat(F)).
    The result is TAGGED as a known duplicate (`is_cfg_duplicate`): the UNet then computes its text-independent blocks once.
    The tag is tied to torch's version counter, which torch operations bump and this library's kernels do NOT: never hand the
    result to a vdx op as its `out=` (nothing in this package does)."""
    b, Cc, F, H, W = lat.shape
    if b != 1 or not lat.is_contiguous():
        raise VdxError("cfg_input: lat must be contiguous (1,C,F,H,W)")
    if ctx is not None and (tuple(ctx.shape) != (1, Cc, 1, H, W) or not ctx.is_contiguous()):
        raise VdxError("cfg_input: ctx must be contiguous (1,C,1,H,W)")
    if out is None:
        out = torch.empty((2, Cc, F, H, W), dtype=torch.float16, device=lat.device)
    _launch("vdx_cfg_input_f16", _p(lat, "lat"), _p(ctx, "ctx"), float(weight), _p(out, "out"), Cc, F, H * W)
    out._vdx_cfg_dup = out._version        # both batch items hold the same values until somebody writes the tensor
    return out


def is_cfg_duplicate(x) -> bool:
    """True for a tensor `cfg_input` produced and nobody has written since (torch's version counter): its two batch items
    are known to be equal, which lets the UNet compute the text-independent blocks once (unet3d.forward)."""
    tag = getattr(x, "_vdx_cfg_dup", None)
    try:
        return tag is not None and tag == x._version
    except Exception:       # inference-mode tensors do not track versions
        return False


def _dpm_args(what, lat, x0_prev, x0_out, out, coeffs):
    """Shared checks of the DPM-Solver++ steps -> (x0_out, out, the six fp32 coefficients)."""
    for name, t in (("x0_prev", x0_prev), ("x0_out", x0_out), ("out", out)):
        if t is not None and (tuple(t.shape) != tuple(lat.shape) or not t.is_contiguous()):
            raise VdxError(f"{what}: {name} must be contiguous and shaped like lat")
    if x0_out is None:
        x0_out = torch.empty_like(lat)
    if out is None:
        out = torch.empty_like(lat)
    if x0_prev is not None and x0_out.data_ptr() == x0_prev.data_ptr():
        raise VdxError(f"{what}: x0_out must not be x0_prev (the history ping-pongs two buffers)")
    c = tuple(float(v) for v in coeffs)
    if len(c) != 6:
        raise VdxError(f"{what}: coeffs = (s0, 1/a0, st/s0, c_d0, c_d1, 1/r0)")
    return x0_out, out, c


def _eps2_like(what, eps2, lat):
    if eps2.dim() < 1 or eps2.shape[0] != 2 or (lat is not None and (tuple(eps2.shape[1:]) != tuple(lat.shape[1:]) or lat.shape[0] != 1)):
        raise VdxError(f"{what}: eps2 must be (2,...) matching lat (1,...)")
    if not (eps2.is_contiguous() and (lat is None or lat.is_contiguous())):
        raise VdxError(f"{what}: tensors must be contiguous")


def _step_noise(what, lat, noise, frames=None):
    """The stochastic steps' trailing arguments (c_n, seed, stream, C, T, HW, s, L) from `noise` = (c_n, seed, stream) and the
    sample's place in the clip: `frames` = (s, T), the sample (1,C,L,H,W) being the frames [s, s + L) of a clip of T; None: the
    sample is the logical tensor itself (of any shape)."""
    import math
    c_n, seed, stream = noise
    c_n = float(c_n)
    if not math.isfinite(c_n):
        raise VdxError(f"{what}: c_n must be finite, got {c_n!r}")
    seed, stream = _noise_int(f"{what}: seed", seed, 0, 2 ** 64), _noise_int(f"{what}: stream", stream, 0, 2 ** 64)
    if frames is None:
        if lat.dim() == 5 and lat.shape[0] == 1:
            _, Cc, L, H, W = lat.shape
            return c_n, seed, stream, Cc, L, H * W, 0, L
        if lat.numel() >= 2 ** 31:
            raise VdxError(f"{what}: a sample that is not (1,C,T,H,W) must have fewer than 2^31 elements")
        return c_n, seed, stream, 1, 1, lat.numel(), 0, 1
    if lat.dim() != 5 or lat.shape[0] != 1:
        raise VdxError(f"{what}: with frames the sample must be (1,C,L,H,W)")
    _, Cc, L, H, W = lat.shape
    s, T = (_noise_int(f"{what}: frames[{k}]", v, 0, 2 ** 31) for k, v in enumerate(frames))
    if s + L > T:
        raise VdxError(f"{what}: the frames [{s}, {s} + {L}) leave the clip of {T} frames")
    return c_n, seed, stream, Cc, T, H * W, s, L


def _one_step(symbol, eps, lat, guidance, coeffs, history, out, rescaled=None, mimic=None, noise=None):
    """Every one-buffer sampler step (csrc/step_common.h `direct_launch`), launched as `symbol`(eps, lat, history, out, buffers,
    scalars, coefficients, size) and named in errors as the wrapper, `symbol` without `vdx_` and `_f16`.  `guidance` None: the
    sampler alone on an eps shaped like lat, else eps = [u; c].  `history` None: the DDIM form -> out; else (x0_prev, x0_out), the
    DPM-Solver++ form through `_dpm_args` -> (out, x0).  `rescaled`: the rescale variants' ((phi, 1 - phi), partials, stats_out);
    `mimic`: the thresholded variants' (workspace,).  `noise`: the stochastic variants' `_step_noise` arguments, which stand where
    the size stands.  One call below the public wrapper and no closure: launch-bound."""
    what = symbol[4:-4]
    if guidance is None:
        if tuple(eps.shape) != tuple(lat.shape) or not (eps.is_contiguous() and lat.is_contiguous()):
            raise VdxError(f"{what}: eps and lat must be contiguous and of equal shape")
    else:
        (_eps2_like if mimic is None else _eps2_5d)(what, eps, lat)
    if history is None:
        if out is None:
            out = torch.empty_like(lat)
        hist = ()
        s1, sa, sp, s1p = (float(c) for c in coeffs)
        c = (s1, sa, sp, s1p)
    else:
        x0_out, out, c = _dpm_args(what, lat, history[0], history[1], out, coeffs)
        hist = (_p(history[0], "x0_prev"), _p(x0_out, "x0_out"))
    bufs, scal, size = (), () if guidance is None else (float(guidance),), (lat.numel(),)
    if rescaled is not None:
        _, pp, sp_ = _rescale_buffers(what, cfg_rescale_rows(lat.numel()), lat, rescaled[1], rescaled[2])
        bufs, scal = (pp, sp_), scal + tuple(float(v) for v in rescaled[0])
    elif mimic is not None:
        _, wp, size = _mimic_ws(what, lat.shape, lat, mimic[0])
        bufs = (wp,)
    elif noise is not None:
        size = noise
    _launch(symbol, _p(eps, "eps" if guidance is None else "eps2"), _p(lat, "lat"), *hist, _p(out, "out"), *bufs, *scal, *c, *size)
    return out if history is None else (out, x0_out)


def cfg_ddim_step(eps2, lat, guidance, coeffs, out=None):
    """fsdp_chunked_coherent.py:141-142.  coeffs = (sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev))."""
    return _one_step("vdx_cfg_ddim_step_f16", eps2, lat, guidance, coeffs, None, out)


def ddim_step(eps, lat, coeffs, out=None):
    """`scheduler.step(eps, t, lat).prev_sample` (fsdp_chunked_coherent.py:142) without the CFG combine."""
    return _one_step("vdx_ddim_step_f16", eps, lat, None, coeffs, None, out)


def cfg_dpm_step(eps2, lat, guidance, coeffs, x0_prev=None, x0_out=None, out=None):
    """`u + gs*(c-u)` + one DPM-Solver++ step (vdx/scheduler.py `DPMSolverMultistepScheduler.step_cfg`) in one kernel ->
    (lat', x0).  coeffs = (s0, 1/a0, st/s0, -at*(exp(-h)-1), half of that, 1/r0); `x0_prev=None`: the first-order form.
    `out` may be `lat`; `x0_out` may not be `x0_prev`."""
    return _one_step("vdx_cfg_dpm_step_f16", eps2, lat, guidance, coeffs, (x0_prev, x0_out), out)


def dpm_step(eps, lat, coeffs, x0_prev=None, x0_out=None, out=None):
    """`scheduler.step(eps, t, lat)` of the DPM-Solver++ scheduler without the CFG combine -> (lat', x0)."""
    return _one_step("vdx_dpm_step_f16", eps, lat, None, coeffs, (x0_prev, x0_out), out)


# the stochastic forms (include/vdx.h "Stochastic sampling"; csrc/step_noise.h; tests/sde_ref.py): `noise` = (c_n, seed, stream), the
# draw being `philox_normal`'s for the whole clip at the sample's place in it (`frames` = (s, T); None: the sample is the clip)
def cfg_ddim_eta_step(eps2, lat, guidance, coeffs, noise, frames=None, out=None):
    """`cfg_ddim_step` with eta > 0: coeffs = (sqrt(1-a_t), sqrt(a_t), sqrt(a_prev), sqrt(1-a_prev-std^2)), then + c_n * w."""
    return _one_step("vdx_cfg_ddim_eta_step_f16", eps2, lat, guidance, coeffs, None, out,
                     noise=_step_noise("cfg_ddim_eta_step", lat, noise, frames))


def ddim_eta_step(eps, lat, coeffs, noise, frames=None, out=None):
    """`ddim_step` with eta > 0 (`DDIMScheduler.step(eta=)`), without the CFG combine."""
    return _one_step("vdx_ddim_eta_step_f16", eps, lat, None, coeffs, None, out, noise=_step_noise("ddim_eta_step", lat, noise, frames))


def cfg_sde_dpm_step(eps2, lat, guidance, coeffs, noise, frames=None, x0_prev=None, x0_out=None, out=None):
    """`cfg_dpm_step` of SDE-DPM-Solver++: coeffs = (s0, 1/a0, (st/s0)*exp(-h), at*(1-exp(-2h)), half of that, 1/r0), then
    + c_n * w -> (lat', x0)."""
    return _one_step("vdx_cfg_sde_dpm_step_f16", eps2, lat, guidance, coeffs, (x0_prev, x0_out), out,
                     noise=_step_noise("cfg_sde_dpm_step", lat, noise, frames))


def sde_dpm_step(eps, lat, coeffs, noise, frames=None, x0_prev=None, x0_out=None, out=None):
    """`dpm_step` of SDE-DPM-Solver++, without the CFG combine -> (lat', x0)."""
    return _one_step("vdx_sde_dpm_step_f16", eps, lat, None, coeffs, (x0_prev, x0_out), out,
                     noise=_step_noise("sde_dpm_step", lat, noise, frames))


def blend_accumulate(full, weight, chunk, w, s, e):
    _, Cc, T, H, W = full.shape
    if tuple(chunk.shape) != (1, Cc, e - s, H, W) or not (chunk.is_contiguous() and full.is_contiguous()):
        raise VdxError("blend_accumulate: chunk shape does not match range")
    if weight.numel() != T or w.numel() != e - s:
        raise VdxError("blend_accumulate: weight vectors")
    _launch("vdx_blend_accumulate_f16", _p(full, "full"), _p(weight, "weight", torch.float32), _p(chunk, "chunk"),
            _p(w, "w", torch.float32), Cc, T, H * W, s, e)


def blend_finalize(full, weight):
    _, Cc, T, H, W = full.shape
    out = torch.empty(full.shape, dtype=torch.float32, device=full.device)
    _launch("vdx_blend_finalize_f32", _p(full, "full"), _p(weight, "weight", torch.float32), _p(out, "out", torch.float32),
            Cc, T, H * W)
    return out


# --------------------------------------------------------------------------------------------
# Temporal co-denoising (vdx/codenoise.py, csrc/codenoise.hip; no reference counterpart)
def _cfg_input_of(what, symbol, z, ctx, weight, out, shape, named, tail):
    """What `cfg_input_window`, `cfg_input_loop` and `cfg_input_tile` share once z and their own range are checked (z first: the
    range is read against its shape): the checks of ctx and of out (`shape`, which the error calls `named`), the launch of
    `symbol`(z, ctx, weight, out, C, T, *tail) and the duplicate tag.  ONE call per launch: these ops are launch-bound."""
    _, Cc, T, H, W = z.shape
    if ctx is not None and (tuple(ctx.shape) != (1, Cc, 1, H, W) or not ctx.is_contiguous()):
        raise VdxError(f"{what}: ctx must be contiguous (1,C,1,H,W)")
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=z.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise VdxError(f"{what}: out must be contiguous {named}")
    _launch(symbol, _p(z, "z"), _p(ctx, "ctx"), float(weight), _p(out, "out"), Cc, T, *tail)
    out._vdx_cfg_dup = out._version        # both batch items hold the same values until somebody writes the tensor
    return out


def cfg_input_window(z, ctx, weight, s: int, e: int, out=None):
    """`cfg_input(z[:, :, s:e], ctx, weight)` without the slice copy: one launch reads frames [s, e) out of the whole clip's
    latent z (1,C,T,H,W) and writes the contiguous (2,C,e-s,H,W) UNet input, TAGGED as a CFG duplicate exactly as `cfg_input`
    tags its result (the same warning applies: never hand it to a vdx op as `out=`)."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError("cfg_input_window: z must be contiguous (1,C,T,H,W)")
    _, Cc, T, H, W = z.shape
    s, e = int(s), int(e)
    if not 0 <= s < e <= T:
        raise VdxError(f"cfg_input_window: bad range [{s},{e}) of {T} frames")
    return _cfg_input_of("cfg_input_window", "vdx_cfg_input_window_f16", z, ctx, weight, out, (2, Cc, e - s, H, W), "(2,C,e-s,H,W)",
                         (H * W, s, e))


COFUSE_MAX_WINDOWS = 64


def _cofuse_args(what, z, windows, table, wn, strided=False):
    """Shared checks of the two fused co-denoising steps -> the launch's leading arguments.  `table`: [(element offset into
    `windows`, first frame, length)] per window, host integers; the library checks every row against T and the buffer.
    `strided`: a row has a fourth entry, the frame stride, which travels as a fourth host array after the lengths; the other
    launches have no place for one and refuse a row whose fourth entry is not 1."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError(f"{what}: z must be contiguous (1,C,T,H,W)")
    if not windows.is_contiguous():
        raise VdxError(f"{what}: the windows buffer must be contiguous")
    _, Cc, T, H, W = z.shape
    K = len(table)
    if not 1 <= K <= COFUSE_MAX_WINDOWS:
        raise VdxError(f"{what}: {K} windows, 1..{COFUSE_MAX_WINDOWS} are supported")
    if tuple(wn.shape) != (K, T) or not wn.is_contiguous():
        raise VdxError(f"{what}: wn must be contiguous fp32 ({K},{T})")
    off = (C.c_int64 * K)(*(int(r[0]) for r in table))
    st = (C.c_int32 * K)(*(int(r[1]) for r in table))
    ln = (C.c_int32 * K)(*(int(r[2]) for r in table))
    sd = ()
    if strided:
        sd = ((C.c_int32 * K)(*(int(r[3]) for r in table)),)
    else:
        for r in table:                                            # a plain loop: no generator's frame on a launch-bound path
            if len(r) > 3 and r[3] != 1:
                raise VdxError(f"{what}: a window row has a frame stride other than 1, which only the strided steps take")
    return (_p(z, "z"), _p(windows, "windows"), windows.numel(), off, st, ln, *sd, K, _p(wn, "wn", torch.float32)), (Cc, T, H * W)


def _co_step(symbol, z, windows, table, wn, tiles, guidance, coeffs, history, out, rescaled=None, strided=False, mimic_ws=None,
             noise=None):
    """Every whole-clip fused step, launched as `symbol`(head, history, out, extras, tail) and named in errors as the wrapper,
    `symbol` without `vdx_` and `_f16`: `tiles` None for `_cofuse_args`' head (`strided`: with its fourth column), else
    `_cotile_args`'.  `history` None: the DDIM form -> out; else (x0_prev, x0_out), the DPM-Solver++ form through `_dpm_args` ->
    (out, x0), as in `_one_step`.  `rescaled`: the rescale variants' ((phi, 1 - phi), partials, stats_out); `mimic_ws`: the
    thresholded variants' statistics workspace; `noise`: the stochastic variants' (c_n, seed, stream), after the coefficients.  One
    call below the public wrapper and no closure: launch-bound."""
    what = symbol[4:-4]
    head, tail = _cofuse_args(what, z, windows, table, wn, strided) if tiles is None else _cotile_args(what, z, windows, table, wn, tiles)
    if history is None:
        if out is None:
            out = torch.empty_like(z)
        elif tuple(out.shape) != tuple(z.shape) or not out.is_contiguous():
            raise VdxError(f"{what}: out must be contiguous and shaped like z")
        hist = ()
        s1, sa, sp, s1p = (float(v) for v in coeffs)
        c = (s1, sa, sp, s1p)
    else:
        x0_out, out, c = _dpm_args(what, z, history[0], history[1], out, coeffs)
        hist = (_p(history[0], "x0_prev"), _p(x0_out, "x0_out"))
    bufs = phis = ()
    if rescaled is not None:
        _, pp, sp_ = _rescale_buffers(what, cofuse_cfg_rescale_rows(tail[0], tail[1]), z, rescaled[1], rescaled[2])
        bufs, phis = (pp, sp_), tuple(float(v) for v in rescaled[0])
    elif mimic_ws is not None:
        bufs = (_mimic_ws(what, z.shape, z, mimic_ws)[1],)
    elif noise is not None:
        c = c + _step_noise(what, z, noise)[:3]
    _launch(symbol, *head, *hist, _p(out, "out"), *bufs, float(guidance), *phis, *c, *tail)
    return out if history is None else (out, x0_out)


def cofuse_cfg_ddim_step(z, windows, table, wn, guidance, coeffs, out=None):
    """One co-denoising DDIM step of the whole clip (include/vdx.h `vdx_cofuse_cfg_ddim_step_f16`): the windows' raw UNet
    outputs, each a contiguous (2,C,L_k,H,W) block at its `table` offset inside `windows`, are averaged per frame with `wn`
    and fed to `cfg_ddim_step`'s chain.  coeffs as for `cfg_ddim_step`; `out` may be `z`."""
    return _co_step("vdx_cofuse_cfg_ddim_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out)


def cofuse_cfg_dpm_step(z, windows, table, wn, guidance, coeffs, x0_prev=None, x0_out=None, out=None):
    """The same fused noise into `cfg_dpm_step`'s chain (`vdx_cofuse_cfg_dpm_step_f16`) -> (z', x0), both of the whole
    clip's shape.  coeffs, `x0_prev`, `x0_out` and `out` as for `cfg_dpm_step`."""
    return _co_step("vdx_cofuse_cfg_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out)


def cofuse_cfg_ddim_eta_step(z, windows, table, wn, guidance, coeffs, noise, out=None):
    """`cofuse_cfg_ddim_step` with eta > 0 (`vdx_cofuse_cfg_ddim_eta_step_f16`): coeffs and `noise` as for `cfg_ddim_eta_step`; the
    sample is the clip."""
    return _co_step("vdx_cofuse_cfg_ddim_eta_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out, noise=noise)


def cofuse_cfg_sde_dpm_step(z, windows, table, wn, guidance, coeffs, noise, x0_prev=None, x0_out=None, out=None):
    """`cofuse_cfg_dpm_step` of SDE-DPM-Solver++ (`vdx_cofuse_cfg_sde_dpm_step_f16`) -> (z', x0); coeffs and `noise` as for
    `cfg_sde_dpm_step`."""
    return _co_step("vdx_cofuse_cfg_sde_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out, noise=noise)


# --------------------------------------------------------------------------------------------
# Seamless looping: ring windows (vdx/codenoise.py `loop_plan`, csrc/codenoise.hip's RING flag; no reference counterpart)
def cfg_input_loop(z, ctx, weight, s: int, L: int, out=None):
    """`cfg_input_window` on a ring: one launch reads the frames `(s + f) mod T`, f in [0, L), out of the whole clip's latent z
    (1,C,T,H,W), `0 <= s < T`, `1 <= L <= T`, and writes the contiguous (2,C,L,H,W) UNet input, TAGGED as a CFG duplicate
    exactly as `cfg_input_window` tags its result.  The library checks `s` and `L`."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError("cfg_input_loop: z must be contiguous (1,C,T,H,W)")
    _, Cc, T, H, W = z.shape
    s, L = int(s), int(L)
    if L < 1:
        raise VdxError(f"cfg_input_loop: bad ring window start {s}, length {L} of {T} frames")
    return _cfg_input_of("cfg_input_loop", "vdx_cfg_input_loop_f16", z, ctx, weight, out, (2, Cc, L, H, W), "(2,C,L,H,W)", (H * W, s, L))


def coloop_cfg_ddim_step(z, windows, table, wn, guidance, coeffs, out=None):
    """`cofuse_cfg_ddim_step` over ring windows (include/vdx.h `vdx_coloop_cfg_ddim_step_f16`): a `table` row (offset, s, L)
    means the frames `(s + f) mod T`; the fuse, the chain, `coeffs` and `out` (which may be `z`) are the same."""
    return _co_step("vdx_coloop_cfg_ddim_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out)


def coloop_cfg_dpm_step(z, windows, table, wn, guidance, coeffs, x0_prev=None, x0_out=None, out=None):
    """`cofuse_cfg_dpm_step` over ring windows (`vdx_coloop_cfg_dpm_step_f16`) -> (z', x0)."""
    return _co_step("vdx_coloop_cfg_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out)


# --------------------------------------------------------------------------------------------
# Strided context windows (vdx/codenoise.py `stride_plan`, csrc/codenoise.hip's `costride_tab`; no reference counterpart)
def cfg_input_stride(z, ctx, weight, s: int, L: int, d: int, out=None):
    """`cfg_input_window` with a frame stride: one launch reads the frames `s + f * d`, f in [0, L), out of the whole clip's latent
    z (1,C,T,H,W), `d >= 1`, `s + (L - 1) * d < T`, and writes the contiguous (2,C,L,H,W) UNet input, TAGGED as a CFG duplicate
    exactly as `cfg_input_window` tags its result.  The library checks `s`, `L` and `d`; `d = 1` gives `cfg_input_window`'s bits."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError("cfg_input_stride: z must be contiguous (1,C,T,H,W)")
    _, Cc, T, H, W = z.shape
    s, L, d = int(s), int(L), int(d)
    if L < 1:
        raise VdxError(f"cfg_input_stride: bad strided window start {s}, length {L}, stride {d} of {T} frames")
    return _cfg_input_of("cfg_input_stride", "vdx_cfg_input_stride_f16", z, ctx, weight, out, (2, Cc, L, H, W), "(2,C,L,H,W)",
                         (H * W, s, L, d))


def costride_cfg_ddim_step(z, windows, table, wn, guidance, coeffs, out=None):
    """`cofuse_cfg_ddim_step` over strided windows (include/vdx.h `vdx_costride_cfg_ddim_step_f16`): a `table` row
    (offset, s, L, d) means the frames `s + f * d`; the fuse, the chain, `coeffs` and `out` (which may be `z`) are the same."""
    return _co_step("vdx_costride_cfg_ddim_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out, strided=True)


def costride_cfg_dpm_step(z, windows, table, wn, guidance, coeffs, x0_prev=None, x0_out=None, out=None):
    """`cofuse_cfg_dpm_step` over strided windows (`vdx_costride_cfg_dpm_step_f16`) -> (z', x0)."""
    return _co_step("vdx_costride_cfg_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out, strided=True)


# --------------------------------------------------------------------------------------------
# Spatially tiled co-denoising (vdx/codenoise.py `tile_plan`, csrc/cotile.hip; no reference counterpart)
COTILE_MAX_TILES = 64


class TileGrid(NamedTuple):
    """The spatial half of a tiled step's window table: `stride` elements between consecutive tiles' blocks of one time window
    (tile (ky, kx) at `(ky * len(xs) + kx) * stride`), the bands' first rows `ys` and columns `xs` (host integers), the tile's
    size `th` x `tw`, and the per-axis normalised weights `wyn` (ny, H), `wxn` (nx, W), fp32 on the device."""
    stride: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    th: int
    tw: int
    wyn: torch.Tensor
    wxn: torch.Tensor


def cfg_input_tile(z, ctx, weight, s: int, e: int, y0: int, th: int, x0: int, tw: int, out=None):
    """`cfg_input(z[:, :, s:e, y0:y0+th, x0:x0+tw], ctx[..., y0:y0+th, x0:x0+tw], weight)` without the slice copies: one launch
    writes the contiguous (2,C,e-s,th,tw) UNet input of one tile of one window, TAGGED as a CFG duplicate exactly as
    `cfg_input_window` tags its result."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError("cfg_input_tile: z must be contiguous (1,C,T,H,W)")
    _, Cc, T, H, W = z.shape
    s, e, y0, th, x0, tw = (int(v) for v in (s, e, y0, th, x0, tw))
    if not 0 <= s < e <= T:
        raise VdxError(f"cfg_input_tile: bad range [{s},{e}) of {T} frames")
    if not (1 <= th <= H and 0 <= y0 <= H - th and 1 <= tw <= W and 0 <= x0 <= W - tw):
        raise VdxError(f"cfg_input_tile: tile [{y0},{y0}+{th}) x [{x0},{x0}+{tw}) leaves the {H}x{W} frame")
    return _cfg_input_of("cfg_input_tile", "vdx_cfg_input_tile_f16", z, ctx, weight, out, (2, Cc, e - s, th, tw), "(2,C,e-s,th,tw)",
                         (H, W, s, e, y0, th, x0, tw))


def _cotile_args(what, z, windows, table, wn, tiles: TileGrid):
    """Shared checks of the two tiled steps -> the launch's leading arguments (those of `_cofuse_args`, then the tile grid) and
    its trailing shape.  The library checks every row and band against the shape and the buffer."""
    head, (Cc, T, _) = _cofuse_args(what, z, windows, table, wn)
    H, W = z.shape[3:]
    ny, nx = len(tiles.ys), len(tiles.xs)
    if ny < 1 or nx < 1 or ny * nx > COTILE_MAX_TILES:
        raise VdxError(f"{what}: {ny} x {nx} tiles, at most {COTILE_MAX_TILES} are supported")
    if tuple(tiles.wyn.shape) != (ny, H) or tuple(tiles.wxn.shape) != (nx, W) or not (tiles.wyn.is_contiguous() and tiles.wxn.is_contiguous()):
        raise VdxError(f"{what}: wyn must be contiguous fp32 ({ny},{H}) and wxn ({nx},{W})")
    if int(tiles.stride) < 0:
        raise VdxError(f"{what}: bad tile stride {tiles.stride}")
    ys = (C.c_int32 * ny)(*(int(v) for v in tiles.ys))
    xs = (C.c_int32 * nx)(*(int(v) for v in tiles.xs))
    grid = (int(tiles.stride), ys, ny, _p(tiles.wyn, "wyn", torch.float32), xs, nx, _p(tiles.wxn, "wxn", torch.float32),
            int(tiles.th), int(tiles.tw))
    return head + grid, (Cc, T, H, W)


def cotile_cfg_ddim_step(z, windows, table, wn, tiles: TileGrid, guidance, coeffs, out=None):
    """One tiled co-denoising DDIM step of the whole clip (include/vdx.h `vdx_cotile_cfg_ddim_step_f16`): `table`, `wn` as for
    `cofuse_cfg_ddim_step`, each time window's block now holding the `len(ys) * len(xs)` tiles' (2,C,L_k,th,tw) outputs at
    `tiles.stride` from one another; the noise is averaged per cell with `wn[kt][t] * wyn[ky][y] * wxn[kx][x]` and fed to
    `cfg_ddim_step`'s chain.  `out` may be `z`."""
    return _co_step("vdx_cotile_cfg_ddim_step_f16", z, windows, table, wn, tiles, guidance, coeffs, None, out)


def cotile_cfg_dpm_step(z, windows, table, wn, tiles: TileGrid, guidance, coeffs, x0_prev=None, x0_out=None, out=None):
    """The same fused noise into `cfg_dpm_step`'s chain (`vdx_cotile_cfg_dpm_step_f16`) -> (z', x0)."""
    return _co_step("vdx_cotile_cfg_dpm_step_f16", z, windows, table, wn, tiles, guidance, coeffs, (x0_prev, x0_out), out)


# --------------------------------------------------------------------------------------------
# CFG rescale (vdx/scheduler.py `guidance_rescale`, csrc/rescale.hip; no reference counterpart)
RESCALE_MAX_ROWS = 256
_RESCALE_WS: dict = {}  # the statistics pass's partial rows, per (device, stream)


def rescale_factors(guidance_rescale):
    """`guidance_rescale` -> the kernels' two scalars (phi, 1 - phi), each formed in Python double and rounded to fp32 ONCE (as
    Python floats holding fp32 values); `ValueError` unless it is a finite number in [0, 1]."""
    import math
    import struct
    if isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, (int, float)) or not math.isfinite(guidance_rescale) \
            or not 0.0 <= guidance_rescale <= 1.0:
        raise ValueError(f"guidance_rescale must be a finite number in [0, 1], got {guidance_rescale!r}")
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]     # noqa: E731
    return f32(float(guidance_rescale)), f32(1.0 - float(guidance_rescale))


def _rescale_buffers(what, rows: int, like, partials, stats_out):
    """-> (partials, its pointer, stats_out's pointer or None): a float64 buffer of at least `rows` rows [4] (the per-stream
    workspace when none is given), and the optional 3 halves."""
    if rows < 1:
        raise VdxError(f"{what}: empty or oversized sample")
    if partials is None:
        partials = _scratch(_RESCALE_WS, like.device, RESCALE_MAX_ROWS * 32, torch.float64)
    elif partials.dtype != torch.float64 or not partials.is_contiguous() or partials.numel() < rows * 4:
        raise VdxError(f"{what}: partials must be contiguous float64 with at least {rows} rows of 4")
    if stats_out is not None and (stats_out.numel() < 3 or not stats_out.is_contiguous()):
        raise VdxError(f"{what}: stats_out must be 3 contiguous halves")
    return partials, _p(partials, "partials", torch.float64), _p(stats_out, "stats_out")


def cfg_rescale_rows(n: int) -> int:
    """Rows the statistics pass writes for a sample of n elements (`vdx_cfg_rescale_rows`): a function of n alone, <= 256."""
    return int(_lib.load().vdx_cfg_rescale_rows(int(n)))


def cofuse_cfg_rescale_rows(C_: int, T: int) -> int:
    return int(_lib.load().vdx_cofuse_cfg_rescale_rows(int(C_), int(T)))


def cfg_rescale_stats(eps2, guidance, partials=None):
    """The statistics pass of the rescaled step (include/vdx.h `vdx_cfg_rescale_stats_f16`) -> float64 (rows, 4): every block's
    [sum c, sum c*c, sum g, sum g*g] with g = u + gs*(c - u), eps2 = [u; c].  A view of the per-stream workspace unless `partials`
    is given: valid until the next statistics pass on this stream."""
    _eps2_like("cfg_rescale_stats", eps2, None)
    n = eps2.numel() // 2
    rows = cfg_rescale_rows(n)
    partials, pp, _ = _rescale_buffers("cfg_rescale_stats", rows, eps2, partials, None)
    _launch("vdx_cfg_rescale_stats_f16", _p(eps2, "eps2"), n, float(guidance), pp)
    return partials.view(-1)[:rows * 4].view(rows, 4)


def cfg_rescale_ddim_step(eps2, lat, guidance, rescale, coeffs, partials, out=None, stats_out=None):
    """`cfg_ddim_step` with the guided noise rescaled by `rescale` (`rescale_factors`' pair) from `cfg_rescale_stats`' rows of
    the same eps2 (`vdx_cfg_rescale_ddim_step_f16`).  `stats_out`: 3 halves that receive [sd_c, sd_g, r], or None."""
    return _one_step("vdx_cfg_rescale_ddim_step_f16", eps2, lat, guidance, coeffs, None, out, rescaled=(rescale, partials, stats_out))


def cfg_rescale_dpm_step(eps2, lat, guidance, rescale, coeffs, partials, x0_prev=None, x0_out=None, out=None, stats_out=None):
    """`cfg_dpm_step` with the rescaled guided noise (`vdx_cfg_rescale_dpm_step_f16`) -> (lat', x0)."""
    return _one_step("vdx_cfg_rescale_dpm_step_f16", eps2, lat, guidance, coeffs, (x0_prev, x0_out), out,
                     rescaled=(rescale, partials, stats_out))


def cofuse_cfg_rescale_stats(z, windows, table, wn, guidance, partials=None):
    """The statistics pass of the rescaled co-denoising step (`vdx_cofuse_cfg_rescale_stats_f16`): `cfg_rescale_stats` of the noise
    fused from the windows as `cofuse_cfg_ddim_step` fuses it, over the whole clip.  z gives the shape only."""
    head, tail = _cofuse_args("cofuse_cfg_rescale_stats", z, windows, table, wn)
    rows = cofuse_cfg_rescale_rows(tail[0], tail[1])
    partials, pp, _ = _rescale_buffers("cofuse_cfg_rescale_stats", rows, z, partials, None)
    _launch("vdx_cofuse_cfg_rescale_stats_f16", *head[1:], float(guidance), pp, *tail)
    return partials.view(-1)[:rows * 4].view(rows, 4)


def cofuse_cfg_rescale_ddim_step(z, windows, table, wn, guidance, rescale, coeffs, partials, out=None, stats_out=None):
    """`cofuse_cfg_ddim_step` with the rescaled guided noise (`vdx_cofuse_cfg_rescale_ddim_step_f16`)."""
    return _co_step("vdx_cofuse_cfg_rescale_ddim_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out,
                    (rescale, partials, stats_out))


def cofuse_cfg_rescale_dpm_step(z, windows, table, wn, guidance, rescale, coeffs, partials, x0_prev=None, x0_out=None, out=None,
                                stats_out=None):
    """`cofuse_cfg_dpm_step` with the rescaled guided noise (`vdx_cofuse_cfg_rescale_dpm_step_f16`) -> (z', x0)."""
    return _co_step("vdx_cofuse_cfg_rescale_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out,
                    (rescale, partials, stats_out))


# --------------------------------------------------------------------------------------------
# Dynamic thresholding with a mimic scale (vdx/scheduler.py `cfg_mimic`, csrc/dynthresh.hip; no reference counterpart)
MIMIC_BINS, MIMIC_MAX_ROWS = 32768, 64
_MIMIC_WS: dict = {}    # the statistics pass's workspace, per (device, stream)


def mimic_factors(mimic_scale, percentile, M: int):
    """(`cfg_mimic`, `cfg_mimic_percentile`, the elements per channel) -> the kernels' scalars (fp32 ms, k, f): ms rounded to fp32
    ONCE (a Python float holding the fp32 value), and the rank pos = q * (M - 1) formed ONCE in Python double and split into
    k = floor(pos) and f = fp32(pos - k).  `ValueError` for a scale that is not a finite number > 0 and a percentile outside
    (0, 1]."""
    import math
    import struct
    if isinstance(mimic_scale, bool) or not isinstance(mimic_scale, (int, float)) or not math.isfinite(mimic_scale) or not mimic_scale > 0:
        raise ValueError(f"cfg_mimic must be a finite number > 0, got {mimic_scale!r}")
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)) or not 0.0 < percentile <= 1.0:
        raise ValueError(f"cfg_mimic_percentile must be a number in (0, 1], got {percentile!r}")
    if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M < 1 << 32:
        raise ValueError(f"cfg_mimic: a channel must hold between 1 and 2^32 - 1 elements, got {M!r}")
    f32 = lambda v: struct.unpack("f", struct.pack("f", v))[0]     # noqa: E731
    pos = float(percentile) * float(M - 1)
    k = min(int(math.floor(pos)), M - 1)
    f = f32(pos - k)
    if not f < 1.0:                                                # the fraction rounded up to 1: the next rank, exactly
        k, f = min(k + 1, M - 1), 0.0
    return f32(float(mimic_scale)), k, f


def mimic_ws_bytes(C_: int, T: int, HW: int) -> int:
    """Bytes of the statistics workspace of a (C, T, HW) sample (`vdx_cfg_mimic_ws_bytes`); 0 for a shape the kernels refuse."""
    return int(_lib.load().vdx_cfg_mimic_ws_bytes(int(C_), int(T), int(HW)))


def mimic_ws_views(ws, C_: int):
    """The workspace's parts as views (include/vdx.h states the layout) -> {"scal": fp16 (C, 4) = (mg, ref_lo, ref_hi, s),
    "maxbits": int32 (C,), "partials": float64 (C, 64, 2), "hist": int32 (C, 32768)}.  For tests and tools: the loop never reads them."""
    up = lambda v: (v + 15) // 16 * 16                              # noqa: E731
    o_max = up(C_ * 8)
    o_part = o_max + up(C_ * 4)
    o_hist = o_part + C_ * MIMIC_MAX_ROWS * 16
    end = o_hist + C_ * MIMIC_BINS * 4
    b = ws.view(torch.uint8).reshape(-1)
    return {"scal": b[:C_ * 8].view(torch.float16).view(C_, 4), "maxbits": b[o_max:o_max + C_ * 4].view(torch.int32),
            "partials": b[o_part:o_hist].view(torch.float64).view(C_, MIMIC_MAX_ROWS, 2),
            "hist": b[o_hist:end].view(torch.int32).view(C_, MIMIC_BINS)}


def _mimic_ws(what, shape, like, ws):
    """-> (the workspace, its pointer, (C, T, HW)) for a sample of `shape` = (.., C, T, h, w): the per-stream workspace when none
    is given, else a contiguous uint8 tensor of at least `mimic_ws_bytes`."""
    Cc, T, HW = int(shape[-4]), int(shape[-3]), int(shape[-2]) * int(shape[-1])
    need = mimic_ws_bytes(Cc, T, HW)
    if need < 1:
        raise VdxError(f"{what}: empty or oversized sample")
    if ws is None:
        ws = _scratch(_MIMIC_WS, like.device, need, torch.uint8)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise VdxError(f"{what}: the workspace must be contiguous uint8 with at least {need} bytes")
    return ws, _p(ws, "ws", torch.uint8), (Cc, T, HW)


def _eps2_5d(what, eps2, lat):
    _eps2_like(what, eps2, lat)
    if eps2.dim() != 5:
        raise VdxError(f"{what}: eps2 must be (2,C,T,H,W): the statistics are per channel")


def cfg_mimic_stats(eps2, guidance, mimic, ws=None, stages: int = 7):
    """The statistics pass of the dynamically thresholded step (include/vdx.h `vdx_cfg_mimic_stats_f16`): three launches (the
    sums, the histogram, the select) that leave every channel's (mg, ref_lo, ref_hi, s) in the workspace -> the workspace, the
    per-stream one unless `ws` is given: valid until the next statistics pass on this stream.  `mimic`: `mimic_factors`' triple
    for this sample's channel size.  `stages`: the launches to run, 1 | 2 | 4 (tests and the benchmark)."""
    _eps2_5d("cfg_mimic_stats", eps2, None)
    ws, wp, shape = _mimic_ws("cfg_mimic_stats", eps2.shape, eps2, ws)
    ms, k, f = mimic
    _launch("vdx_cfg_mimic_stats_f16", _p(eps2, "eps2"), *shape, float(guidance), float(ms), int(k), float(f), wp, int(stages))
    return ws


def cfg_mimic_ddim_step(eps2, lat, guidance, coeffs, ws, out=None):
    """`cfg_ddim_step` with the guided noise thresholded per channel by the scalars `cfg_mimic_stats` of the same eps2 left in
    `ws` (`vdx_cfg_mimic_ddim_step_f16`)."""
    return _one_step("vdx_cfg_mimic_ddim_step_f16", eps2, lat, guidance, coeffs, None, out, mimic=(ws,))


def cfg_mimic_dpm_step(eps2, lat, guidance, coeffs, ws, x0_prev=None, x0_out=None, out=None):
    """`cfg_dpm_step` with the thresholded guided noise (`vdx_cfg_mimic_dpm_step_f16`) -> (lat', x0)."""
    return _one_step("vdx_cfg_mimic_dpm_step_f16", eps2, lat, guidance, coeffs, (x0_prev, x0_out), out, mimic=(ws,))


def cofuse_cfg_mimic_stats(z, windows, table, wn, guidance, mimic, ws=None, stages: int = 7):
    """The statistics pass of the thresholded co-denoising step (`vdx_cofuse_cfg_mimic_stats_f16`): `cfg_mimic_stats` of the noise
    fused from the windows as `cofuse_cfg_ddim_step` fuses it, over the whole clip.  z gives the shape only."""
    head, tail = _cofuse_args("cofuse_cfg_mimic_stats", z, windows, table, wn)
    ws, wp, _ = _mimic_ws("cofuse_cfg_mimic_stats", z.shape, z, ws)
    ms, k, f = mimic
    _launch("vdx_cofuse_cfg_mimic_stats_f16", *head[1:], float(guidance), float(ms), int(k), float(f), wp, int(stages), *tail)
    return ws


def cofuse_cfg_mimic_ddim_step(z, windows, table, wn, guidance, coeffs, ws, out=None):
    """`cofuse_cfg_ddim_step` with the thresholded guided noise (`vdx_cofuse_cfg_mimic_ddim_step_f16`)."""
    return _co_step("vdx_cofuse_cfg_mimic_ddim_step_f16", z, windows, table, wn, None, guidance, coeffs, None, out, mimic_ws=ws)


def cofuse_cfg_mimic_dpm_step(z, windows, table, wn, guidance, coeffs, ws, x0_prev=None, x0_out=None, out=None):
    """`cofuse_cfg_dpm_step` with the thresholded guided noise (`vdx_cofuse_cfg_mimic_dpm_step_f16`) -> (z', x0)."""
    return _co_step("vdx_cofuse_cfg_mimic_dpm_step_f16", z, windows, table, wn, None, guidance, coeffs, (x0_prev, x0_out), out,
                    mimic_ws=ws)


# --------------------------------------------------------------------------------------------
# Masked video-to-video (vdx/inpaint.py, csrc/inpaint.hip; no reference counterpart)
def check_latent_mask(m, T: int, H: int, W: int, what: str = "latent mask"):
    """`m` is a contiguous uint8 (T,H,W) GPU tensor holding only 0 (keep) and 1 (regenerate); `VdxError` / `ValueError`
    otherwise, before any launch.  The values are read ONCE (one sync): the tensor is then tagged with torch's version counter,
    as `cfg_input` tags its result, and checked again only after somebody wrote it."""
    if not torch.is_tensor(m) or not m.is_cuda or m.dtype != torch.uint8 or tuple(m.shape) != (T, H, W) or not m.is_contiguous():
        raise VdxError(f"{what}: expected a contiguous uint8 ({T},{H},{W}) GPU tensor, got "
                       f"{getattr(m, 'dtype', type(m))} {tuple(getattr(m, 'shape', ()))}")
    if getattr(m, "_vdx_mask01", None) != m._version:
        top = int(m.max())
        if top > 1:
            raise ValueError(f"{what}: values must be 0 (keep) or 1 (regenerate), found {top}")
        m._vdx_mask01 = m._version
    return m


def _mask_clip_args(what, z, x0, base, m):
    """Shared checks of the two latent selects: z (1,C,L,H,W), x0 / base (1,C,T,H,W) fp16, m (T,H,W) -> (C, T, L, HW)."""
    if z.dim() != 5 or z.shape[0] != 1 or not z.is_contiguous():
        raise VdxError(f"{what}: z must be contiguous (1,C,L,H,W)")
    _, Cc, L, H, W = z.shape
    if x0.dim() != 5 or tuple(x0.shape[:2]) != (1, Cc) or tuple(x0.shape[3:]) != (H, W) or not x0.is_contiguous():
        raise VdxError(f"{what}: x0 {tuple(x0.shape)} must be contiguous (1,{Cc},T,{H},{W})")
    T = x0.shape[2]
    if base is not None and (tuple(base.shape) != tuple(x0.shape) or not base.is_contiguous()):
        raise VdxError(f"{what}: base must be contiguous and shaped like x0")
    check_latent_mask(m, T, H, W, f"{what}: mask")
    if min(Cc, L, T, H * W) < 1:
        raise VdxError(f"{what}: empty tensor")
    return Cc, T, L, H * W


def mask_renoise(z, x0, base, m, sqrt_ab: float, sqrt_1mab: float, last: bool, s: int):
    """After a scheduler step, IN PLACE on a window's latent z (1,C,L,H,W) fp16 (include/vdx.h `vdx_mask_renoise_f16`): where
    m == 1 z keeps its bits; where m == 0 it takes `add_noise(x0, base, sqrt_ab, sqrt_1mab)`'s, or x0's own with `last`.
    x0, base (1,C,T,H,W) and m (T,H,W) uint8 in {0,1} are the clip's, read at frames [s, s + L).  -> z"""
    Cc, T, L, HW = _mask_clip_args("mask_renoise", z, x0, None if last else base, m)
    s = int(s)
    if not (0 <= s and s + L <= T):
        raise VdxError(f"mask_renoise: window [{s},{s + L}) leaves the clip's {T} frames")
    _launch("vdx_mask_renoise_f16", _p(z, "z"), _p(x0, "x0"), None if last else _p(base, "base"), _p(m, "mask", torch.uint8),
            float(sqrt_ab), float(sqrt_1mab), int(bool(last)), Cc, T, HW, s, L)
    return z


def mask_paste_f32(z, x0, m):
    """IN PLACE on the fp32 blended latent z (1,C,T,H,W): `torch.where(m, z, x0.float())` (`vdx_mask_paste_f32`).  -> z"""
    Cc, T, L, HW = _mask_clip_args("mask_paste_f32", z, x0, None, m)
    if L != T:
        raise VdxError(f"mask_paste_f32: z has {L} frames, the clip {T}")
    _launch("vdx_mask_paste_f32", _p(z, "z", torch.float32), _p(x0, "x0"), _p(m, "mask", torch.uint8), Cc, T, HW)
    return z


MASK_RULES = ("nearest", "any")


def mask_to_latent(pixel_mask, rule: str = "nearest"):
    """Pixel mask (T,H,W) uint8 / bool on the GPU, nonzero = regenerate -> latent mask (T,H/8,W/8) uint8 in {0,1}
    (`vdx_mask_to_latent_u8`).  "nearest": pixel (8y, 8x); "any": a cell regenerates if any of its 64 pixels does."""
    if rule not in MASK_RULES:
        raise ValueError(f"mask_to_latent: rule must be one of {MASK_RULES}, got {rule!r}")
    if pixel_mask.dtype == torch.bool:
        pixel_mask = pixel_mask.view(torch.uint8)
    if not pixel_mask.is_cuda or pixel_mask.dtype != torch.uint8 or pixel_mask.dim() != 3 or not pixel_mask.is_contiguous():
        raise VdxError(f"mask_to_latent: expected a contiguous uint8 (T,H,W) GPU tensor, got {pixel_mask.dtype} "
                       f"{tuple(pixel_mask.shape)}")
    T, H, W = pixel_mask.shape
    if T < 1 or H < 8 or W < 8 or H % 8 or W % 8:
        raise VdxError(f"mask_to_latent: ({T},{H},{W}): H and W must be positive multiples of 8")
    out = torch.empty((T, H // 8, W // 8), dtype=torch.uint8, device=pixel_mask.device)
    _launch("vdx_mask_to_latent_u8", _p(pixel_mask, "pixel_mask", torch.uint8), _p(out, "out", torch.uint8), T, H, W,
            int(rule == "any"))
    out._vdx_mask01 = out._version             # {0,1} by construction
    return out


def mask_composite_u8(generated, original, mask, out=None):
    """`torch.where(mask[..., None] != 0, generated, original)` on contiguous uint8 (T,H,W,3) GPU frames with a (T,H,W) uint8
    mask (`vdx_mask_composite_u8`).  `out` may be `generated`."""
    if out is None:
        out = torch.empty_like(generated)
    for name, t in (("generated", generated), ("original", original), ("out", out)):
        if not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or not t.is_contiguous() \
                or tuple(t.shape) != tuple(generated.shape):
            raise VdxError(f"mask_composite_u8: {name} must be contiguous uint8 (T,H,W,3) on the GPU, all of one shape; got "
                           f"{t.dtype} {tuple(t.shape)}")
    T, H, W, _ = generated.shape
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if not mask.is_cuda or mask.dtype != torch.uint8 or tuple(mask.shape) != (T, H, W) or not mask.is_contiguous():
        raise VdxError(f"mask_composite_u8: mask must be contiguous uint8 ({T},{H},{W}) on the GPU, got {mask.dtype} "
                       f"{tuple(mask.shape)}")
    if T * H * W == 0:
        raise VdxError("mask_composite_u8: empty frames")
    ptr = lambda t: t.data_ptr()     # noqa: E731 (byte tensors: a view may start anywhere, the library picks the access width)
    _launch("vdx_mask_composite_u8", ptr(generated), ptr(original), ptr(mask), ptr(out), T, H, W)
    return out


# --------------------------------------------------------------------------------------------
# Persistent-grid reserve and box probes (include/vdx.h, last section): not on the denoising path
def set_reserved_cus(n: int) -> int:
    """Leave `n` compute units free in every persistent grid (weights-stationary GEMMs, K5 / K7 / K8) for the channel kernels
    of a collective that runs beside the step (vdx/shard.py sets it for world > 1).  Results do not depend on it.
    Returns the CU count the persistent grids now fill."""
    lib = _lib.load()
    _lib.check(lib.vdx_set_reserved_cus(int(n)), "vdx_set_reserved_cus")
    _PLAN_CACHE.clear()          # the tiled GEMM's split rows depend on the reserve (vdx_gemm_plan: rounds of the unreserved CUs)
    return lib.vdx_persistent_grid_cus()


def reserved_cus() -> int:
    return _lib.load().vdx_reserved_cus()


def probe_mfma(device, iters: int = 4000, repeats: int = 3) -> float:
    """Sustained TFLOP/s of a FIXED dense fp16 MFMA stream on this part, in this process (`vdx_probe_mfma_f16`): what the
    box gives the instruction every matrix kernel of the library is made of.  Median of `repeats` timed launches after one
    warm-up launch (~20 ms each at the default `iters`)."""
    n = 2 * torch.cuda.get_device_properties(device).multi_processor_count * 256
    scratch = torch.empty(n, dtype=torch.float32, device=device)
    flops = C.c_double(0.0)
    times = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _launch("vdx_probe_mfma_f16", _p(scratch, "scratch", torch.float32), n, iters, C.byref(flops))
        e1.record()
        e1.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    times.sort()
    return flops.value / (times[len(times) // 2] * 1e-3) / 1e12


def occupancy_hog(blocks: int, lds_bytes: int, micros: int, stream=None) -> None:
    """Enqueue `blocks` workgroups that hold `lds_bytes` of a CU's LDS each for `micros` us and touch no memory — a stand-in
    for the CUs a collective's channel kernels hold (one-GPU rehearsal of the distributed path, bench.py --hog)."""
    st = stream.cuda_stream if stream is not None else _stream()
    _lib.check(_lib.load().vdx_probe_occupancy_hog(int(blocks), int(lds_bytes), int(micros), st), "vdx_probe_occupancy_hog")


# --------------------------------------------------------------------------------------------
# Video-to-video refinement (include/vdx.h, last section): resize, frames -> conv_in rows, posterior, add_noise
_RESIZE_TABLES: dict = {}   # (in_size, out_size, filter, device) -> (bounds, coeffs) int32 device tensors


def _resize_table(in_size: int, out_size: int, filter: str, device):
    key = (in_size, out_size, filter, str(device))
    t = _RESIZE_TABLES.get(key)
    if t is None:
        b, k = clip_resize_coeffs(in_size, out_size, filter)
        t = _RESIZE_TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device))
    return t


def resize_u8(frames, height: int, width: int, filter: str = "bicubic"):
    """uint8 RGB (F, Hi, Wi, 3) on the GPU -> (F, height, width, 3): `PIL.Image.resize((width, height))` bit for bit
    (default filter BICUBIC; 22-bit weights, horizontal pass then vertical, uint8 intermediate).  As in Pillow, a pass whose
    size does not change is skipped (both unchanged: a copy), and a frame more than 100 times taller than wide whose height
    shrinks gets the vertical pass first (`pillow_resizes_vertically_first`)."""
    F, Hi, Wi = check_u8_frames(frames, "resize_u8")
    if height <= 0 or width <= 0:
        raise VdxError(f"resize_u8: target {height}x{width}")
    dev = frames.device
    out = torch.empty((F, height, width, 3), dtype=torch.uint8, device=dev)
    if Hi == height and Wi == width:
        return out.copy_(frames)
    src = frames
    if Wi != width and pillow_resizes_vertically_first(Hi, Wi, height):
        src = torch.empty((F, height, Wi, 3), dtype=torch.uint8, device=dev)
        b, k = _resize_table(Hi, height, filter, dev)
        _launch("vdx_resample_v_u8", *_u8_args(frames), F, Hi, Wi, b.data_ptr(), k.data_ptr(), k.shape[1], height, *_u8_args(src))
        Hi = height
    if Wi != width:
        mid = out if Hi == height else torch.empty((F, Hi, width, 3), dtype=torch.uint8, device=dev)
        b, k = _resize_table(Wi, width, filter, dev)
        _launch("vdx_resample_h_u8", *_u8_args(src), F, Hi, Wi, b.data_ptr(), k.data_ptr(), k.shape[1], width, *_u8_args(mid))
        src = mid
    if Hi != height:
        b, k = _resize_table(Hi, height, filter, dev)
        _launch("vdx_resample_v_u8", *_u8_args(src), F, Hi, width, b.data_ptr(), k.data_ptr(), k.shape[1], height, *_u8_args(out))
    return out


_U8_MAP: dict = {}      # device -> fp16 [256]


def u8_to_unit_lut():
    """The diffusers video preprocessing of one uint8 value, cast to the VAE dtype: fp16(float32(u) / 255 * 2 - 1)
    (numpy float32, every op rounded, as VideoProcessor's pil_to_numpy + normalize evaluate it)."""
    import numpy as np
    u = np.arange(256, dtype=np.float32)
    x = u / np.float32(255.0)
    x = np.float32(2.0) * x
    x = x - np.float32(1.0)
    return torch.from_numpy(x.astype(np.float16))


def frames_to_conv_in(frames, out=None):
    """uint8 (F, H, W, 3) on the GPU -> fp16 rows [F*H*W][64]: the im2col operand of the encoder's conv_in (K = tap*3 + c,
    columns 27..63 zero) of the mapped frames (`u8_to_unit_lut`), zero outside the image — the same rows `conv_in` builds
    from the mapped (F, 3, 1, H, W) tensor."""
    F, H, W = check_u8_frames(frames, "frames_to_conv_in")
    dev = frames.device
    lut = _U8_MAP.get(str(dev))
    if lut is None:
        lut = _U8_MAP[str(dev)] = u8_to_unit_lut().to(dev)
    out, ldo = _out(out, F * H * W, 64, frames, "frames_to_conv_in")
    _launch("vdx_frames_to_conv_in_u8", *_u8_args(frames), F, H, W, lut.data_ptr(), _p(out, "out"), ldo)
    return out


def vae_posterior(moments, n: int, hw: int, eps=None, scale: float = 1.0, out=None, out_offset: int = 0, out_strides=None):
    """DiagonalGaussianDistribution over the encoder's moment rows [n*hw][ld] (mean columns 0..3, logvar 4..7):
    scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps), or scale * mean without `eps` (mode), fp16 after every op.
    Default output (n, 4, h*w); a contiguous `out` + `out_offset` (elements) + `out_strides` = (channel, image) element strides
    write elsewhere, e.g. frames f0.. of a (1, 4, T, h, w) latent: offset f0*hw, strides (T*hw, hw)."""
    r, c, ld = _rows(moments, "moments")
    if r < n * hw or c < 8:
        raise VdxError(f"vae_posterior: moments {tuple(moments.shape)} smaller than [{n * hw}][8]")
    if eps is not None and (eps.dtype != torch.float16 or not eps.is_contiguous() or eps.numel() != n * 4 * hw
                            or eps.device != moments.device):
        raise VdxError("vae_posterior: eps must be contiguous fp16 (n, 4, h, w) on the moments' device")
    if out is None:
        out = torch.empty((n, 4, hw), dtype=torch.float16, device=moments.device)
        out_strides = (hw, 4 * hw)
    elif out_strides is None or out.dtype != torch.float16 or not out.is_contiguous() or out.device != moments.device:
        raise VdxError("vae_posterior: an explicit `out` must be contiguous fp16 on the moments' device, with out_strides")
    cs, fs = out_strides
    if out_offset < 0 or out_offset + 3 * cs + (n - 1) * fs + hw > out.numel():
        raise VdxError("vae_posterior: out too small for its offset and strides")
    _launch("vdx_vae_posterior_f16", _p(moments, "moments"), ld, n, hw, eps.data_ptr() if eps is not None else None,
            int(eps is None), float(scale), out.data_ptr() + 2 * out_offset, cs, fs)
    return out


def add_noise(x0, noise, sqrt_ab: float, sqrt_1mab: float, out=None):
    """DDIMScheduler.add_noise with fp16 coefficients: fp16(fp16(sqrt_ab * x0) + fp16(sqrt_1mab * noise))."""
    if x0.shape != noise.shape or x0.dtype != torch.float16 or noise.dtype != torch.float16 \
            or not (x0.is_contiguous() and noise.is_contiguous()):
        raise VdxError("add_noise: x0 and noise must be contiguous fp16 tensors of one shape")
    if out is None:
        out = torch.empty_like(x0)
    _launch("vdx_add_noise_f16", _p(x0, "x0"), _p(noise, "noise"), _p(out, "out"), float(sqrt_ab), float(sqrt_1mab), x0.numel())
    return out


# --------------------------------------------------------------------------------------------
# MD-VQS: LPIPS-AlexNet and the authenticity gate's frame statistics (InferNet/template/validator/scoring.py:13-67, :269-309;
# include/vdx.h "MD-VQS"; csrc/mdvqs.hip)
LPIPS_STEM_OUT, LPIPS_STEM_K, LPIPS_STEM_KPAD = 55, 363, 384


def lpips_stem(u8, lut, out=None):
    """Resized uint8 frames (F, 224, 224, 3), contiguous on the GPU, -> conv1's im2col rows fp16 [F*3025][384] through the
    fp16 [3][256] table of both affine maps (`vdx.lpips.stem_lut`); see vdx_lpips_stem_u8."""
    F, H, W = check_u8_frames(u8, "lpips_stem")
    if (H, W) != (CLIP_IMAGE, CLIP_IMAGE) or not u8.is_contiguous():
        raise VdxError(f"lpips_stem: expected contiguous (F, 224, 224, 3) frames, got {tuple(u8.shape)}")
    if lut.shape != (3, 256) or not lut.is_contiguous() or lut.device != u8.device:
        raise VdxError("lpips_stem: lut must be contiguous fp16 [3][256] on the frames' device")
    out, ldo = _out(out, F * LPIPS_STEM_OUT * LPIPS_STEM_OUT, LPIPS_STEM_KPAD, u8, "lpips_stem")
    _launch("vdx_lpips_stem_u8", u8.data_ptr(), F, _p(lut, "lut"), _p(out, "out"), ldo)
    return out


def relu(x, out=None):
    """max(x, 0) like torch.relu (vdx_relu_f16); `out=x` runs in place."""
    if not x.is_contiguous():
        raise VdxError("relu: x must be contiguous")
    if out is None:
        out = torch.empty_like(x)
    if out.shape != x.shape or not out.is_contiguous():
        raise VdxError("relu: out must be contiguous and shaped like x")
    _launch("vdx_relu_f16", _p(x, "x"), _p(out, "out"), x.numel())
    return out


def relu_maxpool(x, *, n_img, H, W, out=None):
    """Rows x [n_img*H*W][C] are ReLU'd in place; -> rows [n_img*Ho*Wo][C] of MaxPool2d(3, stride 2) over them,
    Ho = (H - 3) // 2 + 1 (vdx_relu_maxpool_f16)."""
    r, Cc, ldx = _rows(x, "x")
    if r < n_img * H * W or H < 3 or W < 3 or Cc % 8:
        raise VdxError(f"relu_maxpool: x {tuple(x.shape)} does not hold {n_img} images of {H}x{W} (C % 8 == 0, H, W >= 3)")
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out, ldo = _out(out, n_img * Ho * Wo, Cc, x, "relu_maxpool")
    _launch("vdx_relu_maxpool_f16", _p(x, "x"), ldx, n_img, H, W, Cc, _p(out, "out"), ldo)
    return out


def im2col(x, *, n_img, H, W, k, pad, out=None):
    """Channels-last rows x [n_img*H*W][C] (C % 64 == 0) -> stride-1 im2col rows [n_img*Ho*Wo][k*k*C], column
    (ky*k + kx)*C + c, zero outside the image (vdx_im2col_f16)."""
    r, Cc, ldx = _rows(x, "x")
    if r < n_img * H * W or Cc % 64 or not (1 <= k <= 11) or not (0 <= pad < k) or H + 2 * pad < k or W + 2 * pad < k:
        raise VdxError(f"im2col: x {tuple(x.shape)}, {n_img} images of {H}x{W}, k={k}, pad={pad}: not supported")
    Ho, Wo = H + 2 * pad - k + 1, W + 2 * pad - k + 1
    out, ldo = _out(out, n_img * Ho * Wo, k * k * Cc, x, "im2col")
    _launch("vdx_im2col_f16", _p(x, "x"), ldx, n_img, H, W, Cc, k, pad, _p(out, "out"), ldo)
    return out


def lpips_distance(x, lin, *, F, HW, out=None):
    """One LPIPS tap over the F-1 consecutive pairs of tap rows x fp16 [F*HW][C] with fp32 `lin` [C] -> fp32 [F-1]; a given
    `out` is added to (the sum over taps).  vdx_lpips_distance_f16."""
    r, Cc, ldx = _rows(x, "x")
    if F < 2 or r < F * HW or Cc > 512 or lin.numel() != Cc or not lin.is_contiguous():
        raise VdxError(f"lpips_distance: x {tuple(x.shape)}, lin {tuple(lin.shape)}, F={F}, HW={HW}: shapes do not match (C <= 512)")
    acc = out is not None
    if out is None:
        out = torch.empty(F - 1, dtype=torch.float32, device=x.device)
    if out.numel() != F - 1 or not out.is_contiguous():
        raise VdxError("lpips_distance: out must be contiguous fp32 [F-1]")
    _launch("vdx_lpips_distance_f16", _p(x, "x"), ldx, F, HW, Cc, _p(lin, "lin", torch.float32), _p(out, "out", torch.float32), int(acc))
    return out


def frame_stats(frames):
    """uint8 RGB frames (F, H, W, 3) on the GPU (rows and frames may be pitched) -> (grey histograms int32 [F][256] holding
    the uint32 counts, absolute-difference sums int64 [F-1] holding the uint64 sums); vdx_frame_stats_u8.  torch has no
    arithmetic on unsigned 32 / 64-bit tensors: the counts (< 2^31 for H*W < 2^31) and sums (< 2^63) are read as signed."""
    F, H, W = check_u8_frames(frames, "frame_stats")
    if H * W >= 1 << 31:
        raise VdxError("frame_stats: H*W must stay below 2^31")
    hist = torch.empty((F, 256), dtype=torch.int32, device=frames.device)
    diff = torch.empty((max(F - 1, 1),), dtype=torch.int64, device=frames.device)
    _launch("vdx_frame_stats_u8", *_u8_args(frames), F, H, W, hist.data_ptr(), diff.data_ptr() if F > 1 else None)
    return hist, diff[:F - 1]


# --------------------------------------------------------------------------------------------
# Farneback optical flow (cv2_shim.py:99-182; scoring.py:311-339, fsdp_chunked_coherent.py:236-246; include/vdx.h
# "Farneback"; csrc/flow.hip).  vdx/flow.py drives these; images are packed fp32 [n][H][W], flows fp32 [P][H][W][2].
def _f32(t, shape, what, name):
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise VdxError(f"{what}: {name} must be contiguous fp32 {tuple(shape)} on the GPU, got {t.dtype} {tuple(t.shape)}")
    return t.data_ptr()


def flow_grey(frames, bgr: bool = False):
    """uint8 RGB frames (F, H, W, 3) on the GPU -> fp32 grey (F, H, W) with OpenCV's 8-bit weights; `bgr`: COLOR_BGR2GRAY
    applied to the same bytes (vdx_flow_grey_u8)."""
    F, H, W = check_u8_frames(frames, "flow_grey")
    out = torch.empty((F, H, W), dtype=torch.float32, device=frames.device)
    _launch("vdx_flow_grey_u8", *_u8_args(frames), F, H, W, int(bool(bgr)), out.data_ptr())
    return out


def flow_corr1d(img, taps, axis: int):
    """correlate1d(img, taps, axis, mode="mirror") of fp32 images (n, H, W); taps fp32 [2r + 1] on the GPU (vdx_flow_corr1d_f32)."""
    if img.dim() != 3 or axis not in (0, 1):
        raise VdxError(f"flow_corr1d: expected images (n, H, W) and axis 0 or 1, got {tuple(img.shape)}, axis {axis}")
    n, H, W = img.shape
    if taps.dim() != 1 or taps.numel() % 2 != 1 or taps.device != img.device:
        raise VdxError("flow_corr1d: taps must be an odd-length vector on the images' device")
    out = torch.empty_like(img)
    _launch("vdx_flow_corr1d_f32", _f32(img, (n, H, W), "flow_corr1d", "img"), out.data_ptr(), n, H, W,
            _f32(taps, taps.shape, "flow_corr1d", "taps"), taps.numel() // 2, axis)
    return out


def flow_resize(x, height: int, width: int, mul: float = 1.0):
    """`_resize_linear` of fp32 images (n, H, W) or flows (n, H, W, 2) to (height, width), times `mul` (vdx_flow_resize_f32)."""
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[3] != 2) or height <= 0 or width <= 0:
        raise VdxError(f"flow_resize: expected (n, H, W) or (n, H, W, 2) and a positive size, got {tuple(x.shape)} -> {height}x{width}")
    n, H, W = x.shape[:3]
    Cc = 1 if x.dim() == 3 else 2
    out = torch.empty((n, height, width) + tuple(x.shape[3:]), dtype=torch.float32, device=x.device)
    _launch("vdx_flow_resize_f32", _f32(x, x.shape, "flow_resize", "x"), n, H, W, Cc, out.data_ptr(), height, width, float(mul))
    return out


def flow_polyexp(img, taps, inv_g):
    """`_poly_exp` (poly_n 5) of fp32 images (n, H, W) -> (n, 5, H, W) = bx, by, axx, ayy, axy.  `taps` (3, 11) and `inv_g` (5, 6):
    host arrays (`vdx.flow.poly_tables`), passed as float64 kernel arguments; fp64 arithmetic, fp32 planes (vdx_flow_polyexp_f32)."""
    import numpy as np
    if img.dim() != 3:
        raise VdxError(f"flow_polyexp: expected images (n, H, W), got {tuple(img.shape)}")
    n, H, W = img.shape
    k, g = np.ascontiguousarray(taps, np.float64), np.ascontiguousarray(inv_g, np.float64)
    if k.shape != (3, 11) or g.shape != (5, 6):
        raise VdxError(f"flow_polyexp: taps {k.shape} / inv_g {g.shape}: expected (3, 11) and (5, 6)")
    out = torch.empty((n, 5, H, W), dtype=torch.float32, device=img.device)
    fp = C.POINTER(C.c_double)
    _launch("vdx_flow_polyexp_f32", _f32(img, (n, H, W), "flow_polyexp", "img"), n, H, W, k.ctypes.data_as(fp), g.ctypes.data_as(fp),
            out.data_ptr())
    return out


def flow_update(R, flow, step: int = 1, out=None):
    """One `_update_flow` iteration for every pair: R (n, 5, H, W) expansions, flow (P, H, W, 2); pair p uses images p*step and
    p*step + 1 -> the new flow (P, H, W, 2) (`out`, which may not be `flow`); fp64 arithmetic on fp32 planes.  vdx_flow_update_f32."""
    if R.dim() != 4 or R.shape[1] != 5 or flow.dim() != 4 or flow.shape[3] != 2:
        raise VdxError(f"flow_update: expected R (n, 5, H, W) and flow (P, H, W, 2), got {tuple(R.shape)}, {tuple(flow.shape)}")
    n, _, H, W = R.shape
    P = flow.shape[0]
    if step not in (1, 2) or P < 1 or (P - 1) * step + 2 > n or tuple(flow.shape[1:3]) != (H, W) or flow.device != R.device:
        raise VdxError(f"flow_update: {P} pairs of step {step} at {tuple(flow.shape[1:3])} do not fit {n} expansions at {(H, W)}")
    if out is None:
        out = torch.empty_like(flow)
    if out.data_ptr() == flow.data_ptr():
        raise VdxError("flow_update: out may not be the input flow")
    _launch("vdx_flow_update_f32", _f32(R, R.shape, "flow_update", "R"), _f32(flow, flow.shape, "flow_update", "flow"),
            _f32(out, flow.shape, "flow_update", "out"), P, step, H, W)
    return out


def flow_abs_sum(flow):
    """fp32 flows (P, H, W, 2) -> fp32 [P], the sum of |flow| of each pair in a fixed order (vdx_flow_abs_sum_f32)."""
    if flow.dim() != 4 or flow.shape[0] < 1:
        raise VdxError(f"flow_abs_sum: expected flows (P, H, W, 2), got {tuple(flow.shape)}")
    P = flow.shape[0]
    ws = torch.empty((P, 64), dtype=torch.float32, device=flow.device)
    out = torch.empty((P,), dtype=torch.float32, device=flow.device)
    _launch("vdx_flow_abs_sum_f32", _f32(flow, flow.shape, "flow_abs_sum", "flow"), P, flow[0].numel(), ws.data_ptr(), out.data_ptr())
    return out


def flow_remap_absdiff(frames, flow, step: int = 1, want_warped: bool = False):
    """uint8 RGB frames (F, H, W, 3) and flows (P, H, W, 2): pair p warps frame p*step by its flow (`cv2.remap`, bilinear,
    constant-0 border) and compares it with frame p*step + 1 -> (int64 [P] sums of |warp - next| over all bytes, the warped
    frames uint8 (P, H, W, 3) or None).  vdx_flow_remap_absdiff_u8."""
    F, H, W = check_u8_frames(frames, "flow_remap_absdiff")
    if flow.dim() != 4 or flow.shape[0] < 1 or tuple(flow.shape[1:]) != (H, W, 2) or flow.device != frames.device:
        raise VdxError(f"flow_remap_absdiff: flow {tuple(flow.shape)} does not match frames {(H, W)}")
    P = flow.shape[0]
    if step not in (1, 2) or (P - 1) * step + 2 > F:
        raise VdxError(f"flow_remap_absdiff: {P} pairs of step {step} need more than {F} frames")
    diff = torch.empty((P,), dtype=torch.int64, device=frames.device)
    warped = torch.empty((P, H, W, 3), dtype=torch.uint8, device=frames.device) if want_warped else None
    _launch("vdx_flow_remap_absdiff_u8", *_u8_args(frames), _f32(flow, flow.shape, "flow_remap_absdiff", "flow"), P, step, H, W,
            diff.data_ptr(), warped.data_ptr() if want_warped else None)
    return diff, warped


# --------------------------------------------------------------------------------------------
# Motion-compensated frame interpolation (no reference counterpart; include/vdx.h "interpolation"; csrc/interp.hip).
# vdx/interp.py computes the flows and calls this.
def interp_frames(frames, fab, fba, factor: int, out=None):
    """uint8 RGB frames (F, H, W, 3), F >= 2, and their flows fab (frame i -> i+1) and fba (frame i+1 -> i), fp32 (F-1, H, W, 2),
    all on the GPU -> uint8 ((F-1)*factor + 1, H, W, 3): frame i*factor is frame i, the factor-1 frames after it are the
    motion-compensated blends at k / factor (tests/interp_ref.py states them).  One launch (vdx_interp_frames_u8)."""
    F, H, W = check_u8_frames(frames, "interp_frames")
    if isinstance(factor, bool) or not isinstance(factor, int) or not 1 <= factor <= 64:
        raise VdxError(f"interp_frames: factor must be an integer in 1..64, got {factor!r}")
    if F < 2:
        raise VdxError(f"interp_frames: at least two frames are needed, got {F}")
    for name, fl in (("fab", fab), ("fba", fba)):
        if fl.device != frames.device:
            raise VdxError(f"interp_frames: {name} is on {fl.device}, the frames on {frames.device}")
        _f32(fl, (F - 1, H, W, 2), "interp_frames", name)
    n_out = (F - 1) * factor + 1
    if out is None:
        out = torch.empty((n_out, H, W, 3), dtype=torch.uint8, device=frames.device)
    elif (not out.is_cuda or out.device != frames.device or out.dtype != torch.uint8 or tuple(out.shape) != (n_out, H, W, 3)
          or not out.is_contiguous()):
        raise VdxError(f"interp_frames: out must be contiguous uint8 {(n_out, H, W, 3)} on the frames' device")
    _launch("vdx_interp_frames_u8", *_u8_args(frames), fab.data_ptr(), fba.data_ptr(), F, H, W, factor, out.data_ptr(), out.stride(0))
    return out


# --------------------------------------------------------------------------------------------
# Full-reference clip comparison: SSE / SSIM / MS-SSIM (no reference counterpart; include/vdx.h "comparison"; csrc/compare.hip).
# vdx/compare.py drives these and turns the means into the metrics; planes between the scales are packed fp32 [n][H][W].
COMPARE_TAPS, COMPARE_SCALES = 11, 5


def compare_tiles(H: int, W: int) -> int:
    """Blocks per plane of `compare_ssim_scale` at H x W; `VdxError` for a size the kernel does not take (min(H, W) < 11)."""
    n = _lib.load().vdx_compare_tiles(int(H), int(W))
    if n <= 0:
        raise VdxError(f"compare: planes of {H}x{W} are outside what the kernel takes (H, W >= {COMPARE_TAPS}, H*W < 2^28)")
    return n


def _compare_pair(a, b, what):
    """-> (is_u8, n_planes, H, W) of two uint8 RGB clips (F, H, W, 3) or two packed fp32 plane stacks (n, H, W) on one GPU."""
    if a.dtype == torch.uint8:
        F, H, W = check_u8_frames(a, what)
        if b is not None and (check_u8_frames(b, what) != (F, H, W) or b.device != a.device):
            raise VdxError(f"{what}: b {tuple(b.shape)} on {b.device} does not match a {tuple(a.shape)} on {a.device}")
        return True, 3 * F, H, W
    if a.dim() != 3 or a.shape[0] < 1:
        raise VdxError(f"{what}: expected uint8 frames (F, H, W, 3) or fp32 planes (n, H, W), got {a.dtype} {tuple(a.shape)}")
    _f32(a, a.shape, what, "a")
    if b is not None:
        if b.device != a.device:
            raise VdxError(f"{what}: b is on {b.device}, a on {a.device}")
        _f32(b, a.shape, what, "b")
    return False, int(a.shape[0]), int(a.shape[1]), int(a.shape[2])


def _compare_taps(taps):
    import numpy as np
    t = np.ascontiguousarray(taps, np.float64)
    if t.shape != (COMPARE_TAPS,):
        raise VdxError(f"compare: taps {t.shape}: expected ({COMPARE_TAPS},)")
    return t, t.ctypes.data_as(C.POINTER(C.c_double))


def compare_ssim_scale(a, b, taps):
    """One scale of every plane pair: a, b uint8 RGB (F, H, W, 3) or packed fp32 planes (n, H, W) on the GPU; `taps` the 11
    float64 window weights (host) -> (partials fp64 (planes, tiles, 2): every block's sums of ssim and cs; for uint8 input the
    blocks' exact sums of (a - b)^2 int64 (planes, tiles), else None).  vdx_compare_ssim_scale_u8 / _f32."""
    u8, n, H, W = _compare_pair(a, b, "compare_ssim_scale")
    if b is None:
        raise VdxError("compare_ssim_scale: two clips are needed")
    tiles = compare_tiles(H, W)
    t, tp = _compare_taps(taps)
    part = torch.empty((n, tiles, 2), dtype=torch.float64, device=a.device)
    if u8:
        sse = torch.empty((n, tiles), dtype=torch.int64, device=a.device)
        _launch("vdx_compare_ssim_scale_u8", *_u8_args(a), *_u8_args(b), n // 3, H, W, tp, part.data_ptr(), sse.data_ptr())
        return part, sse
    _launch("vdx_compare_ssim_scale_f32", a.data_ptr(), b.data_ptr(), n, H, W, tp, part.data_ptr())
    return part, None


def compare_down2(a, b=None):
    """2x2 mean (fp32, ((p00 + p01) + (p10 + p11)) * 0.25; an odd last row or column is dropped) of every plane of `a` and, when
    given, `b`: uint8 RGB (F, H, W, 3) -> fp32 (3F, H/2, W/2), fp32 (n, H, W) -> (n, H/2, W/2).  -> out_a, or (out_a, out_b).
    vdx_compare_down2_u8 / _f32."""
    u8, n, H, W = _compare_pair(a, b, "compare_down2")
    if H < 2 or W < 2:
        raise VdxError(f"compare_down2: planes of {H}x{W} cannot be halved")
    oa = torch.empty((n, H // 2, W // 2), dtype=torch.float32, device=a.device)
    ob = torch.empty_like(oa) if b is not None else None
    pob = ob.data_ptr() if b is not None else None
    if u8:
        _launch("vdx_compare_down2_u8", *_u8_args(a), *_u8_args(b), n // 3, H, W, oa.data_ptr(), pob)
    else:
        _launch("vdx_compare_down2_f32", a.data_ptr(), b.data_ptr() if b is not None else None, n, H, W, oa.data_ptr(), pob)
    return oa if b is None else (oa, ob)


def compare_finalize(partials, sse_partials, count: int, scale: int, means, sse=None):
    """The blocks' partials (planes, tiles, 2) of one scale, planes = 3 F, summed in a fixed order over `count` positions into
    means[:, :, scale, :] (fp64 (F, 3, 5, 2): ssim, cs); with `sse_partials` (scale 0) also sse (int64 [F]).  vdx_compare_finalize."""
    if (partials.dim() != 3 or partials.shape[2] != 2 or partials.shape[0] % 3 or partials.dtype != torch.float64
            or not partials.is_cuda or not partials.is_contiguous()):
        raise VdxError(f"compare_finalize: partials must be contiguous fp64 (3F, tiles, 2) on the GPU, got {tuple(partials.shape)}")
    F, tiles = partials.shape[0] // 3, partials.shape[1]
    if (means.dtype != torch.float64 or tuple(means.shape) != (F, 3, COMPARE_SCALES, 2) or not means.is_contiguous()
            or means.device != partials.device):
        raise VdxError(f"compare_finalize: means must be contiguous fp64 {(F, 3, COMPARE_SCALES, 2)} on the partials' device")
    if (sse_partials is None) != (sse is None):
        raise VdxError("compare_finalize: sse_partials and sse go together")
    if sse is not None:
        for name, t, shape in (("sse_partials", sse_partials, (3 * F, tiles)), ("sse", sse, (F,))):
            if t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != partials.device:
                raise VdxError(f"compare_finalize: {name} must be contiguous int64 {shape} on the partials' device")
    if not 0 <= int(scale) < COMPARE_SCALES or int(count) < 1:
        raise VdxError(f"compare_finalize: scale {scale}, count {count}")
    _launch("vdx_compare_finalize", partials.data_ptr(), sse_partials.data_ptr() if sse is not None else None, F, tiles,
            float(count), int(scale), means.data_ptr(), sse.data_ptr() if sse is not None else None)
    return means


# --------------------------------------------------------------------------------------------
# FreeInit's frequency mix (no reference counterpart; include/vdx.h "FreeInit"; csrc/freeinit.hip).  vdx/freeinit.py builds the
# filter and calls this.
FREEINIT_MAX_AXIS, FREEINIT_MAX_ELEMS = 512, 1 << 30
_FREEINIT_WS: dict = {}     # the complex fp64 workspace of the five launches
_FREEINIT_TW: dict = {}     # (device, N) -> the axis' twiddle table


def freeinit_twiddles(n: int):
    """The table of an axis of length n: float64 (n, 2) on the host, row j = (cos(2 pi j / n), -sin(2 pi j / n))."""
    import numpy as np
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return torch.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], axis=1))


def _freeinit_table(n: int, device) -> torch.Tensor:
    key = (device.index, n)
    tw = _FREEINIT_TW.get(key)
    if tw is None:
        tw = _FREEINIT_TW[key] = freeinit_twiddles(n).to(device)
    return tw


def freeinit_check_sizes(shape) -> tuple:
    """(n_vol, T, h, w) of a (B, C, T, h, w) latent the mix takes: every one of T, h, w in 1..512 and at most 2^30 elements;
    `VdxError` otherwise.  Needs no library."""
    if len(shape) != 5 or any(int(v) < 1 for v in shape):
        raise VdxError(f"freeinit_mix: expected a (B, C, T, h, w) latent, got shape {tuple(shape)}")
    B, Cc, T, h, w = (int(v) for v in shape)
    if max(T, h, w) > FREEINIT_MAX_AXIS or B * Cc * T * h * w > FREEINIT_MAX_ELEMS:
        raise VdxError(f"freeinit_mix: {tuple(shape)} is outside what the kernels take (T, h, w in 1..{FREEINIT_MAX_AXIS}, "
                       f"at most 2^30 elements)")
    return B * Cc, T, h, w


def freeinit_mix(z_t, eta, filt, out=None):
    """z_t fp16 and eta fp32, both (B, C, T, h, w), and the filter fp32 (T, h, w) in fftshift-ed coordinates, all contiguous on
    one GPU -> fp16 (B, C, T, h, w): Re ifftn(ifftshift(fftshift(fftn(z_t)) filt + fftshift(fftn(eta)) (1 - filt))) over the
    last three axes (tests/freeinit_ref.py states it).  Sizes are checked before anything is launched (vdx_freeinit_mix_f16)."""
    n_vol, T, h, w = freeinit_check_sizes(z_t.shape)
    if not z_t.is_cuda or z_t.dtype != torch.float16 or not z_t.is_contiguous():
        raise VdxError(f"freeinit_mix: z_t must be a contiguous fp16 GPU tensor, got {z_t.dtype} on {z_t.device}")
    for name, t, shape in (("eta", eta, tuple(z_t.shape)), ("filt", filt, (T, h, w))):
        if t.device != z_t.device or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise VdxError(f"freeinit_mix: {name} must be contiguous fp32 {shape} on {z_t.device}, got {t.dtype} "
                           f"{tuple(t.shape)} on {t.device}")
    if out is None:
        out = torch.empty_like(z_t)
    elif out.device != z_t.device or out.dtype != torch.float16 or out.shape != z_t.shape or not out.is_contiguous():
        raise VdxError(f"freeinit_mix: out must be contiguous fp16 {tuple(z_t.shape)} on {z_t.device}")
    nbytes = _lib.load().vdx_freeinit_workspace(n_vol, T, h, w)
    if nbytes == 0:
        raise VdxError(f"freeinit_mix: the library refuses the size {tuple(z_t.shape)}")
    with torch.cuda.device(z_t.device):
        ws = _scratch(_FREEINIT_WS, z_t.device, nbytes, torch.float64)
        tw = [_freeinit_table(n, z_t.device) for n in (T, h, w)]
        _launch("vdx_freeinit_mix_f16", z_t.data_ptr(), eta.data_ptr(), filt.data_ptr(), tw[0].data_ptr(), tw[1].data_ptr(),
                tw[2].data_ptr(), n_vol, T, h, w, ws.data_ptr(), ws.numel() * 8, out.data_ptr())
    return out


# --------------------------------------------------------------------------------------------
# FreeU's two operations on the up path's rows (no reference counterpart; include/vdx.h "FreeU"; csrc/freeu.hip).
# unet3d.py calls both, in place, before the ResNets of up blocks 0 and 1.
_FREEU_TW: dict = {}        # (device, N) -> the axis' twiddle table


def freeu_twiddles(n: int):
    """The table of an axis of length n: float64 (n, 2) on the host, row j = (cos(2 pi j / n), -sin(2 pi j / n)); the
    multiples of a quarter turn are exact (numpy's sin(pi) is 1.2e-16)."""
    import numpy as np
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    for j in range(n):
        if 4 * j % n == 0:
            tw[j] = ((1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0))[4 * j // n]
    return torch.from_numpy(tw)


def _freeu_table(n: int, device) -> torch.Tensor:
    key = (device.index, n)
    tw = _FREEU_TW.get(key)
    if tw is None:
        tw = _FREEU_TW[key] = freeu_twiddles(n).to(device)
    return tw


def _freeu_number(what: str, v, positive: bool) -> float:
    import math
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and v <= 0):
        raise ValueError(f"{what} must be a finite{' positive' if positive else ''} number, got {v!r}")
    return float(v)


def _freeu_ptr(t, name: str) -> int:
    """`_p`, except that the one column of a [M][1] matrix has no stride to speak of."""
    return _p(t.as_strided(t.shape, (t.stride(0), 1)) if t.dim() == 2 and t.shape[1] == 1 else t, name)


def freeu_filter(x, *, n_img, h, w, s, out=None):
    """x fp16 rows [n_img * h * w][C], image i owning rows [i h w, (i + 1) h w) -> the rows with every (h, w) plane through
    diffusers' fourier_filter(threshold=1, scale=s): Re ifft2(ifftshift(fftshift(fft2(plane)) M)), M = s on the 2 x 2 centre
    (tests/freeu_ref.py states it), computed in fp64 and rounded once.  `out=x` filters in place."""
    s = _freeu_number("freeu_filter: s", s, False)
    M, C, ldx = _rows(x, "x")
    if n_img < 1 or h < 1 or w < 1 or C < 1 or M != n_img * h * w:
        raise VdxError(f"freeu_filter: {M} rows are not {n_img} images of {h} x {w}")
    out, ldo = _out(out, M, C, x, "freeu_filter")
    if out.shape[0] != M or out.shape[1] != C:
        raise VdxError(f"freeu_filter: out {tuple(out.shape)} != {(M, C)}")
    if out.data_ptr() != x.data_ptr() or ldo != ldx:
        lo, hi = x.data_ptr(), x.data_ptr() + ((M - 1) * ldx + C) * 2
        if out.data_ptr() < hi and lo < out.data_ptr() + ((M - 1) * ldo + C) * 2:
            raise VdxError("freeu_filter: out overlaps x without being x")
    px, po = _freeu_ptr(x, "x"), _freeu_ptr(out, "out")
    with torch.cuda.device(x.device):
        _launch("vdx_freeu_filter_f16", px, ldx, _freeu_table(h, x.device).data_ptr(), _freeu_table(w, x.device).data_ptr(),
                n_img, h, w, C, s, po, ldo)
    return out


def freeu_scale(x, b):
    """x fp16 rows [M][C], IN PLACE: channels [0, C // 2) of every row become fp16(fp32(x) fp32(b)), torch's half-by-scalar
    multiply; the other channels are not touched.  -> x."""
    b = _freeu_number("freeu_scale: b", b, True)
    M, C, ld = _rows(x, "x")
    if M < 1 or C < 1:
        raise VdxError(f"freeu_scale: empty rows {tuple(x.shape)}")
    px = _freeu_ptr(x, "x")
    with torch.cuda.device(x.device):
        _launch("vdx_freeu_scale_f16", px, ld, M, C, b)
    return x


# --------------------------------------------------------------------------------------------
# Token merging around the spatial self-attention (no reference counterpart; include/vdx.h "Token merging"; csrc/tome.hip).
# unet3d.py calls the four in turn when `enable_tome` is set; vdx/tome.py builds the tables.
def _tome_buf(t, n: int, dtype, what: str, name: str, device) -> int:
    """Pointer of a caller-made device buffer of at least n elements of `dtype`."""
    if not torch.is_tensor(t) or not t.is_cuda or t.device != device or t.dtype != dtype or not t.is_contiguous():
        raise VdxError(f"{what}: {name} must be a contiguous {dtype} tensor on {device}")
    if t.numel() < n:
        raise VdxError(f"{what}: {name} has {t.numel()} elements, need {n}")
    return t.data_ptr()


def _tome_args(what, x, src_idx, dst_idx, n_img, S, r, C):
    """The plan's struct with its tables checked: `x` names the device, the tables are int32 of n_src + n_dst = S entries."""
    for name, v in (("n_img", n_img), ("S", S), ("r", r)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise VdxError(f"{what}: {name} must be an integer, got {v!r}")
    if not torch.is_tensor(src_idx) or not torch.is_tensor(dst_idx):
        raise VdxError(f"{what}: src_idx / dst_idx must be tensors")
    n_src, n_dst = src_idx.numel(), dst_idx.numel()
    if n_img < 1 or S < 1 or n_src < 1 or n_dst < 1 or n_src + n_dst != S or not 1 <= r <= n_src or n_img * S > 0x7fffffff // 4:
        raise VdxError(f"{what}: n_img={n_img} S={S} n_src={n_src} n_dst={n_dst} r={r} is not a plan "
                       "(n_src + n_dst = S, each at least 1, 1 <= r <= n_src)")
    a = _lib.TomeArgs()
    a.src_idx = _tome_buf(src_idx, n_src, torch.int32, what, "src_idx", x.device)
    a.dst_idx = _tome_buf(dst_idx, n_dst, torch.int32, what, "dst_idx", x.device)
    a.n_img, a.S, a.n_src, a.n_dst, a.r, a.C = n_img, S, n_src, n_dst, r, C
    return a


def _tome_rows(t, rows: int, C: int, what: str, name: str):
    """-> (pointer, ld) of fp16 rows covering [rows][C] with a row stride that keeps every row 16-byte aligned."""
    n, c, ld = _rows(t, name)
    if n < rows or c != C or ld % 8:
        raise VdxError(f"{what}: {name} {tuple(t.shape)} with row stride {ld} does not cover [{rows}][{C}] in 16-byte rows")
    return _p(t, name), ld


def _tome_disjoint(a, b, what: str, names: str) -> None:
    la, lb = a.data_ptr(), b.data_ptr()
    ha = la + ((a.shape[0] - 1) * a.stride(0) + a.shape[1]) * 2
    hb = lb + ((b.shape[0] - 1) * b.stride(0) + b.shape[1]) * 2
    if la < hb and lb < ha:
        raise VdxError(f"{what}: {names} overlap")


def tome_match(t, src_idx, dst_idx, *, n_img, S):
    """t fp16 rows [n_img * S][C] -> (node_max fp32 [n_img][n_src], node_idx int32 [n_img][n_src]): per image and source i the
    largest cosine similarity to a destination and the lowest j that reaches it (tests/tome_ref.py `match`).  C % 64 == 0,
    C <= 1280.  The score matrix is never stored."""
    what = "tome_match"
    Cc = t.shape[1] if t.dim() == 2 else 0
    if Cc < 64 or Cc % 64 or Cc > 1280:
        raise VdxError(f"{what}: C={Cc} (a multiple of 64 up to 1280)")
    a = _tome_args(what, t, src_idx, dst_idx, n_img, S, 1, Cc)
    pt, ld = _tome_rows(t, n_img * S, Cc, what, "t")
    inv = torch.empty((n_img, S), dtype=torch.float32, device=t.device)
    node_max = torch.empty((n_img, a.n_src), dtype=torch.float32, device=t.device)
    node_idx = torch.empty((n_img, a.n_src), dtype=torch.int32, device=t.device)
    a.inv, a.node_max, a.node_idx = inv.data_ptr(), node_max.data_ptr(), node_idx.data_ptr()
    with torch.cuda.device(t.device):
        _launch("vdx_tome_match_f16", C.byref(a), pt, ld)
    return node_max, node_idx


def tome_select(node_max, node_idx, src_idx, dst_idx, *, S, r):
    """(node_max fp32, node_idx int32) [n_img][n_src] -> (slot int32 [n_img][S], off int32 [n_img][n_dst + 1], items int32
    [n_img][r]): the r sources with the largest node_max (ties: lower i; NaN last) are merged into destination
    clamp(node_idx[i]); slot is the merged row of every token, (off, items) each destination's merged sources in ascending i."""
    what = "tome_select"
    if not torch.is_tensor(node_max) or node_max.dim() != 2:
        raise VdxError(f"{what}: node_max must be [n_img][n_src]")
    n_img = node_max.shape[0]
    a = _tome_args(what, node_max, src_idx, dst_idx, n_img, S, r, 0)
    if node_max.shape[1] != a.n_src or not torch.is_tensor(node_idx) or tuple(node_idx.shape) != tuple(node_max.shape):
        raise VdxError(f"{what}: node_max / node_idx must both be [{n_img}][{a.n_src}]")
    if _lib.load().vdx_tome_select_lds(a.n_src, a.n_dst) > 160 * 1024 - 256:
        raise VdxError(f"{what}: {a.n_src} sources and {a.n_dst} destinations do not fit the select kernel's LDS")
    a.node_max = _tome_buf(node_max, n_img * a.n_src, torch.float32, what, "node_max", node_max.device)
    a.node_idx = _tome_buf(node_idx, n_img * a.n_src, torch.int32, what, "node_idx", node_max.device)
    slot = torch.zeros((n_img, S), dtype=torch.int32, device=node_max.device)
    off = torch.empty((n_img, a.n_dst + 1), dtype=torch.int32, device=node_max.device)
    items = torch.empty((n_img, r), dtype=torch.int32, device=node_max.device)
    a.slot, a.off, a.items = slot.data_ptr(), off.data_ptr(), items.data_ptr()
    with torch.cuda.device(node_max.device):
        _launch("vdx_tome_select", C.byref(a))
    return slot, off, items


def tome_merge(y, src_idx, dst_idx, slot, off, items, *, n_img, S, r, out=None):
    """y fp16 rows [n_img * S][C] -> the merged rows [n_img * (S - r)][C]: unmerged sources copied in ascending token index,
    then the destinations, each the fp32 mean of itself and its merged sources in ascending i."""
    what = "tome_merge"
    Cc = y.shape[1] if y.dim() == 2 else 0
    if Cc < 8 or Cc % 8:
        raise VdxError(f"{what}: C={Cc} (a multiple of 8)")
    a = _tome_args(what, y, src_idx, dst_idx, n_img, S, r, Cc)
    py, ldy = _tome_rows(y, n_img * S, Cc, what, "y")
    a.slot = _tome_buf(slot, n_img * S, torch.int32, what, "slot", y.device)
    a.off = _tome_buf(off, n_img * (a.n_dst + 1), torch.int32, what, "off", y.device)
    a.items = _tome_buf(items, n_img * r, torch.int32, what, "items", y.device)
    if out is None:
        out = torch.empty((n_img * (S - r), Cc), dtype=torch.float16, device=y.device)
    po, ldo = _tome_rows(out, n_img * (S - r), Cc, what, "out")
    _tome_disjoint(y, out, what, "y and out")
    with torch.cuda.device(y.device):
        _launch("vdx_tome_merge_f16", C.byref(a), py, ldy, po, ldo)
    return out


def tome_unmerge_add(x, slot, t, src_idx, dst_idx, *, n_img, S, r, out=None):
    """x fp16 merged rows [n_img * (S - r)][C], t fp16 rows [n_img * S][C] -> fp16(fp32(x[slot[p]]) + fp32(t[p])) for every token;
    `out=t` adds in place."""
    what = "tome_unmerge_add"
    Cc = t.shape[1] if t.dim() == 2 else 0
    if Cc < 8 or Cc % 8:
        raise VdxError(f"{what}: C={Cc} (a multiple of 8)")
    a = _tome_args(what, t, src_idx, dst_idx, n_img, S, r, Cc)
    px, ldx = _tome_rows(x, n_img * (S - r), Cc, what, "x")
    pt, ldt = _tome_rows(t, n_img * S, Cc, what, "t")
    a.slot = _tome_buf(slot, n_img * S, torch.int32, what, "slot", t.device)
    if out is None:
        out = torch.empty((n_img * S, Cc), dtype=torch.float16, device=t.device)
    po, ldo = _tome_rows(out, n_img * S, Cc, what, "out")
    _tome_disjoint(x, out, what, "x and out")
    if out.data_ptr() != t.data_ptr() or ldo != ldt:
        _tome_disjoint(t, out, what, "t and out (unless out is t)")
    with torch.cuda.device(t.device):
        _launch("vdx_tome_unmerge_add_f16", C.byref(a), px, ldx, pt, ldt, po, ldo)
    return out


# --------------------------------------------------------------------------------------------
# Prompt travel: per-frame text (vdx/travel.py, csrc/travel.hip; no reference counterpart)
def text_travel(keys, uncond, lo, hi, w, s: int, L: int, d: int = 1, ring: bool = False, out=None):
    """One window's UNet text in one launch (include/vdx.h `vdx_text_travel_f16`) -> fp16 (2, L, N, D): item 0 is `uncond` on every
    frame; item 1, frame f, is the plan's blend for the clip frame `s + f * d` (`ring`: mod T) of `keys` fp16 (n_keys, N, D).
    `uncond`: fp16 (N, D) or (1, N, D); `lo`, `hi`: int32 (T,), `w`: fp32 (T,) on the device (`travel.TravelPlan.to`).  `lo` and
    `hi` are checked against n_keys here (one host sync: the call is made once per window, before the loop) and clamped on the
    device; the library checks `s`, `L` and `d` against T."""
    if keys.dim() != 3 or not keys.is_contiguous():
        raise VdxError(f"text_travel: keys must be contiguous (n_keys, N, D), got {tuple(keys.shape)}")
    n_keys, N, D = keys.shape
    if uncond.dim() == 3 and uncond.shape[0] == 1:
        uncond = uncond[0]
    if tuple(uncond.shape) != (N, D) or not uncond.is_contiguous():
        raise VdxError(f"text_travel: uncond must be contiguous ({N}, {D}) or (1, {N}, {D}), got {tuple(uncond.shape)}")
    T = lo.numel()
    for t, name, dt in ((lo, "lo", torch.int32), (hi, "hi", torch.int32), (w, "w", torch.float32)):
        if t.dim() != 1 or t.numel() != T or T < 1 or not t.is_contiguous() or t.dtype != dt or t.device != keys.device:
            raise VdxError(f"text_travel: {name} must be a contiguous {dt} ({T},) on the keys' device")
    lo_min, lo_max, hi_min, hi_max = (int(v) for v in torch.stack([lo.min(), lo.max(), hi.min(), hi.max()]).tolist())
    if min(lo_min, hi_min) < 0 or max(lo_max, hi_max) >= n_keys:
        raise VdxError(f"text_travel: lo / hi name keys outside [0, {n_keys})")
    s, L, d = int(s), int(L), int(d)
    if L < 1:
        raise VdxError(f"text_travel: bad window start {s}, length {L}, stride {d} of {T} frames")
    shape = (2, L, N, D)
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=keys.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise VdxError("text_travel: out must be contiguous (2, L, N, D)")
    if D % 8:       # the scalar path reads where the tensors lie; `_p` asks for the vector path's alignment
        for t, name in ((keys, "keys"), (uncond, "uncond"), (out, "out")):
            if not t.is_cuda or t.dtype != torch.float16:
                raise VdxError(f"text_travel: {name} must be an fp16 GPU tensor")
        ptrs = (keys.data_ptr(), uncond.data_ptr(), out.data_ptr())
    else:
        ptrs = (_p(keys, "keys"), _p(uncond, "uncond"), _p(out, "out"))
    _launch("vdx_text_travel_f16", ptrs[0], n_keys, ptrs[1], _p(lo, "lo", torch.int32), _p(hi, "hi", torch.int32), _p(w, "w", torch.float32),
            T, s, L, d, int(bool(ring)), N, D, ptrs[2])
    return out


def cross_attn_block_pack_kv(k_rows, vt, n_items: int, text_pad: int, out=None):
    """`packing.pack_k5_kv` as one launch (include/vdx.h `vdx_cross_attn_block_pack_kv_f16`): k_rows [n_items*text_pad][inner], vt
    [inner][n_items*text_pad] -> K5's key / value blobs [n_items][heads][3 * 4096] fp16, bit for bit what the torch chain builds."""
    kr, inner, ldk = _rows(k_rows, "k_rows")
    vr, vc, ldvt = _rows(vt, "vt")
    if not cross_attn_block_supported(inner, 1):
        raise VdxError(f"cross_attn_block_pack_kv: inner={inner} not supported by the fused kernel")
    if n_items < 1 or kr < n_items * text_pad or vr < inner or vc < n_items * text_pad:
        raise VdxError(f"cross_attn_block_pack_kv: k_rows {tuple(k_rows.shape)} / vt {tuple(vt.shape)} do not cover {n_items} items of {text_pad} keys")
    shape = (n_items, inner // 64, _lib.load().vdx_cross_attn_block_kv_bytes(inner) // (2 * (inner // 64)))
    if out is None:
        out = torch.empty(shape, dtype=torch.float16, device=k_rows.device)
    elif tuple(out.shape) != shape or not out.is_contiguous():
        raise VdxError(f"cross_attn_block_pack_kv: out must be contiguous {shape}")
    _launch("vdx_cross_attn_block_pack_kv_f16", _p(k_rows, "k_rows"), ldk, _p(vt, "vt"), ldvt, int(n_items), int(text_pad), inner, _p(out, "out"))
    return out


# --------------------------------------------------------------------------------------------
# Regional prompts: the per-pixel blend of the cross-attention sub-block's per-text results (vdx/region.py, csrc/region.hip; no
# reference counterpart)
def region_blend(inputs, table, s: int, L: int, d: int = 1, ring: bool = False, out=None):
    """One window's blend in one launch (include/vdx.h `vdx_region_blend_f16`).  `inputs`: a sequence of 1 to 8 entries, entry j
    the sub-block's rows for text j, fp16 contiguous [L * S][C], or None for a text that was not launched (no weight on any cell
    of the window: it is skipped whatever the table holds); `table`: fp32 contiguous (T, S, len(inputs)) on the device, the
    level's weights (`region.RegionPlan.to`).  Row (f, p) takes the weights of the clip frame `s + f * d` (`ring`: mod T).
    `out`: fp16 [L * S][C], which may be `inputs[0]` (or any one input); by default a new tensor."""
    n_in = len(inputs)
    if not 1 <= n_in <= 8:
        raise VdxError(f"region_blend: {n_in} inputs, 1 to 8 are taken (the base text and at most 7 regions)")
    given = [t for t in inputs if t is not None]
    if not given:
        raise VdxError("region_blend: every input is None")
    if table.dim() != 3 or table.shape[2] != n_in or table.dtype != torch.float32 or not table.is_contiguous() or not table.is_cuda:
        raise VdxError(f"region_blend: the table must be a contiguous fp32 GPU tensor (T, S, {n_in}), got {tuple(table.shape)} {table.dtype}")
    T, S = int(table.shape[0]), int(table.shape[1])
    s, L, d = int(s), int(L), int(d)
    if L < 1 or d < 1 or not 0 <= s < T or s + (L - 1) * d >= (2 * T if ring else T):
        raise VdxError(f"region_blend: bad window start {s}, length {L}, stride {d}{' on the ring' if ring else ''} of {T} frames")
    M, Cc = L * S, int(given[0].shape[-1])
    if out is None:
        out = torch.empty((M, Cc), dtype=torch.float16, device=table.device)
    align = 16 if Cc % 8 == 0 else (8 if Cc % 4 == 0 else 2)
    for t, name in [(t, f"input {j}") for j, t in enumerate(inputs) if t is not None] + [(out, "out")]:
        if not t.is_cuda or t.dtype != torch.float16 or t.device != table.device:
            raise VdxError(f"region_blend: {name} must be an fp16 tensor on the table's device")
        if tuple(t.shape) != (M, Cc) or not t.is_contiguous():
            raise VdxError(f"region_blend: {name} must be contiguous ({M}, {Cc}), got {tuple(t.shape)}")
        if t.data_ptr() % align:
            raise VdxError(f"region_blend: {name} must be {align}-byte aligned at C = {Cc}")
    ptrs = (C.c_void_p * n_in)(*[None if t is None else t.data_ptr() for t in inputs])
    with torch.cuda.device(table.device):
        _launch("vdx_region_blend_f16", ptrs, n_in, _p(table, "table", torch.float32), T, s, L, d, int(bool(ring)), S, Cc, out.data_ptr())
    return out


# --------------------------------------------------------------------------------------------
# LoRA adapters: one weight of the diffusers layout with its adapters merged in (vdx/lora.py, csrc/lora.hip; no reference counterpart)
LORA_MAX_ADAPTERS, LORA_MAX_RANK = 8, 512


def lora_merge(W, adapters, out=None):
    """`W + sum_a s_a up_a @ down_a` in one launch (include/vdx.h `vdx_lora_merge_f16`: fp32 products and sums in a stated order, the
    result rounded to fp16 once).  `W`: fp16 contiguous (n_out, n_in) on the GPU; `adapters`: 1 to 8 entries (up, down, s), `up`
    fp32 contiguous (n_out, R) and `down` fp32 contiguous (R, n_in) on W's device, 1 <= R <= 512, `s` a finite number (rounded to
    fp32 here).  `out`: fp16 contiguous (n_out, n_in), which may be `W`; by default a new tensor."""
    import math
    if not isinstance(W, torch.Tensor) or not W.is_cuda:
        raise VdxError("lora_merge: W must be a GPU tensor (the merge has no CPU fallback)")
    if W.dtype != torch.float16:
        raise VdxError(f"lora_merge: W must be fp16, got {W.dtype}")
    if W.dim() != 2 or not W.is_contiguous() or W.shape[0] < 1 or W.shape[1] < 1:
        raise VdxError(f"lora_merge: W must be contiguous (n_out, n_in), got {tuple(W.shape)}")
    n_out, n_in = int(W.shape[0]), int(W.shape[1])
    adapters = list(adapters)
    A = len(adapters)
    if not 1 <= A <= LORA_MAX_ADAPTERS:
        raise VdxError(f"lora_merge: {A} adapters, 1 to {LORA_MAX_ADAPTERS} are taken")
    if out is None:
        out = torch.empty_like(W)
    elif not isinstance(out, torch.Tensor) or out.device != W.device or out.dtype != torch.float16 or tuple(out.shape) != (n_out, n_in) \
            or not out.is_contiguous():
        raise VdxError(f"lora_merge: out must be a contiguous fp16 ({n_out}, {n_in}) tensor on W's device")
    ranks, scales = [], []
    for a, entry in enumerate(adapters):
        if not isinstance(entry, (tuple, list)) or len(entry) != 3:
            raise VdxError(f"lora_merge: adapter {a} must be (up, down, s)")
        up, down, s = entry
        for t, name in ((up, "up"), (down, "down")):
            if not isinstance(t, torch.Tensor) or t.device != W.device:
                raise VdxError(f"lora_merge: adapter {a}: {name} must be a tensor on W's device")
            if t.dtype != torch.float32:
                raise VdxError(f"lora_merge: adapter {a}: {name} must be fp32, got {t.dtype}")
            if t.dim() != 2 or not t.is_contiguous():
                raise VdxError(f"lora_merge: adapter {a}: {name} must be a contiguous matrix, got {tuple(t.shape)}")
            if t.data_ptr() % 4:
                raise VdxError(f"lora_merge: adapter {a}: {name} must be 4-byte aligned")
        R = int(up.shape[1])
        if not 1 <= R <= LORA_MAX_RANK:
            raise VdxError(f"lora_merge: adapter {a}: rank {R}, 1 to {LORA_MAX_RANK} are taken")
        if tuple(up.shape) != (n_out, R) or tuple(down.shape) != (R, n_in):
            raise VdxError(f"lora_merge: adapter {a}: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit W ({n_out}, {n_in}) at rank {R}")
        s = float(s)
        if not math.isfinite(s) or not math.isfinite(C.c_float(s).value):
            raise VdxError(f"lora_merge: adapter {a}: the scale {s!r} is not a finite fp32 number")
        ranks.append(R)
        scales.append(s)
    if W.data_ptr() % 2 or out.data_ptr() % 2:
        raise VdxError("lora_merge: W and out must be 2-byte aligned")
    ups = (C.c_void_p * A)(*[e[0].data_ptr() for e in adapters])
    downs = (C.c_void_p * A)(*[e[1].data_ptr() for e in adapters])
    with torch.cuda.device(W.device):
        _launch("vdx_lora_merge_f16", W.data_ptr(), n_out, n_in, A, ups, downs, (C.c_int32 * A)(*ranks), (C.c_float * A)(*scales), out.data_ptr())
    return out


# --------------------------------------------------------------------------------------------
# Prompt emphasis: per-token weights on the text encoder's output, mean restored (vdx/prompt.py, csrc/prompt.hip; no reference counterpart)
PROMPT_MAX_TOK = 77


def prompt_weight(z, w, out=None):
    """A1111's emphasis with mean restoration in one launch (include/vdx.h `vdx_prompt_weight_f16`): per sequence
    `y = fp16(fp32(z) w[tok])`, `r = fp32(sum z / sum y)` (fp64 sums and quotient), `out = fp16(fp32(y) r)`.  `z`: fp16 contiguous
    (n_seq, n_tok, D) on the GPU, the CLIP last hidden state, 1 <= n_tok <= 77; `w`: fp32 (n_seq, n_tok), on the host or the device,
    finite (checked here: one copy to the host where it is on the device).  `out`: fp16 contiguous like z, which may be z; by default
    a new tensor.  A sequence whose weights are all exactly 1.0 is not passed to the kernel: its bits are z's, and where that is
    every sequence nothing is launched and, without `out`, z itself is returned."""
    if not isinstance(z, torch.Tensor) or not z.is_cuda:
        raise VdxError("prompt_weight: z must be a GPU tensor (the weighting has no CPU fallback)")
    if z.dtype != torch.float16 or z.dim() != 3 or not z.is_contiguous():
        raise VdxError(f"prompt_weight: z must be contiguous fp16 (n_seq, n_tok, D), got {z.dtype} {tuple(z.shape)}")
    n_seq, n_tok, D = (int(v) for v in z.shape)
    if n_seq < 1 or not 1 <= n_tok <= PROMPT_MAX_TOK or D < 1:
        raise VdxError(f"prompt_weight: z {tuple(z.shape)}: n_seq >= 1, n_tok in 1..{PROMPT_MAX_TOK} and D >= 1 are taken")
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != (n_seq, n_tok):
        raise VdxError(f"prompt_weight: w must be fp32 ({n_seq}, {n_tok}), got {getattr(w, 'dtype', type(w))} {tuple(getattr(w, 'shape', ()))}")
    wh = w.detach().cpu().contiguous()
    if not bool(torch.isfinite(wh).all()):
        raise VdxError("prompt_weight: w holds a weight that is not finite")
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != z.device or out.dtype != torch.float16
                            or tuple(out.shape) != (n_seq, n_tok, D) or not out.is_contiguous()):
        raise VdxError(f"prompt_weight: out must be a contiguous fp16 ({n_seq}, {n_tok}, {D}) tensor on z's device")
    weighted = [i for i in range(n_seq) if bool((wh[i] != 1.0).any())]
    if not weighted:
        if out is None or out.data_ptr() == z.data_ptr():
            return z
        return out.copy_(z)
    with torch.cuda.device(z.device):
        if len(weighted) == n_seq:
            out = torch.empty_like(z) if out is None else out
            _launch("vdx_prompt_weight_f16", z.data_ptr(), _p(wh.to(z.device), "w", torch.float32), out.data_ptr(), n_seq, n_tok, D)
            return out
        # some sequences keep the encoder's bits: the weighted ones are gathered, weighted in place in one launch, and put back
        idx = torch.tensor(weighted, dtype=torch.int64, device=z.device)
        sel = z.index_select(0, idx)
        _launch("vdx_prompt_weight_f16", sel.data_ptr(), _p(wh[weighted].contiguous().to(z.device), "w", torch.float32), sel.data_ptr(),
                len(weighted), n_tok, D)
        if out is None:
            out = z.clone()
        elif out.data_ptr() != z.data_ptr():
            out.copy_(z)
        out.index_copy_(0, idx, sel)
    return out


# --------------------------------------------------------------------------------------------
# Animated GIF of a whole clip: histogram, LUT, index map, strip LZW, sub-blocks (vdx/gif.py, csrc/gif.hip; no reference counterpart)
GIF_BINS = 32768
GIF_DITHERS = {"none": 0, "bayer": 1}
GIF_LZW_STAGES = ("sbits", "soff", "fbits", "slots", "stream", "foff")         # vdx_gif_lzw_offsets


def _gif_u8(t, n: int, what: str, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < n:
        raise VdxError(f"{what}: {name} must be a contiguous uint8 GPU tensor of at least {n} bytes")
    return t.data_ptr()


def gif_hist(frames) -> torch.Tensor:
    """Pixels of the whole clip per 5-5-5 bin -> int32 [32768] on the clip's device holding the uint32 counts (include/vdx.h
    `vdx_gif_hist_u8`); a clip of 2^32 pixels or more is refused."""
    T, H, W = check_u8_frames(frames, "gif_hist")
    if T * H * W >= 1 << 32:
        raise VdxError(f"gif_hist: {T * H * W} pixels do not fit the uint32 counts (2^32 or more)")
    with torch.cuda.device(frames.device):
        hist = torch.empty(GIF_BINS, dtype=torch.int32, device=frames.device)
        _launch("vdx_gif_hist_u8", *_u8_args(frames), T, H, W, hist.data_ptr())
    return hist


def gif_lut(palette) -> torch.Tensor:
    """uint8 [32768]: for every 5-5-5 bin the entry of `palette` (uint8 (n, 3) on the GPU, n in 1..256) nearest to the bin's
    centre, a tie to the lowest index (`vdx_gif_lut`)."""
    if (not isinstance(palette, torch.Tensor) or not palette.is_cuda or palette.dtype != torch.uint8 or palette.dim() != 2
            or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256 or not palette.is_contiguous()):
        raise VdxError(f"gif_lut: palette must be a contiguous uint8 (n, 3) GPU tensor with n in 1..256, got "
                       f"{getattr(palette, 'dtype', type(palette))} {tuple(getattr(palette, 'shape', ()))}")
    with torch.cuda.device(palette.device):
        lut = torch.empty(GIF_BINS, dtype=torch.uint8, device=palette.device)
        _launch("vdx_gif_lut", palette.data_ptr(), int(palette.shape[0]), lut.data_ptr())
    return lut


def gif_index(frames, lut, dither: str = "bayer") -> torch.Tensor:
    """One palette index per pixel -> uint8 (T, H, W): the ordered dither ("bayer") or none, the bin, `lut` (`vdx_gif_index_u8`)."""
    T, H, W = check_u8_frames(frames, "gif_index")
    if dither not in GIF_DITHERS:
        raise VdxError(f"gif_index: dither {dither!r} is not one of {sorted(GIF_DITHERS)}")
    if T * H * W >= 1 << 32:
        raise VdxError(f"gif_index: {T * H * W} pixels (2^32 or more)")
    with torch.cuda.device(frames.device):
        out = torch.empty((T, H, W), dtype=torch.uint8, device=frames.device)
        _launch("vdx_gif_index_u8", *_u8_args(frames), T, H, W, _gif_u8(lut, GIF_BINS, "gif_index", "lut"), GIF_DITHERS[dither],
                out.data_ptr())
    return out


def gif_lzw_workspace(T: int, H: int, W: int, strip_rows: int) -> int:
    """Bytes of workspace `gif_lzw` / `gif_pack` need; `VdxError` for a geometry the encoder does not take."""
    n = _lib.load().vdx_gif_lzw_workspace(T, H, W, strip_rows)
    if n == 0:
        raise VdxError(f"gif_lzw: {T} frames of {W}x{H} in strips of {strip_rows} rows are outside what the encoder takes")
    return n


def gif_lzw_offsets(T: int, H: int, W: int, strip_rows: int) -> dict:
    """The workspace's layout: byte offsets of `GIF_LZW_STAGES`, then "nstrips" and "slot_words" (`vdx_gif_lzw_offsets`)."""
    offs = (C.c_size_t * 8)()
    _lib.check(_lib.load().vdx_gif_lzw_offsets(T, H, W, strip_rows, offs), "vdx_gif_lzw_offsets")
    return dict(zip(GIF_LZW_STAGES + ("nstrips", "slot_words"), (int(v) for v in offs)))


def gif_lzw(idx, strip_rows: int, workspace, lengths=None) -> torch.Tensor:
    """LZW of every strip of `strip_rows` rows of uint8 (T, H, W) indices into `workspace` (`gif_lzw_workspace` bytes, uint8,
    16-byte aligned) -> int32 [T]: the bytes of every frame's data sub-blocks (`vdx_gif_lzw`)."""
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype != torch.uint8 or idx.dim() != 3 or not idx.is_contiguous():
        raise VdxError(f"gif_lzw: idx must be a contiguous uint8 (T, H, W) GPU tensor, got {getattr(idx, 'dtype', type(idx))} "
                       f"{tuple(getattr(idx, 'shape', ()))}")
    T, H, W = (int(v) for v in idx.shape)
    if T < 1 or H < 1 or W < 1:
        raise VdxError(f"gif_lzw: empty indices {tuple(idx.shape)}")
    need = gif_lzw_workspace(T, H, W, strip_rows)
    with torch.cuda.device(idx.device):
        if lengths is None:
            lengths = torch.empty(T, dtype=torch.int32, device=idx.device)
        elif lengths.dtype != torch.int32 or lengths.numel() < T or not lengths.is_cuda or not lengths.is_contiguous():
            raise VdxError(f"gif_lzw: lengths must be a contiguous int32 GPU tensor of at least {T} elements")
        ws = _gif_u8(workspace, need, "gif_lzw", "workspace")
        if ws % 16:
            raise VdxError("gif_lzw: workspace not 16-byte aligned")
        _launch("vdx_gif_lzw", idx.data_ptr(), T, H, W, strip_rows, ws, lengths.data_ptr())
    return lengths


def gif_pack(workspace, T: int, H: int, W: int, strip_rows: int, out) -> torch.Tensor:
    """Every frame's data sub-blocks back to back into `out` (uint8, the sum of `gif_lzw`'s lengths in bytes), from the workspace
    `gif_lzw` left (`vdx_gif_pack`)."""
    need = gif_lzw_workspace(T, H, W, strip_rows)
    with torch.cuda.device(out.device):
        _launch("vdx_gif_pack", _gif_u8(workspace, need, "gif_pack", "workspace"), T, H, W, strip_rows, _gif_u8(out, 1, "gif_pack", "out"),
                out.numel())
    return out


# --------------------------------------------------------------------------------------------
# the portable seeded noise generator "philox4x32-10/v1" (no reference counterpart; include/vdx.h "Portable seeded noise";
# csrc/noise.hip; vdx/noise.py holds the streams' names and the job's `normal`; tests/noise_ref.py is the definition)
NOISE_MAX_DIMS = 5


def _noise_int(what: str, v, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v < hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}), got {v!r}")
    return v


def philox_box(shape, box=None):
    """(shape, start, extent) as tuples of ints of one length, checked on the host: 1..5 axes of size >= 1, fewer than 2^63
    elements, `box` = (start, extent) within the shape with extents >= 1 (None: the whole tensor); `ValueError` otherwise."""
    shape = tuple(shape)
    if not 1 <= len(shape) <= NOISE_MAX_DIMS:
        raise ValueError(f"philox_normal: the logical shape has 1 to {NOISE_MAX_DIMS} axes, got {shape!r}")
    total = 1
    for d, n in enumerate(shape):
        total *= _noise_int(f"philox_normal: shape[{d}]", n, 1, 2 ** 63)
    if total >= 2 ** 63:
        raise ValueError(f"philox_normal: the logical tensor {shape} must have fewer than 2^63 elements")
    if box is None:
        return shape, (0,) * len(shape), shape
    if not isinstance(box, (tuple, list)) or len(box) != 2 or any(not isinstance(v, (tuple, list)) or len(v) != len(shape) for v in box):
        raise ValueError(f"philox_normal: box must be (start, extent), each of {len(shape)} integers, got {box!r}")
    start, extent = tuple(box[0]), tuple(box[1])
    for d, n in enumerate(shape):
        _noise_int(f"philox_normal: extent[{d}]", extent[d], 1, n + 1)
        _noise_int(f"philox_normal: start[{d}] (extent {extent[d]} of {n})", start[d], 0, n - extent[d] + 1)
    return shape, start, extent


def _noise_arrays(shape, start, extent):
    arr = C.c_size_t * len(shape)
    return len(shape), arr(*shape), arr(*start), arr(*extent)


def philox_form(shape, box=None) -> bool:
    """True when that box takes the kernel's fast form (a lane per Philox block), False for the general one (`vdx_noise_form`)."""
    rc = _lib.load().vdx_noise_form(*_noise_arrays(*philox_box(shape, box)))
    if rc < 0:
        _lib.check(rc, "vdx_noise_form")
    return bool(rc)


def philox_normal(shape, seed: int, stream: int = 0, *, box=None, sigma: float = 1.0, dtype=torch.float16, device, out=None):
    """N(0, 1) of the generator "philox4x32-10/v1" (csrc/noise.hip): element i of stream `stream` under `seed`, both in [0, 2^64),
    is a pure function of (seed, stream, i), i the C-order index in the LOGICAL tensor `shape`.  `box` = (start, extent): only that
    box of it, with the bits the whole tensor has there.  -> a new contiguous tensor of the box's shape on `device` (or `out`, of
    that shape and dtype): fp32(n) for `dtype` float32, fp16(fp32(fp16(n)) * fp32(sigma)) for float16 (`sigma` goes with float16
    only).  `ValueError` / `VdxError` before any launch for arguments outside these."""
    import math
    shape, start, extent = philox_box(shape, box)
    seed, stream = _noise_int("philox_normal: seed", seed, 0, 2 ** 64), _noise_int("philox_normal: stream", stream, 0, 2 ** 64)
    if dtype not in (torch.float16, torch.float32):
        raise ValueError(f"philox_normal: dtype must be torch.float16 or torch.float32, got {dtype}")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not math.isfinite(sigma) or abs(sigma) > 3.4028234663852886e38:
        raise ValueError(f"philox_normal: sigma must be a finite number (fp32), got {sigma!r}")
    if dtype == torch.float32 and sigma != 1.0:
        raise ValueError("philox_normal: sigma goes with float16 (the start latent's scale); float32 output is N(0, 1) itself")
    device = torch.device(device)
    if device.type != "cuda":
        raise VdxError(f"philox_normal: expected a GPU device (the generator has no host form in the package), got {device}")
    if out is None:
        out = torch.empty(extent, dtype=dtype, device=device)
    elif not out.is_cuda or tuple(out.shape) != extent or out.dtype != dtype or not out.is_contiguous():
        raise VdxError(f"philox_normal: out must be a contiguous {dtype} GPU tensor of shape {extent}")
    nd, sh, st, ex = _noise_arrays(shape, start, extent)
    with torch.cuda.device(out.device):
        if dtype == torch.float16:
            _launch("vdx_noise_f16", seed, stream, nd, sh, st, ex, float(sigma), _p(out, "out"))
        else:
            _launch("vdx_noise_f32", seed, stream, nd, sh, st, ex, _p(out, "out", torch.float32))
    return out
