"""Host checks of the upsampler convolution's phase form (vdx_gemm_args.upsample = 3): the table packing.pack_upconv_phase
builds, and what the library's host-only queries answer for such a call (no GPU needed)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from upconv_phase_ref import phase_reference

HEADLINE_TILE = "gemm_kernel<256, 320, 4, 2, 1, false, true, 0>"
# the three upsampler launches of the headline step (2 x 24 frames, 72 x 128 latents): n_img, h_in, w_in, C = N
XL_UPSAMPLERS = [(48, 36, 64, 640), (48, 18, 32, 1280), (48, 9, 16, 1280)]


def _lib():
    import vdx  # noqa: F401
    from vdx import _lib
    return _lib


def phase_args(n_img, h, w, cin, N, **over):
    lib = _lib()
    g = lib.GemmArgs()
    g.a = g.w = g.out = g.bias = 1 << 20            # never dereferenced on the host
    g.M, g.N, g.K, g.mode, g.c1 = n_img * 4 * h * w, N, 4 * cin, 1, cin
    g.lda, g.ldo = cin, N
    g.h_in, g.w_in, g.h_out, g.w_out, g.stride, g.upsample = h, w, 2 * h, 2 * w, 1, 3
    for k, v in over.items():
        setattr(g, k, v)
    return g


def kernel_name(g):
    lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.load().vdx_gemm_kernel_name(C.byref(g), buf, len(buf))
    if rc:
        raise lib.VdxError(lib.load().vdx_last_error().decode())
    return buf.value.decode()


def test_phase_table_reproduces_the_conv_on_the_upsampled_image():
    import vdx  # noqa: F401
    from vdx import packing
    g = torch.Generator().manual_seed(11)
    n, cin, hh, ww, N = 2, 3, 5, 7, 4
    x = torch.randn(n, cin, hh, ww, generator=g, dtype=torch.float64)
    w = torch.randn(N, cin, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, padding=1)
    # (the kernels' K order needs whole 64-channel slices: the three channels sit in one zero-padded slice)
    x64, w64 = x.new_zeros(n, 64, hh, ww), w.new_zeros(N, 64, 3, 3)
    x64[:, :cin], w64[:, :cin] = x, w
    table = packing.pack_upconv_phase(w64, dtype=torch.float64)
    assert table.shape == (4 * N, 4 * 64) and table.dtype == torch.float64
    got = phase_reference(x64, table, N)
    assert float((got - want).abs().max()) <= 1e-12


def test_phase_table_is_fp16_rounded_once_from_fp32_sums():
    import vdx  # noqa: F401
    from vdx import packing
    g = torch.Generator().manual_seed(12)
    w = torch.randn(8, 64, 3, 3, generator=g) * 0.05
    t16 = packing.pack_upconv_phase(w)
    assert t16.dtype == torch.float16 and t16.shape == (32, 256)
    assert torch.equal(t16, packing.pack_upconv_phase(w.half().float(), dtype=torch.float32).half())
    # phase 3 (a = b = 1), tap (1, 1) is the lone corner tap ky = kx = 2: no sum, the fp16 weight itself
    assert torch.equal(t16[24:32, 192:256], w[:, :, 2, 2].half())


@pytest.mark.parametrize("n_img,h,w,ch", XL_UPSAMPLERS)
def test_xl_phase_calls_run_the_headline_tile_unsplit(n_img, h, w, ch):
    lib = _lib()
    g = phase_args(n_img, h, w, ch, ch)
    assert kernel_name(g) == HEADLINE_TILE
    s_, k_, b_ = C.c_int32(-1), C.c_int32(-1), C.c_size_t(1)
    assert lib.load().vdx_gemm_plan_ksplit(C.byref(g), C.byref(s_), C.byref(k_), C.byref(b_)) == 0
    assert (s_.value, k_.value, b_.value) == (0, 0, 0)
    v_, sp_ = C.c_int32(-1), C.c_int32(-1)
    assert lib.load().vdx_gemm_plan(C.byref(g), C.byref(v_), C.byref(sp_)) == 0
    assert (v_.value, sp_.value) == (2, 0)


def test_phase_calls_never_plan_the_ring_kernels():
    """16-frame windows: 18 432 rows x 1280 splits into whole rounds of big tiles + a tail; the tail of 73 728 x 1280 would
    price the 128x320 ring best.  The phase form is carried by the tiled gemm_kernel families only."""
    lib = _lib()
    for n_img, h, w, ch in [(32, 36, 64, 640), (32, 18, 32, 1280), (32, 9, 16, 1280), (4, 32, 32, 640), (6, 16, 32, 1280)]:
        g = phase_args(n_img, h, w, ch, ch)
        v_, sp_ = C.c_int32(-1), C.c_int32(-1)
        assert lib.load().vdx_gemm_plan(C.byref(g), C.byref(v_), C.byref(sp_)) == 0
        spans = [(0, 0)] if sp_.value == 0 else [(0, sp_.value), (sp_.value, 0)]
        for rb, re_ in spans:
            g.row_begin, g.row_end = rb, re_
            assert kernel_name(g).startswith("gemm_kernel<"), (n_img, h, w, ch, rb, re_)


def test_virtual_rows_of_a_tail_shape():
    """M_src = 105 pads to 256: row ranges count 4 x 256 virtual rows, start at whole tiles and end within them."""
    lib = _lib()
    assert kernel_name(phase_args(3, 5, 7, 64, 72, row_begin=768, row_end=1024)).startswith("gemm_kernel<")
    with pytest.raises(lib.VdxError, match="rows"):
        kernel_name(phase_args(3, 5, 7, 64, 72, row_end=1025))
    with pytest.raises(lib.VdxError, match="256-row"):
        kernel_name(phase_args(3, 5, 7, 64, 72, row_begin=128))


@pytest.mark.parametrize("over,match", [
    (dict(bias2=1 << 20, rows_per_bias2=16), "bias2"),
    (dict(residual=1 << 20, ldr=64), "residual"),
    (dict(a2=1 << 20, c2=64, lda2=64, K=4 * 128), "second source|one source"),
    (dict(epilogue=1), "GEGLU"),
    (dict(pad_mode=1), "pad_mode"),
    (dict(stride=2), "stride"),
    (dict(ksplit=2, workspace=1 << 20, workspace_bytes=1 << 30), "split-K"),
    (dict(epilogue=8 << 8), "tiled kernels"),          # the ring kernels do not carry it
    (dict(h_out=32, w_out=16), "exact x2"),
])
def test_phase_form_refuses_what_it_cannot_carry(over, match):
    lib = _lib()
    assert kernel_name(phase_args(2, 8, 16, 64, 64)).startswith("gemm_kernel<")
    with pytest.raises(lib.VdxError, match=match):
        kernel_name(phase_args(2, 8, 16, 64, 64, **over))
