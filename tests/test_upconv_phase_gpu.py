"""-m gpu: the upsampler convolution in PHASE form (vdx_gemm_args.upsample = 3): conv3x3 over a nearest-x2 image computed as
four 2x2 convolutions on the source image, one per output parity, with packing.pack_upconv_phase's table (K = 4C).

Shapes are the smallest at which the gather can go wrong: a row tail in every phase, an N tail and borders on every side
(M_src = 105), exactly one 256-row tile per phase (M_src = 256), and M_src = 144 with three 64-channel slices.  Per shape:
  1 exact structure   integer inputs, weights k/8: every sum is exact, so the phase form has the nine-tap gather's bits
  2 phase reference   fp32 convolution with the phase table itself, the tolerance tests/test_ops_gpu.py uses for the x2 gather
  3 nine-tap reference  rel-L2 against the true convolution <= 1.25 x the rel-L2 of a CPU emulation of the phase form
                        (fp16 table, fp32 accumulation, fp16 output) computed here: the emulation is the yardstick
  4 tile family       the pinned 128x128 variant has the planned call's bits
and the forward reaches upsample = 3 with divisible latents, 2 otherwise."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from upconv_phase_ref import phase_reference

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 64, 72), (2, 8, 16, 128, 320), (1, 9, 16, 192, 640)]       # n_img, h, w, C, N


def _ops():
    import vdx  # noqa: F401
    from vdx import ops, packing
    return ops, packing


def h16(x):
    return x.half().float()


def close(out, ref, tol=3e-3):                 # tests/test_ops_gpu.py's bound for fp16-output contractions
    out = out.float().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs()
    bad = err > tol * scale + tol * ref.abs()
    assert not bad.any(), f"max err {err.max().item():.4g} (scale {scale:.4g}), {int(bad.sum())} / {bad.numel()} bad"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run(gpu, x, w, b, form, variant=0):
    """x [n][C][h][w], w [N][C][3][3], b [N] (CPU, fp16-exact) -> rows [n*2h*2w][N] of the kernel in `form` (1 | 3).
    The nine-tap gather takes N in multiples of 64 only: it is given zero filters up to the next one and their columns
    are dropped — a column's sum does not depend on its neighbours, so columns 0..N-1 are the nine-tap gather's own."""
    ops, packing = _ops()
    n, _, hh, ww = x.shape
    N = w.shape[0]
    if form == 1 and N % 64:
        fill = 64 - N % 64
        w, b = F.pad(w, (0, 0, 0, 0, 0, 0, 0, fill)), F.pad(b, (0, fill))
    table = packing.pack_upconv_phase(w) if form == 3 else packing.pack_conv3x3(w).half()
    out = ops.gemm(packing.nchw_to_rows(x).half().to(gpu), table.to(gpu), M=n * 4 * hh * ww, mode=ops.CONV3X3,
                   bias=b.half().to(gpu), conv=(n, hh, ww, 2 * hh, 2 * ww, 1, form), variant=variant)
    return out[:, :N].contiguous()


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """Inputs, the true nine-tap convolution (fp64) and the phase table's own convolution (fp32) of one shape: computed once."""
    _, packing = _ops()
    n, hh, ww, C, N = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = h16(torch.randn(n, C, hh, ww, generator=g))
    w = h16(torch.randn(N, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b = h16(torch.randn(N, generator=g) * 0.1)
    ref9 = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1)
    refp = phase_reference(x, packing.pack_upconv_phase(w).float(), N) + b[None, :, None, None]
    return x, w, b, packing.nchw_to_rows(ref9), packing.nchw_to_rows(refp)


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_has_the_nine_tap_bits_on_exact_sums(gpu, shape):
    n, hh, ww, C, N = shape
    g = torch.Generator().manual_seed(7 + sum(shape))
    x = torch.randint(-4, 5, (n, C, hh, ww), generator=g).float()
    w = torch.randint(-8, 9, (N, C, 3, 3), generator=g).float() / 8
    b = torch.randint(-8, 9, (N,), generator=g).float() / 8
    nine, phase = run(gpu, x, w, b, 1), run(gpu, x, w, b, 3)
    assert torch.isfinite(nine.float()).all() and nine.float().abs().max() > 8
    assert torch.equal(phase, nine), f"{int((phase != nine).sum())} / {nine.numel()} elements differ"


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_against_its_own_table(gpu, shape):
    x, w, b, _, refp = random_case(shape)
    close(run(gpu, x, w, b, 3), refp)


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_against_the_nine_tap_convolution(gpu, shape):
    x, w, b, ref9, refp = random_case(shape)
    emu = rel_l2(refp.half().float(), ref9)                 # fp16 table, fp32 sums, fp16 output
    got = rel_l2(run(gpu, x, w, b, 3).float().cpu(), ref9)
    print(f"{shape}: rel-L2 kernel {got:.3e}, emulation {emu:.3e}")
    assert got <= 1.25 * emu


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_bits_do_not_depend_on_the_tile_family(gpu, shape):
    x, w, b, _, _ = random_case(shape)
    planned = run(gpu, x, w, b, 3)
    assert torch.equal(run(gpu, x, w, b, 3, variant=1), planned)
    assert torch.equal(run(gpu, x, w, b, 3, variant=2), planned)


def test_forward_takes_the_phase_form_for_divisible_latents_only(gpu, monkeypatch):
    ops, _ = _ops()
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    tiny = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
    sd = synthetic_state_dict(RefCfg.tiny(**tiny), seed=1234)
    cfg = UNet3DConfig(block_out_channels=tiny["ch"], cross_attention_dim=tiny["cross"], transformer_in_heads=tiny["in_heads"])
    m = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    phase_tables = {id(m.W[k]) for k in m.W if k.endswith(".upsamplers.0.conv.weight")}
    nine_tap_tables = {id(m.W[k]) for k in m.W if k.endswith(".upsamplers.0.conv.weight_taps9")}
    assert len(phase_tables) == len(nine_tap_tables) == 3
    seen = []
    real = ops.gemm

    def spy(a, w, **kw):
        if kw.get("mode") == ops.CONV3X3 and kw["conv"][6]:
            seen.append((int(kw["conv"][6]), id(w)))
        return real(a, w, **kw)

    monkeypatch.setattr(ops, "gemm", spy)
    g = torch.Generator().manual_seed(3)
    ehs = torch.randn(1, 77, tiny["cross"], generator=g).half().to(gpu)
    for (H, W), form, tables in (((16, 16), 3, phase_tables), ((12, 9), 2, nine_tap_tables)):
        seen.clear()
        out = m(torch.randn(1, 4, 2, H, W, generator=g).half().to(gpu), 301, encoder_hidden_states=ehs).sample
        assert torch.isfinite(out.float()).all()
        assert [f for f, _ in seen] == [form] * 3 and {t for _, t in seen} == tables, (H, W, seen)
