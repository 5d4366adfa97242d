"""-m gpu: FreeU's two kernels (csrc/freeu.hip) against the float64 restatement of tests/freeu_ref.py and their exact properties,
the UNet with `enable_freeu` against the fp32 oracle with FreeU restated in its up blocks, and every entry point that carries
the switch: sharded and shared-prefix forwards, the miner's loop, the job driver.

Measured on an MI355X (profiles/freeu_parity.txt): no element of any case below differs from the restatement's fp16 rounding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import freeu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
SETTING = dict(s1=0.9, s2=0.2, b1=1.2, b2=1.4)
CHANNELS = (1, 40, 64, 640, 1280)
SCALES = (0.9, 0.2, 0.0)


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_filter(gpu, planes, s, n_img=None, **kw):
    """planes fp16 (n, C, H, W) on the host -> the kernel's planes, on the host."""
    from vdx import ops
    n, C, H, W = planes.shape
    n_img = n_img or n
    rows = R.planes_to_rows(planes[:n_img]).contiguous().to(gpu)
    got = ops.freeu_filter(rows, n_img=n_img, h=H, w=W, s=s, **kw)
    return R.rows_to_planes(got.cpu(), n_img, H, W)


# ---- the skip filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.PLANES, ids=lambda v: str(v))
def test_filter_matches_the_restatement(gpu, H, W):
    """Every fp16 value equal, for every channel count, image count and scale.  One restatement per (C, s), at three images; the
    runs on one and two images are held to its first planes."""
    import vdx  # noqa: F401
    worst = 0
    for C in CHANNELS:
        for s in SCALES:
            x, want16, _ = R.make_case(H, W, C, 3, s)
            for n_img in (1, 2, 3):
                got = run_filter(gpu, x, s, n_img)
                bad = R.differing(got, want16[:n_img])
                worst = max(worst, bad)
                if bad:
                    print(f"{H}x{W} C={C} n_img={n_img} s={s}: {bad} of {got.numel()} elements differ")
    print(f"{H}x{W}: most differing elements in a case: {worst}")
    assert worst == 0


def test_filter_identity_batches_runs_and_in_place(gpu):
    import vdx  # noqa: F401
    from vdx import ops
    for (H, W), C in (((5, 9), 40), ((9, 16), 70), ((2, 2), 1), ((1, 1), 64)):
        x, _, _ = R.make_case(H, W, C, 3, 0.9, seed=1)
        x = x.clone()
        x[0, 0].view(-1)[0] = -0.0                                         # s = 1 keeps even a zero's sign
        x[1, 0].view(-1)[0] = 6e-8                                         # and a subnormal
        rows = R.planes_to_rows(x).contiguous().to(gpu)
        # s = 1: the input's bits
        assert same_bits(ops.freeu_filter(rows, n_img=3, h=H, w=W, s=1.0), rows)
        # run to run, and three images at once against one at a time
        a = ops.freeu_filter(rows, n_img=3, h=H, w=W, s=0.2)
        assert same_bits(ops.freeu_filter(rows, n_img=3, h=H, w=W, s=0.2), a)
        P = H * W
        for i in range(3):
            one = ops.freeu_filter(rows[i * P:(i + 1) * P].clone(), n_img=1, h=H, w=W, s=0.2)
            assert same_bits(one, a[i * P:(i + 1) * P])
        # in place, and into a given tensor
        given = torch.full_like(rows, 7.0)
        assert ops.freeu_filter(rows, n_img=3, h=H, w=W, s=0.2, out=given) is given and same_bits(given, a)
        inplace = rows.clone()
        assert ops.freeu_filter(inplace, n_img=3, h=H, w=W, s=0.2, out=inplace) is inplace and same_bits(inplace, a)
        # rows with a stride: a column block of a wider matrix, both ways
        if C > 8:
            wide = torch.zeros((rows.shape[0], C + 24), dtype=torch.float16, device=gpu)
            wide[:, 8:8 + C] = rows
            view = wide[:, 8:8 + C]
            assert same_bits(ops.freeu_filter(view, n_img=3, h=H, w=W, s=0.2), a)
            ops.freeu_filter(view, n_img=3, h=H, w=W, s=0.2, out=view)
            assert same_bits(view, a) and not wide[:, :8].any() and not wide[:, 8 + C:].any()


def test_filter_non_finite_input_stays_in_its_plane(gpu):
    import vdx  # noqa: F401
    H, W, C = 9, 16, 70
    x, _, _ = R.make_case(H, W, C, 3, 0.9, seed=2)
    clean = run_filter(gpu, x, 0.9)
    for bad_value in (float("nan"), float("inf"), float("-inf")):
        y = x.clone()
        y[1, 3, 4, 5] = bad_value
        y[2, 69, 0, 0] = bad_value
        got = run_filter(gpu, y, 0.9)
        torch.cuda.synchronize()
        touched = torch.zeros(3, C, dtype=torch.bool)
        touched[1, 3] = touched[2, 69] = True
        assert same_bits(got[~touched], clean[~touched])                   # every other plane: the bits of the clean run
        assert not torch.isfinite(got[touched].float()).all()              # the plane itself does not come out finite


def test_filter_refuses_what_it_cannot_take(gpu):
    import vdx  # noqa: F401
    from vdx import ops
    rows = torch.zeros((3 * 20, 16), dtype=torch.float16, device=gpu)
    for kw in (dict(n_img=3, h=4, w=4, s=0.9), dict(n_img=0, h=4, w=5, s=0.9), dict(n_img=3, h=4, w=5, s=float("nan")),
               dict(n_img=3, h=4, w=5, s=float("inf"))):
        with pytest.raises((ops.VdxError, ValueError)):
            ops.freeu_filter(rows, **kw)
    with pytest.raises(ops.VdxError):
        ops.freeu_filter(rows, n_img=3, h=4, w=5, s=0.9, out=rows[:, :8])
    with pytest.raises(ops.VdxError):
        ops.freeu_filter(rows.float(), n_img=3, h=4, w=5, s=0.9)
    with pytest.raises(ops.VdxError):                                      # overlapping without being the same rows
        big = torch.zeros((4 * 20, 16), dtype=torch.float16, device=gpu)
        ops.freeu_filter(big[:60], n_img=3, h=4, w=5, s=0.9, out=big[20:])
    for b in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.freeu_scale(rows, b)


# ---- the backbone scale -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 6, 7, 1, 1280], ids=lambda c: f"C{c}")
def test_scale_every_fp16_input(gpu, C):
    """All 65 536 bit patterns in the scaled half, against torch's CPU half multiply; the other half keeps its bits.  C = 16 and
    1280 take the eight-wide path, 6 and 7 the scalar one (7: odd, C // 2 = 3), C = 1 has no scaled channel."""
    import vdx  # noqa: F401
    from vdx import ops
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    half = C // 2
    M = -(-65536 // max(half, 1))
    x = every.flip(0).repeat(-(-M * C // 65536))[:M * C].reshape(M, C).clone()
    if half:
        x[:, :half] = every.repeat(-(-M * half // 65536))[:M * half].reshape(M, half)
    x = x.view(torch.float16)
    for b in (1.2, 1.4, 1.0):
        got = ops.freeu_scale(x.to(gpu), b).cpu()
        want = R.scale_ref(x, b)
        lo_g, lo_w = got[:, :half], want[:, :half]
        wrong = int(((bits(lo_g) != bits(lo_w)) & ~(lo_g.isnan() & lo_w.isnan())).sum())
        print(f"C={C} b={b}: {wrong} of {lo_g.numel()} scaled elements differ from torch's CPU product")
        assert wrong == 0
        assert same_bits(got[:, half:], x[:, half:])
        if b == 1.0:                                                       # the identity on everything that is a number
            num = ~x.isnan()
            assert torch.equal(bits(got)[num], bits(x)[num])


def test_scale_rows_with_a_stride(gpu):
    import vdx  # noqa: F401
    from vdx import ops
    g = torch.Generator().manual_seed(4)
    for C, ld in ((16, 24), (10, 24)):
        wide = torch.randn(33, ld, generator=g).half()
        dev = wide.to(gpu)
        ops.freeu_scale(dev[:, :C], 1.4)
        want = wide.clone()
        want[:, :C] = R.scale_ref(wide[:, :C], 1.4)
        assert same_bits(dev.cpu(), want)


# ---- the UNet -----------------------------------------------------------------------------------------------------------------
def tiny_model(gpu):
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.unet3d_ref import UNet3DConfig as RefCfg, synthetic_state_dict
    sd = synthetic_state_dict(RefCfg.tiny(**TINY), seed=1234)
    cfg = UNet3DConfig(block_out_channels=TINY["ch"], cross_attention_dim=TINY["cross"], transformer_in_heads=TINY["in_heads"])
    return UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu), sd


def test_unet_with_freeu_matches_the_oracle_with_freeu(gpu):
    """(2, 4, 5, 16, 32), t = 7: the bound of test_unet_gpu.py::test_unet_tiny_live_oracle_other_shape for this model at this
    shape, 4e-3; FreeU adds exact arithmetic and gets no margin of its own."""
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg
    m, sd = tiny_model(gpu)
    ref_m = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref_m.load_state_dict({k: v.half().float() for k, v in sd.items()})
    g = torch.Generator().manual_seed(21)
    sample = torch.randn(2, 4, 5, 16, 32, generator=g).half()
    ehs = torch.randn(2, 77, TINY["cross"], generator=g).half()
    R.with_freeu(ref_m, b1=SETTING["b1"], b2=SETTING["b2"], s1=SETTING["s1"], s2=SETTING["s2"])
    with torch.no_grad():
        ref = ref_m(sample.float(), torch.tensor(7), ehs.float()).sample
    x, e = sample.to(gpu), ehs.to(gpu)
    off = m(x, 7, encoder_hidden_states=e).sample
    m.enable_freeu(**SETTING)
    on = m(x, 7, encoder_hidden_states=e).sample
    err, moved = rel_l2(on.float().cpu(), ref), rel_l2(on.float().cpu(), off.float().cpu())
    print(f"FreeU on: rel-L2 {err:.3e} from the oracle with FreeU; {moved:.3f} from the forward without FreeU")
    assert err <= 4e-3
    assert moved > 0.05
    assert same_bits(m(x, 7, encoder_hidden_states=e).sample, on)          # run to run
    m.enable_freeu(1, 1, 1, 1)                                             # the neutral setting: both kernels run, nothing moves
    assert same_bits(m(x, 7, encoder_hidden_states=e).sample, off)
    m.disable_freeu()
    assert same_bits(m(x, 7, encoder_hidden_states=e).sample, off)


def test_sharded_forward_has_the_resident_bits_with_freeu(gpu):
    """tests/test_shard.py::test_unet_through_shard_store_matches_unsharded, FreeU enabled on both."""
    import vdx  # noqa: F401
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128, transformer_in_heads=2)
    sd = synthetic_state_dict(cfg, seed=9, device=gpu)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 4, 4, 16, 32, generator=g).half().to(gpu)
    e = torch.randn(2, 77, 128, generator=g).half().to(gpu)
    a = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu)
    plain = a(x, 501, encoder_hidden_states=e).sample
    want = a.enable_freeu(**SETTING)(x, 501, encoder_hidden_states=e).sample
    assert not torch.equal(want, plain)
    b = UNet3DConditionModel(cfg).load_diffusers_state_dict(sd, device=gpu).shard_(0, 1).enable_freeu(**SETTING)
    for _ in range(2):
        assert torch.equal(b(x, 501, encoder_hidden_states=e).sample, want)
    assert torch.equal(b.disable_freeu()(x, 501, encoder_hidden_states=e).sample, plain)


@pytest.mark.parametrize("F,H,W", [(4, 16, 32), (5, 16, 16), (8, 32, 32), (3, 20, 12), (16, 40, 72)])
def test_cfg_shared_prefix_bit_identical_with_freeu(gpu, F, H, W):
    """tests/test_unet_gpu.py::test_cfg_shared_prefix_bit_identical_tiny's shapes, FreeU enabled."""
    from vdx import ops
    m, _ = tiny_model(gpu)
    m.enable_freeu(**SETTING)
    g = torch.Generator().manual_seed(F * H + W)
    lat = torch.randn(1, 4, F, H, W, generator=g).half().to(gpu)
    ctx = torch.randn(1, 4, 1, H, W, generator=g).half().to(gpu)
    e = torch.randn(2, 77, TINY["cross"], generator=g).half().to(gpu)
    for c in (None, ctx):
        x = ops.cfg_input(lat, c, 0.35)
        shared = m(x, 401, encoder_hidden_states=e).sample
        assert m.last_forward_shared_prefix
        dup = m(x.clone(), 401, encoder_hidden_states=e).sample
        assert not m.last_forward_shared_prefix
        assert torch.isfinite(shared.float()).all() and torch.equal(shared, dup)
    # batch 1, the miner's forward
    one = m(lat, 401, encoder_hidden_states=e[:1]).sample
    assert torch.isfinite(one.float()).all() and torch.equal(m(lat, 401, encoder_hidden_states=e[:1]).sample, one)


def test_miner_trace_with_freeu(gpu):
    """`denoise_with_trace` needs no switch of its own: FreeU is the UNet's state."""
    from vdx.miner import denoise_with_trace, leaf_hash
    from vdx.scheduler import DDIMScheduler
    unet, _ = tiny_model(gpu)
    g = torch.Generator().manual_seed(3)
    z0 = torch.randn(1, 4, 3, 16, 16, generator=g).half().to(gpu)
    emb = torch.randn(1, 77, TINY["cross"], generator=g).half().to(gpu)

    def leaves():
        r = denoise_with_trace(unet, DDIMScheduler(), z0, emb, 3)
        assert torch.isfinite(r["z"].float()).all()
        return [leaf_hash(t, z, e) for t, z, e in zip(r["timesteps"], r["latents"], r["noise_preds"])]
    off = leaves()
    unet.enable_freeu(**SETTING)
    on = [leaves(), leaves()]
    assert on[0] == on[1]
    assert all(a != b for a, b in zip(on[0], off))
    unet.disable_freeu()
    assert leaves() == off


# ---- the job ------------------------------------------------------------------------------------------------------------------
def test_run_job_with_freeu(gpu):
    """The tiny job of tests/test_interp_gpu.py: the record carries the setting, the frames are other frames, FreeInit and
    DPM-Solver++ sample with it, and the pipeline's UNet is handed back as it came."""
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import DiffuserConfig, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)

    def job(**kw):
        got = {}
        cfg = DiffuserConfig(model_id="synthetic:tiny", num_frames=8, steps=2, height=128, width=256, chunk_size=6, overlap=2,
                             mode="chunk", noise_device="cpu", **kw)
        res = run_job(cfg, out_video=None, pipe=pipe, clip_inputs=got)
        assert pipe.unet.freeu is None
        return res, np.stack(got["frames"])
    res0, frames0 = job()
    assert "freeu" not in res0
    res1, frames1 = job(freeu=(1.2, 1.4, 0.9, 0.2))
    assert res1["freeu"] == dict(b1=1.2, b2=1.4, s1=0.9, s2=0.2)
    assert frames1.shape == frames0.shape and not np.array_equal(frames1, frames0)
    assert set(res1) == set(res0) | {"freeu"}
    res2, frames2 = job(freeu=(1.2, 1.4, 0.9, 0.2), free_init_iters=2, scheduler="dpmpp_2m")
    assert res2["freeu"] == res1["freeu"] and res2["free_init"]["iters"] == 2 and res2["scheduler"] == "dpmpp_2m"
    assert frames2.shape == frames0.shape and np.isfinite(res2["temp_instab"]) and frames2.std() > 0
    assert not np.array_equal(frames2, frames1)
    res3, frames3 = job()                                                  # and the default job is still the default job
    assert np.array_equal(frames3, frames0)
