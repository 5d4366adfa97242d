"""-m gpu: video-to-video refinement on libvdx_hip.so — Pillow's bicubic resize, the uint8 -> conv_in map, the (0,1,0,1)
stride-2 conv gather, the encoder against its fp32 restatement (tests/vae_encoder_ref.py; live at tiny widths, the committed
golden at Stable-Diffusion widths), the posterior and add_noise kernels against the torch fp16 expressions, and the pipeline
and CLI with --init_video."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def close(out, ref, tol=3e-3):          # the conv tests' bound (tests/test_ops_gpu.py)
    out = out.float().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    scale = ref.abs().max().item() + 1e-6
    bad = ((out - ref).abs() > tol * scale + tol * ref.abs()).sum().item()
    assert bad == 0, f"{bad} elements outside the bound"


def _vae(gpu, widths=(64, 64, 128, 128), seed=8):
    import vdx  # noqa: F401
    from vdx.vae import AutoencoderKL, VaeConfig
    from vdx.weights import synthetic_vae_encoder_state_dict
    cfg = VaeConfig(block_out_channels=widths)
    sd = synthetic_vae_encoder_state_dict(cfg, seed=seed)
    return AutoencoderKL(cfg).load_diffusers_encoder_state_dict(sd, device=gpu), sd, cfg


def _frames(F_, H, W, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (F_, H, W, 3), dtype=np.uint8))


# ---- 1. resize ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((576, 320), (1024, 576)), ((640, 360), (1024, 576)), ((96, 64), (96, 64)),
                                     ((200, 120), (96, 56)), ((80, 48), (64, 48))])
def test_resize_matches_pillow(gpu, src, dst):
    from PIL import Image
    from vdx import ops
    fr = _frames(2, src[1], src[0], seed=src[0])
    wide = torch.zeros((2, src[1], src[0] + 5, 3), dtype=torch.uint8)     # pitched rows
    wide[:, :, :src[0]] = fr
    out = ops.resize_u8(wide.to(gpu)[:, :, :src[0]], dst[1], dst[0]).cpu().numpy()
    for i in range(2):
        want = np.asarray(Image.fromarray(fr[i].numpy()).resize(dst))
        assert np.array_equal(out[i], want), i


# ---- 2. uint8 frames -> conv_in rows ---------------------------------------------------------------------------------
def test_frames_to_conv_in_equals_conv_in_of_mapped(gpu):
    from vdx import _lib, ops
    fr = _frames(3, 24, 40, seed=1).to(gpu)
    rows = ops.frames_to_conv_in(fr)
    x5 = ops.u8_to_unit_lut().to(gpu)[fr.long()].permute(0, 3, 1, 2).unsqueeze(2).contiguous()   # (F,3,1,H,W)
    cols = torch.empty_like(rows)
    lib = _lib.load()
    _lib.check(lib.vdx_im2col_in_f16(x5.data_ptr(), cols.data_ptr(), 3, 3, 1, 24, 40, 64, ops._stream()), "im2col")
    assert torch.equal(rows, cols)
    assert not rows[:, 27:].any()
    # border taps are 0.0 (the normalised image is padded), not map(0) = -1
    assert (rows[0, :9] == 0).all() and (rows[0, 12:15] != 0).any()
    g = torch.Generator().manual_seed(0)
    w = torch.zeros(128, 64, dtype=torch.float16)
    w[:, :27] = (torch.randn(128, 27, generator=g) / 5).half()
    b = (0.1 * torch.randn(128, generator=g)).half()
    assert torch.equal(ops.conv_in(x5, w.to(gpu), b.to(gpu)), ops.gemm(rows, w.to(gpu), M=rows.shape[0], bias=b.to(gpu)))


# ---- 3. asymmetric stride-2 conv ---------------------------------------------------------------------------------------
def _down_case(gpu, C, H, W, n=1, seed=0):
    from vdx import packing
    g = torch.Generator().manual_seed(seed + C)
    x = torch.randn(n, C, H, W, generator=g).half().float()
    w = (torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5).half().float()
    b = (0.1 * torch.randn(C, generator=g)).half().float()
    rows = packing.nchw_to_rows(x).half().to(gpu).contiguous()
    return x, w, b, rows, packing.pack_conv3x3(w).half().to(gpu), b.half().to(gpu)


@pytest.mark.parametrize("C,H,W", [(128, 576, 1024), (256, 288, 512), (512, 144, 256)])
def test_downsample_conv_full_sizes(gpu, C, H, W):
    from vdx import ops, packing
    x, w, b, rows, wp, bp = _down_case(gpu, C, H, W)
    ref = packing.nchw_to_rows(F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2))
    M = (H // 2) * (W // 2)
    out = ops.gemm(rows, wp, M=M, mode=ops.CONV3X3, bias=bp, conv=(1, H, W, H // 2, W // 2, 2, False), pad_mode=1)
    close(out, ref)
    # a row split gives the same bits
    s = (M // 3) // 64 * 64 + 17
    part = torch.empty_like(out)
    for rb, re_ in ((0, s), (s, 0)):
        ops.gemm(rows, wp, M=M, mode=ops.CONV3X3, bias=bp, conv=(1, H, W, H // 2, W // 2, 2, False), pad_mode=1,
                 row_begin=rb, row_end=re_, out=part)
    assert torch.equal(part, out)


def test_downsample_conv_every_kernel_family(gpu):
    from vdx import ops, packing
    n, C, H, W = 2, 128, 34, 50             # odd tile tails, even sizes
    x, w, b, rows, wp, bp = _down_case(gpu, C, H, W, n=n, seed=3)
    ref = packing.nchw_to_rows(F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2))
    ref_sym = packing.nchw_to_rows(F.conv2d(x, w, b, stride=2, padding=1))
    M = n * (H // 2) * (W // 2)
    geo = (n, H, W, H // 2, W // 2, 2, False)
    # every conv family: automatic (0), the tiled 128x128 / 256x320 / 256x64 forms (1, 2, 6, 5, 9) and the rings (3, 4, 8);
    # 7 (weights-stationary) is plain-mode only
    for v in (0, 1, 2, 3, 4, 5, 6, 8, 9):
        close(ops.gemm(rows, wp, M=M, mode=ops.CONV3X3, bias=bp, conv=geo, variant=v), ref_sym)
        close(ops.gemm(rows, wp, M=M, mode=ops.CONV3X3, bias=bp, conv=geo, variant=v, pad_mode=1), ref)
    # odd input sizes: h_out = h_in // 2
    x, w, b, rows, wp, bp = _down_case(gpu, 64, 9, 13, n=1, seed=5)
    ref = packing.nchw_to_rows(F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2))
    close(ops.gemm(rows, wp, M=4 * 6, mode=ops.CONV3X3, bias=bp, conv=(1, 9, 13, 4, 6, 2, False), pad_mode=1), ref)


def test_downsample_conv_refusals(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    x, w, b, rows, wp, bp = _down_case(gpu, 64, 16, 16)
    with pytest.raises(VdxError, match="pad_mode 1"):
        ops.gemm(rows, wp, M=256, mode=ops.CONV3X3, conv=(1, 16, 16, 16, 16, 1, False), pad_mode=1)
    with pytest.raises(VdxError, match="pad_mode 1"):
        ops.gemm(rows, wp, M=32 * 32, mode=ops.CONV3X3, conv=(1, 16, 16, 32, 32, 1, True), pad_mode=1)
    with pytest.raises(VdxError, match="inconsistent"):
        ops.gemm(rows, wp, M=81, mode=ops.CONV3X3, conv=(1, 16, 16, 9, 9, 2, False), pad_mode=1)
    x2, w2, b2, rows2, wp2, bp2 = _down_case(gpu, 256, 16, 16)
    with pytest.raises(VdxError, match="pad_mode = 1"):
        ops.gemm(rows2, wp2, M=64, mode=ops.CONV3X3, conv=(1, 16, 16, 8, 8, 2, False), pad_mode=1, ksplit=2)
    with pytest.raises(VdxError, match="conv3x3 setting"):
        ops.gemm(rows, wp[:, :64].contiguous(), M=256, pad_mode=1)


# ---- 4. encode parity ---------------------------------------------------------------------------------------------------
def test_encode_tiny_matches_restatement(gpu):
    import vae_encoder_ref as ref
    from vdx import ops
    vae, sd, cfg = _vae(gpu)
    m = ref.AutoencoderKLEncoderRef(ref.VaeConfig(block_out_channels=cfg.block_out_channels)).eval()
    m.load_state_dict({k: v.float() for k, v in sd.items()})
    fr = _frames(2, 64, 128, seed=4)
    x = ref.unit_map(fr)
    with torch.no_grad():
        want = m.moments(x)
    d = vae.encode(x.half().to(gpu)).latent_dist
    got = torch.cat([d.mean, d._cols(4)], 1).float().cpu()
    e = rel_l2(got, want)
    print(f"tiny encoder moments rel-L2 {e:.3e}")
    assert e < 4e-3
    assert torch.equal(d.mode(), d.mean)


def test_encode_full_frame_sd_widths_vs_golden(gpu):
    sys.path.insert(0, GOLD)
    import make_vid2vid_golden as mk
    vae, _, _ = _vae(gpu, widths=(128, 256, 512, 512), seed=mk.WEIGHT_SEED)
    gold = np.load(os.path.join(GOLD, "vid2vid_encoder_full.npz"))
    want = torch.from_numpy(gold["moments"]).float()
    from vdx import ops
    cols = ops.frames_to_conv_in(torch.from_numpy(mk.frame())[None].to(gpu))
    m, hh, ww = vae._encode_rows(cols, 1, mk.H, mk.W)
    got = m[:, :8].float().cpu().reshape(hh, ww, 8).permute(2, 0, 1)
    e = rel_l2(got, want)
    print(f"full-size encoder moments (8,{hh},{ww}) rel-L2 {e:.3e}")
    assert (hh, ww) == (72, 128) and e <= 4e-3


# ---- 5. batch independence -------------------------------------------------------------------------------------------------
def test_encode_batch_independent_and_fast_path_equal(gpu):
    from vdx import ops
    vae, _, _ = _vae(gpu)
    T = 24
    fr = _frames(T, 64, 64, seed=6).to(gpu)
    g = torch.Generator(device=gpu).manual_seed(1)
    noise = torch.randn((T, 4, 8, 8), generator=g, device=gpu, dtype=torch.float16)
    a = vae.encode_frames_u8(fr, noise=noise, batch=1)
    for bsz in (8, 24):
        assert torch.equal(vae.encode_frames_u8(fr, noise=noise, batch=bsz), a), bsz
    x = ops.u8_to_unit_lut().to(gpu)[fr[:8].long()].permute(0, 3, 1, 2).contiguous()
    d = vae.encode(x).latent_dist
    s = d.sample(noise=noise[:8])
    assert torch.equal((0.18215 * s).permute(1, 0, 2, 3), a[0, :, :8])
    mode = vae.encode_frames_u8(fr[:8], posterior="mode")
    assert torch.equal((0.18215 * d.mode()).permute(1, 0, 2, 3), mode[0])


# ---- 6. posterior and add_noise vs the torch fp16 expressions ---------------------------------------------------------------
def test_posterior_kernel_matches_torch(gpu):
    from vdx import ops
    n, h, w = 3, 8, 16
    g = torch.Generator(device=gpu).manual_seed(7)
    mom = torch.randn((n * h * w, 64), generator=g, device=gpu).half()
    mom[:, 4:8] = (torch.rand((n * h * w, 4), generator=g, device=gpu) * 70 - 45).half()    # clamp at both ends
    eps = torch.randn((n, 4, h, w), generator=g, device=gpu, dtype=torch.float16)
    m4 = mom[:, :8].reshape(n, h, w, 8).permute(0, 3, 1, 2)
    mean, logvar = m4[:, :4], m4[:, 4:]
    logvar = torch.clamp(logvar, -30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    want = 0.18215 * (mean + std * eps)
    got = ops.vae_posterior(mom, n, h * w, eps=eps, scale=0.18215).view(n, 4, h, w)
    # the kernel's std alone (mean 0, eps 1, scale 1: out = fp16(0 + fp16(std * 1)) = std) against torch.exp
    one = mom.clone()
    one[:, :4] = 0
    std_k = ops.vae_posterior(one, n, h * w, eps=torch.ones_like(eps)).view(n, 4, h, w)
    d_ulp = (std_k.view(torch.int16).int() - std.contiguous().view(torch.int16).int()).abs()
    print(f"posterior std: {int((d_ulp > 0).sum())} of {d_ulp.numel()} differ from torch.exp (max {int(d_ulp.max())} ulp); "
          f"samples: {int((got != want).sum())} differ")
    assert int(d_ulp.max()) == 0
    assert torch.equal(got, want)
    assert torch.equal(ops.vae_posterior(mom, n, h * w, scale=0.18215).view(n, 4, h, w), 0.18215 * mean)


def test_add_noise_matches_diffusers_expression(gpu):
    from vdx.scheduler import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(50, device=gpu)
    g = torch.Generator(device=gpu).manual_seed(9)
    x0 = torch.randn((1, 4, 6, 8, 16), generator=g, device=gpu, dtype=torch.float16)
    nz = torch.randn((1, 4, 6, 8, 16), generator=g, device=gpu, dtype=torch.float16)
    ac = s.alphas_cumprod.to(device=gpu, dtype=torch.float16)
    for t in (981, 581, 1):
        sa, s1 = ac[t] ** 0.5, (1 - ac[t]) ** 0.5
        assert torch.equal(s.add_noise(x0, nz, t), sa * x0 + s1 * nz), t


# ---- 7. pipeline, tiny synthetic model --------------------------------------------------------------------------------------
def _tiny_pipe(gpu):
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    for mm in (pipe.unet, pipe.text_encoder, pipe.vae):
        mm.to(gpu)
    return pipe


def test_pipeline_vid2vid_start_latent_steps_and_determinism(gpu):
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, seeded_noise, vid2vid_timesteps
    from vdx.weights import synthetic_vae_encoder_state_dict
    pipe = _tiny_pipe(gpu)
    T, H, W, steps, strength = 6, 128, 128, 6, 0.5
    pipe.vae.load_diffusers_encoder_state_dict(synthetic_vae_encoder_state_dict(pipe.vae.cfg, 8), device=gpu)
    fr = _frames(T, H, W, seed=11).to(gpu)
    g = torch.Generator(device=gpu).manual_seed(1)
    x0 = pipe.vae.encode_frames_u8(fr, noise=torch.randn((T, 4, 16, 16), generator=g, device=gpu, dtype=torch.float16))
    emb = torch.randn((2, 77, 128), generator=g, device=gpu, dtype=torch.float16)
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=4, overlap=2, height=H, width=W, mode="hybrid_ctx",
                         device=str(gpu), strength=strength)
    calls = []
    fwd = pipe.unet.forward

    def counting(x, t, *a, **k):
        calls.append(int(t))
        return fwd(x, t, *a, **k)
    pipe.unet.forward = counting
    d = DistributedVideoDiffuser(cfg, pipe.unet, pipe.scheduler, emb[:1], emb[1:], init_latents=x0)
    ts = vid2vid_timesteps(pipe.scheduler, steps, strength)
    assert len(ts) == int(steps * strength) and d.timesteps == ts
    base = seeded_noise((1, 4, T, 16, 16), 1.0, cfg.device)
    start = pipe.scheduler.add_noise(x0, base, ts[0])
    assert torch.equal(d._start, start)
    assert torch.equal(d.ctx, start.mean(dim=2, keepdim=True))
    lat1, info = d()
    windows = len(info["ranges"])
    assert calls == ts * windows and info["steps_run"] == len(ts)
    d2 = DistributedVideoDiffuser(cfg, pipe.unet, pipe.scheduler, emb[:1], emb[1:], init_latents=x0)
    lat2, _ = d2()
    assert torch.equal(lat1, lat2)
    assert not torch.equal(lat1, DistributedVideoDiffuser(cfg, pipe.unet, pipe.scheduler, emb[:1], emb[1:])()[0])


# ---- 8. CLI end to end ------------------------------------------------------------------------------------------------------
def test_cli_init_video_end_to_end(gpu, tmp_path):
    clip = _frames(4, 40, 72, seed=12).numpy()           # not the target size: the resize runs
    np.save(tmp_path / "clip.npy", clip)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out_csv, out_mp4 = tmp_path / "r.csv", tmp_path / "o.mp4"
    r = subprocess.run([sys.executable, "-m", "vdx.pipeline", "--model_id", "synthetic:tiny", "--init_video",
                        str(tmp_path / "clip.npy"), "--strength", "0.5", "--num_frames", "4", "--steps", "4", "--height", "128",
                        "--width", "128", "--chunk_size", "4", "--overlap", "2", "--out_csv", str(out_csv), "--out_video",
                        str(out_mp4)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    from vdx.metrics import CSV_HEADER
    rows = list(csv.reader(open(out_csv)))
    assert rows[0] == CSV_HEADER and len(rows) == 2 and len(rows[1]) == len(CSV_HEADER)
    assert os.path.getsize(out_mp4) > 500
    bad = np.zeros((3, 40, 72, 3), np.uint8)
    np.save(tmp_path / "bad.npy", bad)
    r = subprocess.run([sys.executable, "-m", "vdx.pipeline", "--model_id", "synthetic:tiny", "--init_video",
                        str(tmp_path / "bad.npy"), "--num_frames", "4", "--steps", "2", "--height", "128", "--width", "128",
                        "--out_csv", str(tmp_path / "b.csv"), "--out_video", str(tmp_path / "b.mp4")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode != 0 and "frames" in r.stderr


# ---- 7 (cont.). the pipeline against the fp32 oracle composition --------------------------------------------------------
def test_pipeline_vid2vid_matches_oracle_composition(gpu):
    """Restated encoder + posterior (fp32) -> diffusers' fp16 add_noise -> the oracle's CFG/DDIM loop over the truncated
    schedule (fp32 UNet behind fp16 I/O) -> the oracle's ramp blend, against the HIP pipeline on the same weights and noise."""
    import importlib.util
    import vae_encoder_ref as ref
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    from oracle.ddim_ref import DDIMSchedulerRef
    from oracle.pipeline_ref import base_noise, denoise, my_ranges, plan_chunks, ramp_blend
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg, synthetic_state_dict
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLD, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)

    T, H, W, steps, strength, chunk, ov = 6, 128, 128, 6, 0.5, 4, 2
    h, w = H // 8, W // 8
    tiny = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)
    sd = synthetic_state_dict(RefCfg.tiny(**tiny), seed=1234)
    unet = UNet3DConditionModel(UNet3DConfig(block_out_channels=tiny["ch"], cross_attention_dim=tiny["cross"],
                                             transformer_in_heads=tiny["in_heads"])).load_diffusers_state_dict(sd, device=gpu)
    unet_ref = UNet3DConditionModelRef(RefCfg.tiny(**tiny)).eval()
    unet_ref.load_state_dict({k: v.half().float() for k, v in sd.items()})
    vae, esd, vcfg = _vae(gpu)
    fr = _frames(T, H, W, seed=13)
    noise = torch.randn((T, 4, h, w), generator=torch.Generator().manual_seed(1)).half()
    emb = torch.randn(2, 77, tiny["cross"], generator=torch.Generator().manual_seed(5)).half()

    # ---- HIP path
    x0 = vae.encode_frames_u8(fr.to(gpu), noise=noise.to(gpu))
    cfg = DiffuserConfig(num_frames=T, steps=steps, chunk_size=chunk, overlap=ov, height=H, width=W, mode="hybrid_ctx",
                         device="cuda", noise_device="cpu", strength=strength)
    lat, info = DistributedVideoDiffuser(cfg, unet, DDIMScheduler(), emb[1:].to(gpu), emb[:1].to(gpu), init_latents=x0)()

    # ---- oracle composition on the CPU
    enc = ref.AutoencoderKLEncoderRef(ref.VaeConfig(block_out_channels=vcfg.block_out_channels)).eval()
    enc.load_state_dict({k: v.float() for k, v in esd.items()})
    with torch.no_grad():
        x0_ref = (0.18215 * ref.posterior(enc.moments(ref.unit_map(fr)), noise.float())).half()   # (T,4,h,w)
    x0_ref = x0_ref.permute(1, 0, 2, 3).unsqueeze(0).contiguous()
    rs = DDIMSchedulerRef()
    rs.set_timesteps(steps)
    init = min(int(steps * strength), steps)
    rs.timesteps = rs.timesteps[steps - init:]                # the DDIM step keeps prev_t = t - 1000 // steps
    t0 = int(rs.timesteps[0])
    ac = rs.alphas_cumprod.half()                             # diffusers' add_noise: alphas_cumprod in the sample dtype
    start = ac[t0] ** 0.5 * x0_ref + (1 - ac[t0]) ** 0.5 * base_noise(T, 4, h, w)
    ctx = start.mean(dim=2, keepdim=True)
    cs, ov_, ranges = plan_chunks(T, 1, chunk, ov)
    chunks = [(s, e, denoise(mg.FP32UNetOnHalfIO(unet_ref), rs, start[:, :, s:e].clone(), emb[1:], emb[:1], 7.5, ctx, 0.35))
              for s, e in my_ranges(ranges, 1, 0)]
    lat_ref = ramp_blend(chunks, T, ov_, start)

    assert [tuple(r) for r in info["ranges"]] == [tuple(r) for r in ranges] and info["steps_run"] == init
    e_x0 = rel_l2(x0.float().cpu(), x0_ref.float())
    e_lat = rel_l2(lat.float().cpu(), lat_ref.float())
    print(f"vid2vid vs the oracle composition: x0 rel-L2 {e_x0:.3e}, latent after {init} of {steps} steps {e_lat:.3e}")
    assert e_x0 <= 4e-3
    assert e_lat <= 2e-2                                     # tests/test_e2e_gpu.py's bound on the blended latent


# ---- 9. two ranks (gloo, one shared GPU) -------------------------------------------------------------------------------------
def test_two_ranks_hold_identical_start_latent_and_ctx(gpu, tmp_path):
    """Every rank encodes the whole clip itself: the ranks' clean latents, start latents and ctx are torch.equal (checked
    over gloo inside the worker), and the two-rank result equals the same windows denoised serially in one process."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_pipeline_worker import build
    from dist_vid2vid_worker import VAE_WIDTHS, config
    from vdx.pipeline import DistributedVideoDiffuser, encode_init_video
    from vdx.planner import plan
    from vdx.scheduler import DDIMScheduler
    from vdx.vae import AutoencoderKL, VaeConfig
    world, T, chunk, ov, steps, strength = 2, 8, 4, 2, 4, 0.5
    clip = str(tmp_path / "clip.npy")
    np.save(clip, _frames(T, 72, 96, seed=21).numpy())        # another size: every rank runs the resize too
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", "29701",
                        os.path.join(ROOT, "tests", "dist_vid2vid_worker.py"), str(out), clip, str(T), str(chunk), str(ov),
                        str(steps), str(strength)], capture_output=True, text=True, timeout=900, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == world
    got = torch.load(out, weights_only=True)
    assert got["steps_run"] == int(steps * strength)

    # the same job serially: one process, resident weights, every window in turn
    cfg = config(clip, T, chunk, ov, steps, strength)
    x0, _ = encode_init_video(cfg, AutoencoderKL(VaeConfig(block_out_channels=VAE_WIDTHS)), gpu)
    assert torch.equal(got["x0"], x0.cpu())
    m, emb = build(gpu, 0, 1)
    d = DistributedVideoDiffuser(cfg, m, DDIMScheduler(), emb[1:], emb[:1], init_latents=x0)
    assert torch.equal(got["start"], d._start.cpu()) and torch.equal(got["ctx"], d.ctx.cpu())
    cp = plan(T, world, chunk, ov, no_chunking=False)
    assert [tuple(x) for x in got["ranges"]] == [tuple(x) for x in cp.ranges]
    order = [i for rk in range(world) for i in range(len(cp.ranges)) if i % world == rk]
    den = {i: d.denoise(d._start[:, :, cp.ranges[i][0]:cp.ranges[i][1]].clone()) for i in order}
    want = d.blend([(cp.ranges[i][0], cp.ranges[i][1], den[i]) for i in order], d._start, cp.overlap)
    assert torch.equal(got["lat"], want.cpu())
