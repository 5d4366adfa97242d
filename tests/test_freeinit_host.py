"""FreeInit on the host: the filter of vdx/freeinit.py against the definition (tests/freeinit_ref.py and hand-computed points),
the two forms of the mix against each other in float64, the twiddle tables, the configuration defaults and the refusals that
need no GPU."""
import math

import numpy as np
import pytest
import torch

import freeinit_ref as R

ODD, MIXED = (3, 7, 9), (5, 6, 10)


def test_filter_matches_hand_computed_points():
    from vdx.freeinit import lowpass_filter
    # (4, 6, 8), d_s = d_t = 0.25: the centre is (2, 3, 4); one step in x is (2 * 5 / 8 - 1)^2 = 1/16 = d_s^2
    b = lowpass_filter((4, 6, 8))
    assert b.dtype == torch.float32 and tuple(b.shape) == (4, 6, 8)
    assert float(b[2, 3, 5]) == 0.5                                        # 1 / (1 + 1^4)
    assert float(lowpass_filter((4, 6, 8), "gaussian")[2, 3, 5]) == np.float32(math.exp(-0.5))
    assert float(lowpass_filter((4, 6, 8), "ideal")[2, 3, 5]) == 1.0       # d2 == d_s^2 is inside
    assert float(lowpass_filter((4, 6, 8), "ideal")[2, 3, 6]) == 0.0
    # d_s = 0.5, d_t = 0.25, one step in t: ((0.5 / 0.25) (2 * 3 / 4 - 1))^2 = 1, over d_s^2 = 4; order 2: 1 / (1 + 16)
    assert float(lowpass_filter((4, 6, 8), "butterworth", 0.5, 0.25, 2)[3, 3, 4]) == np.float32(1 / 17)
    # corner (0, 0, 0): d2 = 3, over d_s^2 = 48; order 4
    assert float(b[0, 0, 0]) == np.float32(1 / (1 + 48.0 ** 4))


@pytest.mark.parametrize("method", ["butterworth", "gaussian", "ideal"])
@pytest.mark.parametrize("shape", [MIXED, ODD, (1, 1, 17), (2, 33, 64)])
def test_filter_is_the_definition_point_by_point(shape, method):
    from vdx.freeinit import lowpass_filter
    for d_s, d_t, order in ((0.25, 0.25, 4), (0.5, 0.5, 4), (0.3, 0.7, 2)):
        want = R.lowpass_filter(shape, method, d_s, d_t, order)
        got = lowpass_filter(shape, method, d_s, d_t, order)
        assert torch.equal(got, want.float())


def test_filter_is_one_at_the_shifted_centre_of_even_extents():
    from vdx.freeinit import lowpass_filter
    for method in ("butterworth", "gaussian", "ideal"):
        for T, h, w in ((4, 6, 8), (24, 72, 128), (2, 2, 2)):
            assert float(lowpass_filter((T, h, w), method)[T // 2, h // 2, w // 2]) == 1.0


def test_zero_stop_frequency_gives_the_zero_filter():
    from vdx.freeinit import lowpass_filter
    for method in ("butterworth", "gaussian", "ideal"):
        for d_s, d_t in ((0.0, 0.25), (0.25, 0.0), (0, 0)):
            assert not lowpass_filter(MIXED, method, d_s, d_t).any()
            assert not R.lowpass_filter(MIXED, method, d_s, d_t).any()


def test_filter_refusals():
    from vdx.freeinit import lowpass_filter
    for kw in (dict(method="box"), dict(d_s=-0.1), dict(d_t=-1), dict(d_s=float("nan")), dict(order=0), dict(order=-2),
               dict(order=1.5)):
        with pytest.raises(ValueError):
            lowpass_filter(MIXED, **kw)
    for shape in ((4, 6), (0, 6, 8), (4, 6, 8, 2)):
        with pytest.raises(ValueError):
            lowpass_filter(shape)


@pytest.mark.parametrize("vol", [(1, 4) + MIXED, (1, 4) + ODD, (2, 3, 1, 1, 17), (1, 1, 2, 33, 64)])
def test_difference_form_equals_shift_form_in_float64(vol):
    g = torch.Generator().manual_seed(7)
    z = torch.randn(vol, generator=g).half()
    eta = torch.randn(vol, generator=g)
    for method in ("butterworth", "gaussian", "ideal"):
        H = R.lowpass_filter(vol[2:], method, 0.5, 0.5)
        a, b = R.mix(z, eta, H), R.mix_difference_form(z, eta, H)
        assert float((a - b).abs().max()) < 1e-12
    # an all-zero filter is eta, an all-ones filter z, in either form
    assert float((R.mix(z, eta, torch.zeros(vol[2:])) - eta.double()).abs().max()) < 1e-12
    assert float((R.mix(z, eta, torch.ones(vol[2:])) - z.double()).abs().max()) < 1e-12


def test_real_part_is_part_of_the_definition_for_odd_extents():
    """An fftshift-ed low-pass of odd extent is not Hermitian: the mix of two real volumes has an imaginary part that is no
    rounding error, and the definition drops it.  Even extents with the filter's centre at the zero frequency leave none."""
    g = torch.Generator().manual_seed(7)
    vol = (1, 4) + ODD
    z, eta = torch.randn(vol, generator=g).half(), torch.randn(vol, generator=g)
    im = R.mix_complex(z, eta, R.lowpass_filter(ODD, "butterworth", 0.5, 0.5)).imag.abs().max()
    print(f"largest discarded imaginary part at {ODD}: {float(im):.3f}")
    assert float(im) > 1e-2


def test_twiddle_tables():
    from vdx import ops
    for n in (1, 2, 17, 72, 128, 512):
        tw = ops.freeinit_twiddles(n)
        assert tw.dtype == torch.float64 and tuple(tw.shape) == (n, 2) and tw.is_contiguous()
        assert tw[0].tolist() == [1.0, 0.0]
        j = np.arange(n)
        want = np.stack([np.cos(2 * np.pi * j / n), -np.sin(2 * np.pi * j / n)], 1)
        assert np.abs(tw.numpy() - want).max() <= 2.0 ** -52
        assert np.abs(np.hypot(tw.numpy()[:, 0], tw.numpy()[:, 1]) - 1).max() <= 2.0 ** -52


def test_sizes_the_kernels_do_not_take_are_refused_without_the_library():
    from vdx import ops
    from vdx._lib import VdxError
    assert ops.freeinit_check_sizes((1, 4, 24, 72, 128)) == (4, 24, 72, 128)
    assert ops.freeinit_check_sizes((2, 3, 1, 1, 512)) == (6, 1, 1, 512)
    for shape in ((1, 4, 513, 2, 2), (1, 4, 2, 513, 2), (1, 4, 2, 2, 513), (4, 24, 72, 128), (1, 4, 0, 8, 8),
                  (64, 64, 512, 512, 2)):
        with pytest.raises(VdxError):
            ops.freeinit_check_sizes(shape)


def test_one_iteration_is_the_default_everywhere():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, check_free_init, config_from_args
    c = DiffuserConfig()
    assert (c.free_init_iters, c.free_init_method, c.free_init_spatial, c.free_init_temporal, c.free_init_order) == \
        (1, "butterworth", 0.25, 0.25, 4)
    p = build_arg_parser()
    assert config_from_args(p.parse_args([])) == config_from_args(p.parse_args(["--free_init", "1"]))
    d = config_from_args(p.parse_args([]))
    assert (d.free_init_iters, d.free_init_method, d.free_init_spatial, d.free_init_temporal, d.free_init_order) == \
        (1, "butterworth", 0.25, 0.25, 4)
    e = config_from_args(p.parse_args(["--free_init", "3", "--free_init_method", "gaussian", "--free_init_spatial", "0.5",
                                       "--free_init_temporal", "0.125", "--free_init_order", "2"]))
    assert (e.free_init_iters, e.free_init_method, e.free_init_spatial, e.free_init_temporal, e.free_init_order) == \
        (3, "gaussian", 0.5, 0.125, 2)
    # with one iteration nothing about the option is looked at: halo and video-to-video stay available
    assert check_free_init(DiffuserConfig(init_video="clip.npy", free_init_method="whatever"), "halo") == 1


def test_refusals_raise_before_any_work():
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, check_free_init, run_job
    two = DiffuserConfig(free_init_iters=2)
    assert check_free_init(two) == 2
    with pytest.raises(ValueError, match="allgather"):
        check_free_init(two, "halo")
    with pytest.raises(ValueError, match="allgather"):
        run_job(two, exchange="halo", out_video=None)                      # before any model is loaded: needs no GPU
    vid = DiffuserConfig(free_init_iters=2, init_video="clip.npy")
    with pytest.raises(ValueError, match="init_video"):
        check_free_init(vid)
    with pytest.raises(ValueError, match="init_video"):
        run_job(vid, out_video=None)
    with pytest.raises(ValueError, match="init_latents"):
        DistributedVideoDiffuser(two, None, None, None, None, init_latents=torch.zeros(1))
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            check_free_init(DiffuserConfig(free_init_iters=bad))
    for kw in (dict(free_init_method="box"), dict(free_init_spatial=-0.5), dict(free_init_temporal=-1.0), dict(free_init_order=0)):
        with pytest.raises(ValueError):
            check_free_init(DiffuserConfig(free_init_iters=2, **kw))


def test_iteration_noise_is_seeded_by_the_iteration_and_leaves_the_global_generator_alone():
    from vdx.pipeline import iteration_noise, seeded_noise
    torch.manual_seed(123)
    before = torch.get_rng_state()
    a, b, a2 = (iteration_noise((1, 4, 3, 5, 6), i, "cpu", "cpu") for i in (1, 2, 1))
    assert torch.equal(torch.get_rng_state(), before)
    assert a.dtype == torch.float32 and torch.equal(a, a2) and not torch.equal(a, b)
    base = seeded_noise((1, 4, 3, 5, 6), 1.0, "cpu", "cpu")
    assert not torch.equal(a.half(), base)                                 # the fresh noise is not the base noise again


# ---- the round accounting of `DistributedVideoDiffuser.__call__`, on the CPU (tests/test_halo_host.py's arrangement) -----------
from test_halo_host import cpu_blend  # noqa: E402,F401  (the fixture: ops.blend_* as their torch-CPU statements)

T, CS, OV = 10, 6, 2                                                       # the smallest job with a seam and a ramp


def _stub(lat):              # stands in for the UNet + scheduler steps: any deterministic function of the chunk's content
    x = lat.float()
    return (0.5 * x + 0.25 * torch.roll(x, 1, dims=2) - 0.1 * x.mean(dim=2, keepdim=True)).half()


def _blend_of_stub(start):
    from oracle.pipeline_ref import plan_chunks, ramp_blend
    _, o, ranges = plan_chunks(T, 1, CS, OV, False)
    return ramp_blend([(s, e, _stub(start[:, :, s:e].clone())) for s, e in ranges], T, o, start)


class _Unet:                 # only .config.in_channels is used outside denoise()
    class config:
        in_channels = 4
    W = None


def _diffuser(monkeypatch, iters, fail_at=None):
    """-> (the diffuser, reinit's calls [(z0, iteration, returned)], the context of every denoise call, the filters built)."""
    import vdx.freeinit
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    cfg = DiffuserConfig(num_frames=T, steps=2, chunk_size=CS, overlap=OV, height=32, width=32, mode="hybrid_ctx", device="cpu",
                         noise_device="cpu", free_init_iters=iters)
    d = DistributedVideoDiffuser(cfg, _Unet(), DDIMScheduler(), None, None)
    reinits, ctxs, filters = [], [], []

    def denoise(lat):
        if len(ctxs) == fail_at:
            raise RuntimeError("denoise failed")
        ctxs.append(d.ctx.clone())
        return _stub(lat)

    def reinit(z0, base, scheduler, iteration, filt, noise_device=None):
        out = (0.5 * z0.float() + 0.25 * base.float() + iteration).half()
        reinits.append((z0.clone(), iteration, out))
        return out

    real_filter = vdx.freeinit.lowpass_filter
    d.denoise = denoise
    monkeypatch.setattr(vdx.freeinit, "reinit", reinit)
    monkeypatch.setattr(vdx.freeinit, "lowpass_filter", lambda *a: filters.append(a) or real_filter(*a))
    return d, reinits, ctxs, filters


BYTES = ("network_bytes", "payload_bytes", "payload_bytes_actual")


def test_rounds_are_summed_and_the_context_follows_the_start_latent(cpu_blend, monkeypatch):  # noqa: F811
    from vdx.pipeline import seeded_noise
    base = seeded_noise((1, 4, T, 4, 4), 1.0, "cpu", "cpu")
    d1, reinits, ctxs, filters = _diffuser(monkeypatch, 1)
    lat1, info1 = d1()
    assert torch.equal(lat1, _blend_of_stub(base))
    assert "free_init" not in info1 and reinits == [] and filters == [] and d1.free_init_starts == []
    windows = len(info1["ranges"])
    assert len(ctxs) == windows == 3                                       # (0, 6), (4, 10) and the reference's tail (8, 10)

    d2, reinits, ctxs, filters = _diffuser(monkeypatch, 2)
    ctx0 = d2.ctx
    assert torch.equal(ctx0, base.mean(dim=2, keepdim=True))
    lat2, info2 = d2()
    rec = info2["free_init"]
    assert set(info2) == set(info1) | {"free_init"}
    assert [info2[k] for k in BYTES] == [2 * info1[k] for k in BYTES] and info1["payload_bytes"] == (6 + 6 + 2) * 4 * 2
    assert len(rec["denoise_s"]) == 2 and len(rec["reinit_s"]) == 1 and info2["denoise_s"] == sum(rec["denoise_s"])
    assert len(filters) == 1 and len(reinits) == 1
    z0, iteration, start = reinits[0]
    assert iteration == 1 and torch.equal(z0, lat1)                        # once, with the first round's blend
    assert len(ctxs) == 2 * windows
    assert all(torch.equal(c, ctx0) for c in ctxs[:windows])
    assert all(torch.equal(c, start.mean(dim=2, keepdim=True)) for c in ctxs[windows:])
    assert torch.equal(lat2, _blend_of_stub(start))
    assert len(d2.free_init_starts) == 1 and d2.free_init_starts[0] is start
    assert d2.ctx is ctx0


def test_a_round_that_raises_leaves_the_context_and_the_recorded_starts_alone(cpu_blend, monkeypatch):  # noqa: F811
    d, reinits, ctxs, _ = _diffuser(monkeypatch, 2, fail_at=3)             # the first denoise call of the second round
    ctx0, before = d.ctx, ["the last call's"]
    d.free_init_starts = before
    with pytest.raises(RuntimeError, match="denoise failed"):
        d()
    assert len(reinits) == 1 and len(ctxs) == 3
    assert d.ctx is ctx0 and d.free_init_starts is before


def test_one_halo_round_reports_the_owned_ranges(cpu_blend, monkeypatch):  # noqa: F811
    from vdx.pipeline import seeded_noise
    d, reinits, _, filters = _diffuser(monkeypatch, 1)
    owned, info = d(exchange="halo")
    assert info["owned"] == [(s, e) for s, e, _ in owned] and "free_init" not in info and reinits == [] and filters == []
    edges = sorted(info["owned"])
    assert edges[0][0] == 0 and edges[-1][1] == T and all(a[1] == b[0] for a, b in zip(edges[:-1], edges[1:]))
    want = _blend_of_stub(seeded_noise((1, 4, T, 4, 4), 1.0, "cpu", "cpu"))
    assert all(torch.equal(lat, want[:, :, s:e]) for s, e, lat in owned)
    allgather_info = d()[1]
    assert set(info) == set(allgather_info) | {"owned"} and [info[k] for k in BYTES] == [allgather_info[k] for k in BYTES]
