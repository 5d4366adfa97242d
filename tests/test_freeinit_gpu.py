"""-m gpu: FreeInit's frequency mix (csrc/freeinit.hip) against the float64 restatement of tests/freeinit_ref.py, its exact
properties, and the job with `free_init_iters` on the tiny golden UNet (tests/test_e2e_gpu.py's shapes)."""
import math
import os
import subprocess
import sys

import pytest
import torch

import freeinit_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# profiles/freeinit_parity.txt: the share of elements whose fp16 bits differ from the restatement's rounding, measured on every
# volume below and at the headline extent (1, 4, 24, 72, 128) with all three filters: 0 of 884736 there, 0 everywhere (the
# kernels sum in fp64; what is left is a double that lies within 1e-16 of an fp16 rounding boundary).  An earlier fp32 build
# of the same kernels measured 1.2e-3 to 1.7e-3 at the headline extent and 6 to 9 fp16 ulp at results near zero, where fp16's
# spacing is 6e-8: that is why they are fp64.  The tests allow 4x the measured share, the project's usual margin over a
# measured floor, as a count: ceil(4 * share * elements), which is no element at all.
MEASURED_SHARE = 0.0
SHARE_BOUND = 4 * MEASURED_SHARE

METHODS = ("butterworth", "gaussian", "ideal")
SMALL = [(1, 4, 5, 6, 10),        # mixed odd and even extents
         (1, 4, 3, 7, 9),         # all odd: the discarded imaginary part is about 0.2; catches a kernel that assumes Hermitian H
         (2, 3, 1, 1, 17),        # degenerate axes, a prime, B > 1
         (1, 1, 2, 33, 64)]       # a two-frame volume, one odd and one even spatial extent
HEADLINE = (1, 4, 24, 72, 128)
# every axis length at which the kernels pick another tile width (32 | 33, 64 | 65, 128 | 129, 256 | 257) and the largest, 512
TILE_EDGES = [(1, 2, 33, 65, 129), (1, 1, 32, 64, 128), (1, 1, 257, 3, 2), (1, 1, 3, 2, 257), (1, 1, 2, 256, 3),
              (1, 1, 512, 2, 3), (1, 1, 2, 512, 1), (1, 2, 1, 3, 512)]


def _inputs(vol, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(vol, generator=g).half(), torch.randn(vol, generator=g)


def _check_parity(got16, want64, what):
    ulps, share = R.compare_fp16(got16, want64)
    n = got16.numel()
    allowed = math.ceil(SHARE_BOUND * n)
    print(f"{what}: largest difference {ulps:.2f} fp16 ulp, {round(share * n)} of {n} elements differ (share {share:.2e}; "
          f"allowed {allowed})")
    assert ulps <= 1.0
    assert round(share * n) <= allowed


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("vol", SMALL, ids=lambda v: "x".join(map(str, v)))
def test_mix_matches_the_restatement(gpu, vol, method):
    from vdx.freeinit import freq_mix, lowpass_filter
    z, eta = _inputs(vol)
    filt = lowpass_filter(vol[2:], method, 0.5, 0.5)
    got = freq_mix(z.to(gpu), eta.to(gpu), filt)
    assert got.dtype == torch.float16 and got.shape == z.shape and got.device.type == "cuda"
    _check_parity(got.cpu(), R.mix(z, eta, filt), f"{vol} {method}")


@pytest.mark.parametrize("vol", [HEADLINE] + TILE_EDGES, ids=lambda v: "x".join(map(str, v)))
def test_mix_matches_the_restatement_at_the_headline_and_at_every_tile_width(gpu, vol):
    from vdx.freeinit import freq_mix, lowpass_filter
    z, eta = _inputs(vol)
    filt = lowpass_filter(vol[2:], "butterworth", 0.5, 0.5)
    got = freq_mix(z.to(gpu), eta.to(gpu), filt)
    _check_parity(got.cpu(), R.mix(z, eta, filt), f"{vol} butterworth")


def test_zero_filter_returns_the_fresh_noise_and_ones_filter_the_latent(gpu):
    from vdx.freeinit import freq_mix
    for vol in SMALL + [(1, 2, 24, 40, 72)]:                               # the 576-wide job's extent among them
        z, eta = _inputs(vol, seed=3)
        got = freq_mix(z.to(gpu), eta.to(gpu), torch.zeros(vol[2:]))
        assert torch.equal(got.cpu(), eta.half())
        got = freq_mix(z.to(gpu), eta.to(gpu), torch.ones(vol[2:])).cpu()
        ulps, _ = R.compare_fp16(got, z.double())
        assert ulps <= 1.0


def test_same_bits_on_every_run_and_for_every_batch(gpu):
    from vdx.freeinit import freq_mix, lowpass_filter
    vol = (2, 3, 5, 6, 10)                                                 # 30 rows per volume: the w tiles straddle volumes
    z, eta = _inputs(vol, seed=5)
    zg, eg, filt = z.to(gpu), eta.to(gpu), lowpass_filter(vol[2:], "gaussian", 0.5, 0.5)
    full = freq_mix(zg, eg, filt)
    assert torch.equal(full, freq_mix(zg, eg, filt))
    for b in range(vol[0]):
        for c in range(vol[1]):
            alone = freq_mix(zg[b:b + 1, c:c + 1].contiguous(), eg[b:b + 1, c:c + 1].contiguous(), filt)
            assert torch.equal(alone[0, 0], full[b, c]), (b, c)
    assert torch.equal(freq_mix(zg[1:], eg[1:], filt), full[1:])


def test_nan_and_inf_run_clean_and_stay_in_their_volume(gpu):
    from vdx.freeinit import freq_mix, lowpass_filter
    vol = (1, 4, 3, 7, 9)
    z, eta = _inputs(vol, seed=9)
    filt = lowpass_filter(vol[2:], "butterworth", 0.5, 0.5)
    clean = freq_mix(z.to(gpu), eta.to(gpu), filt)
    z[0, 0, 1, 2, 3] = float("nan")
    z[0, 1, 0, 0, 0] = float("inf")
    eta[0, 2, 2, 6, 8] = float("-inf")
    got = freq_mix(z.to(gpu), eta.to(gpu), filt)
    torch.cuda.synchronize()
    for c in range(3):
        assert not torch.isfinite(got[0, c]).any()                         # a 3-D transform spreads it over the whole volume
    assert torch.equal(got[0, 3], clean[0, 3])                             # and over no other


def test_sizes_outside_the_kernels_are_refused(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    from vdx.freeinit import freq_mix
    for vol in ((1, 1, 513, 1, 1), (1, 1, 1, 1, 600)):
        with pytest.raises(VdxError):
            freq_mix(torch.zeros(vol, dtype=torch.float16, device=gpu), torch.zeros(vol, device=gpu), torch.zeros(vol[2:]))
    z, eta = torch.zeros((1, 1, 2, 3, 4), dtype=torch.float16, device=gpu), torch.zeros((1, 1, 2, 3, 4), device=gpu)
    for bad in (lambda: freq_mix(z, eta, torch.zeros(2, 3, 5)), lambda: freq_mix(z, eta.half(), torch.zeros(2, 3, 4)),
                lambda: freq_mix(z.float(), eta, torch.zeros(2, 3, 4)), lambda: freq_mix(z, eta[:, :, :1], torch.zeros(2, 3, 4)),
                lambda: ops.freeinit_mix(z.cpu(), eta.cpu(), torch.zeros(2, 3, 4))):
        with pytest.raises(VdxError):
            bad()
    lib = ops._lib.load()
    assert lib.vdx_freeinit_workspace(1, 513, 1, 1) == 0 and lib.vdx_freeinit_workspace(4, 24, 72, 128) == 4 * 24 * 72 * 128 * 16
    assert lib.vdx_freeinit_mix_f16(z.data_ptr(), eta.data_ptr(), eta.data_ptr(), eta.data_ptr(), eta.data_ptr(), eta.data_ptr(),
                                    1, 513, 1, 1, eta.data_ptr(), 1 << 20, z.data_ptr(), None) != 0


# ---- the job ------------------------------------------------------------------------------------------------------------------
T, HL, WL, STEPS = 10, 32, 32, 3                                           # tests/test_e2e_gpu.py's shapes


def _config(**kw):
    from vdx.pipeline import DiffuserConfig
    return DiffuserConfig(num_frames=T, steps=STEPS, chunk_size=6, overlap=2, height=HL * 8, width=WL * 8, mode="hybrid_ctx",
                          device="cuda", noise_device="cpu", **kw)


@pytest.fixture(scope="module")
def model(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vdx  # noqa: F401
    from dist_pipeline_worker import build
    return build(gpu, 0, 1)


@pytest.fixture(scope="module")
def one_pass(model):
    """The job without the option: (blended latent, info, context), computed once."""
    from vdx.pipeline import DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    d = DistributedVideoDiffuser(_config(), m, DDIMScheduler(), emb[1:], emb[:1])
    lat, info = d()
    return lat, info, d.ctx.clone()


def test_one_iteration_is_the_job_without_the_option(model, one_pass):
    from vdx.pipeline import DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    d = DistributedVideoDiffuser(_config(free_init_iters=1, free_init_method="gaussian"), m, DDIMScheduler(), emb[1:], emb[:1])
    lat, info = d()
    assert torch.equal(lat, one_pass[0])
    assert "free_init" not in info and set(info) == set(one_pass[1]) and d.free_init_starts == []


def test_two_iterations(gpu, model, one_pass):
    from vdx.freeinit import lowpass_filter
    from vdx.pipeline import DistributedVideoDiffuser, iteration_noise, seeded_noise
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    d = DistributedVideoDiffuser(_config(free_init_iters=2), m, DDIMScheduler(), emb[1:], emb[:1])
    lat, info = d()
    lat1, info1, ctx1 = one_pass
    # the second iteration's start latent: the restatement applied to the first iteration's blend
    assert len(d.free_init_starts) == 1
    start = d.free_init_starts[0]
    assert start.dtype == torch.float16 and start.shape == lat1.shape
    base = seeded_noise(tuple(lat1.shape), 1.0, "cuda", "cpu")
    z_T = d.scheduler.add_noise(lat1.half().contiguous(), base, 999)       # the existing kernel and its fp16 bits
    eta = iteration_noise(tuple(lat1.shape), 1, "cuda", "cpu")
    filt = lowpass_filter((T, HL, WL))                                     # the defaults: butterworth, 0.25, 0.25, order 4
    _check_parity(start.cpu(), R.mix(z_T.cpu(), eta.cpu(), filt), "start latent of iteration 1")
    # the result is another one, the record is filled, the sums cover both passes
    assert lat.shape == lat1.shape and lat.dtype == lat1.dtype and torch.isfinite(lat).all() and not torch.equal(lat, lat1)
    rec = info["free_init"]
    assert (rec["iters"], rec["method"], rec["d_s"], rec["d_t"], rec["order"]) == (2, "butterworth", 0.25, 0.25, 4)
    assert len(rec["denoise_s"]) == 2 and len(rec["reinit_s"]) == 1 and all(v > 0 for v in rec["denoise_s"] + rec["reinit_s"])
    assert info["denoise_s"] == sum(rec["denoise_s"]) and set(info) == set(info1) | {"free_init"}
    assert info["ranges"] == info1["ranges"] and info["payload_bytes"] == 2 * info1["payload_bytes"]
    # the context is iteration 0's again, so a second call is the same job: the same bits
    assert torch.equal(d.ctx, ctx1)
    lat_again, _ = d()
    assert torch.equal(lat_again, lat) and torch.equal(d.free_init_starts[0], start)


def test_halo_is_refused_by_the_call(model):
    from vdx.pipeline import DistributedVideoDiffuser
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    d = DistributedVideoDiffuser(_config(free_init_iters=2), m, DDIMScheduler(), emb[1:], emb[:1])
    with pytest.raises(ValueError, match="allgather"):
        d(exchange="halo")


def test_dpm_solver_runs_with_free_init(model):
    from vdx.pipeline import DistributedVideoDiffuser, make_scheduler
    from vdx.scheduler import DDIMScheduler
    m, emb = model
    lats = []
    for k in (1, 2):
        d = DistributedVideoDiffuser(_config(free_init_iters=k, scheduler="dpmpp_2m"), m, make_scheduler("dpmpp_2m", DDIMScheduler()),
                                     emb[1:], emb[:1])
        lat, info = d()
        assert torch.isfinite(lat).all() and ("free_init" in info) == (k == 2)
        lats.append(lat)
    assert not torch.equal(lats[0], lats[1])


def test_two_ranks_end_with_identical_bits(gpu, tmp_path):
    """Two processes, one rank each, both on this box's one GPU and talking over gloo (tests/test_dist_gpu.py's arrangement):
    every rank re-initialises the whole clip's start latent for itself; the worker compares the ranks' results over gloo."""
    out = tmp_path / "rank0.pt"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29733",
                        os.path.join(ROOT, "tests", "dist_freeinit_worker.py"), str(out), str(T), "6", "2", "2"],
                       capture_output=True, text=True, timeout=900, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2
    got = torch.load(out, weights_only=True)
    assert got["free_init"]["iters"] == 2 and len(got["starts"]) == 1 and torch.isfinite(got["lat"]).all()
