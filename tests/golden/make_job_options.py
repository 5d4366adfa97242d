"""Records tests/golden/job_options_parent.json: for a fixed list of configs, what the job's two entry points do with them --
`run_job(cfg, exchange, out_video=None)` and `DistributedVideoDiffuser(cfg, ...)(exchange)` -- as `[exception type, message]` or,
for an accepted config, "accepted" (`run_job`: it got as far as loading the models) / {"info": its sorted keys} (the call).
Nothing here needs a device: the models' loader, the windows' denoising, the co-denoised round, the blend's two kernels and
FreeInit's re-initialisation are stubbed.

The fixture pins the refusals, their texts and their ORDER (a config that breaks two rules raises the message of the first),
so it is recorded from the commit BEFORE a change to the checks, never from the code under test:

    git worktree add DIR <parent commit>  &&  cp tests/golden/make_job_options.py DIR/tests/golden/
    python DIR/tests/golden/make_job_options.py tests/golden/job_options_parent.json

tests/test_options_host.py imports the runner (`no_device`, `outcomes`, `plan_builds`) from here and replays the recorded configs.
"""
import contextlib
import itertools
import json
import os
import sys
from types import SimpleNamespace
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]

BASE = dict(num_frames=8, steps=2, height=64, width=64, device="cpu", noise_device="cpu", chunk_size=6, overlap=2, mode="chunk")
EXCHANGES = ("allgather", "halo")
ON = {"co_denoise": dict(co_denoise=True), "tile": dict(tile=[64, 64]), "loop": dict(loop=True),
      "context_stride": dict(context_stride=2), "guidance_rescale": dict(guidance_rescale=0.5),
      "free_init": dict(free_init_iters=2), "mask": dict(keep_frames="0:2"), "init_video": dict(init_video="clip.npy"),
      "freeu": dict(freeu=[1.2, 1.4, 0.9, 0.2]), "tome": dict(tome=0.5)}
CO = ON["co_denoise"]
# two rules broken at once (some three): which message comes out is the order of the checks
TWO_RULES = [
    (dict(CO, tile=[64, 64], loop=True), "halo"), (dict(CO, loop=True, context_stride=2, guidance_rescale=0.5), "allgather"),
    (dict(tile=[64, 64]), "halo"), (dict(loop=True), "halo"), (dict(context_stride=2, tile=[64, 64]), "allgather"),
    (dict(context_stride=0), "halo"), (dict(CO, free_init_iters=2), "halo"), (dict(free_init_iters=0, loop=True), "allgather"),
    (dict(freeu=[0.0, 1.4, 0.9, 0.2], tome=0.9), "allgather"), (dict(tome_seed=3, tile=[64, 64]), "allgather"),
    (dict(interpolate=0, free_init_iters=0), "allgather"), (dict(keep_frames="0:2"), "halo"),
    (dict(keep_frames="0:2", init_video="clip.npy", free_init_iters=2), "allgather"),
    (dict(CO, tile=[64, 64], guidance_rescale=1.5), "allgather"),
    (dict(CO, loop=True, guidance_rescale=0.5, guidance_scale=1.0), "allgather"),
    (dict(negative_prompt=None, guidance_rescale=2.0), "allgather"), (dict(CO, tile=[60, 64], guidance_rescale=0.5), "allgather"),
    (dict(tile_overlap=[8, 8], loop=True), "allgather"), (dict(CO, loop=True, chunk_size=8, context_stride=2), "allgather"),
    (dict(CO, context_stride=4, guidance_rescale=0.5), "allgather"), (dict(CO, tile=[64, 64]), "halo"),
    (dict(free_init_iters=0), "ring"), (dict(CO), "ring"), (dict(tome=0.9, freeu=[1.0, 1.0]), "allgather"),
    (dict(mask_rule="bilinear", guidance_rescale=2.0), "allgather"), (dict(CO, tome=0.5, tile=[56, 64]), "allgather"),
    (dict(CO, tile=[64, 64], tile_overlap=[64, 0], loop=True), "allgather"),
    (dict(keep_frames="0:2", mask="m.npy", init_video="clip.npy"), "halo"),
    (dict(CO, context_stride=2, loop=True, tile=[64, 64]), "halo"), (dict(free_init_iters=2, free_init_method="box"), "halo"),
    (dict(interpolate=0, co_denoise=True), "halo"), (dict(CO, loop=True, mode="fsdp", guidance_rescale=0.5), "allgather"),
]


def _host_test_refusals():
    """Every entry of the refusal lists of the four co-denoising host tests, on those tests' own base configs."""
    import test_coloop_host
    import test_costride_host
    import test_cotile_host
    small = dict(num_frames=8, steps=2, chunk_size=6, overlap=2, height=64, width=64, mode="chunk", device="cpu")
    out = [({**small, "co_denoise": True}, "halo")]                                    # tests/test_codenoise_host.py
    for kw, exchange, _ in test_coloop_host.REFUSALS:
        if "world" not in kw:                                                          # the entry points take the group's size
            out.append(({**small, "co_denoise": True, "loop": True, **kw}, exchange))
    for kw, exchange, _ in test_costride_host.REFUSALS:
        out.append(({**small, "co_denoise": True, "context_stride": 2, **kw}, exchange))
    mark = next(m for m in test_cotile_host.test_check_tile_refusals.pytestmark if m.name == "parametrize")
    for kw, exchange, _ in mark.args[1]:
        out.append(({**dict(height=128, width=192, co_denoise=True, tile=(64, 128), device="cpu", num_frames=8, steps=2), **kw}, exchange))
    return out


def configs():
    """[(DiffuserConfig keyword arguments on top of its defaults, exchange)], as JSON holds them (tuples are lists)."""
    out = [(dict(BASE), x) for x in EXCHANGES]                                          # every option off
    out += [({**BASE, **kw}, x) for kw in ON.values() for x in EXCHANGES]                # every option alone
    for a, b in itertools.combinations(ON, 2):                                          # every pair, and with co_denoise beside it
        for x in EXCHANGES:
            out.append(({**BASE, **ON[a], **ON[b]}, x))
            if "co_denoise" not in (a, b):
                out.append(({**BASE, **CO, **ON[a], **ON[b]}, x))
    out += _host_test_refusals()
    out += [({**BASE, **kw}, x) for kw, x in TWO_RULES]
    return json.loads(json.dumps(out))


class Loaded(Exception):
    """`run_job` got past its checks and asked for the models."""


class _Unet:
    config = SimpleNamespace(in_channels=4)
    freeu = tome = None

    def enable_freeu(self, **kw): pass
    def disable_freeu(self): pass
    def enable_tome(self, **kw): pass
    def disable_tome(self): pass


def _co_round(d, start, cp, *a, **k):
    spent = {"denoise_s": 0.0, "emu_gather_delay_s": 0.0, "net_gather_s": 0.0, "network_bytes": 0, "payload_bytes": 0,
             "payload_bytes_actual": 0}
    return start.float(), spent, {"windows": 1, "steps": 2, "exchange_s": 0.0, "bytes_per_step": 0, "tile": {},
                                  "loop": {"windows": []}, "context_stride": {}}


def _blend_accumulate(full, weight, lat, w, s, e):
    full[:, :, s:e] += lat.float() * w.view(1, 1, -1, 1, 1)
    weight[s:e] += w


@contextlib.contextmanager
def no_device():
    """The stubs: everything a job would run on the GPU, and the models' loader."""
    import vdx  # noqa: F401
    from vdx import codenoise, freeinit, ops, pipeline
    from vdx.compat.diffusers_shim import DiffusionPipeline

    def loaded(*a, **k):
        raise Loaded()

    with contextlib.ExitStack() as st:
        for obj, name, new in ((DiffusionPipeline, "from_pretrained", loaded),
                               (pipeline.DistributedVideoDiffuser, "denoise", lambda self, lat, s=None: lat),
                               (pipeline, "co_denoise_round", _co_round), (codenoise, "co_denoise_round", _co_round),
                               (ops, "blend_accumulate", _blend_accumulate),
                               (ops, "blend_finalize", lambda full, weight: full / weight.view(1, 1, -1, 1, 1).clamp(min=1e-6)),
                               (freeinit, "reinit", lambda z0, base, *a, **k: z0.half())):
            st.enter_context(mock.patch.object(obj, name, new))
        st.enter_context(mock.patch.dict(os.environ))
        os.environ.pop("WORLD_SIZE", None)
        yield


def _outcome(fn):
    try:
        return fn()
    except Loaded:
        return "accepted"
    except Exception as err:                    # a refusal: its type and its text
        return [type(err).__name__, str(err)]


def outcomes(kw, exchange):
    """(what `run_job` does with the config, what constructing and calling the diffuser does); inside `no_device()`."""
    from vdx.pipeline import DiffuserConfig, DistributedVideoDiffuser, run_job
    from vdx.scheduler import DDIMScheduler
    job = _outcome(lambda: run_job(DiffuserConfig(**kw), exchange, out_video=None))
    call = _outcome(lambda: {"info": sorted(DistributedVideoDiffuser(DiffuserConfig(**kw), _Unet(), DDIMScheduler(), None, None)(exchange)[1])})
    return job, call


def plan_builds(kw, exchange, run):
    """How often `run()` builds a ring plan or a strided plan (`codenoise.loop_plan`, `codenoise.stride_plan`); inside
    `no_device()`."""
    from vdx import codenoise
    n = {"loop_plan": 0, "stride_plan": 0}

    def counted(name, real):
        def f(*a, **k):
            n[name] += 1
            return real(*a, **k)
        return f

    with mock.patch.object(codenoise, "loop_plan", counted("loop_plan", codenoise.loop_plan)), \
            mock.patch.object(codenoise, "stride_plan", counted("stride_plan", codenoise.stride_plan)):
        run()
    return n


PLAN_JOBS = {"loop": ({**BASE, **CO, "loop": True}, "allgather"), "context_stride": ({**BASE, **CO, "context_stride": 2}, "allgather")}


def _job_as_recorded(kw, exchange):
    """A job on the recorded commit: `run_job`'s checks (up to the models' loader), then the diffuser's call."""
    def run():
        assert outcomes(kw, exchange)[0] == "accepted"
    return run


def main(path):
    with no_device():
        entries = []
        for kw, exchange in configs():
            job, call = outcomes(kw, exchange)
            entries.append({"cfg": kw, "exchange": exchange, "run_job": job, "call": call})
        builds = {name: plan_builds(kw, x, _job_as_recorded(kw, x)) for name, (kw, x) in PLAN_JOBS.items()}
    with open(path, "w") as f:
        json.dump({"entries": entries, "plan_builds": builds}, f, indent=0, sort_keys=True)
        f.write("\n")
    refused = sum(isinstance(e["run_job"], list) for e in entries), sum(isinstance(e["call"], list) for e in entries)
    print(f"{len(entries)} configs; refused by run_job {refused[0]}, by the call {refused[1]}; plan builds {builds} -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
