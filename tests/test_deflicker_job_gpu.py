"""GPU: `--deflicker` through the job (vdx/pipeline.py `run_job`): the file holds the filtered, then interpolated, frames; the
numbers and the scored frames stay the generated ones'."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = ["--model_id", "synthetic:tiny", "--num_frames", "8", "--steps", "2", "--height", "128", "--width", "256",
        "--chunk_size", "6", "--overlap", "2", "--mode", "chunk", "--noise_device", "cpu"]
PARAMS = {"strength": 0.5, "sigma": 10.0, "passes": 1}


def test_run_job_filters_what_it_writes_and_nothing_else(gpu, tmp_path):
    from vdx import deflicker, interp, video
    from vdx.compat.diffusers_shim import DiffusionPipeline
    from vdx.pipeline import DiffuserConfig, build_arg_parser, config_from_args, run_job
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16)
    res, files, taken = {}, {}, {}
    for name, extra, kw in (("none", [], {}), ("on", ["--deflicker", "0.5"], {}), ("on_gpu", ["--deflicker", "0.5"], {"gpu_video_write": True}),
                            ("two", ["--deflicker", "0.5", "--deflicker_sigma", "10", "--interpolate", "2"], {})):
        mp4, got = tmp_path / f"{name}.mp4", {}
        cfg = config_from_args(build_arg_parser().parse_args(BASE + extra))
        assert cfg.deflicker == ((0.5, 10.0) if extra else None) and cfg.deflicker_passes == 1
        res[name] = run_job(cfg, out_video=str(mp4), pipe=pipe, clip_inputs=got, **kw)
        files[name], taken[name] = mp4.read_bytes(), np.stack(got["frames"])
    assert "deflicker" not in res["none"] and set(res["on"]) == set(res["none"]) | {"deflicker"}
    for name in ("on", "on_gpu", "two"):                                # the record; the numbers and the scored frames are the generated ones'
        assert res[name]["deflicker"] == PARAMS
        assert np.array_equal(taken[name], taken["none"])
        assert all(res[name][k] == res["none"][k] for k in ("temp_instab", "flow_err", "num_frames"))
    assert (res["on"]["frames_written"], res["two"]["frames_written"]) == (8, 15)
    assert files["on_gpu"] == files["on"] != files["none"]              # host writer and GPU writer alike
    # the files hold the encoder's rendering of exactly filter_frames(generated), and of its interpolation
    filtered = deflicker.filter_frames(taken["none"], 0.5, 10.0, device=gpu)
    for name, clip, fps in (("on", filtered, 8), ("two", interp.interpolate_frames(filtered, 2), 16)):
        want = tmp_path / f"want_{name}.mp4"
        video.write_frames(want, clip, fps)
        assert want.read_bytes() == files[name]
    # the config's own form, two passes
    got = run_job(DiffuserConfig(**{**vars(cfg), "interpolate": 1, "deflicker": (1.0, 4.0), "deflicker_passes": 2}), out_video=None, pipe=pipe)
    assert got["deflicker"] == {"strength": 1.0, "sigma": 4.0, "passes": 2} and got["frames_written"] is None
