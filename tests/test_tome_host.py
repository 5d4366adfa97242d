"""-m "not gpu": token merging's host side: the partition tables against `tomesd`'s own construction restated literally
(tests/tome_ref.py), the refusals, the job's fields, flags and records, and the C-ABI rows of the new entry points."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tome_ref as R  # noqa: E402

import vdx  # noqa: E402,F401
from vdx import _lib  # noqa: E402
from vdx.tome import check_params, partition  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(2, 2), (5, 7), (8, 16), (9, 9), (18, 32), (72, 128)]
STRIDES = [(2, 2), (1, 2), (3, 2)]


@pytest.mark.parametrize("sx,sy", STRIDES)
@pytest.mark.parametrize("hh,ww", GRIDS)
def test_partition_is_tomesds(hh, ww, sx, sy):
    a_idx, b_idx = R.tomesd_partition(hh, ww, sx, sy)
    for ratio in (0.25, 0.5, 0.75):
        part = partition(hh, ww, ratio, sx, sy)
        assert part.src_idx.dtype == torch.int32 and part.dst_idx.dtype == torch.int32
        assert torch.equal(part.src_idx.long(), a_idx.sort().values) and torch.equal(part.dst_idx.long(), b_idx.sort().values)
        assert part.n_dst == (hh // sy) * (ww // sx) and part.n_src == hh * ww - part.n_dst
        assert part.r == min(a_idx.numel(), int(hh * ww * ratio))               # tomesd: r = min(a.shape[1], int(N ratio))


@pytest.mark.parametrize("sx,sy", STRIDES)
@pytest.mark.parametrize("hh,ww", GRIDS)
def test_seeded_offsets(hh, ww, sx, sy):
    one, two, other = partition(hh, ww, 0.5, sx, sy, seed=5), partition(hh, ww, 0.5, sx, sy, seed=5), partition(hh, ww, 0.5, sx, sy, seed=6)
    assert torch.equal(one.dst_idx, two.dst_idx) and torch.equal(one.src_idx, two.src_idx)
    assert tuple(one.offsets.shape) == (hh // sy, ww // sx)
    if one.n_dst == 0:                                                          # a grid without cells: nothing to draw
        assert one.n_src == hh * ww and one.r == int(hh * ww * 0.5)
        return
    assert int(one.offsets.min()) >= 0 and int(one.offsets.max()) < sx * sy
    a_idx, b_idx = R.tomesd_partition(hh, ww, sx, sy, rand_idx=one.offsets[..., None])
    assert torch.equal(one.src_idx.long(), a_idx.sort().values) and torch.equal(one.dst_idx.long(), b_idx.sort().values)
    y, x = one.dst_idx.long() // ww, one.dst_idx.long() % ww                     # one destination inside every cell
    cells = (y // sy) * (ww // sx) + x // sx
    assert bool((y < hh // sy * sy).all()) and bool((x < ww // sx * sx).all()) and torch.equal(cells.sort().values, torch.arange(one.n_dst))
    if hh * ww >= 81:
        assert not torch.equal(one.dst_idx, other.dst_idx)


def test_against_tomesd_if_installed():
    """`tomesd`'s own matching, where it is importable (it is not expected to be: then the definition stays the restatement
    above and this test skips).  With one merge (r = 1) and the identity as the merged tensor, every row of its output names
    the tokens it holds: a row among the first N - n_dst - 1 is an unmerged source, the last n_dst rows are the destinations,
    one of them with the merged source added."""
    try:
        from tomesd.merge import bipartite_soft_matching_random2d
    except ImportError as e:
        pytest.skip(f"tomesd is not installed ({e}): the partition is pinned to its construction restated in tests/tome_ref.py")
    for hh, ww, sx, sy in [(8, 16, 2, 2), (9, 9, 2, 2), (5, 7, 1, 2), (18, 32, 3, 2)]:
        N = hh * ww
        part = partition(hh, ww, 0.5, sx, sy)
        src, dst = set(part.src_idx.tolist()), set(part.dst_idx.tolist())
        metric = torch.randn(1, N, 16, generator=torch.Generator().manual_seed(N))
        merge, _ = bipartite_soft_matching_random2d(metric, ww, hh, sx, sy, 1, no_rand=True)
        rows = merge(torch.eye(N).unsqueeze(0), mode="sum")[0]
        assert rows.shape == (N - 1, N)
        unm = rows[:N - part.n_dst - 1].nonzero()[:, 1].tolist()
        held = rows[N - part.n_dst - 1:].nonzero()[:, 1].tolist()
        assert len(unm) == part.n_src - 1 and set(unm) <= src
        assert len(held) == part.n_dst + 1 and dst <= set(held) and len(set(held) - dst) == 1 and set(held) - dst <= src
        assert set(unm) | set(held) == set(range(N))


@pytest.mark.parametrize("kw", [dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=0.0), dict(ratio=-0.1), dict(ratio=0.76),
                                dict(ratio=0.5, sx=1, sy=1), dict(ratio=0.5, sx=0), dict(ratio=0.5, sy=-1), dict(ratio=0.6, sx=1, sy=2),
                                dict(ratio=0.5, max_downsample=3), dict(ratio=0.5, max_downsample=16), dict(ratio="0.5"),
                                dict(ratio=True)], ids=str)
def test_enable_tome_refusals_leave_the_state(kw):
    from vdx.unet3d import UNet3DConditionModel, UNet3DConfig
    m = UNet3DConditionModel(UNet3DConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128, transformer_in_heads=2))
    assert m.tome is None
    with pytest.raises(ValueError):
        m.enable_tome(**kw)
    assert m.tome is None
    m.enable_tome(0.75, seed=2)
    with pytest.raises(ValueError):
        m.enable_tome(**kw)
    assert m.tome == {"ratio": 0.75, "sx": 2, "sy": 2, "seed": 2, "max_downsample": 1}
    assert m.enable_tome(0.5, sx=1, sy=2).tome["ratio"] == 0.5                   # the upper end of (0, 1 - 1 / (sx sy)]
    assert m.disable_tome().tome is None


def test_config_fields_flags_and_check():
    from vdx.pipeline import DiffuserConfig, build_arg_parser, check_tome, config_from_args
    cfg = DiffuserConfig()
    assert cfg.tome is None and cfg.tome_seed is None and check_tome(cfg) is None
    p = build_arg_parser()
    a = p.parse_args([])
    assert a.tome is None and a.tome_seed is None
    cfg = config_from_args(p.parse_args(["--tome", "0.5", "--tome_seed", "7"]))
    assert cfg.tome == 0.5 and isinstance(cfg.tome, float) and cfg.tome_seed == 7 and isinstance(cfg.tome_seed, int)
    assert check_tome(cfg) == {"ratio": 0.5, "sx": 2, "sy": 2, "seed": 7, "max_downsample": 1}
    assert check_params(0.25) == {"ratio": 0.25, "sx": 2, "sy": 2, "seed": None, "max_downsample": 1}
    for bad in (dict(tome=0.8), dict(tome=0.0), dict(tome=float("nan")), dict(tome_seed=3)):
        with pytest.raises(ValueError):
            check_tome(DiffuserConfig(**bad))
    with pytest.raises(SystemExit):
        p.parse_args(["--tome", "half"])
    with pytest.raises(SystemExit):
        p.parse_args(["--tome", "0.5", "--tome_seed", "1.5"])


def test_run_job_refuses_a_bad_ratio_before_any_work():
    from vdx.pipeline import DiffuserConfig, run_job
    with pytest.raises(ValueError, match="tome"):
        run_job(DiffuserConfig(model_id="synthetic:tiny", tome=0.9))


def test_run_job_refuses_a_grid_the_select_cannot_hold():
    """The select kernel keeps an image's keys in LDS; the job knows its frame and refuses before anything is loaded."""
    from vdx.pipeline import DiffuserConfig, run_job
    from vdx.tome import SELECT_LDS_MAX, check_grid, select_lds
    lib = _lib.load()
    for n_src, n_dst in [(6912, 2304), (1, 1), (3, 1), (12288, 4096), (8193, 100), (0, 1), (5, 0)]:
        assert select_lds(n_src, n_dst) == lib.vdx_tome_select_lds(n_src, n_dst)
    p = check_params(0.5)
    check_grid(72, 128, p)                                                     # the headline frame
    check_grid(128, 128, p)                                                    # 12288 sources: the last power of two that fits
    assert select_lds(12288, 4096) <= SELECT_LDS_MAX < select_lds(19200, 6400)
    with pytest.raises(ValueError, match="select"):
        check_grid(160, 160, p)
    with pytest.raises(ValueError, match="select"):
        run_job(DiffuserConfig(model_id="synthetic:tiny", tome=0.5, height=1280, width=1280))


def test_shim_pipeline_has_the_switch():
    from vdx.compat.diffusers_shim import DiffusionPipeline

    class U:
        def enable_tome(self, **kw):
            self.kw = kw

        def disable_tome(self):
            self.kw = None
    pipe = DiffusionPipeline.__new__(DiffusionPipeline)
    pipe.unet = U()
    pipe.enable_tome(0.25, seed=1)
    assert pipe.unet.kw == dict(ratio=0.25, sx=2, sy=2, seed=1, max_downsample=1)
    pipe.disable_tome()
    assert pipe.unet.kw is None


def test_abi_rows_and_struct_layout(tmp_path):
    names = {"vdx_tome_match_f16", "vdx_tome_select_lds", "vdx_tome_select", "vdx_tome_merge_f16", "vdx_tome_unmerge_add_f16"}
    assert names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.vdx_tome_select_lds(6912, 2304) == 8192 * 8 + 2304 * 4 + 6912 and lib.vdx_tome_select_lds(0, 1) == 0
    a = _lib.TomeArgs()
    assert lib.vdx_tome_select(ctypes.byref(a), None) != 0 and b"tome_select" in lib.vdx_last_error()      # refused in the library too
    a.n_img, a.S, a.n_src, a.n_dst, a.r = 1, 4, 3, 1, 4
    assert lib.vdx_tome_select(ctypes.byref(a), None) != 0 and b"r=4" in lib.vdx_last_error()
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("gcc") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.skip("no C compiler here")
    lines = ['    printf("sizeof %zu\\n", sizeof(vdx_tome_args));']
    lines += [f'    printf("{f} %zu\\n", offsetof(vdx_tome_args, {f}));' for f, _ in _lib.TomeArgs._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vdx.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True, timeout=120)
    got = dict((k, int(v)) for k, v in (ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()))
    want = {"sizeof": ctypes.sizeof(_lib.TomeArgs), **{f: getattr(_lib.TomeArgs, f).offset for f, _ in _lib.TomeArgs._fields_}}
    assert got == want


def test_reference_select_orders_as_stated():
    """The restatement's own order: descending value, ties to the lower i, -0 = +0, NaN below -inf."""
    v = torch.tensor([0.5, float("nan"), 0.5, -0.0, 0.0, float("-inf"), float("inf"), float("nan")])
    key = R.orderable(v)
    order = sorted(range(8), key=lambda i: (-int(key[i]), i))
    assert order == [6, 0, 2, 3, 4, 5, 1, 7]
