"""-m gpu: `ops.lora_merge` (csrc/lora.hip) bit for bit against tests/lora_ref.py, the expression restated in torch fp32 on the
CPU: every access width (scalar, 8-byte, 16-byte), tail tiles on both axes, more than one tile on both axes, ranks at, below and
above the LDS chunk, several adapters of different ranks, the largest rank; in place, run to run, a canary behind `out`, special
values in W, a zero `down` column, the wrapper's refusals; and `lora.merge_state_dict` above it."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lora_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = 32      # csrc/lora.hip LM_RC: the ranks staged through LDS at a time


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _case(n_out, n_in, ranks, seed, scales=None):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(n_out, n_in, generator=g) / max(n_in, 1) ** 0.5).half()
    ads = []
    for a, R in enumerate(ranks):
        up = torch.randn(n_out, R, generator=g)
        down = torch.randn(R, n_in, generator=g) / (R * max(n_in, 1)) ** 0.5
        s = scales[a] if scales is not None else 0.75
        ads.append((up, down, s))
    return W, ads


def _run(gpu, W, ads, **kw):
    from vdx import ops
    return ops.lora_merge(W.to(gpu), [(u.to(gpu), d.to(gpu), s) for u, d, s in ads], **kw)


SHAPES = [
    ("1x1 R1", 1, 1, (1,), None),
    ("65x67 R3 scalar, tails on both axes", 65, 67, (3,), None),
    ("70x68 R5 8-byte", 70, 68, (5,), None),
    ("130x72 R33 16-byte, rank crosses the chunk", 130, 72, (33,), None),
    ("130x72 R chunk", 130, 72, (CHUNK,), None),
    ("130x72 R chunk-1", 130, 72, (CHUNK - 1,), None),
    ("130x72 R chunk+1", 130, 72, (CHUNK + 1,), None),
    ("64x576 R4 conv flatten", 64, 576, (4,), None),
    ("320x1024 R16", 320, 1024, (16,), None),
    ("33x520 R2 three column tiles, the last 8 wide", 33, 520, (2,), None),
    ("128x128 two adapters R4 R8", 128, 128, (4, 8), (0.5, -1.25)),
    ("eight adapters R1", 40, 264, (1,) * 8, (1.0, 0.5, -0.25, 2.0, 0.125, -1.0, 0.3, 0.7)),
    ("16x16 R512", 16, 16, (512,), None),
]


@pytest.mark.parametrize("name,n_out,n_in,ranks,scales", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_matches_the_restatement_bit_for_bit(gpu, name, n_out, n_in, ranks, scales):
    W, ads = _case(n_out, n_in, ranks, seed=n_out * 1000 + n_in + sum(ranks), scales=scales)
    want = L.merge(W, ads)
    got = _run(gpu, W, ads)
    assert got.dtype == torch.float16 and tuple(got.shape) == (n_out, n_in)
    assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(got), _bits(W))            # the adapters moved the weight


def test_conv_weight_flattened_is_the_conv_adapter(gpu):
    """(co, ci, 3, 3) with down (R, ci, 3, 3) and up (co, R, 1, 1): the flattened merge is the conv adapter's
    `W + s * einsum(up, down)` within the derived fp32 bound, element by element in W's own layout."""
    g = torch.Generator().manual_seed(3)
    co, ci, R, s = 64, 64, 4, 0.5
    W = (torch.randn(co, ci, 3, 3, generator=g) / 24).half()
    down, up = torch.randn(R, ci, 3, 3, generator=g) / 24, torch.randn(co, R, 1, 1, generator=g)
    got = _run(gpu, W.reshape(co, -1), [(up.reshape(co, R), down.reshape(R, -1), s)]).cpu().reshape(W.shape)
    assert torch.equal(_bits(got), _bits(L.merge_nd(W, [(up.reshape(co, R), down.reshape(R, -1), s)])))
    exact = W.double() + s * torch.einsum("or,rikl->oikl", up.reshape(co, R).double(), down.double())
    assert float((got.double() - exact).abs().max()) <= 2.0 ** -11 * float(exact.abs().max()) + 1e-6


def test_in_place_equals_out_of_place_and_runs_repeat(gpu):
    W, ads = _case(130, 72, (33,), seed=11)
    first = _run(gpu, W, ads)
    again = _run(gpu, W, ads)
    assert torch.equal(_bits(first), _bits(again))
    Wd = W.to(gpu)
    from vdx import ops
    dev_ads = [(u.to(gpu), d.to(gpu), s) for u, d, s in ads]
    ret = ops.lora_merge(Wd, dev_ads, out=Wd)
    assert ret.data_ptr() == Wd.data_ptr() and torch.equal(_bits(Wd), _bits(first))


@pytest.mark.parametrize("n_out,n_in", [(65, 67), (70, 68), (130, 72)], ids=["scalar", "8-byte", "16-byte"])
def test_canary_behind_out_stays_intact(gpu, n_out, n_in):
    from vdx import ops
    W, ads = _case(n_out, n_in, (5,), seed=7)
    n = n_out * n_in
    buf = torch.full((n + 4096,), -2.5, dtype=torch.float16, device=gpu)
    out = buf[:n].view(n_out, n_in)
    ops.lora_merge(W.to(gpu), [(u.to(gpu), d.to(gpu), s) for u, d, s in ads], out=out)
    assert torch.equal(_bits(out), _bits(L.merge(W, ads)))
    assert bool((buf[n:] == -2.5).all())


def test_special_values_in_w_follow_the_expression(gpu):
    W, ads = _case(70, 72, (5,), seed=21)
    W[0, 0], W[1, 1], W[2, 2], W[3, 3], W[4, 4], W[69, 71] = float("nan"), float("inf"), float("-inf"), -0.0, 65504.0, -65504.0
    want = L.merge(W, ads)
    got = _run(gpu, W, ads).cpu()
    assert bool(torch.isnan(got[0, 0])) and bool(torch.isnan(want[0, 0]))
    mask = torch.ones_like(W, dtype=torch.bool)
    mask[0, 0] = False
    assert torch.equal(_bits(got)[mask], _bits(want)[mask])
    assert got[1, 1] == float("inf") and got[2, 2] == float("-inf")
    clean, _ = _case(70, 72, (5,), seed=21)
    special = torch.zeros_like(mask)
    for i, j in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (69, 71)):
        special[i, j] = True
    assert torch.equal(_bits(got)[~special], _bits(_run(gpu, clean, ads))[~special])       # the others are unaffected


def test_non_finite_adapter_values_stay_in_their_row_and_column(gpu):
    W, ads = _case(40, 72, (3,), seed=5)
    up, down, s = ads[0]
    up[7, 1], down[2, 9] = float("inf"), float("nan")
    got = _run(gpu, W, [(up, down, s)]).cpu()
    want = L.merge(W, [(up, down, s)])
    bad = torch.isnan(want) | torch.isinf(want)
    assert bool(bad[7].all()) and bool(bad[:, 9].all()) and int(bad.sum()) == 72 + 40 - 1
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(_bits(got)[~bad], _bits(want)[~bad])


def test_zero_down_column_leaves_the_column_of_w(gpu):
    W, ads = _case(66, 72, (4,), seed=9, scales=(-0.5,))
    W[5, 10] = -0.0
    ads[0][1][:, 10] = 0.0
    got = _run(gpu, W, ads).cpu()
    assert torch.equal(_bits(got), _bits(L.merge(W, ads)))
    col, wcol = got[:, 10], W[:, 10]
    keep = torch.ones(66, dtype=torch.bool)
    keep[5] = False
    assert torch.equal(_bits(col)[keep], _bits(wcol)[keep])
    assert int(_bits(col)[5]) == 0 and int(_bits(wcol)[5]) == -32768                       # -0 -> +0, as the expression gives


def test_wrapper_refuses_what_the_kernel_does_not_take(gpu):
    from vdx import ops
    from vdx._lib import VdxError
    W, ads = _case(16, 24, (4,), seed=1)
    Wd = W.to(gpu)
    up, down, s = (t.to(gpu) if isinstance(t, torch.Tensor) else t for t in ads[0])
    bad = [
        (W, [(up, down, s)]),                                  # W on the CPU
        (Wd.float(), [(up, down, s)]),                         # dtype of W
        (Wd, [(up.half(), down, s)]),                          # dtype of up
        (Wd, [(up, down.double(), s)]),                        # dtype of down
        (Wd, [(up[:15], down, s)]),                            # up rows
        (Wd, [(up, down[:, :23].contiguous(), s)]),            # down columns
        (Wd, [(up, down[:3], s)]),                             # ranks disagree
        (Wd.t(), [(up, down, s)]),                             # not contiguous
        (Wd, [(up, down, float("nan"))]),                      # scale
        (Wd, [(up, down, 1e39)]),                              # no finite fp32
        (Wd, []),                                              # no adapter
        (Wd, [(up, down, s)] * 9),                             # A = 9
        (Wd, [(torch.zeros(16, 513, device=gpu), torch.zeros(513, 24, device=gpu), s)]),       # R = 513
        (Wd, [(up.cpu(), down, s)]),                           # device of up
    ]
    for w, a in bad:
        with pytest.raises(VdxError, match="lora_merge"):
            ops.lora_merge(w, a)
    with pytest.raises(VdxError, match="out must"):
        ops.lora_merge(Wd, [(up, down, s)], out=torch.empty(16, 25, dtype=torch.float16, device=gpu))


def test_library_rechecks_its_arguments(gpu):
    import ctypes as C

    from vdx import _lib
    lib = _lib.load()
    W = torch.zeros(4, 8, dtype=torch.float16, device=gpu)
    up, down = torch.zeros(4, 2, device=gpu), torch.zeros(2, 8, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream

    def call(A, R, s, w=W.data_ptr(), u=up.data_ptr(), n_out=4):
        return lib.vdx_lora_merge_f16(w, n_out, 8, A, (C.c_void_p * 8)(*[u] * 8), (C.c_void_p * 8)(*[down.data_ptr()] * 8),
                                      (C.c_int32 * 8)(*[R] * 8), (C.c_float * 8)(*[s] * 8), W.data_ptr(), stream)
    assert call(1, 2, 1.0) == 0
    for kw in (dict(A=0, R=2, s=1.0), dict(A=9, R=2, s=1.0), dict(A=1, R=0, s=1.0), dict(A=1, R=513, s=1.0),
               dict(A=1, R=2, s=float("inf")), dict(A=1, R=2, s=1.0, w=None), dict(A=1, R=2, s=1.0, u=None),
               dict(A=1, R=2, s=1.0, n_out=0)):
        assert call(**kw) != 0, kw
        assert b"lora_merge" in lib.vdx_last_error()
    torch.cuda.synchronize()


# ---- merge_state_dict -----------------------------------------------------------------------------------------------------------
def test_merge_state_dict(gpu):
    from vdx import lora
    from vdx.unet3d import UNet3DConfig
    from vdx.weights import synthetic_state_dict
    cfg = UNet3DConfig(block_out_channels=(64, 128, 128, 128), cross_attention_dim=128, transformer_in_heads=2)
    sd = synthetic_state_dict(cfg, 1234, "cpu")
    shapes = lora.targets("unet", cfg)
    mods = ["down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q", "down_blocks.0.attentions.0.proj_in",
            "down_blocks.0.resnets.0.conv1", "down_blocks.0.temp_convs.0.conv1.2"]
    parts = {("unet", m): v for m, v in L.seeded_adapter(shapes, mods, 4, seed=2, alpha=2.0).items()}
    a = lora.read_lora(L.adapter_file_dict(parts, "peft"), "a", unet_cfg=cfg)
    parts_b = {("unet", m): v for m, v in L.seeded_adapter(shapes, mods[:2], 8, seed=3).items()}
    b = lora.read_lora(L.adapter_file_dict(parts_b, "kohya"), "b", unet_cfg=cfg)
    assert lora.merge_state_dict(sd, "unet", [a], [0.0], gpu) is sd                       # scale 0: the input dict itself
    assert lora.merge_state_dict(sd, "unet", [], [], gpu) is sd
    assert lora.merge_state_dict(sd, "text_encoder", [a], [1.0], gpu) is sd               # no module of that component
    out = lora.merge_state_dict(sd, "unet", [a, b], [0.5, 1.0], gpu)
    want = L.hand_merge(sd, "unet", [(a, 0.5), (b, 1.0)])
    touched = {m + ".weight" for m in mods}
    assert set(out) == set(sd)
    for k in sd:
        if k in touched:
            assert out[k] is not sd[k] and out[k].device == sd[k].device and out[k].shape == sd[k].shape and out[k].dtype == torch.float16
            assert torch.equal(_bits(out[k]), _bits(want[k])) and not torch.equal(_bits(out[k]), _bits(sd[k])), k
        else:
            assert out[k] is sd[k], k
    only_a = lora.merge_state_dict(sd, "unet", [a, b], [0.5, 0.0], gpu)                   # b dropped on the host
    want_a = L.hand_merge(sd, "unet", [(a, 0.5)])
    assert all(torch.equal(_bits(only_a[k]), _bits(want_a[k])) for k in touched)
    from vdx._lib import VdxError
    short = {k: v for k, v in sd.items() if k != mods[0] + ".weight"}
    with pytest.raises(VdxError, match="attn1.to_q"):
        lora.merge_state_dict(short, "unet", [a], [1.0], gpu)
