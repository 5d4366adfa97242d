"""-m gpu: LoRA adapters through the diffusers shim into the tiny UNet and text encoder (vdx/compat/diffusers_shim.py, vdx/lora.py),
at (2, 4, 5, 16, 32), t = 7.  A seeded adapter covers every attention projection, both feed-forward projections, every proj_in /
proj_out, one 3x3 conv1 and one temporal conv.  The HIP forward with the adapter loaded lies within the live-oracle bound of
`UNet3DConditionModelRef` loaded with the same merged fp16 weights (merged here on the CPU by tests/lora_ref.py); the adapter moves
the oracle by more than ten times that bound; weight 0 and `unload_lora_weights` are the base bit for bit; two adapters equal a
hand-merged state dict loaded directly, bit for bit; and a text-encoder adapter gives the embeddings of a `CLIPTextModel` loaded
with the hand-merged dict."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lora_ref as L  # noqa: E402

pytestmark = pytest.mark.gpu
TINY = dict(ch=(64, 128, 128, 128), cross=128, in_heads=2)          # as in tests/test_freeu_gpu.py
BOUND = 4e-3                                                        # test_unet_tiny_live_oracle_other_shape's
MAGNITUDE, RANK = 0.1, 4


def unet_modules(shapes):
    """Every attention projection, ff.net.0.proj, ff.net.2, proj_in / proj_out of every transformer, one conv1 and one temporal conv."""
    ends = (".to_q", ".to_k", ".to_v", ".to_out.0", ".ff.net.0.proj", ".ff.net.2", ".proj_in", ".proj_out")
    return [m for m in shapes if m.endswith(ends)] + ["down_blocks.1.resnets.0.conv1", "up_blocks.1.temp_convs.0.conv3.3"]


def unet_adapter_dict(cfg, seed, convention="peft", magnitude=MAGNITUDE, rank=RANK, alpha=None):
    from vdx import lora
    shapes = lora.targets("unet", cfg)
    parts = {("unet", m): v for m, v in L.seeded_adapter(shapes, unet_modules(shapes), rank, seed, magnitude=magnitude, alpha=alpha).items()}
    return L.adapter_file_dict(parts, convention)


def inputs():
    g = torch.Generator().manual_seed(21)
    return torch.randn(2, 4, 5, 16, 32, generator=g).half(), torch.randn(2, 77, TINY["cross"], generator=g).half()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def oracle(sd, sample, ehs):
    from oracle.unet3d_ref import UNet3DConditionModelRef, UNet3DConfig as RefCfg
    ref = UNet3DConditionModelRef(RefCfg.tiny(**TINY)).eval()
    ref.load_state_dict({k: v.half().float() for k, v in sd.items()})
    with torch.no_grad():
        return ref(sample.float(), torch.tensor(7), ehs.float()).sample


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def world(gpu):
    import vdx  # noqa: F401
    from vdx import weights
    from vdx.compat.diffusers_shim import DiffusionPipeline
    pipe = DiffusionPipeline.from_pretrained("synthetic:tiny", torch_dtype=torch.float16).to(gpu)
    sample, ehs = inputs()
    base_sd = weights.synthetic_state_dict(pipe.unet.cfg, 1234, "cpu")
    run = lambda unet=None: (unet or pipe.unet)(sample.to(gpu), 7, encoder_hidden_states=ehs.to(gpu)).sample.clone()     # noqa: E731
    base_out = run()
    return dict(pipe=pipe, sample=sample, ehs=ehs, base_sd=base_sd, run=run, base_out=base_out,
                a=unet_adapter_dict(pipe.unet.cfg, 31, "peft"), b=unet_adapter_dict(pipe.unet.cfg, 32, "kohya", rank=8, alpha=4.0))


def test_adapter_covers_what_it_should(world):
    from vdx import lora
    ad = lora.read_lora(world["a"], "a", unet_cfg=world["pipe"].unet.cfg, text_cfg=world["pipe"].text_encoder.cfg)
    mods = set(ad.of("unet"))
    shapes = lora.targets("unet", world["pipe"].unet.cfg)
    for end in (".attn1.to_q", ".attn1.to_k", ".attn1.to_v", ".attn1.to_out.0", ".attn2.to_q", ".attn2.to_k", ".attn2.to_v", ".attn2.to_out.0",
                ".ff.net.0.proj", ".ff.net.2", ".proj_in", ".proj_out"):
        assert {m for m in shapes if m.endswith(end)} <= mods and any(m.endswith(end) for m in mods), end
    assert len(shapes["down_blocks.1.resnets.0.conv1"]) == 4 and shapes["down_blocks.1.resnets.0.conv1"][2:] == (3, 3)
    assert shapes["up_blocks.1.temp_convs.0.conv3.3"][2:] == (3, 1, 1)
    assert {"down_blocks.1.resnets.0.conv1", "up_blocks.1.temp_convs.0.conv3.3"} <= mods


def test_forward_with_adapter_matches_the_oracle_on_the_merged_weights(world):
    """The merge adds exact, separately pinned arithmetic and gets no margin of its own: the bound is the live oracle test's.  On the
    CPU oracle alone the merged and the base forwards differ by at least ten times the bound (checked on the CPU before this
    adapter's magnitude was fixed: 0.1 gives 0.303, 0.05 gives 0.154), so an adapter that was dropped, halved or applied to the wrong module fails."""
    from vdx import lora
    pipe = world["pipe"]
    ad = pipe.load_lora_weights(world["a"], adapter_name="a")
    try:
        assert pipe.get_active_adapters() == ["a"]
        out = world["run"]()
        merged_sd = L.hand_merge(world["base_sd"], "unet", [(ad, 1.0)])
        ref_merged = oracle(merged_sd, world["sample"], world["ehs"])
        ref_base = oracle(world["base_sd"], world["sample"], world["ehs"])
        err, moved, moved_hip = rel_l2(out.float().cpu(), ref_merged), rel_l2(ref_merged, ref_base), rel_l2(out.float().cpu(), world["base_out"].float().cpu())
        print(f"lora: HIP vs oracle on merged weights rel-L2 {err:.3e}; oracle merged vs base {moved:.3e}; HIP merged vs base {moved_hip:.3e}")
        assert moved >= 10 * BOUND
        assert err <= BOUND
        assert moved_hip > BOUND
        world["out_a"] = out
        assert isinstance(ad, lora.LoraAdapter)
    finally:
        pipe.unload_lora_weights()


def test_weight_zero_and_unload_are_the_base_bit_for_bit(world):
    pipe = world["pipe"]
    pipe.load_lora_weights(world["a"], adapter_name="a")
    with_a = world["run"]()
    assert not torch.equal(_bits(with_a), _bits(world["base_out"]))
    pipe.set_adapters("a", 0.0)
    assert pipe.get_active_adapters() == ["a"] and torch.equal(_bits(world["run"]()), _bits(world["base_out"]))
    pipe.set_adapters(["a"], [1.0])
    assert torch.equal(_bits(world["run"]()), _bits(with_a))
    pipe.unfuse_lora()
    assert pipe.get_active_adapters() == [] and torch.equal(_bits(world["run"]()), _bits(world["base_out"]))
    pipe.fuse_lora(lora_scale=1.0)
    assert pipe.get_active_adapters() == ["a"] and torch.equal(_bits(world["run"]()), _bits(with_a))
    pipe.unload_lora_weights()
    assert pipe.get_active_adapters() == [] and pipe._lora == {} and torch.equal(_bits(world["run"]()), _bits(world["base_out"]))
    with pytest.raises(ValueError, match="no adapter named"):
        pipe.set_adapters("a")


def test_two_adapters_equal_a_hand_merged_state_dict(world, gpu):
    from vdx.unet3d import UNet3DConditionModel
    pipe = world["pipe"]
    a = pipe.load_lora_weights(world["a"], adapter_name="a")
    b = pipe.load_lora_weights(world["b"], adapter_name="b")
    try:
        assert pipe.get_active_adapters() == ["a", "b"]
        pipe.set_adapters(["a", "b"], [0.5, 1.0])
        got = world["run"]()
        direct = UNet3DConditionModel(pipe.unet.cfg).load_diffusers_state_dict(L.hand_merge(world["base_sd"], "unet", [(a, 0.5), (b, 1.0)]), device=gpu)
        assert set(direct.W) == set(pipe.unet.W) and all(torch.equal(direct.W[k], pipe.unet.W[k]) for k in direct.W)
        assert torch.equal(_bits(got), _bits(world["run"](direct)))
        assert pipe.lora_records() == [{"name": "a", "scale": 0.5, "rank": 4, "unet_modules": len(a.of("unet")), "text_modules": 0},
                                       {"name": "b", "scale": 1.0, "rank": 8, "unet_modules": len(b.of("unet")), "text_modules": 0}]
        with pytest.raises(ValueError, match="already loaded"):
            pipe.load_lora_weights(world["a"], adapter_name="a")
        with pytest.raises(ValueError, match="twice"):
            pipe.set_adapters(["a", "a"])
        with pytest.raises(ValueError, match="finite"):
            pipe.set_adapters(["a"], [float("nan")])
        assert torch.equal(_bits(world["run"]()), _bits(got))            # a refused call changes nothing
    finally:
        pipe.unload_lora_weights()


def test_text_encoder_adapter_through_the_shim(world, gpu):
    from vdx import lora, weights
    from vdx.clip_text import CLIPTextModel
    pipe = world["pipe"]
    tcfg = pipe.text_encoder.cfg
    shapes = lora.targets("text_encoder", tcfg)
    parts = {("text_encoder", m): v for m, v in L.seeded_adapter(shapes, list(shapes), 4, seed=41, magnitude=0.5).items()}
    ids = pipe.tokenizer(["a rocket in space", ""], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    base = pipe.text_encoder(ids.to(gpu))[0].clone()
    unet_before = {k: v.data_ptr() for k, v in pipe.unet.W.items()}
    ad = pipe.load_lora_weights(L.adapter_file_dict(parts, "kohya", text_model_prefix=True), adapter_name="te")
    try:
        assert {k: v.data_ptr() for k, v in pipe.unet.W.items()} == unet_before          # the UNet was not re-loaded
        got = pipe.text_encoder(ids.to(gpu))[0].clone()
        hand = L.hand_merge(weights.synthetic_clip_state_dict(tcfg, 11, "cpu"), "text_encoder", [(ad, 1.0)])
        direct = CLIPTextModel(tcfg).load_transformers_state_dict(hand, device=gpu)
        assert torch.equal(_bits(got), _bits(direct(ids.to(gpu))[0])) and not torch.equal(_bits(got), _bits(base))
        assert ad.record(1.0)["text_modules"] == len(shapes) == 12 and ad.record(1.0)["unet_modules"] == 0
    finally:
        pipe.unload_lora_weights()
    assert torch.equal(_bits(pipe.text_encoder(ids.to(gpu))[0]), _bits(base))
