"""The LoRA merge restated on the CPU (not a test): csrc/lora.hip's expression in torch fp32 tensors with explicit loops over the
ranks and the adapters, no `addmm`, no matmul:

    acc_a = 0.0f;  for r ascending:  acc_a = acc_a + (up_a[:, r] * down_a[r, :])       one fp32 product, one fp32 sum per term
    d     = 0.0f;  for a ascending:  d = d + (s_a * acc_a)
    out   = fp16_rn( fp32(W) + d )

torch's CPU fp32 `*` and `+` on tensors are single IEEE operations per element (no fused multiply-add), which is what the kernel is
built to evaluate.  `seeded_adapter` / `adapter_file_dict` generate the adapters every LoRA test uses, in either key convention."""
import ctypes

import torch


def f32(x: float) -> float:
    return ctypes.c_float(float(x)).value


def merge_scale(scale: float, alpha: float, R: int) -> float:
    """s = fp32(scale * alpha / R), float64 on the host, rounded once."""
    return f32(float(scale) * float(alpha) / int(R))


def delta(adapters, n_out, n_in):
    """d fp32 (n_out, n_in) of `adapters` = [(up fp32 (n_out, R), down fp32 (R, n_in), s)]."""
    d = torch.zeros((n_out, n_in), dtype=torch.float32)
    for up, down, s in adapters:
        up, down = up.detach().cpu().float(), down.detach().cpu().float()
        assert tuple(up.shape) == (n_out, down.shape[0]) and down.shape[1] == n_in
        acc = torch.zeros((n_out, n_in), dtype=torch.float32)
        for r in range(down.shape[0]):
            acc = acc + (up[:, r:r + 1] * down[r:r + 1, :])
        d = d + (torch.tensor(f32(s), dtype=torch.float32) * acc)
    return d


def merge(W, adapters):
    """fp16 (n_out, n_in): the merged weight, bit for bit what `ops.lora_merge` must return."""
    W = W.detach().cpu()
    assert W.dtype == torch.float16 and W.dim() == 2
    return (W.float() + delta(adapters, *W.shape)).half()


def merge_nd(W, adapters):
    """`merge` on a weight of any rank >= 2 (a conv weight), flattened over its input axes and shaped back."""
    return merge(W.detach().cpu().reshape(W.shape[0], -1), adapters).reshape(W.shape)


# ---- seeded adapters --------------------------------------------------------------------------------------------------------
def seeded_adapter(shapes, modules, rank, seed, magnitude=1.0, alpha=None, dtype=torch.float32):
    """{module: (down, up, alpha or None)} for `modules` of `shapes` = {module: weight shape}: down (R, ci, kh, kw...) in the
    target's own input axes, up (co, R, 1, 1...) with one trailing 1 per input axis beyond the first, values N(0, 1) scaled so
    that up @ down has about `magnitude` times the size of a fan-in scaled weight."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m in modules:
        shape = shapes[m]
        n_in = 1
        for x in shape[1:]:
            n_in *= x
        down = (torch.randn((rank,) + tuple(shape[1:]), generator=g) / n_in ** 0.5).to(dtype)
        up = (magnitude * torch.randn((shape[0], rank) + (1,) * (len(shape) - 2), generator=g) / rank ** 0.5).to(dtype)
        out[m] = (down, up, alpha)
    return out


def kohya_name(component, module):
    return ("lora_unet_" if component == "unet" else "lora_te_") + module.replace(".", "_")


def adapter_file_dict(parts, convention="peft", text_model_prefix=False):
    """{(component, module): (down, up, alpha or None)} -> the file's dict of tensors in `convention`: "peft" (lora_A / lora_B),
    "diffusers_old" (lora.down / lora.up) or "kohya"."""
    sd = {}
    for (comp, module), (down, up, alpha) in parts.items():
        if convention == "kohya":
            base = kohya_name(comp, ("text_model." + module) if comp == "text_encoder" and text_model_prefix else module)
            kd, ku, ka = base + ".lora_down.weight", base + ".lora_up.weight", base + ".alpha"
        else:
            base = comp + "." + (("text_model." + module) if comp == "text_encoder" and text_model_prefix else module)
            dn, un = ("lora_A", "lora_B") if convention == "peft" else ("lora.down", "lora.up")
            kd, ku, ka = f"{base}.{dn}.weight", f"{base}.{un}.weight", base + ".alpha"
        sd[kd], sd[ku] = down.clone(), up.clone()
        if alpha is not None:
            sd[ka] = torch.tensor(float(alpha))
    return sd


def hand_merge(sd, component, adapters_and_scales):
    """A state dict merged on the CPU by `merge_nd`: `adapters_and_scales` = [(LoraAdapter, scale)]; scale 0 entries are dropped
    as the host drops them.  The reference of every bit-for-bit test above the kernel."""
    out = dict(sd)
    strip = (lambda k: k[len("text_model."):] if k.startswith("text_model.") else k) if component == "text_encoder" else (lambda k: k)
    for k, W in sd.items():
        if not k.endswith(".weight"):
            continue
        module = strip(k)[:-len(".weight")]
        entries = []
        for ad, scale in adapters_and_scales:
            if scale != 0 and (component, module) in ad.modules:
                down, up, alpha = ad.modules[(component, module)]
                entries.append((up, down, merge_scale(scale, alpha, down.shape[0])))
        if entries:
            out[k] = merge_nd(W.half(), entries).to(W.device)
    return out
