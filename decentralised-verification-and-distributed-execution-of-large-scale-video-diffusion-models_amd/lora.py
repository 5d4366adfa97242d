"""LoRA adapters (diffusers' `load_lora_weights` / `set_adapters` / `fuse_lora`, peft's merge; unpinned, no reference counterpart):
read an adapter file, and merge adapters into a state dict of the diffusers / transformers layout BEFORE the loaders pack it.

Why before packing: `UNet3DConditionModel.load_diffusers_state_dict` derives up to five layouts from one projection (`to_qkv`,
`k7_qkv`, `k7b`, `k5`, `k8`, some with a LayerNorm folded in).  An unmerged adapter would touch every fused kernel, a delta on the
packed tensors would need one form per layout.  Merged here, `W' = W + sum_a s_a up_a @ down_a` (`ops.lora_merge`, csrc/lora.hip: a
stated fp32 order, one rounding to fp16), the loaders pack the result like any checkpoint: no kernel, packing routine or launch of
the forward changes, and every rank of a job merges the same bits for itself.

Two key conventions are read into `{(component, module): (down, up, alpha)}`, component "unet" or "text_encoder":
  peft / diffusers   unet.<module>.lora_A.weight / .lora_B.weight (A = down, B = up), the older <module>.lora.down.weight /
                     .lora.up.weight, text_encoder.<module>... with or without `text_model.`, an optional <module>.alpha
  kohya              lora_unet_<module, '_' for '.'>.lora_down.weight / .lora_up.weight / .alpha, lora_te_... for the text encoder;
                     the underscore names are resolved through a table of the model's own module names, never by splitting
`down` is (R, n_in) and `up` (n_out, R) fp32, conv adapters flattened (`down` (R, ci, kh, kw), `up` (co, R, 1, 1)); a linear adapter
on a 1x1 conv is taken when the flattened shapes agree.  `alpha` absent means alpha = R.  The scalar of a merge is
`s = fp32(scale * alpha / R)`, formed in float64 and rounded once.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import VdxError

COMPONENTS = ("unet", "text_encoder")
MAX_ADAPTERS, MAX_RANK = 8, 512
# markers of the variants that are not read: LoHa, LoKr, LoCon's mid tensor, DoRA, embedding adapters, full differences
_OTHER_VARIANTS = ("hada_", "lokr_", "lora_mid", "magnitude", "dora_scale", "lora_embedding", ".diff", "lora_magnitude_vector")
_DOWN_SUFFIXES = (".lora_A.weight", ".lora.down.weight")
_UP_SUFFIXES = (".lora_B.weight", ".lora.up.weight")


@dataclass
class LoraAdapter:
    """One adapter file: `modules[(component, module)] = (down fp32 (R, n_in), up fp32 (n_out, R), alpha)` on the CPU, and for each
    entry the file's key of its `down` tensor (`keys`), which error messages name."""
    name: str
    modules: Dict[Tuple[str, str], Tuple[torch.Tensor, torch.Tensor, float]]
    keys: Dict[Tuple[str, str], str] = field(default_factory=dict)

    def of(self, component: str) -> Dict[str, Tuple[torch.Tensor, torch.Tensor, float]]:
        return {m: v for (c, m), v in self.modules.items() if c == component}

    @property
    def rank(self):
        """The modules' rank: an integer where they share one, else the sorted list of the ranks that occur."""
        ranks = sorted({int(d.shape[0]) for d, _, _ in self.modules.values()})
        return ranks[0] if len(ranks) == 1 else ranks

    def record(self, scale: float) -> dict:
        return {"name": self.name, "scale": float(scale), "rank": self.rank, "unet_modules": len(self.of("unet")),
                "text_modules": len(self.of("text_encoder"))}


def clip_state_dict_spec(cfg) -> Dict[str, Tuple[int, ...]]:
    """`transformers.CLIPTextModel`'s table (names without `text_model.` -> shapes) for a `CLIPTextConfig`: the keys of
    `weights.synthetic_clip_state_dict`, without building its tensors."""
    d, f = cfg.hidden_size, cfg.intermediate_size
    spec: Dict[str, Tuple[int, ...]] = {"embeddings.token_embedding.weight": (cfg.vocab_size, d),
                                        "embeddings.position_embedding.weight": (cfg.max_position_embeddings, d)}

    def lin(name, co, ci):
        spec[name + ".weight"], spec[name + ".bias"] = (co, ci), (co,)

    def norm(name):
        spec[name + ".weight"], spec[name + ".bias"] = (d,), (d,)

    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}"
        norm(p + ".layer_norm1"); norm(p + ".layer_norm2")
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(f"{p}.self_attn.{n}", d, d)
        lin(p + ".mlp.fc1", f, d)
        lin(p + ".mlp.fc2", d, f)
    norm("final_layer_norm")
    return spec


def targets(component: str, cfg) -> Dict[str, Tuple[int, ...]]:
    """module -> the shape of its `.weight`, for every module of `component` an adapter can name: the linear and conv weights of
    the model's state-dict table (embeddings and norms are none)."""
    if component == "unet":
        from .weights import state_dict_spec
        spec = state_dict_spec(cfg)
    elif component == "text_encoder":
        spec = clip_state_dict_spec(cfg)
    else:
        raise ValueError(f"lora: unknown component {component!r} (expected one of {COMPONENTS})")
    return {k[:-len(".weight")]: s for k, s in spec.items() if k.endswith(".weight") and len(s) >= 2 and not k.startswith("embeddings.")}


def kohya_table(modules) -> Dict[str, str]:
    """name with '.' -> '_' |-> name, over the model's own module names; `ValueError` if two modules share an underscore name (the
    table must resolve every name uniquely: nothing is ever guessed by splitting)."""
    table: Dict[str, str] = {}
    for m in modules:
        u = m.replace(".", "_")
        if u in table:
            raise ValueError(f"lora: modules {table[u]!r} and {m!r} share the kohya name {u!r}")
        table[u] = m
    return table


def _default_cfgs(unet_cfg, text_cfg):
    if unet_cfg is None:
        from .unet3d import UNet3DConfig
        unet_cfg = UNet3DConfig.zeroscope()
    if text_cfg is None:
        from .clip_text import CLIPTextConfig
        text_cfg = CLIPTextConfig.sd2()
    return unet_cfg, text_cfg


def _load(path) -> Dict[str, torch.Tensor]:
    path = os.fspath(path)
    if "://" in path or not os.path.isfile(path):
        raise ValueError(f"lora: {path!r} is not a local file (nothing is ever downloaded)")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"lora: {path!r} does not hold a dict of tensors")
    return sd


def _split(key: str):
    """A file key -> (component, module as the file spells it, part "down" | "up" | "alpha", kohya?) or None where the key follows
    neither convention."""
    for prefix, comp in (("lora_unet_", "unet"), ("lora_te_", "text_encoder")):
        if key.startswith(prefix):
            rest = key[len(prefix):]
            for suffix, part in ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha")):
                if rest.endswith(suffix):
                    return comp, rest[:-len(suffix)], part, True
            return None
    for prefix, comp in (("unet.", "unet"), ("text_encoder.", "text_encoder")):
        if key.startswith(prefix):
            rest = key[len(prefix):]
            for suffixes, part in ((_DOWN_SUFFIXES, "down"), (_UP_SUFFIXES, "up"), ((".alpha",), "alpha")):
                for suffix in suffixes:
                    if rest.endswith(suffix):
                        return comp, rest[:-len(suffix)], part, False
            return None
    return None


def read_lora(path_or_dict, name: Optional[str] = None, *, unet_cfg=None, text_cfg=None) -> LoraAdapter:
    """A `.safetensors` file, a `torch.load(weights_only=True)` file (local paths only) or a dict of tensors -> `LoraAdapter`,
    checked against the models of `unet_cfg` (default: Zeroscope's `UNet3DConfig`) and `text_cfg` (default: SD-2's
    `CLIPTextConfig`).  `ValueError` that names the key, before anything is launched, for: a module the model does not have, half a
    pair, shapes that do not fit the target, a rank outside 1..512, a non-finite alpha, non-finite values in down / up, any other
    LoRA variant (LoHa, LoKr, `lora_mid`, DoRA's `magnitude`), a key of neither convention, and an empty file."""
    if isinstance(path_or_dict, dict):
        sd, default = path_or_dict, "adapter"
    else:
        sd, default = _load(path_or_dict), os.path.splitext(os.path.basename(os.fspath(path_or_dict)))[0]
    name = default if name is None else name
    if not isinstance(name, str) or not name:
        raise ValueError(f"lora: the adapter's name must be a non-empty string, got {name!r}")
    if not sd:
        raise ValueError(f"lora: adapter {name!r} is empty: no tensors")
    unet_cfg, text_cfg = _default_cfgs(unet_cfg, text_cfg)
    shapes = {"unet": targets("unet", unet_cfg), "text_encoder": targets("text_encoder", text_cfg)}
    kohya = {c: kohya_table(shapes[c]) for c in COMPONENTS}
    parts: Dict[Tuple[str, str], Dict[str, Tuple[str, object]]] = {}
    for key in sd:
        if not isinstance(key, str):
            raise ValueError(f"lora: key {key!r} is not a string")
        for marker in _OTHER_VARIANTS:
            if marker in key:
                raise ValueError(f"lora: key {key!r}: this LoRA variant ({marker.strip('._')}) is not read; only plain down / up pairs are")
        got = _split(key)
        if got is None:
            raise ValueError(f"lora: key {key!r} follows neither the peft / diffusers nor the kohya convention")
        comp, spelled, part, is_kohya = got
        if is_kohya:
            u = spelled[len("text_model_"):] if comp == "text_encoder" and spelled.startswith("text_model_") else spelled
            module = kohya[comp].get(u)
        else:
            module = spelled[len("text_model."):] if comp == "text_encoder" and spelled.startswith("text_model.") else spelled
            module = module if module in shapes[comp] else None
        if module is None:
            raise ValueError(f"lora: key {key!r} names a module the {comp} does not have")
        slot = parts.setdefault((comp, module), {})
        if part in slot:
            raise ValueError(f"lora: keys {slot[part][0]!r} and {key!r} both give {part} of {comp} module {module!r}")
        slot[part] = (key, sd[key])
    modules, keys = {}, {}
    for (comp, module), slot in parts.items():
        if "down" not in slot or "up" not in slot:
            have = slot.get("down") or slot.get("up") or slot["alpha"]
            raise ValueError(f"lora: key {have[0]!r}: {comp} module {module!r} has only half of its down / up pair")
        (kd, down), (ku, up) = slot["down"], slot["up"]
        for k, t in ((kd, down), (ku, up)):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                raise ValueError(f"lora: key {k!r} must be an fp16, bf16 or fp32 tensor")
            if t.dim() < 2:
                raise ValueError(f"lora: key {k!r}: shape {tuple(t.shape)} is no down / up matrix")
        R = int(down.shape[0])
        if not 1 <= R <= MAX_RANK:
            raise ValueError(f"lora: key {kd!r}: rank {R}, 1 to {MAX_RANK} are taken")
        wshape = shapes[comp][module]
        n_out, n_in = wshape[0], math.prod(wshape[1:])
        if down.numel() != R * n_in or (down.dim() > 2 and tuple(down.shape[1:]) != tuple(wshape[1:])):
            raise ValueError(f"lora: key {kd!r}: shape {tuple(down.shape)} does not fit {module}.weight {tuple(wshape)} (expected ({R}, {n_in}) "
                             f"or ({R}, {', '.join(str(x) for x in wshape[1:])}))")
        if tuple(up.shape[:2]) != (n_out, R) or up.numel() != n_out * R:
            raise ValueError(f"lora: key {ku!r}: shape {tuple(up.shape)} does not fit {module}.weight {tuple(wshape)} at rank {R} (expected "
                             f"({n_out}, {R}) with trailing 1s at most)")
        down = down.detach().to("cpu", torch.float32).reshape(R, n_in).contiguous()       # fp16 / bf16 / fp32 -> fp32 is exact
        up = up.detach().to("cpu", torch.float32).reshape(n_out, R).contiguous()
        for k, t in ((kd, down), (ku, up)):
            if not bool(torch.isfinite(t).all()):
                raise ValueError(f"lora: key {k!r} holds non-finite values")
        alpha = float(R)
        if "alpha" in slot:
            ka, a = slot["alpha"]
            try:
                alpha = float(a.double().item()) if isinstance(a, torch.Tensor) else float(a)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"lora: key {ka!r} must be one number") from None
            if not math.isfinite(alpha):
                raise ValueError(f"lora: key {ka!r}: alpha {alpha!r} is not finite")
        modules[(comp, module)] = (down, up, alpha)
        keys[(comp, module)] = kd
    return LoraAdapter(name, modules, keys)


def merge_scale(scale: float, alpha: float, R: int) -> float:
    """`s = fp32(scale * alpha / R)`: formed in float64, rounded to fp32 once; `ValueError` where that is not finite."""
    import ctypes
    s = ctypes.c_float(float(scale) * float(alpha) / int(R)).value
    if not math.isfinite(s):
        raise ValueError(f"lora: scale {scale!r} * alpha {alpha!r} / rank {R} is not a finite fp32 number")
    return s


def _strip(component: str, key: str) -> str:
    return key[len("text_model."):] if component == "text_encoder" and key.startswith("text_model.") else key


def merge_state_dict(sd: Dict[str, torch.Tensor], component: str, adapters: Sequence[LoraAdapter], scales: Sequence[float], device) -> dict:
    """`sd` (diffusers layout for "unet", transformers layout for "text_encoder", with or without `text_model.`) with `adapters` at
    `scales` merged into every weight they name.  Adapters whose scale is 0 are dropped here, on the host, so scale 0 is the base
    bit for bit (a -0 weight stays -0); with none left, or none that names a module of `component`, `sd` itself is returned.
    Otherwise a new dict: untouched tensors are the same objects; each targeted weight is taken as the loaders take it (fp16),
    uploaded to `device`, merged by `ops.lora_merge` and returned on the input tensor's device in its shape.  Everything is checked
    before the first launch: `VdxError` for a module `sd` lacks or a shape that does not fit, naming the adapter's key."""
    if component not in COMPONENTS:
        raise ValueError(f"lora: unknown component {component!r} (expected one of {COMPONENTS})")
    adapters, scales = list(adapters), [float(s) for s in scales]
    if len(adapters) != len(scales):
        raise ValueError(f"lora: {len(adapters)} adapters and {len(scales)} scales")
    for ad, s in zip(adapters, scales):
        if not math.isfinite(s):
            raise ValueError(f"lora: adapter {ad.name!r}: the scale {s!r} is not finite")
    live = [(ad, s) for ad, s in zip(adapters, scales) if s != 0 and ad.of(component)]
    if len(live) > MAX_ADAPTERS:
        raise ValueError(f"lora: {len(live)} adapters are active, {MAX_ADAPTERS} at most")
    if not live:
        return sd
    key_of = {_strip(component, k)[:-len(".weight")]: k for k in sd if k.endswith(".weight")}
    plan: Dict[str, list] = {}
    for ad, s in live:
        for module, (down, up, alpha) in ad.of(component).items():
            k = key_of.get(module)
            if k is None:
                raise VdxError(f"lora: key {ad.keys.get((component, module), module)!r} of adapter {ad.name!r} names {module!r}, which the "
                               f"{component}'s state dict does not hold")
            W = sd[k]
            if W.dim() < 2 or W.shape[0] != up.shape[0] or W[0].numel() != down.shape[1]:
                raise VdxError(f"lora: key {ad.keys.get((component, module), module)!r} of adapter {ad.name!r}: down {tuple(down.shape)} / up "
                               f"{tuple(up.shape)} do not fit {k} {tuple(W.shape)}")
            plan.setdefault(k, []).append((up, down, merge_scale(s, alpha, down.shape[0])))
    from . import ops
    dev = torch.device(device)
    out = dict(sd)
    for k, entries in plan.items():
        W = sd[k]
        w2 = W.detach().to(dev, torch.float16).reshape(W.shape[0], -1).contiguous()
        merged = ops.lora_merge(w2, [(up.to(dev), down.to(dev), s) for up, down, s in entries], out=w2 if w2.data_ptr() != W.data_ptr() else None)
        out[k] = merged.reshape(W.shape).to(W.device)
    return out


def lora_records(pairs) -> List[dict]:
    """[(LoraAdapter, scale), ...] -> the job's "lora" entry: what `read_lora` found, per adapter."""
    return [ad.record(s) for ad, s in pairs]


def apply_job_adapters(pipe, pairs, device) -> List[dict]:
    """`run_job`'s use of the pipeline's LoRA surface: the adapters of `pairs` = ((path, scale), ...) become the pipe's whole
    active set (what it had loaded before is unloaded), named after their files, merged on `device` -> the job's "lora" records."""
    pipe.unload_lora_weights()
    names = []
    for i, (path, _) in enumerate(pairs):
        name = os.path.splitext(os.path.basename(os.fspath(path)))[0] or f"lora_{i}"
        name = name if name not in names else f"{name}_{i}"
        pipe._lora[name] = read_lora(path, name, unet_cfg=pipe.unet.cfg, text_cfg=pipe.text_encoder.cfg)
        names.append(name)
    pipe.set_adapters(names, [s for _, s in pairs], device=device)
    return pipe.lora_records()
