"""LoRA state dicts -> the engine's merge inputs (`StableDiffusionPipeline.load_lora_weights`, agd_lora_add).

Accepted formats [upstream-knowledge: diffusers 0.21.2 `LoraLoaderMixin`, kohya-ss sd-scripts]:
  kohya        lora_unet_<module with _>.lora_down.weight / .lora_up.weight / .alpha, lora_te_<text module with _>.*
               (scale alpha / rank; no .alpha key: 1)
  diffusers    unet.<module>.lora.{down,up}.weight; text_encoder.<module>.lora_linear_layer.{down,up}.weight
  attn-procs   [unet.]<block>.attn{1,2}.processor.to_{q,k,v,out}_lora.{down,up}.weight;
               text_encoder.<layer>.self_attn.[processor.]to_{q,k,v,out}_lora.{down,up}.weight
Targets: in the UNet's transformer blocks attn1 / attn2 to_q, to_k, to_v, to_out.0, ff.net.0.proj, ff.net.2, proj_in, proj_out; in the
text encoder q/k/v/out_proj, fc1, fc2.  Anything else (conv / LoCon keys on resnets and samplers, time_emb_proj, LDM-named kohya keys,
LoHa / LoKr, shape or rank mismatches) raises a ValueError naming the first key that cannot be placed."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import torch

from .config import SDConfig, text_param_shapes, unet_param_shapes

WEIGHT_NAMES = ("pytorch_lora_weights.safetensors", "pytorch_lora_weights.bin")
_UNET_TAILS = ("transformer_blocks.0.attn1.to_q", "transformer_blocks.0.attn1.to_k", "transformer_blocks.0.attn1.to_v",
               "transformer_blocks.0.attn1.to_out.0", "transformer_blocks.0.attn2.to_q", "transformer_blocks.0.attn2.to_k",
               "transformer_blocks.0.attn2.to_v", "transformer_blocks.0.attn2.to_out.0", "transformer_blocks.0.ff.net.0.proj",
               "transformer_blocks.0.ff.net.2", "proj_in", "proj_out")
_TEXT_TAILS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2")
_PROC = re.compile(r"^(?P<parent>.+?)\.(?:processor\.)?to_(?P<p>q|k|v|out)_lora\.(?P<part>down|up)\.weight$")


@dataclass
class LoraEntry:
    key: str                 # the engine key ("unet.<diffusers key>", "text.encoder.layers.<l>.<...>.weight")
    down: torch.Tensor       # fp32 [rank, in]
    up: torch.Tensor         # fp32 [out, rank]
    alpha: float             # the merge scales up @ down by alpha / rank


def target_modules(cfg: SDConfig) -> Dict[str, Tuple[str, Tuple[int, int]]]:
    """Canonical module path -> (engine key, (out, in)).  UNet paths are diffusers module paths ("down_blocks.0.attentions.0.proj_in"),
    text paths carry transformers' "text_model." prefix."""
    out: Dict[str, Tuple[str, Tuple[int, int]]] = {}
    ushapes = unet_param_shapes(cfg.unet)
    blocks = sorted({k[:k.index(".transformer_blocks.")] for k in ushapes if ".transformer_blocks.0.attn1.to_q.weight" in k})
    for b in blocks:
        for t in _UNET_TAILS:
            m = f"{b}.{t}"
            s = ushapes[m + ".weight"]
            out[m] = ("unet." + m + ".weight", (int(s[0]), int(s[1])))
    if cfg.text is not None:
        tshapes = text_param_shapes(cfg.text)
        for l in range(cfg.text.num_hidden_layers):
            for t in _TEXT_TAILS:
                m = f"encoder.layers.{l}.{t}"
                s = tshapes[m + ".weight"]
                out["text_model." + m] = ("text." + m + ".weight", (int(s[0]), int(s[1])))
    return out


def _place(key: str, kohya: Dict[str, str]) -> Optional[Tuple[str, str]]:
    """(canonical module, "down" | "up" | "alpha") of one state-dict key, or None."""
    if key.startswith(("lora_unet_", "lora_te_")):
        for suf, part in ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".alpha", "alpha")):
            if key.endswith(suf):
                m = kohya.get(key[:-len(suf)])
                return (m, part) if m else None
        return None
    text = key.startswith("text_encoder.")
    k = key[len("text_encoder."):] if text else (key[len("unet."):] if key.startswith("unet.") else key)
    mp = _PROC.match(k)
    if mp:
        p = mp.group("p")
        tail = ({"q": "q_proj", "k": "k_proj", "v": "v_proj", "out": "out_proj"} if text else
                {"q": "to_q", "k": "to_k", "v": "to_v", "out": "to_out.0"})[p]
        module, part = mp.group("parent") + "." + tail, mp.group("part")
    else:
        for suf, part_ in ((".lora.down.weight", "down"), (".lora.up.weight", "up"),
                           (".lora_linear_layer.down.weight", "down"), (".lora_linear_layer.up.weight", "up")):
            if k.endswith(suf):
                module, part = k[:-len(suf)], part_
                break
        else:
            return None
    if text and not module.startswith("text_model."):
        module = "text_model." + module
    return module, part


def lora_to_engine(sd: Dict[str, torch.Tensor], cfg: SDConfig) -> List[LoraEntry]:
    """A LoRA state dict -> one LoraEntry per target (ValueError naming the first key it cannot place)."""
    targets = target_modules(cfg)
    kohya = {("lora_te_" if m.startswith("text_model.") else "lora_unet_") + m.replace(".", "_"): m for m in targets}
    parts: Dict[str, Dict[str, Tuple[str, torch.Tensor]]] = {}
    for key, t in sd.items():
        pl = _place(key, kohya)
        if pl is None or pl[0] not in targets:
            raise ValueError(f"LoRA: cannot place key '{key}' (supported: linear LoRA on the UNet transformer blocks' attn1 / attn2 / ff / "
                             "proj_in / proj_out and the text encoder's q/k/v/out_proj / fc1 / fc2, in kohya, diffusers or attn-procs naming)")
        module, part = pl
        if part in parts.setdefault(module, {}):
            raise ValueError(f"LoRA: key '{key}' duplicates '{parts[module][part][0]}'")
        parts[module][part] = (key, t)
    out: List[LoraEntry] = []
    for module, p in parts.items():
        any_key = next(iter(p.values()))[0]
        if "down" not in p or "up" not in p:
            raise ValueError(f"LoRA: key '{any_key}' has no matching {'up' if 'down' in p else 'down'} factor")
        (kd, d), (ku, u) = p["down"], p["up"]
        d, u = d.detach().to("cpu", torch.float32), u.detach().to("cpu", torch.float32)
        for k_, t_ in ((kd, d), (ku, u)):
            if t_.ndim == 4 and tuple(t_.shape[2:]) != (1, 1):
                raise ValueError(f"LoRA: key '{k_}' is a {t_.shape[2]}x{t_.shape[3]} conv factor (conv LoRA is not supported)")
            if t_.ndim not in (2, 4):
                raise ValueError(f"LoRA: key '{k_}' has shape {tuple(t_.shape)} (a linear or 1x1-conv factor expected)")
        d, u = d.reshape(d.shape[0], d.shape[1]), u.reshape(u.shape[0], u.shape[1])
        key, (n_out, n_in) = targets[module]
        r = d.shape[0]
        if u.shape[1] != r:
            raise ValueError(f"LoRA: key '{ku}' has rank {u.shape[1]}, its down factor '{kd}' rank {r}")
        if d.shape[1] != n_in or u.shape[0] != n_out:
            raise ValueError(f"LoRA: key '{kd}': factors [{r}, {d.shape[1]}] / [{u.shape[0]}, {r}] do not fit the [{n_out}, {n_in}] matrix {key}")
        alpha = float(r)
        if "alpha" in p:
            a = p["alpha"][1]
            alpha = float(a.reshape(-1)[0]) if torch.is_tensor(a) else float(a)
            if not alpha > 0:
                raise ValueError(f"LoRA: key '{p['alpha'][0]}': alpha {alpha} must be positive")
        out.append(LoraEntry(key, d.contiguous(), u.contiguous(), alpha))
    if not out:
        raise ValueError("LoRA: the state dict holds no LoRA factors")
    return out


def load_lora_state_dict(path_or_dict: Union[str, os.PathLike, Dict[str, torch.Tensor]], weight_name: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """A state dict as given, or read from a file / directory (`weight_name` in it, else pytorch_lora_weights.safetensors, then .bin)."""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    path = os.fspath(path_or_dict)
    if os.path.isdir(path):
        names = [weight_name] if weight_name else list(WEIGHT_NAMES)
        for n in names:
            if os.path.isfile(os.path.join(path, n)):
                path = os.path.join(path, n)
                break
        else:
            raise FileNotFoundError(f"LoRA: no {' or '.join(names)} in {path}")
    elif not os.path.isfile(path):
        raise FileNotFoundError(f"LoRA: {path} does not exist")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)
