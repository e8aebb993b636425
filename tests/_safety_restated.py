"""Restatement of the Stable-Diffusion safety checker the reference runs behind `pipeline(...)` (reference
data_generation/data_generation.py:59-62), for the tests: the CLIPImageProcessor front end, the tower through transformers, and the
per-image decision.  [upstream-knowledge: diffusers 0.21.2 StableDiffusionSafetyChecker / transformers 4.30.2 CLIPImageProcessor]"""
from __future__ import annotations

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def preprocess(images_u8: np.ndarray, size: int = 224, mean=CLIP_MEAN, std=CLIP_STD) -> np.ndarray:
    """CLIPImageProcessor.preprocess on the pipeline's PIL images (`numpy_to_pil`): resize the shortest edge to `size` with PIL
    BICUBIC on the uint8 image, center crop (the identity for square images), rescale by 1/255 (float64, then float32),
    normalize (x - mean) / std in float32.  Returns pixel_values [B, 3, size, size] float32."""
    from PIL import Image
    out = []
    for im in images_u8:
        r = np.asarray(Image.fromarray(im).resize((size, size), resample=Image.BICUBIC))
        x = (r * (1 / 255)).astype(np.float32)
        x = (x - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
        out.append(x.transpose(2, 0, 1))
    return np.stack(out).astype(np.float32)


def hf_tower(scfg, sd):
    """transformers CLIPVisionModel + the checker's visual_projection, loaded from the diffusers state dict (fp32, CPU)."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    vc = CLIPVisionConfig(hidden_size=scfg.hidden_size, intermediate_size=scfg.intermediate_size, num_hidden_layers=scfg.num_hidden_layers,
                          num_attention_heads=scfg.num_attention_heads, image_size=scfg.image_size, patch_size=scfg.patch_size,
                          hidden_act=scfg.hidden_act, layer_norm_eps=scfg.layer_norm_eps, projection_dim=scfg.projection_dim)
    m = CLIPVisionModel(vc).eval()
    # checker keys are "vision_model." + CLIPVisionModel keys; transformers 4.x names those "vision_model.…", 5.x drops the prefix
    own = {k[len("vision_model."):]: v for k, v in sd.items() if k.startswith("vision_model.")}
    if not any(k.startswith("vision_model.") for k in m.state_dict()):
        own = {k[len("vision_model."):]: v for k, v in own.items()}
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    proj = sd["visual_projection.weight"].float()

    @torch.no_grad()
    def embeds(pixel_values: torch.Tensor) -> torch.Tensor:
        """StableDiffusionSafetyChecker.forward: pooled_output = vision_model(clip_input)[1]; image_embeds = visual_projection(pooled)."""
        pooled = m(pixel_values=pixel_values.float())[1]
        return pooled @ proj.t()
    return embeds


def cosine_distance(image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> np.ndarray:
    """diffusers safety_checker.cosine_distance: mm(normalize(image_embeds), normalize(text_embeds).t()), as float32 numpy."""
    a = torch.nn.functional.normalize(image_embeds.float())
    b = torch.nn.functional.normalize(text_embeds.float())
    return torch.mm(a, b.t()).cpu().float().numpy()


def decide(special_cos: np.ndarray, cos: np.ndarray, special_w, concept_w):
    """StableDiffusionSafetyChecker.forward's loop, per image: adjustment starts at 0.0; each special-care concept scores
    round(cos - threshold + adjustment, 3) and a score > 0 sets adjustment = 0.01 (seen by the special concepts after it too);
    then each concept scores the same way and any score > 0 marks the image (has_nsfw_concepts).  `cos` is float32 and the
    threshold a Python float (`.item()`), which NumPy 1.x subtracts in float64 before `round` (= np.round); float64 here."""
    flags, details = [], []
    for i in range(len(cos)):
        adjustment = 0.0
        special_scores, concept_scores = [], []
        for j in range(special_cos.shape[1]):
            s = np.round(np.float64(np.float32(special_cos[i][j])) - float(np.float32(special_w[j])) + adjustment, 3)
            special_scores.append(s)
            if s > 0:
                adjustment = 0.01
        bad = []
        for k in range(cos.shape[1]):
            s = np.round(np.float64(np.float32(cos[i][k])) - float(np.float32(concept_w[k])) + adjustment, 3)
            concept_scores.append(s)
            if s > 0:
                bad.append(k)
        flags.append(len(bad) > 0)
        details.append({"special_scores": special_scores, "concept_scores": concept_scores, "bad_concepts": bad})
    return flags, details
