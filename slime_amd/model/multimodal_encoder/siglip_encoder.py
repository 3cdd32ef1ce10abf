"""``SigLipVisionTower``: the plugin contract of ``CLIPVisionTower`` (constructor arguments, ``load_model``, ``delay_load``,
``forward`` on a tensor or a list, the ``out_dtype=`` extension, the dtype / device / config / hidden_size / num_patches
properties, the two-stream split, ``k_split``) over a SigLIP vision tower (HF ``SiglipVisionModel``) run by ``slime_siglip_forward``.

A SigLIP tower has no class token and no pre-LayerNorm, a conv bias, a position table of P rows and the tanh-form GELU;
``post_layernorm`` and the pooling head (``head.*``) belong to a checkpoint, are accepted on load and never run: LLaVA-style models
take ``hidden_states[select_layer]``.  ``select_feature='patch'`` returns all P tokens; ``'cls_patch'`` raises at construction.
Supported: head_dim 64, at most 24 patches per side, an intermediate size that is a multiple of 128 (the patch-16 base / large
checkpoints up to 384 pixels); anything else is refused by name before any device work (``ops.check_siglip_config``).
"""
from __future__ import annotations

import json
import os
from typing import Dict

import torch
import torch.nn as nn

from ... import ops
from ...image_processor import SiglipImageProcessor
from ...weights import SiglipVisionConfig, make_siglip_state_dict
from .clip_encoder import CLIPVisionTower, HipVisionModelBase, _Encoder, _read_hf_weights, _resolve_local

SYNTHETIC_SIGLIP_PREFIX = "synthetic-siglip:"
SIGLIP_MODEL_TYPES = ("siglip_vision_model", "siglip")


class _SiglipEmbeddings(nn.Module):
    def __init__(self, c: SiglipVisionConfig):
        super().__init__()
        self.patch_embedding = nn.Conv2d(3, c.hidden_size, c.patch_size, c.patch_size, bias=True)
        self.position_embedding = nn.Embedding(c.num_patches, c.hidden_size)


class _SiglipTransformer(nn.Module):
    def __init__(self, c: SiglipVisionConfig):
        super().__init__()
        self.embeddings = _SiglipEmbeddings(c)
        self.encoder = _Encoder(c)
        self.post_layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class HipSiglipVisionModel(HipVisionModelBase):
    """Parameter container with HF ``SiglipVisionModel`` state-dict keys (either key generation) whose forward is the HIP tower."""
    TOP_LEVEL = ("embeddings", "encoder", "post_layernorm", "head")
    DROPPED = ("head.",)

    def __init__(self, config: SiglipVisionConfig, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__(config, compute_dtype)
        self.vision_model = _SiglipTransformer(config)
        self.requires_grad_(False)

    def _anchor(self) -> torch.Tensor:
        return self.vision_model.embeddings.position_embedding.weight

    def _pack(self, select_layer: int) -> ops.PackedTower:
        return ops.pack_siglip_tower(self.state_dict(), self.config, self.operand_dtype(), self.device, select_layer)


def read_hf_config(path: str) -> dict:
    return json.load(open(os.path.join(path, "config.json")))


def is_siglip_dir(path: str) -> bool:
    """An existing directory whose config.json says ``model_type`` siglip_vision_model or siglip."""
    f = os.path.join(path, "config.json")
    if not (os.path.isdir(path) and os.path.isfile(f)):
        return False
    try:
        return json.load(open(f)).get("model_type") in SIGLIP_MODEL_TYPES
    except (OSError, ValueError):
        return False


def _read_siglip_config(path: str) -> SiglipVisionConfig:
    cfg = read_hf_config(path)
    cfg = cfg.get("vision_config", cfg)
    d = SiglipVisionConfig()
    hf_default = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224)   # HF SiglipVisionConfig's
    return SiglipVisionConfig(**{k: cfg.get(k, hf_default.get(k, getattr(d, k))) for k in d.to_dict()})


def _tower_keys_only(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The vision tower's entries of a checkpoint that may hold a whole SiglipModel (text tower, logit scale / bias)."""
    return {k: v for k, v in sd.items() if not k.startswith("text_model") and k not in ("logit_scale", "logit_bias")}


class SigLipVisionTower(CLIPVisionTower):
    # only the never-run ``post_layernorm`` may be absent (``head.*`` is dropped on load), nothing may be left over: a CLIP-layout
    # checkpoint (class_embedding, pre_layrnorm) does not load as SigLIP
    LAYOUT = "SigLIP"

    def __init__(self, vision_tower, args, delay_load=False):
        feature = getattr(args, "mm_vision_select_feature", "patch")
        if feature != "patch":
            raise ValueError(f"Unexpected select feature for a SigLIP tower: {feature!r} (it has no class token: 'patch' returns all "
                             f"of its tokens, 'cls_patch' does not exist)")
        super().__init__(vision_tower, args, delay_load=delay_load)

    def _synthetic_seed(self):
        name = self.vision_tower_name
        return int(name[len(SYNTHETIC_SIGLIP_PREFIX):] or 1234) if name.startswith(SYNTHETIC_SIGLIP_PREFIX) else None

    def _config_only(self) -> SiglipVisionConfig:
        if self._synthetic_seed() is not None:
            return SiglipVisionConfig()
        return _read_siglip_config(_resolve_local(self.vision_tower_name))

    def _source(self):
        seed = self._synthetic_seed()
        if seed is not None:                         # offline stand-in for siglip-large-patch16-384
            cfg = SiglipVisionConfig()
            sd, proc = make_siglip_state_dict(cfg, seed=seed), SiglipImageProcessor(cfg.image_size)
        else:
            path = _resolve_local(self.vision_tower_name)
            cfg, sd = _read_siglip_config(path), _tower_keys_only(_read_hf_weights(path))
            proc = SiglipImageProcessor.from_pretrained(path, cfg.image_size)
        ops.check_siglip_config(cfg)                 # activation, head_dim, patches per side, intermediate size: refused by name
        return HipSiglipVisionModel, cfg, sd, proc

    def _select(self, image_features):
        return image_features                        # 'patch' = all P tokens

    def _keep_cls(self) -> bool:
        return False
