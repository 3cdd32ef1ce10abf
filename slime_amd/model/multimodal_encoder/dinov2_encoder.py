"""``Dinov2VisionTower``: the plugin contract of ``SigLipVisionTower`` (constructor arguments, ``load_model``, ``delay_load``,
``forward`` on a tensor or a list, the ``out_dtype=`` extension, the dtype / device / config / hidden_size / num_patches
properties, the two-stream split, ``k_split``) over a DINOv2 vision tower (HF ``Dinov2Model`` / ``Dinov2WithRegistersModel``) run by
``slime_dinov2_forward``.

A DINOv2 crop is ``[cls + pos[0]] [R register tokens] [P patches]``: no pre-LayerNorm, a conv bias, LayerScale behind the attention
and the MLP (folded into out_proj / fc2 at pack time), a position table made for 37 x 37 patches that is interpolated to the run
grid once, at pack time.  ``mask_token`` and the final ``layernorm`` belong to a checkpoint, are accepted on load and never run:
LLaVA-style models take ``hidden_states[select_layer]``.  The run size is ``preprocessor_config.json``'s ``crop_size`` where the
directory has one (224 for the released checkpoints), else ``config.json``'s ``image_size``; ``config.image_size``, ``num_patches``
and ``num_patches_per_side`` follow it.  ``select_feature='patch'`` returns the P patch rows; ``'cls_patch'`` returns class token +
patches for a tower without registers and raises at construction for one with registers (its rows are not contiguous).
Supported: ViT-B/14 and ViT-L/14 (head_dim 64, the plain GELU MLP), at most 24 patches per side, at most 16 registers; anything
else is refused by name before any device work (``ops.check_dinov2_config``).
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn as nn

from ... import ops
from ...image_processor import Dinov2ImageProcessor
from ...weights import Dinov2VisionConfig, DINOV2_L_REG4_224, make_dinov2_state_dict, strip_dinov2_prefix
from .clip_encoder import CLIPVisionTower, HipVisionModelBase, _read_hf_weights, _resolve_local

SYNTHETIC_DINOV2_PREFIX = "synthetic-dinov2:"
DINOV2_MODEL_TYPES = ("dinov2", "dinov2_with_registers")


class _PatchEmbeddings(nn.Module):
    def __init__(self, c: Dinov2VisionConfig):
        super().__init__()
        self.projection = nn.Conv2d(3, c.hidden_size, c.patch_size, c.patch_size, bias=True)


class _Dinov2Embeddings(nn.Module):
    def __init__(self, c: Dinov2VisionConfig):
        super().__init__()
        self.cls_token = nn.Parameter(torch.empty(1, 1, c.hidden_size))
        self.mask_token = nn.Parameter(torch.zeros(1, c.hidden_size))
        if c.num_register_tokens > 0:
            self.register_tokens = nn.Parameter(torch.empty(1, c.num_register_tokens, c.hidden_size))
        self.patch_embeddings = _PatchEmbeddings(c)
        self.position_embeddings = nn.Parameter(torch.empty(1, 1 + c.table_grid ** 2, c.hidden_size))


class _SelfAttention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.query, self.key, self.value = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)


class _SelfOutput(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.dense = nn.Linear(d, d)


class _Attention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.attention, self.output = _SelfAttention(d), _SelfOutput(d)


class _LayerScale(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.lambda1 = nn.Parameter(torch.ones(d))


class _Mlp(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(d, f), nn.Linear(f, d)


class _Layer(nn.Module):
    def __init__(self, c: Dinov2VisionConfig):
        super().__init__()
        self.norm1 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.attention = _Attention(c.hidden_size)
        self.layer_scale1 = _LayerScale(c.hidden_size)
        self.norm2 = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.mlp = _Mlp(c.hidden_size, c.intermediate_size)
        self.layer_scale2 = _LayerScale(c.hidden_size)


class _Encoder(nn.Module):
    def __init__(self, c: Dinov2VisionConfig):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c) for _ in range(c.num_hidden_layers)])


class _Dinov2Transformer(nn.Module):
    def __init__(self, c: Dinov2VisionConfig):
        super().__init__()
        self.embeddings = _Dinov2Embeddings(c)
        self.encoder = _Encoder(c)
        self.layernorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)


class HipDinov2VisionModel(HipVisionModelBase):
    """Parameter container with HF ``Dinov2Model`` / ``Dinov2WithRegistersModel`` state-dict keys (bare, or behind the prefix of a
    model that wraps one) whose forward is the HIP tower."""
    TOP_LEVEL = ("embeddings", "encoder", "layernorm")

    def __init__(self, config: Dinov2VisionConfig, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__(config, compute_dtype)
        self.vision_model = _Dinov2Transformer(config)
        self.requires_grad_(False)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for k in [k for k in state_dict if k.startswith(prefix)]:
            bare = next(iter(strip_dinov2_prefix({k[len(prefix):]: None})))
            if prefix + bare != k:
                state_dict[prefix + bare] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _anchor(self) -> torch.Tensor:
        return self.vision_model.embeddings.cls_token

    def _pack(self, select_layer: int) -> ops.PackedTower:
        return ops.pack_dinov2_tower(self.state_dict(), self.config, self.operand_dtype(), self.device, select_layer)


def is_dinov2_dir(path: str) -> bool:
    """An existing directory whose config.json (or its ``vision_config``) says ``model_type`` dinov2 or dinov2_with_registers."""
    f = os.path.join(path, "config.json")
    if not (os.path.isdir(path) and os.path.isfile(f)):
        return False
    try:
        top = json.load(open(f))
    except (OSError, ValueError):
        return False
    vision = top.get("vision_config")
    return top.get("model_type") in DINOV2_MODEL_TYPES or (isinstance(vision, dict) and vision.get("model_type") in DINOV2_MODEL_TYPES)


def _run_size(path: str, config_image_size: int) -> int:
    """``preprocessor_config.json``'s ``crop_size`` where the directory has one, else ``config.json``'s ``image_size``."""
    f = os.path.join(path, "preprocessor_config.json")
    if os.path.isfile(f):
        crop = json.load(open(f)).get("crop_size")
        if isinstance(crop, dict):
            crop = crop.get("height")
        if crop:
            return int(crop)
    return int(config_image_size)


def _read_dinov2_config(path: str) -> Dinov2VisionConfig:
    """config.json (flat, or with the tower's fields under ``vision_config``) -> Dinov2VisionConfig at the directory's run size."""
    top = json.load(open(os.path.join(path, "config.json")))
    cfg = top.get("vision_config", top)
    model_type = cfg.get("model_type", top.get("model_type"))
    if model_type not in DINOV2_MODEL_TYPES:
        raise ValueError(f"vision tower {path!r} has model_type={model_type!r}: not a DINOv2 tower ({' / '.join(DINOV2_MODEL_TYPES)})")
    hf = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, mlp_ratio=4, image_size=224, patch_size=14,
              layer_norm_eps=1e-6, hidden_act="gelu", use_swiglu_ffn=False, num_register_tokens=0)       # HF Dinov2Config's defaults
    if model_type == "dinov2_with_registers":
        hf["num_register_tokens"] = 4
    v = {k: cfg.get(k, d) for k, d in hf.items()}
    table_image = int(v.pop("image_size"))
    return Dinov2VisionConfig(image_size=_run_size(path, table_image), table_grid=table_image // int(v["patch_size"]),
                              model_type=model_type, **v)


class Dinov2VisionTower(CLIPVisionTower):
    # only the never-read ``mask_token`` and ``layernorm`` may be absent, nothing may be left over: a CLIP or SigLIP checkpoint does
    # not load as DINOv2
    LAYOUT, TOLERATED = "DINOv2", ("embeddings.mask_token", ".layernorm.")

    def __init__(self, vision_tower, args, delay_load=False):
        feature = getattr(args, "mm_vision_select_feature", "patch")
        if feature not in ("patch", "cls_patch"):
            raise ValueError(f"Unexpected select feature: {feature}")
        self._seed = (int(vision_tower[len(SYNTHETIC_DINOV2_PREFIX):] or 1234)
                      if vision_tower.startswith(SYNTHETIC_DINOV2_PREFIX) else None)
        cfg = DINOV2_L_REG4_224 if self._seed is not None else _read_dinov2_config(_resolve_local(vision_tower))
        if feature == "cls_patch" and cfg.num_register_tokens > 0:
            raise ValueError(f"Unexpected select feature for a DINOv2 tower with {cfg.num_register_tokens} register tokens: 'cls_patch' "
                             f"(the class token and the patches are not contiguous rows; 'patch' returns the patches)")
        ops.check_dinov2_config(cfg)                 # SwiGLU, activation, head_dim, width, run size, registers: refused by name
        self._cfg = cfg
        super().__init__(vision_tower, args, delay_load=delay_load)

    def _config_only(self) -> Dinov2VisionConfig:
        return self._cfg

    def _source(self):
        cfg = self._cfg                              # read and checked at construction
        if self._seed is not None:                   # offline stand-in: ViT-L/14, 4 registers, table for 37 x 37, run at 224
            sd = make_dinov2_state_dict(cfg, seed=self._seed)
            proc = Dinov2ImageProcessor(cfg.image_size * 256 // 224, cfg.image_size)
        else:
            path = _resolve_local(self.vision_tower_name)
            sd = _read_hf_weights(path, keep=None)   # every key: ``projection`` is the conv here
            proc = Dinov2ImageProcessor.from_pretrained(path, cfg.image_size)
        return HipDinov2VisionModel, cfg, sd, proc

    def _select(self, image_features):
        """``feature_select`` on an HF-like output (all S rows per state)."""
        if self.select_feature == "patch":
            return image_features[:, self._cfg.n_prefix:]
        return image_features                        # 'cls_patch': no registers (checked at construction), all rows
