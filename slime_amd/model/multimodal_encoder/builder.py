"""``build_vision_tower`` -- same contract as llava/model/multimodal_encoder/builder.py:5-11."""
import os

from .clip_encoder import CLIPVisionTower, SYNTHETIC_PREFIX, _resolve_local
from .siglip_encoder import SigLipVisionTower, SYNTHETIC_SIGLIP_PREFIX, is_siglip_dir
from .dinov2_encoder import Dinov2VisionTower, SYNTHETIC_DINOV2_PREFIX, is_dinov2_dir


def is_siglip_tower(vision_tower: str) -> bool:
    """A SigLIP tower is selected by an existing directory whose config.json has ``model_type`` siglip_vision_model or siglip (its
    ``vision_config`` is used), by a hub-style name containing ``siglip`` (resolved from the local HF cache), or by the offline
    stand-in ``synthetic-siglip:<seed>``."""
    if os.path.exists(vision_tower):
        return is_siglip_dir(vision_tower)
    return vision_tower.startswith(SYNTHETIC_SIGLIP_PREFIX) or "siglip" in vision_tower.lower()


def is_dinov2_tower(vision_tower: str) -> bool:
    """A DINOv2 tower is selected by an existing directory whose config.json has ``model_type`` dinov2 or dinov2_with_registers, by
    a hub-style name containing ``dinov2`` (resolved from the local HF cache), or by the offline stand-in
    ``synthetic-dinov2:<seed>`` (ViT-L/14, 4 registers, run at 224)."""
    if os.path.exists(vision_tower):
        return is_dinov2_dir(vision_tower)
    return vision_tower.startswith(SYNTHETIC_DINOV2_PREFIX) or "dinov2" in vision_tower.lower()


def build_vision_tower(vision_tower_cfg, **kwargs):
    """Reads ``mm_vision_tower`` (else ``vision_tower``) from the config; accepts an existing path,
    hub-style names starting with ``openai`` / ``laion`` or containing ``ShareGPT4V`` (resolved from the
    local HF cache: there is no network here), plus the offline stand-in ``synthetic:<seed>``; SigLIP towers
    (:func:`is_siglip_tower`) go to ``SigLipVisionTower``, DINOv2 towers (:func:`is_dinov2_tower`) to ``Dinov2VisionTower``.
    Anything else raises ``ValueError('Unknown vision tower: ...')`` like the reference."""
    vision_tower = getattr(vision_tower_cfg, "mm_vision_tower", getattr(vision_tower_cfg, "vision_tower", None))
    if vision_tower is None:
        raise ValueError("Unknown vision tower: None")
    if is_siglip_tower(vision_tower):
        return SigLipVisionTower(vision_tower, args=vision_tower_cfg, **kwargs)
    if is_dinov2_tower(vision_tower):
        if not os.path.exists(vision_tower) and not vision_tower.startswith(SYNTHETIC_DINOV2_PREFIX):
            try:                                 # a hub-style name: known only if the local HF cache holds it
                _resolve_local(vision_tower)
            except FileNotFoundError as e:
                raise ValueError(f"Unknown vision tower: {vision_tower} (a DINOv2 name that is not in the local HF cache; pass a "
                                 f"directory with config.json + model.safetensors, or '{SYNTHETIC_DINOV2_PREFIX}<seed>')") from e
        return Dinov2VisionTower(vision_tower, args=vision_tower_cfg, **kwargs)
    if (os.path.exists(vision_tower) or vision_tower.startswith("openai") or vision_tower.startswith("laion")
            or "ShareGPT4V" in vision_tower or vision_tower.startswith(SYNTHETIC_PREFIX)):
        return CLIPVisionTower(vision_tower, args=vision_tower_cfg, **kwargs)
    raise ValueError(f"Unknown vision tower: {vision_tower}")
