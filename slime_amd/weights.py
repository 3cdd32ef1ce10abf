"""Deterministic synthetic weights + state-dict key layout for the SliME visual hot path.

There is no network on either box, so neither the CLIP-ViT-L/14-336 checkpoint nor a SliME
checkpoint is available.  Both the build container (where the reference is imported to make
golden vectors) and the GPU box regenerate *identical* weights from a seed with a CPU
``torch.Generator`` (bit-reproducible for a fixed torch build).

Key layout follows the reference's checkpoints:

* tower  : HF ``CLIPVisionModel`` keys.  transformers==4.37.2 (pinned by the reference,
  ``pyproject.toml:17``) prefixes them with ``vision_model.``; transformers 5.x dropped the
  prefix.  :func:`canonical_tower_key` accepts both.
* adapter: ``mm_projector.*`` (GatedBlock, ``llava/model/multimodal_projector/builder.py:38-74``) and
  ``sampler.post_qformer.*`` (Resampler, ``llava/model/multimodal_resampler/sampler.py:115-137``).

The scales differ on purpose from HF's ``_init_weights``: q/k projections are O(1) so that the
attention logits have unit-order spread (HF's init makes softmax almost uniform, which would
make attention parity vacuous); biases and LayerNorm affine parameters are non-trivial so every
epilogue path is exercised; ``w_gate`` is non-zero (the reference zero-inits it, which makes the
gate a constant 0.5/0.5).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, asdict
from typing import Dict

import numpy as np
import torch


@dataclass(frozen=True)
class VisionConfig:
    """Geometry of the CLIP vision tower (HF ``CLIPVisionConfig`` field names)."""
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    image_size: int = 336
    patch_size: int = 14
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid * self.grid

    @property
    def seq_len(self) -> int:
        return self.num_patches + 1

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    def to_dict(self):
        return asdict(self)


CLIP_L_336 = VisionConfig()
# Small geometry used by the golden-vector fixtures: full tensors fit in a few hundred KB.
# Same image/patch geometry (336/14 -> S=577) so every shape-dependent code path is shared.
TINY = VisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2)


@dataclass(frozen=True)
class AdapterConfig:
    """Geometry of the SliME adapter (``mm_projector_type='gated'`` + ``post_qformer``)."""
    mm_hidden_size: int = 1024      # tower width
    hidden_size: int = 4096         # LLM width
    head_dim: int = 128             # resamplers use embed_dim // 128 heads (projector/builder.py:46)
    global_queries: int = 576       # GatedBlock.attn grid 24x24 (projector/builder.py:41-43)
    local_queries: int = 144        # mm_resampler_dim (scripts/llama/llama3_8b_sft.sh:46)
    ln_eps: float = 1e-6            # Resampler norm_layer eps (sampler.py:106)

    @property
    def num_heads(self) -> int:
        return self.mm_hidden_size // self.head_dim


ADAPTER_8B = AdapterConfig()
ADAPTER_TINY = AdapterConfig(mm_hidden_size=128, hidden_size=256)   # 1 head of 128 (reference: width // 128)


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return g


def _normal(g, shape, std, mean=0.0):
    return torch.randn(shape, generator=g, dtype=torch.float32) * std + mean


def make_tower_state_dict(cfg: VisionConfig = CLIP_L_336, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """fp32 state dict with transformers-4.37 key names (``vision_model.`` prefix)."""
    g = _gen(seed)
    D, F, P = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    sd: Dict[str, torch.Tensor] = {}
    p = "vision_model."
    sd[p + "embeddings.class_embedding"] = _normal(g, (D,), D ** -0.5)
    sd[p + "embeddings.patch_embedding.weight"] = _normal(g, (D, 3, P, P), 0.02)
    sd[p + "embeddings.position_embedding.weight"] = _normal(g, (cfg.seq_len, D), 0.02)
    sd[p + "pre_layrnorm.weight"] = _normal(g, (D,), 0.1, 1.0)   # sic: HF's typo is the real key
    sd[p + "pre_layrnorm.bias"] = _normal(g, (D,), 0.05)
    depth_scale = (2 * cfg.num_hidden_layers) ** -0.5
    for i in range(cfg.num_hidden_layers):
        q = f"{p}encoder.layers.{i}."
        sd[q + "layer_norm1.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "layer_norm1.bias"] = _normal(g, (D,), 0.05)
        for name, std in (("q_proj", D ** -0.5), ("k_proj", D ** -0.5),
                          ("v_proj", D ** -0.5), ("out_proj", D ** -0.5 * depth_scale * 2.0)):
            sd[q + f"self_attn.{name}.weight"] = _normal(g, (D, D), std)
            sd[q + f"self_attn.{name}.bias"] = _normal(g, (D,), 0.02)
        sd[q + "layer_norm2.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "layer_norm2.bias"] = _normal(g, (D,), 0.05)
        sd[q + "mlp.fc1.weight"] = _normal(g, (F, D), (2 * D) ** -0.5 * 2.0)
        sd[q + "mlp.fc1.bias"] = _normal(g, (F,), 0.02)
        sd[q + "mlp.fc2.weight"] = _normal(g, (D, F), F ** -0.5 * depth_scale * 2.0)
        sd[q + "mlp.fc2.bias"] = _normal(g, (D,), 0.02)
    sd[p + "post_layernorm.weight"] = _normal(g, (D,), 0.1, 1.0)
    sd[p + "post_layernorm.bias"] = _normal(g, (D,), 0.05)
    return sd


@dataclass(frozen=True)
class SiglipVisionConfig:
    """Geometry of a SigLIP vision tower (HF ``SiglipVisionConfig`` field names; defaults: siglip-large-patch16-384).  No class
    token: ``seq_len == num_patches``."""
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    image_size: int = 384
    patch_size: int = 16
    layer_norm_eps: float = 1e-6
    hidden_act: str = "gelu_pytorch_tanh"

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid * self.grid

    @property
    def seq_len(self) -> int:
        return self.num_patches

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    def to_dict(self):
        return asdict(self)


SIGLIP_L_384 = SiglipVisionConfig()
# the TINY tower's widths on a patch-16 grid of 24 x 24 (S = 576: the adapter's token grid)
SIGLIP_TINY = SiglipVisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2)


def make_siglip_state_dict(cfg: SiglipVisionConfig = SIGLIP_L_384, seed: int = 1234, head: bool = True) -> Dict[str, torch.Tensor]:
    """fp32 state dict with HF ``SiglipVisionModel`` key names (``vision_model.`` prefix, as make_tower_state_dict): a conv bias, a
    position table of P rows, no class embedding and no pre-LayerNorm; ``post_layernorm.*`` and (``head``) the pooling head
    ``head.*`` are part of a checkpoint and are never run here.  Scales as in :func:`make_tower_state_dict`."""
    g = _gen(seed)
    D, F, P = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    sd: Dict[str, torch.Tensor] = {}
    p = "vision_model."
    sd[p + "embeddings.patch_embedding.weight"] = _normal(g, (D, 3, P, P), 0.02)
    sd[p + "embeddings.patch_embedding.bias"] = _normal(g, (D,), 0.05)
    sd[p + "embeddings.position_embedding.weight"] = _normal(g, (cfg.num_patches, D), 0.02)
    depth_scale = (2 * cfg.num_hidden_layers) ** -0.5
    for i in range(cfg.num_hidden_layers):
        q = f"{p}encoder.layers.{i}."
        sd[q + "layer_norm1.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "layer_norm1.bias"] = _normal(g, (D,), 0.05)
        for name, std in (("q_proj", D ** -0.5), ("k_proj", D ** -0.5),
                          ("v_proj", D ** -0.5), ("out_proj", D ** -0.5 * depth_scale * 2.0)):
            sd[q + f"self_attn.{name}.weight"] = _normal(g, (D, D), std)
            sd[q + f"self_attn.{name}.bias"] = _normal(g, (D,), 0.02)
        sd[q + "layer_norm2.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "layer_norm2.bias"] = _normal(g, (D,), 0.05)
        sd[q + "mlp.fc1.weight"] = _normal(g, (F, D), (2 * D) ** -0.5 * 2.0)
        sd[q + "mlp.fc1.bias"] = _normal(g, (F,), 0.02)
        sd[q + "mlp.fc2.weight"] = _normal(g, (D, F), F ** -0.5 * depth_scale * 2.0)
        sd[q + "mlp.fc2.bias"] = _normal(g, (D,), 0.02)
    sd[p + "post_layernorm.weight"] = _normal(g, (D,), 0.1, 1.0)
    sd[p + "post_layernorm.bias"] = _normal(g, (D,), 0.05)
    if head:
        h = p + "head."
        sd[h + "probe"] = _normal(g, (1, 1, D), 0.02)
        sd[h + "attention.in_proj_weight"] = _normal(g, (3 * D, D), D ** -0.5)
        sd[h + "attention.in_proj_bias"] = _normal(g, (3 * D,), 0.02)
        sd[h + "attention.out_proj.weight"] = _normal(g, (D, D), D ** -0.5)
        sd[h + "attention.out_proj.bias"] = _normal(g, (D,), 0.02)
        sd[h + "layernorm.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[h + "layernorm.bias"] = _normal(g, (D,), 0.05)
        sd[h + "mlp.fc1.weight"] = _normal(g, (F, D), D ** -0.5)
        sd[h + "mlp.fc1.bias"] = _normal(g, (F,), 0.02)
        sd[h + "mlp.fc2.weight"] = _normal(g, (D, F), F ** -0.5)
        sd[h + "mlp.fc2.bias"] = _normal(g, (D,), 0.02)
    return sd


@dataclass(frozen=True)
class Dinov2VisionConfig:
    """Geometry of a DINOv2 vision tower (HF ``Dinov2Config`` / ``Dinov2WithRegistersConfig`` field names; defaults: ViT-L/14 without
    registers).  ``image_size`` is the size the tower RUNS at, as for every tower config of this package (224: the released
    checkpoints' ``crop_size``); ``table_grid`` is the grid the position table was made for (HF's ``image_size`` 518 / 14 = 37 in
    the released checkpoints): the table is interpolated to the run grid once, at pack time.  A crop is
    ``[cls] [num_register_tokens registers] [num_patches patches]``: ``n_prefix`` rows in front of the patches."""
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    mlp_ratio: int = 4
    image_size: int = 224
    patch_size: int = 14
    layer_norm_eps: float = 1e-6
    hidden_act: str = "gelu"
    table_grid: int = 37
    use_swiglu_ffn: bool = False
    num_register_tokens: int = 0
    model_type: str = "dinov2"            # or "dinov2_with_registers": HF interpolates the position table with antialias=True there

    @property
    def intermediate_size(self) -> int:
        return int(self.hidden_size * self.mlp_ratio)

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def num_patches(self) -> int:
        return self.grid * self.grid

    @property
    def n_prefix(self) -> int:
        return 1 + self.num_register_tokens

    @property
    def seq_len(self) -> int:
        return self.n_prefix + self.num_patches

    @property
    def head_dim(self) -> int:
        return self.hidden_size // self.num_attention_heads

    @property
    def antialias(self) -> bool:
        return self.model_type == "dinov2_with_registers"

    def to_dict(self):
        return asdict(self)


DINOV2_L_224 = Dinov2VisionConfig()
DINOV2_L_REG4_224 = Dinov2VisionConfig(num_register_tokens=4, model_type="dinov2_with_registers")


def make_dinov2_state_dict(cfg: Dinov2VisionConfig = DINOV2_L_224, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """fp32 state dict with HF ``Dinov2Model`` / ``Dinov2WithRegistersModel`` key names (no prefix, as HF saves them): class, mask
    and register tokens, a position table of 1 + table_grid^2 rows, a conv with bias, per layer norm1 / attention / LayerScale /
    norm2 / MLP / LayerScale, the final ``layernorm`` (part of a checkpoint, never run here).  Scales as in
    :func:`make_tower_state_dict`; the LayerScale lambdas are log-uniform in [1e-4, 1] (the released checkpoints train them from
    1.0 and reach both ends of that range)."""
    g = _gen(seed)
    D, F, P, R = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size, cfg.num_register_tokens
    sd: Dict[str, torch.Tensor] = {}
    e = "embeddings."
    sd[e + "cls_token"] = _normal(g, (1, 1, D), D ** -0.5)
    sd[e + "mask_token"] = _normal(g, (1, D), 0.02)
    if R > 0:
        sd[e + "register_tokens"] = _normal(g, (1, R, D), D ** -0.5)
    sd[e + "position_embeddings"] = _normal(g, (1, 1 + cfg.table_grid ** 2, D), 0.02)
    sd[e + "patch_embeddings.projection.weight"] = _normal(g, (D, 3, P, P), 0.02)
    sd[e + "patch_embeddings.projection.bias"] = _normal(g, (D,), 0.05)
    depth_scale = (2 * cfg.num_hidden_layers) ** -0.5

    def lam():
        return torch.exp(torch.rand((D,), generator=g, dtype=torch.float32) * math.log(1e-4))

    for i in range(cfg.num_hidden_layers):
        q = f"encoder.layer.{i}."
        sd[q + "norm1.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "norm1.bias"] = _normal(g, (D,), 0.05)
        for name, std in (("attention.attention.query", D ** -0.5), ("attention.attention.key", D ** -0.5),
                          ("attention.attention.value", D ** -0.5), ("attention.output.dense", D ** -0.5 * depth_scale * 2.0)):
            sd[q + f"{name}.weight"] = _normal(g, (D, D), std)
            sd[q + f"{name}.bias"] = _normal(g, (D,), 0.02)
        sd[q + "layer_scale1.lambda1"] = lam()
        sd[q + "norm2.weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[q + "norm2.bias"] = _normal(g, (D,), 0.05)
        sd[q + "mlp.fc1.weight"] = _normal(g, (F, D), (2 * D) ** -0.5 * 2.0)
        sd[q + "mlp.fc1.bias"] = _normal(g, (F,), 0.02)
        sd[q + "mlp.fc2.weight"] = _normal(g, (D, F), F ** -0.5 * depth_scale * 2.0)
        sd[q + "mlp.fc2.bias"] = _normal(g, (D,), 0.02)
        sd[q + "layer_scale2.lambda1"] = lam()
    sd["layernorm.weight"] = _normal(g, (D,), 0.1, 1.0)
    sd["layernorm.bias"] = _normal(g, (D,), 0.05)
    return sd


DINOV2_KEY_PREFIXES = ("dinov2_with_registers.", "dinov2.", "vision_model.", "backbone.")


def strip_dinov2_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """HF saves a bare ``Dinov2Model`` without a prefix; a model that wraps it (classification, backbone, this package's parameter
    container) prefixes every key with the attribute that holds it.  Both are accepted."""
    def bare(k: str) -> str:
        for p in DINOV2_KEY_PREFIXES:
            if k.startswith(p):
                return bare(k[len(p):])
        return k
    return {bare(k): v for k, v in sd.items()}


def canonical_tower_key(key: str) -> str:
    """Map either HF naming generation onto the prefix-free form used internally."""
    return key[len("vision_model."):] if key.startswith("vision_model.") else key


def strip_tower_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {canonical_tower_key(k): v for k, v in sd.items()}


# --- 2-D sin/cos position table of the Resampler (sampler.py:39-88), restated with numpy -----------

def sincos_pos_embed_2d(embed_dim: int, grid_size: int) -> np.ndarray:
    """[grid*grid, embed_dim] float64->float32 table; first half encodes the w index, second the h
    index (``np.meshgrid(grid_w, grid_h)`` puts w first, sampler.py:45-49)."""
    assert embed_dim % 4 == 0
    gh = np.arange(grid_size, dtype=np.float32)
    gw = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(gw, gh), axis=0).reshape(2, 1, grid_size, grid_size)

    def one_d(dim, pos):
        omega = np.arange(dim // 2, dtype=np.float32)
        omega /= dim / 2.0
        omega = 1.0 / 10000 ** omega
        out = np.einsum("m,d->md", pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)

    return np.concatenate([one_d(embed_dim // 2, grid[0]), one_d(embed_dim // 2, grid[1])], axis=1)


def _resampler_state(g, prefix: str, D: int, n_query_side: int) -> Dict[str, torch.Tensor]:
    nq = n_query_side * n_query_side
    sd = {}
    # pos_embed is an fp16 Parameter in the reference (sampler.py:115-117)
    sd[prefix + "pos_embed"] = torch.from_numpy(sincos_pos_embed_2d(D, n_query_side)).to(torch.float16)
    sd[prefix + "query"] = _normal(g, (nq, D), 0.5)
    sd[prefix + "attn.in_proj_weight"] = _normal(g, (3 * D, D), D ** -0.5)
    sd[prefix + "attn.in_proj_bias"] = _normal(g, (3 * D,), 0.02)
    sd[prefix + "attn.out_proj.weight"] = _normal(g, (D, D), D ** -0.5)
    sd[prefix + "attn.out_proj.bias"] = _normal(g, (D,), 0.02)
    for ln in ("ln_q", "ln_kv", "ln_post"):
        sd[prefix + ln + ".weight"] = _normal(g, (D,), 0.1, 1.0)
        sd[prefix + ln + ".bias"] = _normal(g, (D,), 0.05)
    return sd


def make_adapter_state_dict(cfg: AdapterConfig = ADAPTER_8B, seed: int = 4321) -> Dict[str, torch.Tensor]:
    """State dict for ``mm_projector`` (GatedBlock) and ``sampler`` (post_qformer), reference key names."""
    g = _gen(seed)
    D, H = cfg.mm_hidden_size, cfg.hidden_size
    sd: Dict[str, torch.Tensor] = {}
    sd["mm_projector.projection.0.weight"] = _normal(g, (H, D), D ** -0.5)
    sd["mm_projector.projection.0.bias"] = _normal(g, (H,), 0.02)
    sd["mm_projector.projection.2.weight"] = _normal(g, (H, H), H ** -0.5)
    sd["mm_projector.projection.2.bias"] = _normal(g, (H,), 0.02)
    sd.update(_resampler_state(g, "mm_projector.attn.", D, int(math.isqrt(cfg.global_queries))))
    # bf16 Parameters in the reference (projector/builder.py:63-64); w_noise is unused at inference
    sd["mm_projector.w_gate"] = _normal(g, (D, 2), 0.05).to(torch.bfloat16)
    sd["mm_projector.w_noise"] = torch.zeros(D, 2, dtype=torch.bfloat16)
    sd["mm_projector.mean"] = torch.tensor([0.0], dtype=torch.bfloat16)
    sd["mm_projector.std"] = torch.tensor([1.0], dtype=torch.bfloat16)
    sd.update(_resampler_state(g, "sampler.post_qformer.", D, int(math.isqrt(cfg.local_queries))))
    return sd


def make_router_attention_state_dict(H: int, seed: int = 2468) -> Dict[str, torch.Tensor]:
    """fp32 state dict of ``TextGuidedRouterAttention`` (resampler/builder.py:120-136; key names and shapes of the reference's
    ``selector``), seeded and NON-DEGENERATE: LayerNorm weights 1 + 0.1 n, matrices scaled by fan_in^-1/2 so that the logits vary
    (with the reference's 0.02 initialisation every score is 1 / T to six digits and a comparison shows nothing).  ``query`` and
    ``self_attn.*`` take no part in the forward pass; they are there so that a checkpoint loads under ``strict=True``."""
    g = _gen(seed)
    sd: Dict[str, torch.Tensor] = {"query": _normal(g, (1, H), 0.02)}
    for attn in ("self_attn", "cross_attn"):
        sd[f"{attn}.in_proj_weight"] = _normal(g, (3 * H, H), H ** -0.5)
        sd[f"{attn}.in_proj_bias"] = _normal(g, (3 * H,), 0.02)
        sd[f"{attn}.out_proj.weight"] = _normal(g, (H, H), H ** -0.5)
        sd[f"{attn}.out_proj.bias"] = _normal(g, (H,), 0.02)
    for ln in ("ln_q", "ln_kv", "ln_post"):
        sd[ln + ".weight"] = _normal(g, (H,), 0.1, 1.0)
        sd[ln + ".bias"] = _normal(g, (H,), 0.05)
    sd["prob_proj.0.weight"] = _normal(g, (H // 4, H), H ** -0.5)
    sd["prob_proj.0.bias"] = _normal(g, (H // 4,), 0.02)
    sd["prob_proj.2.weight"] = _normal(g, (1, H // 4), (H // 4) ** -0.5)
    sd["prob_proj.2.bias"] = _normal(g, (1,), 0.02)
    return sd


def sub_state(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """Entries under ``prefix`` with the prefix removed."""
    n = len(prefix)
    return {k[n:]: v for k, v in sd.items() if k.startswith(prefix)}


def synthetic_pixels(n_crops: int, seed: int = 0, image_size: int = 336) -> torch.Tensor:
    """N(0,1) ``pixel_values`` [n,3,S,S] fp32 (synthetic inputs)."""
    g = _gen(seed)
    return torch.randn((n_crops, 3, image_size, image_size), generator=g, dtype=torch.float32)
