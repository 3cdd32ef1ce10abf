"""``build_vision_sampler`` and ``TextGuidedSampler`` (llava/model/multimodal_resampler/builder.py:222-302).

``TextGuidedSampler`` owns ``post_qformer`` (the 144-query local compression ``Resampler``) and the
text-guided top-p router over the merged local tokens.  Both routers of the reference are implemented:
``mm_resampler_type='cosine'`` (the released configuration: scripts/llama/llama3_8b_sft.sh:43) and 'qformer', the attention
router ``TextGuidedRouterAttention`` (:94-162).  They differ in the scores only; the selection, the ``ops.RouterState`` it
leaves on the device and the splice that reads it are shared.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn

from .sampler import IdentityMap, Resampler
from ... import ops


class TextGuidedRouterAttention(nn.Module):
    """The attention router's parameters (resampler/builder.py:101-136: the reference's state-dict keys and shapes, so that a
    ``sampler.bin`` trained with ``--mm_resampler_type qformer`` loads under ``strict=True``) and their packed form.  The two
    ``nn.MultiheadAttention`` modules are parameter containers: the arithmetic runs in ``ops.router_attention_scores`` (eval
    path; ``query`` and ``self_attn`` take no part in it, as in the reference's forward)."""

    def __init__(self, grid_size, embed_dim, num_heads, kv_dim=None, temp=1.0):
        super().__init__()
        if kv_dim is not None and kv_dim != embed_dim:
            raise NotImplementedError("attention router: kv_dim != embed_dim (a kv_proj) is not built by TextGuidedSampler")
        self.num_queries = 1
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.temp = temp
        self.query = nn.Parameter(torch.zeros(self.num_queries, embed_dim))
        nn.init.trunc_normal_(self.query, std=.02)
        self.self_attn = nn.MultiheadAttention(embed_dim, num_heads, batch_first=False)
        self.cross_attn = nn.MultiheadAttention(embed_dim, num_heads, batch_first=False)
        self.ln_q = nn.LayerNorm(embed_dim)
        self.ln_kv = nn.LayerNorm(embed_dim)
        self.ln_post = nn.LayerNorm(embed_dim)
        self.prob_proj = nn.Sequential(nn.Linear(embed_dim, embed_dim // 4), nn.ReLU(), nn.Linear(embed_dim // 4, 1))
        self._packed: Dict = {}

    def _apply(self, fn, *a, **kw):
        self._packed.clear()
        return super()._apply(fn, *a, **kw)

    def _load_from_state_dict(self, *a, **kw):
        self._packed.clear()
        return super()._load_from_state_dict(*a, **kw)

    def operand_dtype(self) -> torch.dtype:
        wd = self.query.dtype
        return wd if wd in (torch.bfloat16, torch.float16) else torch.bfloat16

    def packed(self, dtype: torch.dtype) -> ops.PackedRouterAttention:
        key = (dtype, str(self.query.device))
        if key not in self._packed:
            self._packed[key] = ops.pack_router_attention(self.state_dict(), self.embed_dim, dtype, self.query.device)
        return self._packed[key]


class TextGuidedSampler(nn.Module):
    def __init__(self, projector_type, config):
        super().__init__()
        if projector_type not in ("cosine", "qformer"):
            raise NotImplementedError(f"mm_resampler_type={projector_type!r}: the routers are 'cosine' and 'qformer'")
        self.router_type = projector_type
        self.num_queries = config.mm_resampler_dim
        self.topp = config.mm_resampler_topp
        self.temp = config.mm_resampler_temp
        self.grid_size = int(math.sqrt(self.num_queries))
        if projector_type == "qformer":
            if config.hidden_size % 128 != 0 or config.hidden_size > ops.ROUTER_ATTN_MAX_H:
                raise ValueError(f"mm_resampler_type='qformer': hidden_size={config.hidden_size} must be a multiple of 128 "
                                 f"(heads of 128) up to {ops.ROUTER_ATTN_MAX_H}")
            self.selector = TextGuidedRouterAttention(grid_size=1, embed_dim=config.hidden_size,
                                                      num_heads=config.hidden_size // 128, temp=self.temp)
        self.post_qformer = Resampler(grid_size=self.grid_size, embed_dim=config.mm_hidden_size,
                                      num_heads=config.mm_hidden_size // 128, kv_dim=config.mm_hidden_size,
                                      llm_hidden_size=config.hidden_size)

    def _pra(self, operand_dtype: Optional[torch.dtype]) -> ops.PackedRouterAttention:
        return self.selector.packed(operand_dtype or self.selector.operand_dtype())

    @torch.no_grad()
    def forward(self, local_f, text_embedding, attn_mask=None, operand_dtype: Optional[torch.dtype] = None):
        """local_f [T, H], text_embedding [L, H], attn_mask [L] -> kept rows of local_f in ascending
        order (resampler/builder.py:248-281, eval path).  ``operand_dtype`` (extension, attention router only): the 16-bit MFMA
        operand type; default the selector weights' 16-bit type, else bf16."""
        if self.router_type == "cosine":
            keep = ops.router_topp(local_f, text_embedding, attn_mask, float(self.topp), float(self.temp))
            return local_f[keep]
        if local_f.shape[0] == 0:
            return local_f
        x = local_f.float().contiguous()
        st = ops.router_attention_select_batched_device(self._pra(operand_dtype), x, [0], [x.shape[0]], text_embedding.unsqueeze(0),
                                                        None if attn_mask is None else attn_mask.unsqueeze(0), float(self.topp),
                                                        float(self.temp))
        return local_f[st.keep[0, :st.counts[0]].long()]

    @torch.no_grad()
    def select_batched(self, tokens, row_off, n_rows, text_embedding, attn_mask=None, operand_dtype: Optional[torch.dtype] = None):
        """Router for all images of a step at once (ops.router_topp_batched: one launch pair, one D2H): per image the kept
        local-token indices, ascending.  Same per-image arithmetic as ``forward``."""
        if self.router_type == "cosine":
            return ops.router_topp_batched(tokens, row_off, n_rows, text_embedding, attn_mask, float(self.topp), float(self.temp))
        st = self.select_batched_device(tokens, row_off, n_rows, text_embedding, attn_mask, operand_dtype)
        return [st.keep[b, :st.counts[b]].long() for b in range(len(n_rows))]

    @torch.no_grad()
    def select_batched_device(self, tokens, row_off, n_rows, text_embedding, attn_mask=None, operand_dtype: Optional[torch.dtype] = None):
        """``select_batched`` with the kept indices left on the device (``ops.RouterState``; its ``counts`` are on the host)."""
        if self.router_type == "cosine":
            return ops.router_select_batched_device(tokens, row_off, n_rows, text_embedding, attn_mask, float(self.topp), float(self.temp))
        return ops.router_attention_select_batched_device(self._pra(operand_dtype), tokens, row_off, n_rows, text_embedding, attn_mask,
                                                          float(self.topp), float(self.temp))


def build_vision_sampler(config, delay_load=False, **kwargs):
    mm_resampler_type = getattr(config, "mm_resampler_type", None)
    if mm_resampler_type == "identity" or mm_resampler_type is None:
        return IdentityMap()
    return TextGuidedSampler(mm_resampler_type, config)
