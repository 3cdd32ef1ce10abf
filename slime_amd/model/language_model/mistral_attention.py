"""Mistral / Mixtral prefill self-attention on the HIP path: the language models of llava/model/language_model/llava_mistral.py
and llava_mixtral.py.

``MistralAttention`` and ``MixtralAttention`` are LlamaAttention (no projection biases, head_dim 128, default rotary embedding,
grouped-query heads) with one difference: ``config.sliding_window = W`` lets query row i see key row j only if ``i - j < W``.
``replace_mistral_attn_with_hip_attn`` / ``replace_mixtral_attn_with_hip_attn`` patch the installed transformers the way
``replace_llama_attn_with_hip_attn`` does (same helper functions, llama_attention.py) and call
``ops.llama_attention_forward_window`` (``slime_llama_attn_forward_window``: q/k/v projection GEMM, RoPE, sliding-window causal
GQA attention over the un-padded tokens, o_proj GEMM) with ``window = config.sliding_window`` (None -> 0: plain causal, the Llama
launches).  Mixtral's sparse MoE block stays HF's.  ``HipMistralAttention`` is the standalone module form.  Prefill only.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ... import ops
from .llama_attention import (HipLlamaAttention, _install_patch, _patched_forward, _restore_patch, _self_attn_return_arity)

MISTRAL_ROPE_THETA = 10000.0            # MistralConfig's default (Mistral-7B-v0.1; v0.2 and Mixtral-8x7B set 1e6)


def _window(sliding_window) -> int:
    """``config.sliding_window`` -> the C ABI's ``window`` (None: 0, no window)."""
    if sliding_window is None:
        return 0
    w = int(sliding_window)
    if w < 1:
        raise ValueError(f"sliding_window must be None or >= 1, got {sliding_window!r}")
    return w


class HipMistralAttention(HipLlamaAttention):
    """``HipLlamaAttention`` (HF parameter names ``q_proj`` / ``k_proj`` / ``v_proj`` / ``o_proj``, no biases) with
    ``sliding_window=None | int``."""

    def __init__(self, hidden_size: int = 4096, num_heads: int = 32, num_key_value_heads: int = 8, head_dim: int = 128,
                 rope_theta: float = MISTRAL_ROPE_THETA, sliding_window: Optional[int] = None,
                 compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__(hidden_size, num_heads, num_key_value_heads, head_dim, rope_theta, compute_dtype)
        self.sliding_window = sliding_window
        _window(sliding_window)

    @torch.no_grad()
    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                position_ids: Optional[torch.Tensor] = None, past_key_value=None, output_attentions: bool = False,
                use_cache: bool = False, past_key_values=None, **_):
        """``attention_mask`` is the [B, S] key-padding mask; returns (output, None, None) as ``HipLlamaAttention`` does."""
        if past_key_value is not None or past_key_values is not None or use_cache:
            raise NotImplementedError("HipMistralAttention implements the prefill pass (no KV cache)")
        if output_attentions:
            raise NotImplementedError("the fused prefill attention never materialises the attention weights")
        dt = hidden_states.dtype if hidden_states.dtype in (torch.bfloat16, torch.float16) else self.compute_dtype
        out = ops.llama_attention_forward_window(self.packed(dt), hidden_states, position_ids, attention_mask, hidden_states.dtype,
                                                 _window(self.sliding_window))
        return out, None, None


def _attend(attn, packed, hidden_states, position_ids, attention_mask):
    return ops.llama_attention_forward_window(packed, hidden_states, position_ids, attention_mask, hidden_states.dtype,
                                              _window(getattr(attn.config, "sliding_window", None)))


_FAMILIES = {"mistral": ("MistralAttention", "MistralModel", "MistralDecoderLayer"),
             "mixtral": ("MixtralAttention", "MixtralModel", "MixtralDecoderLayer")}
_PATCH_STATE: Dict[str, Dict[str, object]] = {"mistral": {}, "mixtral": {}}


def _module(family: str):
    import importlib
    return importlib.import_module(f"transformers.models.{family}.modeling_{family}")


def _replace(family: str):
    import transformers
    M = _module(family)
    attn, model, layer = _FAMILIES[family]
    state = _PATCH_STATE[family]
    stock = state.get("forward", getattr(M, attn).forward)
    forward = _patched_forward(attn, stock, _self_attn_return_arity(M, layer), _attend, MISTRAL_ROPE_THETA)
    _install_patch(state, M, getattr(M, attn), getattr(M, model), forward)
    return transformers


def _restore(family: str) -> None:
    if not _PATCH_STATE[family]:
        return
    M = _module(family)
    attn, model, _ = _FAMILIES[family]
    _restore_patch(_PATCH_STATE[family], M, getattr(M, attn), getattr(M, model))


def replace_mistral_attn_with_hip_attn():
    """Patch HF ``MistralAttention.forward`` (and the mask builders ``modeling_mistral`` looks up: ``create_causal_mask`` and
    ``create_sliding_window_causal_mask`` where the installed version has them) -- see ``replace_llama_attn_with_hip_attn``.  The window
    is ``config.sliding_window``.  Returns the ``transformers`` module; ``restore_mistral_attn()`` undoes the patch."""
    return _replace("mistral")


def restore_mistral_attn():
    _restore("mistral")


def replace_mixtral_attn_with_hip_attn():
    """The same for ``MixtralAttention.forward`` / ``modeling_mixtral``; the sparse MoE block is untouched.
    ``restore_mixtral_attn()`` undoes the patch."""
    return _replace("mixtral")


def restore_mixtral_attn():
    _restore("mixtral")
