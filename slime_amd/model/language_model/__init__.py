from .llama_attention import HipLlamaAttention, replace_llama_attn_with_hip_attn  # noqa: F401
from .mistral_attention import (HipMistralAttention, replace_mistral_attn_with_hip_attn, replace_mixtral_attn_with_hip_attn,  # noqa: F401
                                restore_mistral_attn, restore_mixtral_attn)
