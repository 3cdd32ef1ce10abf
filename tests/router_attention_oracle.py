"""float64 restatement of the attention text-guided router (``TextGuidedRouterAttention.forward``, llava/model/multimodal_resampler/
builder.py:149-162, eval path) and the bounds of the two row kernels it adds (``ln_gather_kernel``, ``router_prob_head_kernel``).
Plain module (no fixtures, not a conftest); pure torch, works on CPU and GPU tensors.  Used by test_router_attention_host.py and
test_gpu_router_attention.py.

The arithmetic.  H = hidden size, heads = H / 128, head_dim 128, LayerNorm eps 1e-5 (nn.LayerNorm's default).  Per image, x [T, H] the
merged local tokens, text [L, H], mask [L]:
    xq = ln_q(x);  tk = ln_kv(text)
    q = xq Wq^T + bq;  k = tk Wk^T + bk;  v = tk Wv^T + bv            (cross_attn.in_proj_weight rows [q; k; v])
    ctx = softmax over the keys with mask != 0 of (q k^T / sqrt(128)) v, per head
    y = ln_post(ctx Wo^T + bo);  logit = relu(y W1^T + b1) . w2 + b2;  scores = softmax(logit / temp) over the T tokens
``TextGuidedSampler.forward`` then applies softmax(scores / temp) again, sorts and cuts at top-p: oracle.slime_oracle.router_select.

The bounds extend part (A) of rowwise_conformance.py (same conventions: e = 2^-24, u = unit roundoff of T, sums of depth L carry
e L sum|terms|, a factor 1 + 2^-10 for second-order products, rsqrtf at A_RSQRT e relative).

(A') Gathered LayerNorm, ``ln_gather_kernel``: one wave per row, a lane adds its 4 ceil(D / 256) values in turn, then six butterfly
     levels: L = 4 ceil(D / 256) + 6.  The mean and the variance are DIVIDED by D (correctly rounded), where slime_layernorm
     multiplies by an exact 1 / D: for a D that is no power of two (5120) each division rounds once more, so
         d_mu  = e (L + 1) mean|x|                      (dx = 0: the kernel holds the fp32 row exactly)
         d_var = A + e (L + 4) (var + A) + e v          (one more e than (A) for the division; A from d_mu as in (A))
     and the rest is (A) unchanged.  ``ln_gather_bound`` evaluates (A) with L + 1: the extra e enters d_mu directly and d_var through
     the (L + 3) -> (L + 4) factor, which is what L + 1 gives.  out_t: round_T(y, dy).  The gather itself is exact (a copy).
(H)  Probability head: logit = b2 + sum_j relu(h_j) w2_j over N1 fp32 values.  relu is exact; each product is fused into the running
     sum (one rounding per fma), the chain is at most N1 / 64 deep per lane plus six butterfly levels, then one addition of b2:
         d_logit = e (N1 + 2) sum_j |relu(h_j) w2_j| + e |logit|
     (N1 + 2 is the loose form the issue states: depth N1 / 64 + 6 <= N1 + 2 for every N1 >= 128.)
(S)  Per-image softmax of n logits, score_i = expf(l_i / temp - m) / S with S the fp32 sum of the numerators (n / 256 values per
     thread, six butterfly levels, four partial sums).  The scores of a segment sum to (sum of the numerators) / S up to the n
     divisions' roundings: S carries (n / 256 + 8) e relative and every quotient e, so |sum - 1| <= (n / 256 + 9) e <= n e for the
     segments tested (n >= 12; n = 1 gives exactly 1).  The GPU test asserts n e, as the issue states it, summing in float64.
None of these constants was fitted to a kernel's output; test_router_attention_host.py checks that a torch fp32 emulation stays
inside each bound and that a broken variant (one-pass variance; dropped bias) leaves it.
"""
from __future__ import annotations

import math
import os
from typing import Dict, Optional

import numpy as np
import torch

import rowwise_conformance as RC
from rowwise_conformance import E32, SLACK, round_T   # noqa: F401

EPS = 1e-5
HEAD_DIM = 128


# ================================================================================================ the recorded reference
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "router_attention.npz")


def golden():
    return np.load(GOLDEN)


def golden_case(g, name):
    bf = lambda a: torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float()
    H = int(g[f"{name}.H"])
    from slime_amd import weights as W
    return dict(H=H, sd=W.make_router_attention_state_dict(H, seed=int(g[f"{name}.seed"])), x=bf(g[f"{name}.x_bf16"]),
                text=bf(g[f"{name}.text_bf16"]), mask=torch.from_numpy(g[f"{name}.mask"]), logit=torch.from_numpy(g[f"{name}.logit"]),
                scores=torch.from_numpy(g[f"{name}.scores"]), kept=torch.from_numpy(g[f"{name}.kept"]),
                drift={t: tuple(float(v) for v in g[f"{name}.drift_{t}"]) for t in ("bf16", "fp16")})


CASES = ("h256_t288", "h256_single_key", "h512_left_pad")


# ================================================================================================ the float64 oracle
def _ln(x, w, b, eps=EPS):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + eps) * w + b


def _f64(sd: Dict[str, torch.Tensor], key: str, dev) -> torch.Tensor:
    return sd[key].detach().to(device=dev).double()


def stages(sd, x, text, mask=None, operand_dtype: Optional[torch.dtype] = None) -> Dict[str, torch.Tensor]:
    """Every stage of the router in float64.  ``operand_dtype``: the four GEMM weights (and only they) are rounded to that 16-bit type first
    -- the oracle "on the T-rounded operands" of the real-width GPU test; None: the weights as they are."""
    dev = x.device
    H = x.shape[-1]
    heads = H // HEAD_DIM
    g = lambda k: _f64(sd, k, dev)
    gw = (lambda k: sd[k].detach().to(device=dev).float().to(operand_dtype).double()) if operand_dtype is not None else g
    x, text = x.double(), text.double()
    valid = torch.ones(text.shape[0], dtype=torch.bool, device=dev) if mask is None else mask.to(dev).ne(0)
    xq = _ln(x, g("ln_q.weight"), g("ln_q.bias"))
    tk = _ln(text[valid], g("ln_kv.weight"), g("ln_kv.bias"))
    in_w, in_b = gw("cross_attn.in_proj_weight"), g("cross_attn.in_proj_bias")
    q = xq @ in_w[:H].T + in_b[:H]
    k = tk @ in_w[H:2 * H].T + in_b[H:2 * H]
    v = tk @ in_w[2 * H:].T + in_b[2 * H:]
    T, Lv = q.shape[0], k.shape[0]
    qh, kh, vh = (t.view(-1, heads, HEAD_DIM).transpose(0, 1) for t in (q, k, v))
    att = torch.softmax(qh @ kh.transpose(1, 2) / math.sqrt(HEAD_DIM), dim=-1)            # [heads, T, Lv]
    ctx = (att @ vh).transpose(0, 1).reshape(T, H)
    o = ctx @ gw("cross_attn.out_proj.weight").T + g("cross_attn.out_proj.bias")
    y = _ln(o, g("ln_post.weight"), g("ln_post.bias"))
    h = y @ gw("prob_proj.0.weight").T + g("prob_proj.0.bias")
    logit = torch.relu(h) @ g("prob_proj.2.weight").view(-1) + g("prob_proj.2.bias").view(())      # w2 stays fp32: no MFMA operand
    return {"xq": xq, "tk": tk, "q": q, "k": k, "v": v, "ctx": ctx, "o": o, "y": y, "h": h, "logit": logit, "n_keys": Lv}


def logits(sd, x, text, mask=None, operand_dtype=None) -> torch.Tensor:
    return stages(sd, x, text, mask, operand_dtype)["logit"]


def scores(sd, x, text, mask=None, temp: float = 1.0, operand_dtype=None) -> torch.Tensor:
    """What ``TextGuidedRouterAttention.forward`` returns: softmax(logit / temp) over the T tokens, float64."""
    return torch.softmax(logits(sd, x, text, mask, operand_dtype) / temp, dim=-1)


def select(scores_: torch.Tensor, topp: float, temp: float) -> torch.Tensor:
    """``TextGuidedSampler.forward`` on the selector's output (oracle.slime_oracle.router_select: the second softmax / temp, sort,
    cumulative sum <= top-p plus one, ascending)."""
    from oracle import slime_oracle as O
    return O.router_select(scores_, topp, temp)


def select_device_order(scores_: torch.Tensor, topp: float, temp: float) -> torch.Tensor:
    """``select`` with equal probabilities ordered by ascending index -- the order ``router_select_kernel`` documents ("ties by
    ascending index") and rowwise_conformance.router_expected pins.  torch.sort(descending=True) without ``stable`` leaves the order
    of equal keys to the implementation, so on tied scores (one valid key: every token gets the same score) the reference's own kept
    set is not a specification.  Without ties this IS oracle.slime_oracle.router_select, which is asserted here."""
    from oracle import slime_oracle as O
    probs = torch.softmax(scores_ / temp, dim=-1)
    sp, si = torch.sort(probs, descending=True, stable=True)
    k = int((torch.cumsum(sp, 0) <= topp).sum())
    kept = (si[:k + 1] if k < probs.numel() else si).sort()[0]
    if torch.unique(probs).numel() == probs.numel():
        assert torch.equal(kept, O.router_select(scores_, topp, temp))
    return kept


def rel_l2(a, b) -> float:
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm())


def max_abs(a, b) -> float:
    return float((a.double().cpu().reshape(-1) - b.double().cpu().reshape(-1)).abs().max())


# ================================================================================================ (A') gathered LayerNorm
def ln_gather_depth(D: int) -> int:
    return 4 * ((D + 255) // 256) + 6


def ln_gather_bound(x, w, b, dtype, eps: float = EPS):
    """x [rows, D] float64 (the gathered rows) -> (y, bound of the T output), float64.  Part (A) with the kernel's own depth and the
    extra e of the divisions by D (module docstring)."""
    y, dy = RC.ln_bound(x, 0.0, ln_gather_depth(x.shape[-1]) + 1, w.double(), b.double(), eps)
    return y, round_T(y, dy, dtype)


def emulate_ln_gather(src, idx, w, b, dtype, eps: float = EPS, one_pass: bool = False) -> torch.Tensor:
    """``ln_gather_kernel`` in torch fp32: gather, mean = sum / D, two-pass variance / D, rsqrt, (d rstd) w + b, T."""
    x = src.float()[idx] if idx is not None else src.float()
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    d = x - mean
    var = ((x * x).sum(-1, keepdim=True) / D - mean * mean).clamp_min(0.0) if one_pass else (d * d).sum(-1, keepdim=True) / D
    return ((d * torch.rsqrt(var + eps)) * w.float() + b.float()).to(dtype)


def ln_gather_inputs(D: int, rows: int = 37, seed: int = 0, device="cpu"):
    """(src [rows, D] fp32, idx int64, w, b): random rows 3 n + 0.7, row 5 with |mean| = 1000 sigma, an ``idx`` that repeats,
    reverses and skips source rows (longer than the source)."""
    g = torch.Generator(device="cpu").manual_seed(6151 * seed + D)
    src = 3.0 * torch.randn(rows, D, generator=g) + 0.7
    src[5] = torch.randn(D, generator=g) + 1000.0
    idx = torch.cat([torch.arange(rows - 1, -1, -2), torch.tensor([5, 5, 0, rows - 1, 5]), torch.arange(1, rows, 3), torch.arange(0, rows, 2)]).long()
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    return src.to(device), idx.to(device), w.to(device), b.to(device)


# ================================================================================================ (H) probability head, (S) softmax
def head_bound(h, w2, b2: float):
    """h [rows, N1], w2 [N1] -> (logit, bound), float64: term (H)."""
    h, w2 = h.double(), w2.double()
    terms = torch.relu(h) * w2
    logit = terms.sum(-1) + b2
    return logit, (E32 * (h.shape[-1] + 2) * terms.abs().sum(-1) + E32 * logit.abs()) * SLACK


def emulate_head(h, w2, b2: float, drop_bias: bool = False) -> torch.Tensor:
    """``router_prob_head_kernel`` in torch fp32."""
    s = (torch.relu(h.float()) * w2.float()).sum(-1)
    return s if drop_bias else s + torch.tensor(b2, dtype=torch.float32, device=h.device)


def head_inputs(N1: int, rows: int, seed: int = 0, device="cpu"):
    g = torch.Generator(device="cpu").manual_seed(7723 * seed + N1 + rows)
    h = torch.randn(rows, N1, generator=g)
    w2 = torch.randn(N1, generator=g) * N1 ** -0.5
    return h.to(device), w2.to(device), 0.37


def segment_softmax(logit, n_rows, temp: float):
    """float64 softmax(logit / temp) of every segment -> list of tensors (an empty tensor for an empty segment)."""
    out, o = [], 0
    for n in n_rows:
        out.append(torch.softmax(logit[o:o + n].double() / temp, dim=-1))
        o += n
    return out
