"""Towers with the erf GELU (HF ``hidden_act='gelu'``: the OpenCLIP family) and width 768: what their tests share.  Plain module
(no fixtures, not a conftest); importable without a GPU and without the HIP library.

It restates what it needs NEXT TO tests/gemm_conformance.py and tests/tower_conformance.py and never writes into their tables
(``FORMS``, ``WAVE_FORMS``, ... are read by other test modules at collection):

  * the GEMM form ``fold_gelu_t`` -- the LayerNorm-fold consumer (term (6) of gemm_conformance's bound) followed by the erf GELU
    (term (4)) and one RNE to T (term (2)): its case (the buffers of ``fold_quickgelu_t`` under the epilogue SLIME_EPI_BIAS_GELU_T),
    float64 reference, per-element bound, fp32 emulation and three wrong variants of that emulation;
  * the yardstick of the tower: HF ``CLIPVisionModel(CLIPVisionConfig(..., hidden_act=...))`` built from a config (no download),
    fp32 or float64 on the CPU, ``output_hidden_states=True``, loaded with ``weights.make_tower_state_dict``;
  * the two replay backends of tower_conformance with fc1's epilogue taken from the activation (``replay_vit`` itself is used as it
    is: it asks the backend for fc1 by name);
  * ``tower_error_bound``: tower_conformance's float64 forward-error bound with the erf GELU's derivative and rounding in place of
    the quick-GELU's.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
from typing import Dict, Optional

import torch

import gemm_conformance as GC
import tower_conformance as TC

FORM = "fold_gelu_t"
ACTS = ("quick_gelu", "gelu")
TILES = (3, 15, 18, 4, 10, 11, 12)                        # every kernel family launch_epi can pick (gemm_conformance.TILE_FAMILY)
FOLD_K = (64, 192, 2112)                                   # one k-tile, fewer k-tiles than ring stages, both sides of KTAG / long K
VARIANTS = ("quickgelu", "gelu_before_fold", "no_mu_colsum")


# ------------------------------------------------------------------------------------------------ the GEMM form
class FoldGeluCase(GC.Case):
    """A gemm_conformance.Case whose epilogue / fold do not come from the FORMS table: BIAS_GELU_T with ln_stats."""

    @property
    def epilogue(self):
        return GC.EPI_BIAS_GELU_T

    @property
    def fold(self):
        return True


def fold_n(tile: int):
    """The two N of a family's walk: 256 and the next width its tile allows (384 for the 128- and 64-wide tiles, 512 for 256)."""
    return (256, 384 if 384 in GC.TILE_N[tile] else 512)


def make_case(kind: str, dtype, M: int, N: int, K: int, **kw) -> FoldGeluCase:
    """The padded, poisoned buffers gemm_conformance.make_case builds for ``fold_quickgelu_t`` (un-normalised rows with a mean, one
    row at |mu| = 10 sigma, statistics and colsum of the operands as they are), under the form ``fold_gelu_t``."""
    c = GC.make_case(kind, dtype, "fold_quickgelu_t", M, N, K, **kw)
    f = FoldGeluCase(**{fl.name: getattr(c, fl.name) for fl in dataclasses.fields(c)})
    f.form = FORM
    return f


def reference(c: FoldGeluCase) -> GC.Ref:
    """float64: gemm_conformance.reference gives the folded pre-activation x and its bound dx (term (6)); out = GELU(x)."""
    r = GC.reference(c)
    assert r.x is not None and torch.equal(r.out, r.x), "the base module knows this form now: use its reference"
    r.out = GC._gelu64(r.x)
    return r


def bound(c: FoldGeluCase, r: GC.Ref) -> torch.Tensor:
    """Terms (6) -> (4) -> (2): the fold's dx through the erf GELU (its derivative, the A-S form's absolute error, the fp32
    evaluation), then one RNE to T.  Exactly what ``gelu_t`` gets from gemm_conformance.bound, with the fold's dx."""
    return GC._round_T(r.out, GC._d_gelu(r.x, r.dx), c.dtype)


def check(c: FoldGeluCase, r: GC.Ref, outs: Dict[str, torch.Tensor], bm: int = 128):
    """(worst |err| / bound, message or None) of the C window."""
    bd = bound(c, r)
    ratio, ex, *_ = GC.worst(outs["C"], r.out, bd)
    return ratio, (None if ex <= 0 else GC.describe_failure(FORM, outs["C"], r.out, bd, bm))


def emulate(c: FoldGeluCase, variant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The kernel's arithmetic in torch fp32 (gemm_conformance.emulate's fold branch with ``gelu_erf``), or one wrong variant:
    "quickgelu"        x sigmoid(1.702 x) on the folded pre-activation (the tower's other activation);
    "gelu_before_fold" the GELU on the accumulator, the fold's affine map after it;
    "no_mu_colsum"     rstd acc + bias: the mean term of the fold left out."""
    assert variant is None or variant in VARIANTS
    b, M, N, K = c.buf, c.M, c.N, c.K
    dev = b["A"].win.device
    Aw, Bw = b["A"].win.float(), b["B"].win.float()
    acc = torch.zeros((M, N), dtype=torch.float32, device=dev)
    for k0 in range(0, K, 32):
        acc = acc + Aw[:, k0:k0 + 32] @ Bw[:, k0:k0 + 32].T
    bias = (b["bias"].win.view(-1) if c.has_bias else torch.zeros(N, device=dev)).view(1, N)
    st = b["ln_stats"].win.view(M, K // 64, 2)
    sx, sq = torch.zeros(M, device=dev), torch.zeros(M, device=dev)
    for i in range(K // 64):
        sx, sq = sx + st[:, i, 0], sq + st[:, i, 1]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    mu = sx * inv
    rstd = torch.rsqrt((sq * inv - mu * mu).clamp_min(0.0) + c.ln_eps)
    shift = (-mu * rstd)[:, None] * b["colsum"].win.view(1, N) + bias
    if variant == "no_mu_colsum":
        shift = bias.expand(M, N)
    if variant == "gelu_before_fold":
        y = rstd[:, None] * GC._gelu_erf32(acc) + shift
    else:
        x = rstd[:, None] * acc + shift
        if variant == "quickgelu":
            cc = torch.tensor(-1.702, dtype=torch.float32) * torch.tensor(GC.LOG2E, dtype=torch.float32)
            y = x * (1.0 / (1.0 + torch.exp2(cc.to(dev) * x)))
        else:
            y = GC._gelu_erf32(x)
    outs = c.windows()
    outs["C"] = y.to(c.dtype)
    return outs


# ------------------------------------------------------------------------------------------------ the HF yardstick
def vision_config(image: int, patch: int, D: int, inter: int, layers: int, act: str = "gelu"):
    from slime_amd.weights import VisionConfig
    assert D % 64 == 0 and act in ACTS
    return VisionConfig(hidden_size=D, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=D // 64, image_size=image,
                        patch_size=patch, hidden_act=act)


def hf_config_dict(cfg) -> dict:
    return dict(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
                num_attention_heads=cfg.num_attention_heads, image_size=cfg.image_size, patch_size=cfg.patch_size,
                layer_norm_eps=cfg.layer_norm_eps, hidden_act=cfg.hidden_act)


def hf_model(cfg, sd, dtype=torch.float32):
    """HF CLIPVisionModel from a config, weights from ``sd`` (make_tower_state_dict's keys): every parameter must be given, no key
    may be left over (HF's own position_ids buffer aside)."""
    from transformers import CLIPVisionConfig, CLIPVisionModel
    from slime_amd.weights import strip_tower_prefix
    m = CLIPVisionModel(CLIPVisionConfig(**hf_config_dict(cfg))).eval()
    if not any(k.startswith("vision_model.") for k in m.state_dict()):          # transformers 5.x dropped the prefix (weights.py)
        sd = strip_tower_prefix(sd)
    res = m.load_state_dict(sd, strict=False)
    missing = [k for k in res.missing_keys if "position_ids" not in k]
    assert not missing and not res.unexpected_keys, (missing[:3], res.unexpected_keys[:3])
    return m.to(dtype)


def hf_states(cfg, sd, pixels, dtype=torch.float32):
    """hidden_states of HF's forward with output_hidden_states=True: L + 1 tensors [n, S, D] of ``dtype``, on the CPU."""
    m = hf_model(cfg, sd, dtype)
    with torch.no_grad():
        out = m(pixel_values=pixels.to(dtype), output_hidden_states=True)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    return [h.detach() for h in out.hidden_states]


def write_hf_dir(path, sd, cfg, nested_config: bool = False, hidden_act: Optional[str] = None) -> str:
    """A CLIP directory as CLIPVisionTower.load_model reads it: config.json (flat, or under ``vision_config``), model.safetensors,
    preprocessor_config.json of the tower's image size."""
    from safetensors.torch import save_file
    v = hf_config_dict(cfg)
    if hidden_act is not None:
        v["hidden_act"] = hidden_act
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "clip", "vision_config": v, "text_config": {"hidden_size": 8}} if nested_config else
                  dict(v, model_type="clip_vision_model"), f)
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(path, "model.safetensors"))
    s = cfg.image_size
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"crop_size": {"height": s, "width": s}, "size": {"shortest_edge": s}, "do_normalize": True,
                   "image_mean": [0.48145466, 0.4578275, 0.40821073], "image_std": [0.26862954, 0.26130258, 0.27577711],
                   "rescale_factor": 1 / 255, "resample": 3}, f)
    return str(path)


def rel_l2(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_token(a, b) -> float:
    """Largest per-token rel-L2 ([.., D] rows)."""
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)).max())


# ------------------------------------------------------------------------------------------------ replay backends
def fc1_epilogue(act: str) -> int:
    return {"quick_gelu": GC.EPI_BIAS_QUICKGELU_T, "gelu": GC.EPI_BIAS_GELU_T}[act]


class TorchBackend(TC.TorchBackend):
    """tower_conformance.TorchBackend with fc1's activation taken from ``act``."""

    def __init__(self, dtype=None, act: str = "gelu"):
        super().__init__(dtype)
        self.act = act

    def gemm_fold(self, A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits=1):
        if name != "w_fc1" or self.act != "gelu":
            return super().gemm_fold(A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits)
        w = TC._flat(T[name], w_off, N * K).view(N, K).double()
        bias = TC._flat(T["b_fc1"], b_off, N).double()
        cs = TC._flat(T[colsum_name], b_off, N).double()
        st = stats.reshape(A.shape[0], -1, 2)
        mu = st[..., 0].sum(1, keepdim=True) / K
        var = st[..., 1].sum(1, keepdim=True) / K - mu * mu
        y = (A.double() @ w.t() - mu * cs) / torch.sqrt(var + eps) + bias
        return self._t(GC._gelu64(y))


class HipBackend(TC.HipBackend):
    """tower_conformance.HipBackend with fc1's epilogue taken from ``act`` (SLIME_EPI_BIAS_GELU_T with ln_stats for 'gelu')."""

    def __init__(self, dtype, device, act: str = "gelu"):
        super().__init__(dtype, device)
        self.act = act

    def gemm_fold(self, A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits=1):
        if name == "w_fc1":
            epilogue = fc1_epilogue(self.act)
        return super().gemm_fold(A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits)


# ------------------------------------------------------------------------------------------------ float64 forward-error bound
GELU_LIPSCHITZ = 1.13


def tower_error_bound(sd, T, cfg, pixels, layers_run: int, u_ref: float = TC.U64, states=None):
    """tower_conformance.tower_error_bound for a tower whose MLP activation is the erf GELU y = x Phi(x): the same two running
    bounds (the replay's at 2^-53 with both LayerNorms folded, the reference's at u_ref by two passes), carried through the same
    float64 values, with the activation's two constants derived for this function instead of the quick-GELU:
      * an input error passes with max |y'|, y' = Phi(x) + x phi(x); y'' = (2 - x^2) phi(x) vanishes at x = sqrt 2, where
        y' = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 0.92135 + 0.20755 = 1.1289 <= 1.13 (quick-GELU: 1.0998 <= 1.1);
      * its own rounding, as 0.5 x (1 + erf(x / sqrt 2)) (ATen's and this module's form): the argument's two roundings move erf by
        at most 2 u |t| erf'(t) <= u; erf itself within 4 ulp, |erf| <= 1; the sum 1 + erf rounds by u |1 + erf| <= 2 u -- 7 u on the
        bracket, absolute, hence 3.5 u |x| on the product -- and the two products add 2 u |y| <= 2 u |x|: 5.5 u |x| <= 8 u |x|, the
        weight tower_conformance gives the quick-GELU's five operations.
    ``states``: the local form (every link from the given state, no input error), as there."""
    n, D, heads = pixels.shape[0], cfg.hidden_size, cfg.num_attention_heads
    p, eps, dh = cfg.patch_size, cfg.layer_norm_eps, 64
    S = (cfg.image_size // p) ** 2 + 1
    U64 = TC.U64
    X = torch.nn.functional.unfold(pixels.double(), kernel_size=p, stride=p).transpose(1, 2)
    pw = sd["embeddings.patch_embedding.weight"].double().reshape(D, -1)
    cls, pos = sd["embeddings.class_embedding"].double(), sd["embeddings.position_embedding.weight"].double()[:S]
    h0 = torch.cat([cls.expand(n, 1, D), X @ pw.t()], 1) + pos
    zero = torch.zeros(n, X.shape[1], 1, dtype=torch.float64)
    start = []
    for u in (U64, u_ref):
        e = torch.cat([torch.zeros(n, 1, 1, dtype=torch.float64), TC._lin_err(X, zero, pw, None, u)], 1) + u * TC._rn(h0)
        h, e = TC._ln_err(h0, e, sd["pre_layrnorm.weight"].double(), sd["pre_layrnorm.bias"].double(), eps, u)
        start.append(e.reshape(-1, 1))
    h, (ef, ed) = h.reshape(-1, D), start
    out = [(ef + ed).expand(-1, D).contiguous()]
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = dh ** -0.5 * TC.LOG2E
    heads_of = lambda t: t.reshape(n, S, heads, dh).transpose(1, 2)
    per_head = lambda E: E.reshape(n, 1, S, 1).expand(n, heads, S, 1)
    join = lambda E: (E * E).sum(1).sqrt().reshape(-1, 1)
    dd = lambda k: sd[k].double()
    for l in range(layers_run):
        if states is not None:
            h, ef, ed = states[l], torch.zeros(n * S, 1, dtype=torch.float64), torch.zeros(n * S, 1, dtype=torch.float64)
        q_ = f"encoder.layers.{l}."
        W = torch.cat([dd(q_ + f"self_attn.{x}_proj.weight") for x in "qkv"], 0)
        b = torch.cat([dd(q_ + f"self_attn.{x}_proj.bias") for x in "qkv"], 0)
        g1, b1, g2, b2 = (dd(q_ + k) for k in ("layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"))
        Wo, bo, W1, c1, W2, c2 = (dd(q_ + k) for k in ("self_attn.out_proj.weight", "self_attn.out_proj.bias", "mlp.fc1.weight",
                                                       "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"))
        dbp = TC._gam(D + 2, U64) * rs * (b.abs() + W.abs() @ b1.abs())
        yf, Ef = TC._fold_err(h, ef, T["w_qkv"][l].double(), T["colsum_qkv"][l].double(), T["b_qkv"][l].double(), dbp, eps, U64)
        qf, kf, vf = (heads_of(yf[:, i * D:(i + 1) * D]) for i in range(3))
        _, Ecf = TC._attn_err(qf, per_head(Ef), kf, per_head(Ef), vf, per_head(Ef), TC.LN2, U64)
        x1, Ex1 = TC._ln_err(h, ed, g1, b1, eps, u_ref)
        yd, Ed = x1 @ W.t() + b, TC._lin_err(x1, Ex1, W, b, u_ref)
        qd, kd, vd = (heads_of(yd[:, i * D:(i + 1) * D]) for i in range(3))
        cd, Ecd = TC._attn_err(qd, per_head(Ed), kd, per_head(Ed), vd, per_head(Ed), dh ** -0.5, u_ref)
        ctx = cd.transpose(1, 2).reshape(-1, D)
        h1 = h + ctx @ Wo.t() + bo
        ef = ef + TC._lin_err(ctx, join(Ecf), Wo, bo, U64) + 2 * U64 * TC._rn(h1)
        ed = ed + TC._lin_err(ctx, join(Ecd), Wo, bo, u_ref) + 2 * u_ref * TC._rn(h1)
        dbp = TC._gam(D + 2, U64) * (c1.abs() + W1.abs() @ b2.abs())
        _, Ezf = TC._fold_err(h1, ef, T["w_fc1"][l].double(), T["colsum_fc1"][l].double(), T["b_fc1"][l].double(), dbp, eps, U64)
        x2, Ex2 = TC._ln_err(h1, ed, g2, b2, eps, u_ref)
        z, Ezd = x2 @ W1.t() + c1, TC._lin_err(x2, Ex2, W1, c1, u_ref)
        a = GC._gelu64(z)
        Eaf, Ead = GELU_LIPSCHITZ * Ezf + 8 * U64 * TC._rn(z), GELU_LIPSCHITZ * Ezd + 8 * u_ref * TC._rn(z)
        h2 = h1 + a @ W2.t() + c2
        ef = ef + TC._lin_err(a, Eaf, W2, c2, U64) + 2 * U64 * TC._rn(h2)
        ed = ed + TC._lin_err(a, Ead, W2, c2, u_ref) + 2 * u_ref * TC._rn(h2)
        h = h2
        out.append((ef + ed).expand(-1, D).contiguous())
    return out
