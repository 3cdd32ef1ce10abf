"""SigLIP vision towers (patch 16, head_dim 64, the tanh-form GELU): what their tests share.  Plain module (no fixtures, not a
conftest); importable without a GPU and without the HIP library.  It stands NEXT TO tests/gemm_conformance.py,
tests/tower_conformance.py and tests/gelu_tower_conformance.py and writes into none of their tables:

  * the GEMM form ``fold_gelu_tanh_t`` -- the LayerNorm-fold consumer followed by x sigmoid(2 sqrt(2 / pi) (x + 0.044715 x^3)) and
    one RNE to T (SLIME_EPI_BIAS_GELU_TANH_T = 9): its case (the buffers of ``fold_quickgelu_t`` with a quarter of the bias columns
    moved so that pre-activations fall into [-5, -2.5], where the three GELU forms are many ulps of T apart), float64 reference,
    per-element bound, fp32 emulation and the wrong restatements (erf and quick forms);
  * the front end's plain form in float64 (conv + pos', no class row, no LayerNorm) with its per-element bound;
  * the yardstick: HF ``SiglipVisionModel`` built from a config (no download), loaded with ``weights.make_siglip_state_dict``;
  * ``replay_siglip``: csrc/api.hip's layer loop in its plain form on the two backends of tower_conformance (S = P rows, the plain
    front end, fc1 under epilogue 9), with wrong variants;
  * ``siglip_error_bound``: the float64 forward-error bound of tower_conformance for this layout and activation.
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

FORM = "fold_gelu_tanh_t"
EPI_BIAS_GELU_TANH_T = 9
TILES = (3, 15, 18, 4, 10, 11, 12)                        # every kernel family launch_epi can pick (gemm_conformance.TILE_FAMILY)
FOLD_K = (64, 192, 2112)                                   # one k-tile, fewer k-tiles than ring stages, both sides of KTAG / long K
VARIANTS = ("erf", "quickgelu")                            # the other two activations restated on the folded pre-activation
SQRT_2_PI = math.sqrt(2.0 / math.pi)
CUBIC = 0.044715
TAIL = (-5.0, -2.5)                                        # where tanh- and erf-GELU differ by >= 7 ulp of bf16 and >= 20 ulp of fp16
TAIL_SHARE = 0.05
TAIL_BIAS = -3.75                                          # the middle of TAIL


# ------------------------------------------------------------------------------------------------ the activation
def gelu_tanh64(x):
    """F.gelu(approximate='tanh') = 0.5 x (1 + tanh(c (x + 0.044715 x^3))) in the form the kernel evaluates, x sigmoid(2 c (...))."""
    return x * torch.sigmoid(2.0 * SQRT_2_PI * x * (1.0 + CUBIC * x * x))


def gelu_tanh32(x):
    """gelu_tanh of csrc/gemm.hip, operation by operation in fp32."""
    cc = torch.tensor(-2.0 * 0.79788456080286535588 * 1.4426950408889634, dtype=torch.float32).to(x.device)
    u = x * (0.044715 * (x * x) + 1.0)
    return x * (1.0 / (1.0 + torch.exp2(cc * u)))


def d_gelu_tanh(x, dx):
    """The fold bound's activation term for this form: gemm_conformance._d_quickgelu with this function's derivative and argument.
    y = x s, s = sigmoid(2 c u), u = x (1 + a x^2):  y' = s + 2 c x (1 + 3 a x^2) s (1 - s).  In fp32 the argument t = C u of
    v_exp carries x x, the fma, the product with x, the rounded constant and the product with it (5 roundings; 7 E32 taken), so
    e = 2^t is off by ln 2 |t| 7 E32 + 2 E32 relative (v_exp within 1 ulp + the result's own rounding); s = 1 / (1 + e) moves by
    (1 - s) of that; the sum, v_rcp and the last product add 4 E32; a flushed exponential moves y by at most |x| FLUSH32."""
    u = x * (1.0 + CUBIC * x * x)
    s = torch.sigmoid(2.0 * SQRT_2_PI * u)
    y = x * s
    dydx = (s + 2.0 * SQRT_2_PI * x * (1.0 + 3.0 * CUBIC * x * x) * s * (1 - s)).abs()
    eps_e = math.log(2.0) * (2.0 * SQRT_2_PI * GC.LOG2E * u.abs()) * 7 * GC.E32 + 2 * GC.E32
    return dydx * dx + y.abs() * ((1 - s) * eps_e + 4 * GC.E32) + x.abs() * GC.FLUSH32


# ------------------------------------------------------------------------------------------------ the GEMM form
class FoldGeluTanhCase(GC.Case):
    """A gemm_conformance.Case whose epilogue / fold do not come from the FORMS table: BIAS_GELU_TANH_T with ln_stats."""

    @property
    def epilogue(self):
        return EPI_BIAS_GELU_TANH_T

    @property
    def fold(self):
        return True


def fold_n(tile: int):
    return (256, 384 if 384 in GC.TILE_N[tile] else 512)


def make_case(kind: str, dtype, M: int, N: int, K: int, **kw) -> FoldGeluTanhCase:
    """gemm_conformance.make_case's buffers for ``fold_quickgelu_t``; with a bias, every fourth column's is set to TAIL_BIAS: the
    folded product is about N(0, 1) ("random") or small ("tails"), so most of that quarter lies in TAIL."""
    c = GC.make_case(kind, dtype, "fold_quickgelu_t", M, N, K, **kw)
    if c.has_bias:
        c.buf["bias"].win[0, ::4] = TAIL_BIAS
    f = FoldGeluTanhCase(**{fl.name: getattr(c, fl.name) for fl in dataclasses.fields(c)})
    f.form = FORM
    return f


def reference(c: FoldGeluTanhCase) -> GC.Ref:
    r = GC.reference(c)
    assert r.x is not None and torch.equal(r.out, r.x), "the base module knows this form now: use its reference"
    r.out = gelu_tanh64(r.x)
    return r


def tail_share(r: GC.Ref) -> float:
    return float(((r.x >= TAIL[0]) & (r.x <= TAIL[1])).double().mean())


def bound(c: FoldGeluTanhCase, r: GC.Ref) -> torch.Tensor:
    """The fold's dx (term (6)) through the activation, then one RNE to T (term (2))."""
    return GC._round_T(r.out, d_gelu_tanh(r.x, r.dx), c.dtype)


def check(c: FoldGeluTanhCase, r: GC.Ref, outs: Dict[str, torch.Tensor], bm: int = 128):
    bd = bound(c, r)
    ratio, ex, *_ = GC.worst(outs["C"], r.out, bd)
    return ratio, (None if ex <= 0 else GC.describe_failure(FORM, outs["C"], r.out, bd, bm))


def restate64(c: FoldGeluTanhCase, r: GC.Ref, variant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The EXACT float64 value of a form on the reference's pre-activation, rounded once to T: the form itself (None), or the erf /
    quick form in its place.  No accumulation or fold error at all: a variant that leaves the bound does so by its function alone."""
    y = {None: gelu_tanh64, "erf": GC._gelu64, "quickgelu": lambda x: x * torch.sigmoid(1.702 * x)}[variant](r.x)
    outs = c.windows()
    outs["C"] = y.to(c.dtype)
    return outs


def emulate(c: FoldGeluTanhCase, variant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The kernel's arithmetic in torch fp32 (gelu_tower_conformance.emulate's fold, with gelu_tanh)."""
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
    x = rstd[:, None] * acc + ((-mu * rstd)[:, None] * b["colsum"].win.view(1, N) + bias)
    if variant == "erf":
        y = GC._gelu_erf32(x)
    elif variant == "quickgelu":
        y = x * (1.0 / (1.0 + torch.exp2((torch.tensor(-1.702) * torch.tensor(GC.LOG2E)).to(dev) * x)))
    else:
        y = gelu_tanh32(x)
    outs = c.windows()
    outs["C"] = y.to(c.dtype)
    return outs


# ------------------------------------------------------------------------------------------------ the HF yardstick
def siglip_config(image: int, patch: int, D: int, inter: int, layers: int, **kw):
    from slime_amd.weights import SiglipVisionConfig
    assert D % 64 == 0
    return SiglipVisionConfig(hidden_size=D, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=D // 64,
                              image_size=image, patch_size=patch, **kw)


def hf_model(cfg, sd, dtype=torch.float32):
    """HF SiglipVisionModel from a config, weights from ``sd`` (make_siglip_state_dict's keys, head included): every parameter must
    be given and no key may be left over."""
    from transformers import SiglipVisionConfig, SiglipVisionModel
    from slime_amd.weights import strip_tower_prefix
    m = SiglipVisionModel(SiglipVisionConfig(**cfg.to_dict())).eval()
    if not any(k.startswith("vision_model.") for k in m.state_dict()):          # transformers 5.x dropped the prefix
        sd = strip_tower_prefix(sd)
    res = m.load_state_dict(sd, strict=False)
    missing = [k for k in res.missing_keys if "position_ids" not in k]
    assert not missing and not res.unexpected_keys, (missing[:3], res.unexpected_keys[:3])
    return m.to(dtype)


def hf_states(cfg, sd, pixels, dtype=torch.float32):
    """hidden_states of HF's forward with output_hidden_states=True: L + 1 tensors [n, P, D] of ``dtype``, on the CPU."""
    m = hf_model(cfg, sd, dtype)
    with torch.no_grad():
        out = m(pixel_values=pixels.to(dtype), output_hidden_states=True)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    return [h.detach() for h in out.hidden_states]


def write_hf_dir(path, sd, cfg, nested_config: bool = False, resample: int = 3, **over) -> str:
    """A SigLIP directory as SigLipVisionTower.load_model reads it: config.json (model_type siglip_vision_model, or siglip with the
    tower under ``vision_config``), model.safetensors, preprocessor_config.json."""
    from safetensors.torch import save_file
    v = dict(cfg.to_dict(), **over)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "siglip", "vision_config": dict(v, model_type="siglip_vision_model"), "text_config": {"hidden_size": 8}}
                  if nested_config else dict(v, model_type="siglip_vision_model"), f)
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(path, "model.safetensors"))
    s = cfg.image_size
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"do_resize": True, "size": {"height": s, "width": s}, "do_normalize": True, "image_mean": [0.5, 0.5, 0.5],
                   "image_std": [0.5, 0.5, 0.5], "rescale_factor": 1 / 255, "resample": resample,
                   "image_processor_type": "SiglipImageProcessor"}, f)
    return str(path)


def rel_l2(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_token(a, b) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)).max())


# ------------------------------------------------------------------------------------------------ the front end in float64
def embed64(pixels, T, cfg, dtype=None):
    """h = conv(T(pixels)) + pos' in float64 over the operands as they are held (``T["patch_w"]`` [D, kpad], ``T["pos"]`` [P, D]) and
    the per-element bound of the kernel's fp32 result: the MFMA accumulation of K = 3 p^2 products and one fp32 addition."""
    p, D = cfg.patch_size, cfg.hidden_size
    px = pixels.double() if dtype is None else pixels.to(dtype).double()
    x = torch.nn.functional.unfold(px, kernel_size=p, stride=p).transpose(1, 2)                      # [n, P, 3 p p], (c, ky, kx) order
    w = T["patch_w"].double()[:, :x.shape[-1]]
    pos = T["pos"].double()[None]
    h = x @ w.t() + pos
    S = x.abs() @ w.abs().t() + pos.abs()
    return h.reshape(-1, D), (GC.E32 * (x.shape[-1] + 4) * S).reshape(-1, D)


# ------------------------------------------------------------------------------------------------ replay backends
class TorchBackend(TC.TorchBackend):
    """tower_conformance.TorchBackend plus the plain front end, fc1 under the tanh form (``act``: 'erf' / 'quick' restate it)."""

    def __init__(self, dtype=None, act: str = "tanh"):
        super().__init__(dtype)
        self.act = act

    def patch_embed_plain(self, pixels, T, cfg, n: int, bias_folded: bool = True):
        p, D = cfg.patch_size, cfg.hidden_size
        px = self._t(pixels.double())
        x = torch.nn.functional.unfold(px, kernel_size=p, stride=p).transpose(1, 2)
        pos = T["pos"].double() if bias_folded else T["pos_without_bias"].double()
        h = self._f((x @ T["patch_w"].double()[:, :x.shape[-1]].t() + pos[None]).reshape(-1, D))
        hi, lo = self._split(h)
        return hi, lo.reshape(-1).clone(), self._stats(hi)

    def gemm_fold(self, A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits=1):
        if epilogue != EPI_BIAS_GELU_TANH_T:
            return super().gemm_fold(A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits)
        w = TC._flat(T[name], w_off, N * K).view(N, K).double()
        bias = TC._flat(T["b_fc1"], b_off, N).double()
        cs = TC._flat(T[colsum_name], b_off, N).double()
        st = stats.reshape(A.shape[0], -1, 2)
        mu = st[..., 0].sum(1, keepdim=True) / K
        var = st[..., 1].sum(1, keepdim=True) / K - mu * mu
        y = (A.double() @ w.t() - mu * cs) / torch.sqrt(var + eps) + bias
        y = {"tanh": gelu_tanh64, "erf": GC._gelu64, "quick": lambda v: v * torch.sigmoid(1.702 * v)}[self.act](y)
        return self._t(y)


class HipBackend(TC.HipBackend):
    """tower_conformance.HipBackend plus slime_patch_embed_plain."""

    def patch_embed_plain(self, pixels, T, cfg, n: int, bias_folded: bool = True):
        D, M = cfg.hidden_size, n * cfg.num_patches
        kpad = (3 * cfg.patch_size ** 2 + 63) // 64 * 64
        xn = torch.empty(M, D, dtype=self.dtype, device=self.dev)
        lo = torch.empty(M * D, dtype=torch.int8, device=self.dev)
        stats = torch.empty(M, D // 64, 2, dtype=torch.float32, device=self.dev)
        self._ok(self.lib.slime_patch_embed_plain(pixels.data_ptr(), self.code(pixels.dtype), T["patch_w_frag"].data_ptr(), T["pos"].data_ptr(),
                                                  None, xn.data_ptr(), lo.data_ptr(), stats.data_ptr(), self.code(self.dtype), n,
                                                  cfg.image_size, cfg.patch_size, kpad, D, self._s()), "slime_patch_embed_plain")
        return xn, lo, stats


BROKEN = ("bias_not_folded", "class_row_offset", "fold_off_by_one_layer")


def replay_siglip(be, T, cfg, pixels, layers_run: int, *, out_dtype=torch.float32, want_out: bool = True, want_hidden: bool = False,
                  want_states: bool = False, k_split=(1, 1, 1, 1), broken: Optional[str] = None):
    """csrc/api.hip vit_run in its plain form on pixels [n, 3, image, image] -> {"out": [n P, D] out_dtype, "hidden": fp32 [n P, D],
    "states": fp32 [layers_run + 1, n P, D]} (the requested ones).  ``broken``: the conv bias left out of pos'; the output gather
    starting at row 1 of every crop (a class-row offset, the crop's last row replaced by the next crop's first); fc1 of layer l with
    the folded weights of layer l + 1."""
    assert broken is None or broken in BROKEN
    n = pixels.shape[0]
    P, D, F = cfg.num_patches, cfg.hidden_size, cfg.intermediate_size
    S, M, heads, eps = P, n * P, cfg.num_attention_heads, cfg.layer_norm_eps
    sq, so, s1, s2 = k_split
    res = {}
    xn, lo, stats = be.patch_embed_plain(pixels, T, cfg, n, bias_folded=broken != "bias_not_folded")
    states = [None] * (layers_run + 1)
    if want_states:
        states[0] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32)
    for l in range(layers_run):
        l1 = (l + 1) % layers_run if broken == "fold_off_by_one_layer" else l
        qkv = be.gemm_fold(xn, stats.reshape(-1), T, "w_qkv", l * 3 * D * D, 3 * D, D, l * 3 * D, "colsum_qkv", eps, GC.EPI_BIAS_T, sq)
        ctx = be.attention_packed(qkv, 0, D, 2 * D, n, S, heads, 64)
        stats = be.gemm_resid_split(ctx, T, "w_o", l * D * D, D, D, l * D, xn, lo, D, so)
        ff = be.gemm_fold(xn, stats.reshape(-1), T, "w_fc1", l1 * F * D, F, D, l1 * F, "colsum_fc1", eps, EPI_BIAS_GELU_TANH_T, s1)
        stats = be.gemm_resid_split(ff, T, "w_fc2", l * D * F, D, F, l * D, xn, lo, D, s2)
        if want_states:
            states[l + 1] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32)
    if want_states:
        res["states"] = states
    if want_hidden:
        res["hidden"] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32)
    if want_out:
        if broken == "class_row_offset":
            flat = be.gather_rows_split(xn, lo, 1, 0, n * S, 1, out_dtype)
            res["out"] = torch.cat([flat[1:], flat[:1]], 0)
        else:
            res["out"] = be.gather_rows_split(xn, lo, S, 0, n, S, out_dtype)
    return res


# ------------------------------------------------------------------------------------------------ float64 forward-error bound
TANH_GELU_LIPSCHITZ = 1.13


def tanh_gelu_max_slope() -> float:
    """max |y'| of the tanh form over a fine grid (test_siglip_tower_cpu asserts it below TANH_GELU_LIPSCHITZ)."""
    x = torch.linspace(-12.0, 12.0, 2400001, dtype=torch.float64)
    u = x * (1.0 + CUBIC * x * x)
    s = torch.sigmoid(2.0 * SQRT_2_PI * u)
    return float((s + 2.0 * SQRT_2_PI * x * (1.0 + 3.0 * CUBIC * x * x) * s * (1 - s)).abs().max())


def siglip_error_bound(sd, T, cfg, pixels, layers_run: int, u_ref: float = TC.U64):
    """gelu_tower_conformance.tower_error_bound for the SigLIP layout: the same two running bounds (the replay's at 2^-53 with both
    LayerNorms folded, the reference's at u_ref by two passes) carried through the same float64 values.  What differs:
      * the start: h0 = conv(pixels) + bias + pos, a linear map of K = 3 p^2 products and two additions (the replay adds the
        pre-summed pos' = pos + bias: one rounding of the table, one of the sum) -- no class row, no LayerNorm;
      * the activation y = x sigmoid(2 c (x + a x^3)): an input error passes with max |y'| <= 1.13 (``tanh_gelu_max_slope``: 1.1290 at
        x = 1.47); its own rounding, as 0.5 x (1 + tanh(c x (1 + a x^2))) (ATen's form): the argument's five roundings move tanh by at
        most 5 u |t| tanh'(t) <= 5 u 0.45 < 2.5 u, tanh itself within 4 ulp, |tanh| <= 1, the sum 1 + tanh rounds by 2 u -- 8.5 u on the
        bracket, absolute, hence 4.25 u |x| on the product -- and the two products add 2 u |x|: 6.25 u |x| <= 8 u |x|, the weight
        tower_conformance gives the quick-GELU."""
    n, D, heads = pixels.shape[0], cfg.hidden_size, cfg.num_attention_heads
    p, eps, dh = cfg.patch_size, cfg.layer_norm_eps, 64
    S = cfg.num_patches
    U64 = TC.U64
    X = torch.nn.functional.unfold(pixels.double(), kernel_size=p, stride=p).transpose(1, 2)
    pw = sd["embeddings.patch_embedding.weight"].double().reshape(D, -1)
    cb, pos = sd["embeddings.patch_embedding.bias"].double(), sd["embeddings.position_embedding.weight"].double()
    h0 = X @ pw.t() + cb + pos
    zero = torch.zeros(n, X.shape[1], 1, dtype=torch.float64)
    start = []
    for u in (U64, u_ref):
        e = TC._lin_err(X, zero, pw, cb, u) + 2 * u * TC._rn(h0) + 2 * u * TC._rn((cb + pos).expand(n, -1, -1))
        start.append(e.reshape(-1, 1))
    h, (ef, ed) = h0.reshape(-1, D), start
    out = [(ef + ed).expand(-1, D).contiguous()]
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = dh ** -0.5 * TC.LOG2E
    heads_of = lambda t: t.reshape(n, S, heads, dh).transpose(1, 2)
    per_head = lambda E: E.reshape(n, 1, S, 1).expand(n, heads, S, 1)
    join = lambda E: (E * E).sum(1).sqrt().reshape(-1, 1)
    dd = lambda k: sd[k].double()
    for l in range(layers_run):
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
        a = gelu_tanh64(z)
        Eaf, Ead = TANH_GELU_LIPSCHITZ * Ezf + 8 * U64 * TC._rn(z), TANH_GELU_LIPSCHITZ * Ezd + 8 * u_ref * TC._rn(z)
        h2 = h1 + a @ W2.t() + c2
        ef = ef + TC._lin_err(a, Eaf, W2, c2, U64) + 2 * U64 * TC._rn(h2)
        ed = ed + TC._lin_err(a, Ead, W2, c2, u_ref) + 2 * u_ref * TC._rn(h2)
        h = h2
        out.append((ef + ed).expand(-1, D).contiguous())
    return out
