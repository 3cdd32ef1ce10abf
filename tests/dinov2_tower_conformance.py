"""DINOv2 vision towers (class + register tokens, LayerScale, an interpolated position table): what their tests share.  Plain module
(no fixtures, not a conftest); importable without a GPU and without the HIP library.  It stands NEXT TO tests/tower_conformance.py,
tests/gelu_tower_conformance.py and tests/siglip_tower_conformance.py and writes into none of their tables:

  * the yardstick: HF ``Dinov2Model`` / ``Dinov2WithRegistersModel`` built from a config (no download), loaded with
    ``weights.make_dinov2_state_dict``, and a DINOv2 directory as the loader reads it;
  * the front end's prefix form in float64 (prefix rows as they are, conv + pos' behind them) with its per-element bound;
  * ``replay_dinov2``: csrc/api.hip's layer loop in its prefix form on the two backends of tower_conformance (S = n_prefix + P rows,
    the prefix front end, fc1 under the exact GELU), with wrong variants; ``broken_host``: wrong pack-time algebra;
  * ``dinov2_error_bound``: the float64 forward-error bound of gelu_tower_conformance for this layout.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Optional

import torch

import gemm_conformance as GC
import gelu_tower_conformance as G
import siglip_tower_conformance as S
import tower_conformance as TC

rel_l2, worst_token = G.rel_l2, G.worst_token
embed64 = S.embed64                                        # the patch rows: conv + pos' over T["patch_w"], T["pos"] (no row offset in it)


# ------------------------------------------------------------------------------------------------ the HF yardstick
def dinov2_config(image: int, D: int, layers: int, registers: int = 0, table_grid: Optional[int] = None, patch: int = 14, **kw):
    """A tower ``D`` wide run at ``image`` pixels; ``registers`` > 0 makes it the registers model (antialiased table)."""
    from slime_amd.weights import Dinov2VisionConfig
    assert D % 64 == 0
    return Dinov2VisionConfig(hidden_size=D, num_hidden_layers=layers, num_attention_heads=D // 64, image_size=image, patch_size=patch,
                              table_grid=image // patch if table_grid is None else table_grid, num_register_tokens=registers,
                              model_type="dinov2_with_registers" if registers else "dinov2", **kw)


def hf_config_dict(cfg) -> dict:
    """HF's fields: ``image_size`` there is the size the position table was made for."""
    d = dict(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
             mlp_ratio=cfg.mlp_ratio, image_size=cfg.table_grid * cfg.patch_size, patch_size=cfg.patch_size,
             layer_norm_eps=cfg.layer_norm_eps, hidden_act=cfg.hidden_act, use_swiglu_ffn=cfg.use_swiglu_ffn)
    if cfg.model_type == "dinov2_with_registers":
        d["num_register_tokens"] = cfg.num_register_tokens
    return d


def hf_model(cfg, sd, dtype=torch.float32):
    """HF Dinov2Model / Dinov2WithRegistersModel from a config, weights from ``sd`` (make_dinov2_state_dict's keys): every parameter
    must be given and no key may be left over."""
    if cfg.model_type == "dinov2_with_registers":
        from transformers import Dinov2WithRegistersConfig as Cfg, Dinov2WithRegistersModel as Model
    else:
        from transformers import Dinov2Config as Cfg, Dinov2Model as Model
    m = Model(Cfg(**hf_config_dict(cfg))).eval()
    res = m.load_state_dict(sd, strict=False)
    assert not res.missing_keys and not res.unexpected_keys, (res.missing_keys[:3], res.unexpected_keys[:3])
    return m.to(dtype)


def hf_states(cfg, sd, pixels, dtype=torch.float32):
    """hidden_states of HF's forward with output_hidden_states=True: L + 1 tensors [n, S, D] of ``dtype``, on the CPU."""
    m = hf_model(cfg, sd, dtype)
    with torch.no_grad():
        out = m(pixel_values=pixels.to(dtype), output_hidden_states=True)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    return [h.detach() for h in out.hidden_states]


def write_hf_dir(path, sd, cfg, nested_config: bool = False, preprocessor: bool = True, **over) -> str:
    """A DINOv2 directory as Dinov2VisionTower reads it: config.json (flat, or the tower under ``vision_config``), model.safetensors
    and (``preprocessor``) a preprocessor_config.json whose crop_size is the run size."""
    from safetensors.torch import save_file
    v = dict(hf_config_dict(cfg), model_type=cfg.model_type, **over)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"model_type": "llava", "vision_config": v, "text_config": {"hidden_size": 8}} if nested_config else v, f)
    save_file({k: t.contiguous() for k, t in sd.items()}, os.path.join(path, "model.safetensors"))
    pp = os.path.join(path, "preprocessor_config.json")
    if preprocessor:
        s = cfg.image_size
        with open(pp, "w") as f:
            json.dump({"crop_size": {"height": s, "width": s}, "size": {"shortest_edge": s * 256 // 224}, "do_center_crop": True,
                       "do_normalize": True, "image_mean": [0.485, 0.456, 0.406], "image_std": [0.229, 0.224, 0.225],
                       "rescale_factor": 1 / 255, "resample": 3, "image_processor_type": "BitImageProcessor"}, f)
    elif os.path.exists(pp):
        os.remove(pp)
    return str(path)


# ------------------------------------------------------------------------------------------------ replay backends
class TorchBackend(G.TorchBackend):
    """gelu_tower_conformance.TorchBackend (fc1 under the exact GELU) plus the prefix front end."""

    def __init__(self, dtype=None):
        super().__init__(dtype, "gelu")

    def patch_embed_prefix(self, pixels, T, cfg, n: int):
        p, D = cfg.patch_size, cfg.hidden_size
        px = self._t(pixels.double())
        x = torch.nn.functional.unfold(px, kernel_size=p, stride=p).transpose(1, 2)
        patches = x @ T["patch_w"].double()[:, :x.shape[-1]].t() + T["pos"].double()[None]
        h = self._f(torch.cat([T["cls"].double()[None].expand(n, -1, -1), patches], 1).reshape(-1, D))
        hi, lo = self._split(h)
        return hi, lo.reshape(-1).clone(), self._stats(hi)


class HipBackend(G.HipBackend):
    """gelu_tower_conformance.HipBackend (fc1 under SLIME_EPI_BIAS_GELU_T) plus slime_patch_embed_prefix."""

    def __init__(self, dtype, device):
        super().__init__(dtype, device, "gelu")

    def patch_embed_prefix(self, pixels, T, cfg, n: int):
        D, M = cfg.hidden_size, n * cfg.seq_len
        kpad = (3 * cfg.patch_size ** 2 + 63) // 64 * 64
        xn = torch.empty(M, D, dtype=self.dtype, device=self.dev)
        lo = torch.empty(M * D, dtype=torch.int8, device=self.dev)
        stats = torch.empty(M, D // 64, 2, dtype=torch.float32, device=self.dev)
        self._ok(self.lib.slime_patch_embed_prefix(pixels.data_ptr(), self.code(pixels.dtype), T["patch_w_frag"].data_ptr(), T["cls"].data_ptr(),
                                                   cfg.n_prefix, T["pos"].data_ptr(), None, xn.data_ptr(), lo.data_ptr(), stats.data_ptr(),
                                                   self.code(self.dtype), n, cfg.image_size, cfg.patch_size, kpad, D, self._s()),
                 "slime_patch_embed_prefix")
        return xn, lo, stats


REPLAY_BROKEN = ("prefix_offset_by_one", "fold_off_by_one_layer")


def replay_dinov2(be, T, cfg, pixels, layers_run: int, *, keep_prefix: int = 0, out_dtype=torch.float32, want_out: bool = True,
                  want_hidden: bool = False, want_states: bool = False, k_split=(1, 1, 1, 1), broken: Optional[str] = None):
    """csrc/api.hip vit_run in its prefix form on pixels [n, 3, image, image] -> {"out": [n (S | P), D] out_dtype, "hidden": fp32
    [n S, D], "states": fp32 [layers_run + 1, n S, D]} (the requested ones).  ``broken``: the patch gather starting one row early (the
    last prefix row in, the last patch out); fc1 of layer l with the folded weights of layer l + 1."""
    assert broken is None or broken in REPLAY_BROKEN
    n = pixels.shape[0]
    P, D, F, npre = cfg.num_patches, cfg.hidden_size, cfg.intermediate_size, cfg.n_prefix
    S_, heads, eps = npre + P, cfg.num_attention_heads, cfg.layer_norm_eps
    sq, so, s1, s2 = k_split
    res = {}
    xn, lo, stats = be.patch_embed_prefix(pixels, T, cfg, n)
    states = [None] * (layers_run + 1)
    if want_states:
        states[0] = be.gather_rows_split(xn, lo, S_, 0, n, S_, torch.float32)
    for l in range(layers_run):
        l1 = (l + 1) % layers_run if broken == "fold_off_by_one_layer" else l
        qkv = be.gemm_fold(xn, stats.reshape(-1), T, "w_qkv", l * 3 * D * D, 3 * D, D, l * 3 * D, "colsum_qkv", eps, GC.EPI_BIAS_T, sq)
        ctx = be.attention_packed(qkv, 0, D, 2 * D, n, S_, heads, 64)
        stats = be.gemm_resid_split(ctx, T, "w_o", l * D * D, D, D, l * D, xn, lo, D, so)
        ff = be.gemm_fold(xn, stats.reshape(-1), T, "w_fc1", l1 * F * D, F, D, l1 * F, "colsum_fc1", eps, GC.EPI_BIAS_GELU_T, s1)
        stats = be.gemm_resid_split(ff, T, "w_fc2", l * D * F, D, F, l * D, xn, lo, D, s2)
        if want_states:
            states[l + 1] = be.gather_rows_split(xn, lo, S_, 0, n, S_, torch.float32)
    if want_states:
        res["states"] = states
    if want_hidden:
        res["hidden"] = be.gather_rows_split(xn, lo, S_, 0, n, S_, torch.float32)
    if want_out:
        first = npre - 1 if broken == "prefix_offset_by_one" else npre
        res["out"] = be.gather_rows_split(xn, lo, S_, 0 if keep_prefix else first, n, S_ if keep_prefix else P, out_dtype)
    return res


# ------------------------------------------------------------------------------------------------ wrong pack-time algebra
HOST_BROKEN = ("layerscale_not_folded", "lambdas_swapped", "registers_with_position", "antialias_swapped", "bias_not_folded")


def broken_host(sd, cfg, layers_run: int, variant: str):
    """``ops.dinov2_host_tensors`` in float64 with one step of the pack-time algebra done wrongly."""
    from slime_amd import ops
    assert variant in HOST_BROKEN
    dd = lambda k: sd[k].detach().double()
    if variant == "lambdas_swapped":
        swapped = dict(sd)
        for l in range(cfg.num_hidden_layers):
            a, b = f"encoder.layer.{l}.layer_scale1.lambda1", f"encoder.layer.{l}.layer_scale2.lambda1"
            swapped[a], swapped[b] = sd[b], sd[a]
        return ops.dinov2_host_tensors(swapped, cfg, None, layers_run)
    if variant == "antialias_swapped":
        other = "dinov2" if cfg.antialias else "dinov2_with_registers"
        return ops.dinov2_host_tensors(sd, dataclasses.replace(cfg, model_type=other), None, layers_run)
    T = dict(ops.dinov2_host_tensors(sd, cfg, None, layers_run))
    if variant == "layerscale_not_folded":
        for w, b, lin in (("w_o", "b_o", "attention.output.dense"), ("w_fc2", "b_fc2", "mlp.fc2")):
            T[w] = torch.stack([dd(f"encoder.layer.{l}.{lin}.weight") for l in range(layers_run)])
            T[b] = torch.stack([dd(f"encoder.layer.{l}.{lin}.bias") for l in range(layers_run)])
    elif variant == "registers_with_position":
        assert cfg.num_register_tokens > 0
        T["cls"] = T["cls"].clone()
        T["cls"][1:] += dd("embeddings.position_embeddings")[0, 1:cfg.n_prefix]
    elif variant == "bias_not_folded":
        T["pos"] = T["pos"] - dd("embeddings.patch_embeddings.projection.bias")[None]
    return T


# ------------------------------------------------------------------------------------------------ float64 forward-error bound
def dinov2_error_bound(sd, T, cfg, pixels, layers_run: int, u_ref: float = TC.U64):
    """gelu_tower_conformance.tower_error_bound for the DINOv2 layout: the same two running bounds (the replay's at 2^-53 with both
    LayerNorms folded, the reference's at u_ref by two passes) carried through the same float64 values.  What differs:
      * the start.  Prefix row 0 = cls_token + position 0: one addition on either side, u |h0| each; the register rows are copies: no
        error.  Patch rows: h0 = conv(pixels) + bias + pos~, pos~ the table interpolated in fp32 by the SAME function call on
        either side (HF casts the table to fp32 whatever the model's dtype): identical values, no error term; the replay adds the
        pre-summed pos' = pos~ + bias, as the SigLIP layout does -- siglip_error_bound's start;
      * LayerScale.  The reference computes lambda * fl(x W^T + b): the Linear's bound times lambda, element by element, plus one
        rounding u |lambda o|.  The replay computes x W'^T + b' with W' = fl(lambda W), b' = fl(lambda b): one more rounding per
        product.  Both are ``_lin_err`` over W' = diag(lambda) W, b' = lambda b (lambda > 0 leaves |W'| = lambda |W|) with one extra
        term in gamma (K + 2): an input error passes with ||W'||_2 on either side."""
    n, D, heads = pixels.shape[0], cfg.hidden_size, cfg.num_attention_heads
    p, eps, dh, npre = cfg.patch_size, cfg.layer_norm_eps, 64, cfg.n_prefix
    S_ = cfg.seq_len
    U64 = TC.U64
    dd = lambda k: sd[k].double()
    X = torch.nn.functional.unfold(pixels.double(), kernel_size=p, stride=p).transpose(1, 2)
    pw = dd("embeddings.patch_embeddings.projection.weight").reshape(D, -1)
    cb = dd("embeddings.patch_embeddings.projection.bias")
    pos = T["pos"].double() - cb                             # the interpolated table (float64 host tensors: pos' - bias is exact to 1 ulp)
    pre = T["cls"].double()
    h0 = torch.cat([pre[None].expand(n, -1, -1), X @ pw.t() + cb + pos], 1)
    zero = torch.zeros(n, X.shape[1], 1, dtype=torch.float64)
    start = []
    for u in (U64, u_ref):
        e_patch = TC._lin_err(X, zero, pw, cb, u) + 2 * u * TC._rn(h0[:, npre:]) + 2 * u * TC._rn((cb + pos).expand(n, -1, -1))
        e_pre = torch.zeros(n, npre, 1, dtype=torch.float64)
        e_pre[:, 0] = u * TC._rn(h0[:, 0])
        start.append(torch.cat([e_pre, e_patch], 1).reshape(-1, 1))
    h, (ef, ed) = h0.reshape(-1, D), start
    out = [(ef + ed).expand(-1, D).contiguous()]
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = dh ** -0.5 * TC.LOG2E
    heads_of = lambda t: t.reshape(n, S_, heads, dh).transpose(1, 2)
    per_head = lambda E: E.reshape(n, 1, S_, 1).expand(n, heads, S_, 1)
    join = lambda E: (E * E).sum(1).sqrt().reshape(-1, 1)
    for l in range(layers_run):
        q_ = f"encoder.layer.{l}."
        a_ = q_ + "attention.attention."
        W = torch.cat([dd(a_ + f"{x}.weight") for x in ("query", "key", "value")], 0)
        b = torch.cat([dd(a_ + f"{x}.bias") for x in ("query", "key", "value")], 0)
        g1, b1, g2, b2 = (dd(q_ + k) for k in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"))
        lam1, lam2 = dd(q_ + "layer_scale1.lambda1"), dd(q_ + "layer_scale2.lambda1")
        Wo, bo = dd(q_ + "attention.output.dense.weight") * lam1[:, None], dd(q_ + "attention.output.dense.bias") * lam1
        W1, c1 = dd(q_ + "mlp.fc1.weight"), dd(q_ + "mlp.fc1.bias")
        W2, c2 = dd(q_ + "mlp.fc2.weight") * lam2[:, None], dd(q_ + "mlp.fc2.bias") * lam2
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
        ef = ef + TC._lin_err(ctx, join(Ecf), Wo, bo, U64, extra=2) + 2 * U64 * TC._rn(h1)
        ed = ed + TC._lin_err(ctx, join(Ecd), Wo, bo, u_ref, extra=2) + 2 * u_ref * TC._rn(h1)
        dbp = TC._gam(D + 2, U64) * (c1.abs() + W1.abs() @ b2.abs())
        _, Ezf = TC._fold_err(h1, ef, T["w_fc1"][l].double(), T["colsum_fc1"][l].double(), T["b_fc1"][l].double(), dbp, eps, U64)
        x2, Ex2 = TC._ln_err(h1, ed, g2, b2, eps, u_ref)
        z, Ezd = x2 @ W1.t() + c1, TC._lin_err(x2, Ex2, W1, c1, u_ref)
        a = GC._gelu64(z)
        Eaf, Ead = G.GELU_LIPSCHITZ * Ezf + 8 * U64 * TC._rn(z), G.GELU_LIPSCHITZ * Ezd + 8 * u_ref * TC._rn(z)
        h2 = h1 + a @ W2.t() + c2
        ef = ef + TC._lin_err(a, Eaf, W2, c2, U64, extra=2) + 2 * U64 * TC._rn(h2)
        ed = ed + TC._lin_err(a, Ead, W2, c2, u_ref, extra=2) + 2 * u_ref * TC._rn(h2)
        h = h2
        out.append((ef + ed).expand(-1, D).contiguous())
    return out
