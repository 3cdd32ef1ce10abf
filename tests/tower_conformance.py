"""Tower and Llama attention conformance: the two composite entries that carry most of the arithmetic, replayed through the
element-wise bounded kernel entries.

``slime_vit_forward`` / ``_ex`` / ``_ksplit`` / ``_states`` (csrc/api.hip: vit_run, vit_plan) and ``slime_llama_attn_forward`` /
``_resid`` (csrc/prefill.hip: llama_attn_run) are glue around kernels that each have an element-wise test of their own
(gemm_conformance, attention_conformance, rowwise_conformance): per-layer slices of stacked weights, q/k/v column offsets into one
buffer, a split residual stream updated in place, a statistics plane per 64 columns, a workspace whose regions alias in time, the
choice of o_proj's epilogue.  The kernels are deterministic and the GEMM dispatch is a function of (M, N, K, dtype, epilogue, operand
form), so a test that makes the same launches through the public C ABI -- every intermediate in a tensor of its own, every offset
computed here in Python -- must reproduce the fused entry BIT FOR BIT (the argument of tests/adapter_conformance.py, unchanged).

``replay_vit`` and ``replay_llama_attn`` restate the two drivers as calls on a *backend*:
  * ``HipBackend``   (adapter_conformance.HipBackend + the tower's and the Llama layer's launches) calls the C ABI on the packed device
                     tensors; it never sees the library's workspace;
  * ``TorchBackend`` the same operations in float64 with nothing rounded (``dtype=None``), for the CPU tests that hold the replay
                     -- and with it the pack-time LayerNorm fold, which a replay from the packed tensors cannot see -- against the
                     oracle; ``TorchBackend(T)`` rounds where the kernels round, which is where the split stream's lower part exists.
``BROKEN`` names deliberately wrong variants of the glue (``replay_*(..., broken=name)``) and of the fold (``fold_variant``);
``applies`` says, from the case alone, where each can show.  ``tower_error_bound`` / ``llama_error_bound`` are the float64
forward-error bounds of the CPU tests.  Importable without a GPU and without the HIP library.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

import adapter_conformance as AC
from gemm_conformance import (EPI_BIAS_F32, EPI_BIAS_QUICKGELU_T, EPI_BIAS_RESID_SPLIT_LN, EPI_BIAS_RESID_T, EPI_BIAS_T)

LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
DTYPES = AC.DTYPES
DT_ID = AC.DT_ID
U64, U32 = 2.0 ** -53, 2.0 ** -24
LAYER_WEIGHTS = ("w_qkv", "w_o", "w_fc1", "w_fc2")
FORMS = ("frag", "row_major", "both")                      # how a static operand stands in the descriptor

GLUE_BROKEN = ("layer_slice_plus_1", "kv_columns_swapped", "ctx_over_qkv", "stats_group_plus_1", "cls_drop_at_row_0",
               "snapshot_index_minus_1", "ldlo_in_elements_of_T")
FOLD_BROKEN = ("colsum_of_unrounded_w", "bias_without_w_beta", "q_scale_not_on_bias", "gamma_on_rows")
BROKEN = GLUE_BROKEN + FOLD_BROKEN


def applies(broken: str, *, layers_run: int, n: int = 1, keep_cls: int = 0, want_out: bool = True, want_states: bool = False,
            rounded: bool = False) -> bool:
    """Whether the wrong variant ``broken`` can change what a case returns, from the case alone.
    layer_slice_plus_1     : layer l reads the slice of layer (l + 1) mod layers_run: needs two layers.
    kv_columns_swapped, stats_group_plus_1, bias_without_w_beta, q_scale_not_on_bias, gamma_on_rows: need one layer.
    ctx_over_qkv           : ctx at the head of the q/k/v buffer; a launch has no order among its crops, the variant is evaluated
                             with the crops in descending order (one legal schedule): crop b's context lands on the q/k/v rows of
                             crop b / 3, which is still unread iff b / 3 < b: needs two crops and one layer.
    cls_drop_at_row_0      : needs ``out`` without the class token.
    snapshot_index_minus_1 : needs the states and one layer.
    ldlo_in_elements_of_T  : the lower part's row stride D / 2 instead of D bytes; needs one layer, two rows (always) and a lower
                             part that is not identically zero, i.e. a backend that rounds.
    colsum_of_unrounded_w  : equals the shipped fold where nothing is rounded."""
    if broken == "layer_slice_plus_1":
        return layers_run >= 2
    if broken in ("kv_columns_swapped", "stats_group_plus_1", "bias_without_w_beta", "q_scale_not_on_bias", "gamma_on_rows"):
        return layers_run >= 1
    if broken == "ctx_over_qkv":
        return layers_run >= 1 and n >= 2
    if broken == "cls_drop_at_row_0":
        return want_out and not keep_cls
    if broken == "snapshot_index_minus_1":
        return want_states and layers_run >= 1
    if broken == "ldlo_in_elements_of_T":
        return layers_run >= 1 and rounded
    if broken == "colsum_of_unrounded_w":
        return layers_run >= 1 and rounded
    raise KeyError(broken)


# ------------------------------------------------------------------------------------------------ cases
def tower_config(image: int, patch: int, D: int, inter: int, layers: int):
    from slime_amd.weights import VisionConfig
    return VisionConfig(hidden_size=D, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=D // 64, image_size=image,
                        patch_size=patch)


def tower_state(cfg, seed: int = 11):
    from slime_amd import weights as W
    return W.strip_tower_prefix(W.make_tower_state_dict(cfg, seed=seed))


def fold_variant(Wm, bm, gamma, beta, row_scale, dtype, variant: Optional[str]):
    """ops.fold_ln restated with one named defect (variant = None: the shipped algebra, for the restatement's own check)."""
    W64, g64, be64 = Wm.double(), gamma.double(), beta.double()
    Wp = W64 * (g64.repeat(W64.shape[0] // g64.numel())[:, None] if variant == "gamma_on_rows" else g64[None, :])
    bp = bm.double() + (0 if variant == "bias_without_w_beta" else W64 @ be64)
    if row_scale is not None:
        Wp = Wp * row_scale[:, None]
        if variant != "q_scale_not_on_bias":
            bp = bp * row_scale
    if dtype is None:
        return Wp, bp, Wp.sum(1)
    Wt = Wp.float().to(dtype)
    cs = (Wp if variant == "colsum_of_unrounded_w" else Wt.double()).sum(1).float()
    return Wt, bp.float(), cs


def host_tensors(sd, cfg, dtype, layers_run: int, variant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """ops.tower_host_tensors for ``layers_run`` layers; with ``variant`` the two folded GEMMs of every layer come from
    ``fold_variant`` instead."""
    from slime_amd import ops
    T = ops.tower_host_tensors(sd, cfg, dtype, select_layer=layers_run)
    if variant is None or layers_run == 0:
        return T
    D = cfg.hidden_size
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = cfg.head_dim ** -0.5 * LOG2E
    for l in range(layers_run):
        p = f"encoder.layers.{l}."
        Wm = torch.cat([sd[p + f"self_attn.{x}_proj.weight"].float() for x in "qkv"], 0)
        bm = torch.cat([sd[p + f"self_attn.{x}_proj.bias"].float() for x in "qkv"], 0)
        T["w_qkv"][l], T["b_qkv"][l], T["colsum_qkv"][l] = fold_variant(Wm, bm, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"],
                                                                        rs, dtype, variant)
        T["w_fc1"][l], T["b_fc1"][l], T["colsum_fc1"][l] = fold_variant(sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"],
                                                                        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"], None,
                                                                        dtype, variant)
    return T


def with_form(pt, host: Dict[str, torch.Tensor], form: str):
    """(tensors, descriptor) of a packed tower with its four layer matrices given as ``form``: the fragment-order image alone (what
    pack_tower leaves by default), the row-major matrix alone, or both.  The conv weight has one form (patch_w_frag)."""
    assert form in FORMS
    T = dict(pt.tensors)
    d = type(pt.desc).from_buffer_copy(pt.desc)
    if pt.layers_run == 0:
        return T, d
    for name in LAYER_WEIGHTS:
        frag = pt.tensors[name + "_frag"]
        assert frag is not None
        T[name] = host[name].to(frag.device).contiguous() if form != "frag" else None
        T[name + "_frag"] = frag if form != "row_major" else None
        for k in (name, name + "_frag"):
            setattr(d, k, None if T[k] is None else T[k].data_ptr())
    return T, d


def _flat(t, off: int, numel: int):
    """``numel`` elements of a stacked tensor from element ``off``: a layer's slice, by an offset of the replay's own."""
    return None if t is None else t.reshape(-1)[off:off + numel]


# ------------------------------------------------------------------------------------------------ backends
class TorchBackend:
    """The operations of both replays in float64.  dtype = None: nothing is rounded (T and fp32 results stay float64, the split
    stream's upper part is the row itself and its lower part zero); otherwise stores are rounded to T / fp32 where the kernels round
    and the stream is split as include/slime_hip.h says (ops.resid_split / resid_join).  Every tensor it hands back is float64."""

    def __init__(self, dtype=None):
        self.dtype = dtype

    def _t(self, x):
        return x if self.dtype is None else x.to(self.dtype).double()

    def _f(self, x):
        return x if self.dtype is None else x.float().double()

    def _split(self, c):
        if self.dtype is None:
            return c, torch.zeros_like(c)
        from slime_amd import ops
        hi, lo = ops.resid_split(c.float(), self.dtype)
        return hi.double(), lo.double()

    def _join(self, hi, lo):
        if self.dtype is None:
            return hi + lo
        from slime_amd import ops
        return ops.resid_join(hi.to(self.dtype), lo.to(torch.int8)).double()

    @staticmethod
    def _stats(rows):
        g = rows.view(rows.shape[0], -1, 64)
        return torch.stack([g.sum(-1), (g * g).sum(-1)], dim=-1)

    def patch_embed_prenorm(self, pixels, T, cfg, n: int):
        """include/slime_hip.h: pre_layrnorm(cat(cls, conv(pixels)) + pos) -> (x16, lo8 (flat), stats of the ROUNDED rows)."""
        p, D = cfg.patch_size, cfg.hidden_size
        px = self._t(pixels.double())
        x = torch.nn.functional.unfold(px, kernel_size=p, stride=p).transpose(1, 2)                 # [n, P, 3 p p], (c, ky, kx) order
        x = x @ T["patch_w"].double()[:, :x.shape[-1]].t()
        h = torch.cat([T["cls"].double().expand(n, 1, D), x], dim=1) + T["pos"].double()[None, :x.shape[1] + 1]
        mu = h.mean(-1, keepdim=True)
        var = ((h - mu) ** 2).mean(-1, keepdim=True)
        h = self._f(((h - mu) / torch.sqrt(var + cfg.layer_norm_eps) * T["pre_ln_w"].double() + T["pre_ln_b"].double()).reshape(-1, D))
        hi, lo = self._split(h)
        return hi, lo.reshape(-1).clone(), self._stats(hi)

    def gemm_fold(self, A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits=1):
        """The LayerNorm-fold consumer: epi(rstd (A W'^T - mu colsum) + b') with mu / rstd from the row's partial sums."""
        w = _flat(T[name], w_off, N * K).view(N, K).double()
        bias = _flat(T["b_" + name[2:]], b_off, N).double()
        cs = _flat(T[colsum_name], b_off, N).double()
        st = stats.reshape(A.shape[0], -1, 2)
        mu = st[..., 0].sum(1, keepdim=True) / K
        var = st[..., 1].sum(1, keepdim=True) / K - mu * mu
        y = (A.double() @ w.t() - mu * cs) / torch.sqrt(var + eps) + bias
        if epilogue == EPI_BIAS_QUICKGELU_T:
            y = y * torch.sigmoid(1.702 * y)
        return self._t(y)

    def gemm_resid_split(self, A, T, name, w_off, N, K, b_off, xn, lo, ldlo, splits=1):
        """SLIME_EPI_BIAS_RESID_SPLIT_LN: c = A W^T + b + join(xn, lo); xn, lo = split(c) in place (row r of the lower part at
        ldlo * r bytes); returns the partial sums of the UNROUNDED c."""
        w = _flat(T[name], w_off, N * K).view(N, K).double()
        bias = _flat(T["b_" + name[2:]], b_off, N).double()
        M = A.shape[0]
        idx = torch.arange(M)[:, None] * ldlo + torch.arange(N)[None, :]
        c = self._f(A.double() @ w.t() + bias + self._join(xn, lo[idx]))
        hi, l8 = self._split(c)
        xn.copy_(hi)
        if ldlo >= N:
            lo[idx] = l8
        else:                                            # overlapping rows (a wrong stride): stored in row order
            for r in range(M):
                lo[idx[r]] = l8[r]
        return self._stats(c)

    def attention_packed(self, qkv, q_col, k_col, v_col, n, S, heads, dh):
        """slime_attention on three column blocks of one [n S, ld] buffer; q in log2 units."""
        D = heads * dh
        blk = lambda c: qkv[:, c:c + D].double().reshape(n, S, heads, dh).transpose(1, 2)
        p = torch.softmax((blk(q_col) @ blk(k_col).transpose(-1, -2)) * LN2, dim=-1)
        return self._t((p @ blk(v_col)).transpose(1, 2).reshape(n * S, D))

    def gather_rows_split(self, xn, lo, rows_in, row_off, groups, rows_out, out_dtype):
        D = xn.shape[1]
        h = self._join(xn, lo[:xn.numel()].view_as(xn)).view(groups, rows_in, D)[:, row_off:row_off + rows_out]
        h = h.reshape(groups * rows_out, D)
        return h if self.dtype is None else h.to(out_dtype).double()

    # ---- the Llama layer
    def gemm(self, A, T, name, bias, epilogue, out=None, resid=None):
        acc = A.double() @ T[name].double().t()
        if epilogue == EPI_BIAS_RESID_T:
            acc = acc + resid.double()
        r = self._f(acc) if epilogue == EPI_BIAS_F32 else self._t(acc)
        if out is None:
            return r
        out.copy_(r)
        return out

    def rope(self, qkv, pos, n_rot_heads, n_q_heads, dh, inv_freq, q_scale):
        """include/slime_hip.h slime_rope: angle = (float)pos * inv_freq in fp32 (the reference's definition), rotate_half, the q
        heads scaled by q_scale; in place on the first n_rot_heads heads of every row."""
        ang = (pos.to(torch.float32)[:, None] * inv_freq.float()[None, :]).double()
        cos, sin = torch.cat([ang.cos()] * 2, -1)[:, None], torch.cat([ang.sin()] * 2, -1)[:, None]
        x = qkv[:, :n_rot_heads * dh].double().view(-1, n_rot_heads, dh)
        rot = torch.cat([-x[..., dh // 2:], x[..., :dh // 2]], -1)
        y = x * cos + rot * sin
        y[:, :n_q_heads] *= q_scale
        qkv[:, :n_rot_heads * dh] = self._t(y.reshape(-1, n_rot_heads * dh))

    def prefill_attention(self, qkv, q_col, k_col, v_col, batch, S, HQ, HKV, dh, kv_start, kv_len):
        """slime_prefill_attention: causal GQA inside [kv_start, kv_start + kv_len), zero rows outside; q in log2 units."""
        q = qkv[:, q_col:q_col + HQ * dh].double().view(batch, S, HQ, dh)
        k = qkv[:, k_col:k_col + HKV * dh].double().view(batch, S, HKV, dh).repeat_interleave(HQ // HKV, dim=2)
        v = qkv[:, v_col:v_col + HKV * dh].double().view(batch, S, HKV, dh).repeat_interleave(HQ // HKV, dim=2)
        out = torch.zeros(batch, S, HQ * dh, dtype=torch.float64)
        for b in range(batch):
            s0, ln = (0, S) if kv_start is None else (int(kv_start[b]), int(kv_len[b]))
            if ln <= 0:
                continue
            sl = slice(s0, s0 + ln)
            lg = (q[b, sl].transpose(0, 1) @ k[b, sl].transpose(0, 1).transpose(1, 2)) * LN2
            lg = lg.masked_fill(~torch.ones(ln, ln, dtype=torch.bool).tril(), float("-inf"))
            out[b, sl] = (torch.softmax(lg, -1) @ v[b, sl].transpose(0, 1)).transpose(0, 1).reshape(ln, HQ * dh)
        return self._t(out.view(batch * S, HQ * dh))


class HipBackend(AC.HipBackend):
    """adapter_conformance.HipBackend (its GEMM and attention wrappers, its kernel list) plus the launches only the tower and the
    Llama layer make: the fused front end, the two LayerNorm-fold GEMM forms (optionally as slime_gemm_ksplit), attention on column
    blocks of one buffer, the split-stream gather, RoPE and the causal attention."""

    def _gemm_ex(self, name, wname, frag, splits, **f):
        buf = C.create_string_buffer(128)
        self._ok(self.lib.slime_gemm_kernel_name(f["M"], f["N"], f["K"], f["dtype"], f["epilogue"], int(frag), buf, 128), "kernel_name")
        self.kernels.append((name, f["M"], f["N"], f["K"], f["epilogue"], buf.value.decode()))
        g = self._lib.GemmArgs(**f)
        if splits == 1:
            self._ok(self.lib.slime_gemm_ex(C.byref(g), self._s()), f"slime_gemm_ex {wname}")
            return
        need = self.lib.slime_gemm_ksplit_workspace_bytes(f["M"], f["N"], splits)
        ws = AC.GuardedWorkspace(need, self.dev)
        self._ok(self.lib.slime_gemm_ksplit(C.byref(g), splits, ws.ptr(), need, self._s()), f"slime_gemm_ksplit {wname}")
        assert ws.intact(), "slime_gemm_ksplit wrote outside its workspace"

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def patch_embed_prenorm(self, pixels, T, cfg, n: int):
        D, M = cfg.hidden_size, n * cfg.seq_len
        kpad = (3 * cfg.patch_size ** 2 + 63) // 64 * 64
        xn = torch.empty(M, D, dtype=self.dtype, device=self.dev)
        lo = torch.empty(M * D, dtype=torch.int8, device=self.dev)
        stats = torch.empty(M, D // 64, 2, dtype=torch.float32, device=self.dev)
        self._ok(self.lib.slime_patch_embed_prenorm(pixels.data_ptr(), self.code(pixels.dtype), T["patch_w_frag"].data_ptr(), T["cls"].data_ptr(),
                                                    T["pos"].data_ptr(), T["pre_ln_w"].data_ptr(), T["pre_ln_b"].data_ptr(),
                                                    float(cfg.layer_norm_eps), None, xn.data_ptr(), lo.data_ptr(), stats.data_ptr(),
                                                    self.code(self.dtype), n, cfg.image_size, cfg.patch_size, kpad, D, self._s()),
                 "slime_patch_embed_prenorm")
        return xn, lo, stats

    def gemm_fold(self, A, stats, T, name, w_off, N, K, b_off, colsum_name, eps, epilogue, splits=1):
        w, wf = _flat(T.get(name), w_off, N * K), _flat(T.get(name + "_frag"), w_off, N * K)
        M = A.shape[0]
        out = torch.empty(M, N, dtype=self.dtype, device=self.dev)
        st = stats.reshape(-1)
        self._gemm_ex(name, name, wf is not None, splits, A=A.data_ptr(), lda=A.stride(0), B=self._p(w),
                      bias=_flat(T["b_" + name[2:]], b_off, N).data_ptr(), C=out.data_ptr(), ldc=N, M=M, N=N, K=K, dtype=self.code(self.dtype),
                      epilogue=epilogue, ln_stats=st.data_ptr(), ln_groups=K // 64, ln_colsum=_flat(T[colsum_name], b_off, N).data_ptr(),
                      ln_eps=float(eps), B_frag=self._p(wf))
        return out

    def gemm_resid_split(self, A, T, name, w_off, N, K, b_off, xn, lo, ldlo, splits=1):
        w, wf = _flat(T.get(name), w_off, N * K), _flat(T.get(name + "_frag"), w_off, N * K)
        M = A.shape[0]
        stats = torch.empty(M, N // 64, 2, dtype=torch.float32, device=self.dev)
        self._gemm_ex(name, name, wf is not None, splits, A=A.data_ptr(), lda=A.stride(0), B=self._p(w),
                      bias=_flat(T["b_" + name[2:]], b_off, N).data_ptr(), C=xn.data_ptr(), ldc=xn.stride(0), M=M, N=N, K=K,
                      dtype=self.code(self.dtype), epilogue=EPI_BIAS_RESID_SPLIT_LN, stats_out=stats.data_ptr(), B_frag=self._p(wf),
                      lo8=lo.data_ptr(), ldlo=ldlo)
        return stats

    def attention_packed(self, qkv, q_col, k_col, v_col, n, S, heads, dh):
        ld, es, D = qkv.stride(0), qkv.element_size(), heads * dh
        o = torch.empty(n * S, D, dtype=qkv.dtype, device=qkv.device)
        base = qkv.data_ptr()
        self._ok(self.lib.slime_attention(base + q_col * es, S * ld, ld, base + k_col * es, S * ld, ld, base + v_col * es, S * ld, ld,
                                          o.data_ptr(), S * D, D, n, heads, dh, S, S, self.code(qkv.dtype), self._s()), "slime_attention")
        return o

    def gather_rows_split(self, xn, lo, rows_in, row_off, groups, rows_out, out_dtype):
        D = xn.shape[1]
        out = torch.empty(groups * rows_out, D, dtype=out_dtype, device=xn.device)
        self._ok(self.lib.slime_gather_rows_split(xn.data_ptr(), lo.data_ptr(), self.code(xn.dtype), rows_in, row_off, out.data_ptr(),
                                                  self.code(out_dtype), groups, rows_out, D, self._s()), "slime_gather_rows_split")
        return out

    # ---- the Llama layer (the two plain GEMMs are adapter_conformance.HipBackend.gemm)
    def gemm(self, A, T, name, bias, epilogue, out=None, resid=None):
        if epilogue != EPI_BIAS_RESID_T:
            return super().gemm(A, T, name, bias, epilogue, out=out)
        w, wf = T.get(name), T.get(name + "_frag")
        M, K = A.shape
        N = (w if w is not None else wf).shape[0]
        if out is None:
            out = torch.empty(M, N, dtype=A.dtype, device=A.device)
        self._gemm_ex(name, name, wf is not None, 1, A=A.data_ptr(), lda=A.stride(0), B=self._p(w), bias=None, C=out.data_ptr(), ldc=N, M=M,
                      N=N, K=K, dtype=self.code(A.dtype), epilogue=epilogue, B_frag=self._p(wf), resid=resid.data_ptr(), ldr=resid.stride(0))
        return out

    def rope(self, qkv, pos, n_rot_heads, n_q_heads, dh, inv_freq, q_scale):
        self._ok(self.lib.slime_rope(qkv.data_ptr(), qkv.stride(0), pos.data_ptr(), qkv.shape[0], n_rot_heads, n_q_heads, dh,
                                     inv_freq.data_ptr(), float(q_scale), self.code(qkv.dtype), self._s()), "slime_rope")

    def prefill_attention(self, qkv, q_col, k_col, v_col, batch, S, HQ, HKV, dh, kv_start, kv_len):
        ld, es = qkv.stride(0), qkv.element_size()
        o = torch.empty(batch * S, HQ * dh, dtype=qkv.dtype, device=qkv.device)
        base = qkv.data_ptr()
        self._ok(self.lib.slime_prefill_attention(base + q_col * es, S * ld, ld, base + k_col * es, S * ld, ld, base + v_col * es, S * ld, ld,
                                                  o.data_ptr(), S * HQ * dh, HQ * dh, batch, HQ, HKV, dh, S, self._p(kv_start),
                                                  self._p(kv_len), self.code(qkv.dtype), self._s()), "slime_prefill_attention")
        return o


# ------------------------------------------------------------------------------------------------ replays
def replay_vit(be, T, cfg, pixels, layers_run: int, *, keep_cls: int = 0, out_dtype=torch.float32, want_out: bool = True,
               want_hidden: bool = False, want_states: bool = False, k_split=(1, 1, 1, 1), broken: Optional[str] = None):
    """csrc/api.hip vit_run on pixels [n, 3, image, image] (fp32 or T) -> {"out": [n (S | P), D] out_dtype, "hidden": fp32 [n S, D],
    "states": fp32 [layers_run + 1, n S, D]} (the requested ones).  The residual stream (xn, lo) is updated in place by the two
    split-residual GEMMs of a layer, as the header says of that epilogue; stats, qkv, ctx and ff are new tensors at every launch."""
    n = pixels.shape[0]
    g = cfg.image_size // cfg.patch_size
    P = g * g
    S, D, F = P + 1, cfg.hidden_size, cfg.intermediate_size
    M, G, heads = n * S, D // 64, cfg.num_attention_heads
    eps = cfg.layer_norm_eps
    ldlo = D // 2 if broken == "ldlo_in_elements_of_T" else D             # bytes: one signed byte per element
    q_col, k_col, v_col = (0, 2 * D, D) if broken == "kv_columns_swapped" else (0, D, 2 * D)
    sq, so, s1, s2 = k_split
    res = {}
    xn, lo, stats = be.patch_embed_prenorm(pixels, T, cfg, n)
    states = [None] * (layers_run + 1)
    states[0] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32) if want_states else None

    def plane(st):
        """The statistics the consumer reads: [M, G, 2] from the first float (the wrong variant: from the second group's)."""
        st = st.reshape(-1)
        return torch.cat([st[2:], st[:2]]) if broken == "stats_group_plus_1" else st

    for l in range(layers_run):
        ls = (l + 1) % layers_run if broken == "layer_slice_plus_1" else l
        qkv = be.gemm_fold(xn, plane(stats), T, "w_qkv", ls * 3 * D * D, 3 * D, D, ls * 3 * D, "colsum_qkv", eps, EPI_BIAS_T, sq)
        if broken == "ctx_over_qkv":
            flat = qkv.view(-1)
            for b in reversed(range(n)):
                flat[b * S * D:(b + 1) * S * D] = be.attention_packed(qkv[b * S:(b + 1) * S], q_col, k_col, v_col, 1, S, heads, 64).view(-1)
            ctx = flat[:M * D].view(M, D).clone()
        else:
            ctx = be.attention_packed(qkv, q_col, k_col, v_col, n, S, heads, 64)
        stats = be.gemm_resid_split(ctx, T, "w_o", ls * D * D, D, D, ls * D, xn, lo, ldlo, so)
        ff = be.gemm_fold(xn, plane(stats), T, "w_fc1", ls * F * D, F, D, ls * F, "colsum_fc1", eps, EPI_BIAS_QUICKGELU_T, s1)
        stats = be.gemm_resid_split(ff, T, "w_fc2", ls * D * F, D, F, ls * D, xn, lo, ldlo, s2)
        if want_states:
            states[l if broken == "snapshot_index_minus_1" else l + 1] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32)
    if want_states:
        res["states"] = states
    if want_hidden:
        res["hidden"] = be.gather_rows_split(xn, lo, S, 0, n, S, torch.float32)
    if want_out:
        row_off = 0 if keep_cls or broken == "cls_drop_at_row_0" else 1
        res["out"] = be.gather_rows_split(xn, lo, S, row_off, n, S if keep_cls else P, out_dtype)
    return res


def llama_q_scale() -> float:
    """llama_attn_run's q scale: the fp32 product of the two fp32 constants 128^-0.5 and log2(e)."""
    f = torch.tensor([0.08838834764831845, 1.4426950408889634], dtype=torch.float32)
    return float(f[0] * f[1])


def replay_llama_attn(be, T, hidden: int, n_heads: int, n_kv_heads: int, x, pos, kv_start, kv_len, batch: int, S: int, *, epilogue: int,
                      resid=None, out=None, broken: Optional[str] = None):
    """csrc/prefill.hip llama_attn_run on x T [batch S, hidden], pos int32 [batch S]: the q/k/v GEMM (no bias), RoPE in place on the
    q and k heads of the packed rows, causal GQA attention on three column blocks of them, o_proj with epilogue BIAS_T, BIAS_F32 or
    BIAS_RESID_T (``resid``; ``out`` may be ``resid``)."""
    dh = 128
    HQ, HKV = n_heads, n_kv_heads
    k_col, v_col = HQ * dh, (HQ + HKV) * dh
    if broken == "kv_columns_swapped":
        k_col, v_col = v_col, k_col
    qkv = be.gemm(x, T, "w_qkv", None, EPI_BIAS_T)
    assert tuple(qkv.shape) == (batch * S, (HQ + 2 * HKV) * dh)
    be.rope(qkv, pos, HQ + HKV, HQ, dh, T["inv_freq"], llama_q_scale())
    ctx = be.prefill_attention(qkv, 0, k_col, v_col, batch, S, HQ, HKV, dh, kv_start, kv_len)
    return be.gemm(ctx, T, "w_o", None, epilogue, out=out, resid=resid)




# ------------------------------------------------------------------------------------------------ float64 forward-error bounds
# Running first-order bounds, one number per row: E[r] >= ||computed row r - exact row r||_2 (hence >= every element's error).
# An input error passes a step through that step's Lipschitz constant in the 2-norm (||W||_2 for a Linear, 2 rstd max|gamma| for a
# LayerNorm, the softmax Jacobian for attention); the step's own rounding is bounded element by element with the textbook
# gamma_k = k u / (1 - k u) of a k-term sum (Higham, Accuracy and Stability, ch. 3) and enters as that row's 2-norm.  Products of
# two error terms are dropped (they are u times smaller than what is kept).  No constant here was measured.
def _gam(k, u):
    return k * u / (1 - k * u)


def _rn(t):
    return t.norm(dim=-1, keepdim=True)


def _spec(W):
    return float(torch.linalg.matrix_norm(W.double(), 2))


def _lin_err(x, E, W, b, u, extra: int = 1):
    """Row error of fl(x W^T + b) for rows within E of x: ||W||_2 E + || gamma_{K + extra} (|x| |W|^T + |b|) ||_2."""
    return _spec(W) * E + _rn(_gam(W.shape[1] + extra, u) * (x.abs() @ W.abs().t() + (0 if b is None else b.abs())))


def _ln_err(x, E, w, b, eps, u):
    """(y, row error) of y = (x - mu) rstd w + b by two passes.  Input error: d = x - mu is a projection of x (||dd|| <= E), var =
    |d|^2 / D moves by at most 2 |d| E / D, rstd = (var + eps)^-1/2 by at most rstd^3 |d| E / D, and rstd^2 |d|^2 / D <= 1, so
    ||d(d rstd)|| <= rstd E + |d| rstd^3 |d| E / D <= 2 rstd E.  Rounding: mean gamma_D, d one subtraction, var gamma_{D+2},
    rstd three operations, the scale and shift four."""
    D = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    r = (var + eps) ** -0.5
    y = d * r * w + b
    dd = _gam(D, u) * x.abs().mean(-1, keepdim=True) + u * d.abs()
    dvar = (2 * d.abs() * dd).mean(-1, keepdim=True) + _gam(D + 2, u) * var
    dr = 0.5 * r ** 3 * dvar + 3 * u * r
    rounding = w.abs() * (r * dd + d.abs() * dr) + 3 * u * (d * r * w).abs() + u * y.abs()
    return y, float(w.abs().max()) * 2 * r * E + _rn(rounding)


def _fold_err(x, E, Wp, cs, bp, dbp, eps, u):
    """(y, row error) of the consumer's formula y = rstd (x W'^T - mu colsum) + b' with mu = sum / K, var = sumsq / K - mu^2.  In exact
    arithmetic it is LayerNorm-without-affine followed by W' (colsum = W' 1), so an input error passes as through ``_ln_err`` and
    ``_lin_err``: ||W'||_2 2 rstd E.  Its own rounding is where the fold differs: the one-pass variance loses gamma_{K+2} mean(x^2)
    + 2 |mu| dmu, not a multiple of var, and the cancellation in acc - mu colsum enters through |x| |W'|^T and |mu colsum|
    separately, not through their difference.  W' carries the pack's two roundings (gamma, row scale): K + 2; dbp = the pack's
    error of b'."""
    K = x.shape[-1]
    mu = x.mean(-1, keepdim=True)
    m2 = (x * x).mean(-1, keepdim=True)
    var = m2 - mu * mu
    r = (var + eps) ** -0.5
    t = x @ Wp.t() - mu * cs
    y = r * t + bp
    dmu = _gam(K, u) * x.abs().mean(-1, keepdim=True)
    dvar = _gam(K + 2, u) * m2 + 2 * mu.abs() * dmu + 3 * u * mu * mu + u * var.abs()
    dr = 0.5 * r ** 3 * dvar + 3 * u * r
    dacc = _gam(K + 2, u) * (x.abs() @ Wp.abs().t())
    dcs = _gam(K + 2, u) * Wp.abs().sum(1)
    dt = dacc + dmu * cs.abs() + mu.abs() * dcs + u * (mu * cs).abs() + u * t.abs()
    rounding = r * dt + t.abs() * dr + u * (r * t).abs() + dbp + u * y.abs()
    return y, _spec(Wp) * 2 * r * E + _rn(rounding)


def _attn_err(q, Eq, k, Ek, v, Ev, scale, u, mask=None):
    """(ctx, row error per head) of softmax(scale q k^T) v on [.., S, dh] operands with row errors [.., S, 1].  A logit moves by at
    most dl_ij = scale (Eq_i |k_j| + |q_i| Ek_j) + scale gamma_{dh+1} (|q| |k|^T)_ij + u |logit_ij|; with m_i = max_j dl_ij the
    softmax Jacobian gives d ctx_i = sum_j p_ij (dl_j - mean_p dl)(v_j - ctx_i), at most 2 m_i sum_j p_ij |v_j - ctx_i|; the values'
    own error passes as sum_j p_ij Ev_j; exp, the S-term sum, the division and the S-term weighted sum round by gamma_{S+6} +
    gamma_S of |p| |v|."""
    S = k.shape[-2]
    lg = scale * (q @ k.transpose(-1, -2))
    dl = scale * (Eq * _rn(k).transpose(-1, -2) + _rn(q) * Ek.transpose(-1, -2) + _gam(q.shape[-1] + 1, u) * (q.abs() @ k.abs().transpose(-1, -2)))
    dl = dl + u * lg.abs()
    if mask is not None:
        lg = lg.masked_fill(~mask, float("-inf"))
        dl = dl.masked_fill(~mask, 0.0)
    p = torch.softmax(lg, -1)
    ctx = p @ v
    m = dl.amax(-1, keepdim=True)
    spread = (p * (v.unsqueeze(-3) - ctx.unsqueeze(-2)).norm(dim=-1)).sum(-1, keepdim=True)        # sum_j p_ij |v_j - ctx_i|
    return ctx, 2 * m * spread + p @ Ev + (_gam(S + 6, u) + _gam(S, u)) * _rn(p @ v.abs())


def tower_error_bound(sd, T, cfg, pixels, layers_run: int, u_ref: float = U64, states=None):
    """Bound of |float64 replay - reference| for every hidden state: a list of [n S, D] (one number per row, repeated along it),
    entry i after i layers.  With ``states`` (float64 [n S, D] each) the bound is LOCAL: entry i + 1 bounds |replay's layer i -
    reference's layer i| when both start from states[i] (no input error), which is how a chain is held link by link; without, the
    errors run through all layers, and since every step passes them with its worst-case Lipschitz constant (attention: the largest
    logit error times the spread of the values) the running bound grows by three to four orders of magnitude per layer.
    It is the sum of two running error bounds carried through the same float64 values,
      * the replay's: unit roundoff 2^-53, both LayerNorms folded (``_fold_err``), logits in log2 units;
      * the reference's: unit roundoff u_ref (2^-53 for the oracle's layer functions evaluated in float64, 2^-24 for
        oracle.tower_forward as it stands), LayerNorm by two passes and then the Linear (``_ln_err``, ``_lin_err``).
    Quick-GELU passes an error with its Lipschitz constant, max |d/dx x sigmoid(1.702 x)| = 1.0998 <= 1.1, and rounds by 8 u |x| (exp,
    add, divide, two products, each within one or two ulp).  A q/k/v row's error bounds each head's share of it; a context row's error
    is the root of the heads' squares."""
    n, D, heads = pixels.shape[0], cfg.hidden_size, cfg.num_attention_heads
    p, eps, dh = cfg.patch_size, cfg.layer_norm_eps, 64
    S = (cfg.image_size // p) ** 2 + 1
    X = torch.nn.functional.unfold(pixels.double(), kernel_size=p, stride=p).transpose(1, 2)
    pw = sd["embeddings.patch_embedding.weight"].double().reshape(D, -1)
    cls, pos = sd["embeddings.class_embedding"].double(), sd["embeddings.position_embedding.weight"].double()[:S]
    h0 = torch.cat([cls.expand(n, 1, D), X @ pw.t()], 1) + pos
    zero = torch.zeros(n, X.shape[1], 1, dtype=torch.float64)
    start = []
    for u in (U64, u_ref):
        e = torch.cat([torch.zeros(n, 1, 1, dtype=torch.float64), _lin_err(X, zero, pw, None, u)], 1) + u * _rn(h0)
        h, e = _ln_err(h0, e, sd["pre_layrnorm.weight"].double(), sd["pre_layrnorm.bias"].double(), eps, u)
        start.append(e.reshape(-1, 1))
    h, (ef, ed) = h.reshape(-1, D), start
    out = [(ef + ed).expand(-1, D).contiguous()]
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = dh ** -0.5 * LOG2E
    heads_of = lambda t: t.reshape(n, S, heads, dh).transpose(1, 2)
    per_head = lambda E: E.reshape(n, 1, S, 1).expand(n, heads, S, 1)
    join = lambda E: (E * E).sum(1).sqrt().reshape(-1, 1)                       # [n, heads, S, 1] -> [n S, 1]
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
        # q/k/v and attention: the replay's path (fold; the three column blocks' errors are each bounded by the row's)
        dbp = _gam(D + 2, U64) * rs * (b.abs() + W.abs() @ b1.abs())
        yf, Ef = _fold_err(h, ef, T["w_qkv"][l].double(), T["colsum_qkv"][l].double(), T["b_qkv"][l].double(), dbp, eps, U64)
        qf, kf, vf = (heads_of(yf[:, i * D:(i + 1) * D]) for i in range(3))
        _, Ecf = _attn_err(qf, per_head(Ef), kf, per_head(Ef), vf, per_head(Ef), LN2, U64)
        # the reference's path
        x1, Ex1 = _ln_err(h, ed, g1, b1, eps, u_ref)
        yd, Ed = x1 @ W.t() + b, _lin_err(x1, Ex1, W, b, u_ref)
        qd, kd, vd = (heads_of(yd[:, i * D:(i + 1) * D]) for i in range(3))
        cd, Ecd = _attn_err(qd, per_head(Ed), kd, per_head(Ed), vd, per_head(Ed), dh ** -0.5, u_ref)
        ctx = cd.transpose(1, 2).reshape(-1, D)
        h1 = h + ctx @ Wo.t() + bo
        ef = ef + _lin_err(ctx, join(Ecf), Wo, bo, U64) + 2 * U64 * _rn(h1)
        ed = ed + _lin_err(ctx, join(Ecd), Wo, bo, u_ref) + 2 * u_ref * _rn(h1)
        # the MLP
        dbp = _gam(D + 2, U64) * (c1.abs() + W1.abs() @ b2.abs())
        _, Ezf = _fold_err(h1, ef, T["w_fc1"][l].double(), T["colsum_fc1"][l].double(), T["b_fc1"][l].double(), dbp, eps, U64)
        x2, Ex2 = _ln_err(h1, ed, g2, b2, eps, u_ref)
        z, Ezd = x2 @ W1.t() + c1, _lin_err(x2, Ex2, W1, c1, u_ref)
        a = z * torch.sigmoid(1.702 * z)
        Eaf, Ead = 1.1 * Ezf + 8 * U64 * _rn(z), 1.1 * Ezd + 8 * u_ref * _rn(z)
        h2 = h1 + a @ W2.t() + c2
        ef = ef + _lin_err(a, Eaf, W2, c2, U64) + 2 * U64 * _rn(h2)
        ed = ed + _lin_err(a, Ead, W2, c2, u_ref) + 2 * u_ref * _rn(h2)
        h = h2
        out.append((ef + ed).expand(-1, D).contiguous())
    return out


def llama_error_bound(wq, wk, wv, wo, x, pos, n_heads, n_kv_heads, kv_start, kv_len, inv_freq, u_ref: float = U64):
    """Bound of |float64 replay - oracle.prefill_oracle.llama_attention_forward on float64 operands| [B S, D], one number per row.
    Both evaluate the same sequence (projections, RoPE, causal GQA softmax, o_proj), so the bound is that sequence's running error
    at 2^-53 plus the same at u_ref, plus what separates the two RoPE tables: the oracle's cos / sin are fp32 (LlamaRotaryEmbedding),
    the replay's are the float64 cos / sin of the same fp32 angle; an fp32 entry lies within two fp32 ulp of the true value, within
    2^-23 in absolute terms since |cos|, |sin| <= 1.  A rotation keeps a head's 2-norm, so RoPE passes a row error unchanged and adds
    (2 table error + 3 u) |head|."""
    B, S, D = x.shape
    dh, g = 128, n_heads // n_kv_heads
    x = x.double().reshape(B * S, D)
    ang = (pos.reshape(-1).to(torch.float32)[:, None] * inv_freq.float()[None, :]).double()
    cos, sin = torch.cat([ang.cos()] * 2, -1)[:, None], torch.cat([ang.sin()] * 2, -1)[:, None]
    zero = torch.zeros(B * S, 1, dtype=torch.float64)
    total = 0
    for u, tab in ((U64, 0.0), (u_ref, 2.0 ** -23)):
        proj = []
        for w, nh in ((wq, n_heads), (wk, n_kv_heads), (wv, n_kv_heads)):
            y = (x @ w.double().t()).view(B * S, nh, dh)
            E = _lin_err(x, zero, w.double(), None, u).view(B * S, 1, 1).expand(B * S, nh, 1)
            proj.append((y, E))
        roped = []
        for y, E in proj[:2]:
            r = y * cos + torch.cat([-y[..., dh // 2:], y[..., :dh // 2]], -1) * sin
            roped.append((r, E + (2 * tab + 3 * u) * _rn(y)))
        shape = lambda t, nh: t.view(B, S, nh, -1).transpose(1, 2)
        (q, Eq), (k, Ek), (v, Ev) = ((shape(t, t.shape[1]), shape(E, t.shape[1])) for t, E in (roped[0], roped[1], proj[2]))
        k, Ek, v, Ev = (t.repeat_interleave(g, dim=1) for t in (k, Ek, v, Ev))
        ctx = torch.zeros(B, S, n_heads * dh, dtype=torch.float64)
        Ectx = torch.zeros(B, S, 1, dtype=torch.float64)
        for b in range(B):
            s0, ln = (0, S) if kv_start is None else (int(kv_start[b]), int(kv_len[b]))
            if ln <= 0:
                continue
            sl = slice(s0, s0 + ln)
            mask = torch.ones(ln, ln, dtype=torch.bool).tril()
            c, Ec = _attn_err(q[b][:, sl], Eq[b][:, sl], k[b][:, sl], Ek[b][:, sl], v[b][:, sl], Ev[b][:, sl], dh ** -0.5, u, mask)
            ctx[b, sl], Ectx[b, sl] = c.transpose(0, 1).reshape(ln, -1), (Ec * Ec).sum(0).sqrt()
        total = total + _lin_err(ctx.view(B * S, -1), Ectx.view(B * S, 1), wo.double(), None, u)
    return total.expand(-1, D).contiguous()
