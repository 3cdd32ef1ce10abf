"""Adapter conformance: the fused adapter entries replayed through the element-wise bounded kernel entries.

The adapter (csrc/api.hip: slime_resampler_forward, slime_mlp_forward, slime_gated_forward, slime_adapter_forward,
slime_adapter_forward_ragged) is glue around kernels that each have an element-wise test of their own: segment offsets into a
stacked operand, crop selection, a 32-bit row map, a workspace whose regions alias in time, the choice between the GEMM's mix
epilogue and slime_gate_premix, the choice between the direct store and fp32 rows + slime_merge_rows_batched.  The kernels are
deterministic and the GEMM dispatch is a function of (M, N, K, dtype, epilogue, operand form), so a test that performs the same
launch sequence through the public C ABI -- the same M, N, K, epilogue and weight pointers at every GEMM, every intermediate in a
tensor of its own, every index computed here in integer torch / Python -- must reproduce the fused entry BIT FOR BIT.  No tolerance
is involved: the kernels' arithmetic is bounded elsewhere (gemm_conformance, attention_conformance, rowwise_conformance), and glue
that is bit-equal to an independent index computation closes the chain.

``replay_*`` restate the five functions of api.hip as calls on a *backend* with seven operations (select_crops, layernorm, gemm,
attention, gate_weights, gate_premix, merge_rows_batched):
  * ``HipBackend``   calls the C ABI; it never sees the library's workspace;
  * ``TorchBackend`` the same operations in float64 with plain torch ops (``dtype=None``: nothing is rounded), for the CPU tests that
                     hold the replay against the oracle and show that the layouts discriminate the broken glue variants.
The index glue (``global_crop_index``, ``local_crop_index``, ``row_map_uniform``, ``ragged_crop_index``, ``ragged_row_map``,
``segments``) takes ``broken=<name>`` for the deliberately wrong versions of BROKEN; ``applies`` says, from the layout alone, where a
variant can show at all.  Importable without a GPU and without the HIP library.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import torch

from gemm_conformance import (EPI_BIAS_F32, EPI_BIAS_GELU_MIX_T, EPI_BIAS_GELU_T, EPI_BIAS_T, Padded, SENTINEL_BYTE, TAIL)

LN2 = math.log(2.0)
DTYPES = (torch.bfloat16, torch.float16)
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


# ------------------------------------------------------------------------------------------------ layouts
@dataclass(frozen=True)
class Layout:
    name: str
    D: int
    heads: int
    H: int
    P: int
    q: int
    n_images: int
    nw: int
    nh: int
    row_major_w1: bool = False         # w1_frag = NULL in the descriptor, the row-major w1 kept: gate_premix although H % 256 == 0
    dtypes: tuple = DTYPES

    @property
    def n_local(self):
        return self.nw * self.nh

    @property
    def g(self):
        return math.isqrt(self.q)

    @property
    def n_crops(self):
        return self.n_images * (1 + self.n_local)

    @property
    def rows_per_image(self):
        return self.P + self.n_local * self.q


LAYOUTS = {
    "a": Layout("a", 128, 1, 256, 16, 4, 3, 2, 3),                   # mix in the GEMM, nw != nh, g = 2
    "b": Layout("b", 128, 2, 128, 9, 1, 2, 3, 1),                    # H % 256 != 0: gate_premix; P % 4 != 0; head_dim 64; g = 1
    "c": Layout("c", 256, 2, 256, 64, 9, 2, 1, 2),                   # the D = 256 LayerNorm instantiations, g = 3
    "d": Layout("d", 128, 1, 256, 16, 4, 4, 0, 0),                   # global-only batch (post = NULL)
    "e": Layout("e", 128, 1, 256, 576, 144, 1, 2, 2, dtypes=(torch.bfloat16,)),     # the product grid once
    "f": Layout("f", 128, 1, 256, 16, 4, 3, 2, 3, row_major_w1=True),               # gate_premix with H % 256 == 0
    # e has head_dim 128 like the product, so its attention is attn_kernel<T, 128, 288> streaming 576 keys in two chunks; attn64r
    # serves head_dim 64 with 321..608 keys only: the same grid with two heads of 64
    "g": Layout("g", 128, 2, 256, 576, 144, 1, 2, 2, dtypes=(torch.bfloat16,)),
}
RAGGED_GRIDS = ([(2, 3), (0, 0), (1, 1), (3, 1)], [(0, 0), (0, 0)], [(1, 2)])       # P, q, D, H of layout a


@dataclass
class Tiny:
    """A packed tiny adapter: the state dict (fp32, for the oracle) and the packed GatedBlock / post_qformer."""
    layout: Layout
    cfg: object
    sd: dict
    pg: object
    post: object
    dtype: torch.dtype


def adapter_config(L: Layout):
    from slime_amd import weights as W
    return W.AdapterConfig(mm_hidden_size=L.D, hidden_size=L.H, head_dim=L.D // L.heads, global_queries=L.P, local_queries=L.q)


def make_tiny(L: Layout, dtype, device, seed: int = 97) -> Tiny:
    """dtype = torch.float32 on the CPU packs the unrounded operands (TorchBackend(None))."""
    from slime_amd import ops, weights as W
    cfg = adapter_config(L)
    sd = W.make_adapter_state_dict(cfg, seed=seed)
    proj = W.sub_state(sd, "mm_projector.")
    pg = ops.pack_gated(proj, cfg, dtype, device)
    post = ops.pack_resampler(W.sub_state(sd, "sampler.post_qformer."), L.D, L.heads, L.P, dtype, device, cfg.ln_eps)
    if L.row_major_w1:
        m = pg.mlp
        w1 = proj["projection.0.weight"].detach().to(device=device, dtype=torch.float32).to(dtype).contiguous()
        m.tensors["w1"], m.tensors["w1_frag"] = w1, None
        m.desc.w1, m.desc.w1_frag = w1.data_ptr(), None
    return Tiny(L, cfg, sd, pg, post, dtype)


def make_feats(n_crops: int, P: int, D: int, dtype=None, seed: int = 5) -> torch.Tensor:
    """Tower-like features (unit-variance tokens with a per-crop offset), rounded to T (dtype = None: fp32, unrounded)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n_crops, P, D, generator=g) + 0.3 * torch.randn(n_crops, 1, D, generator=g)
    return f if dtype is None else f.to(dtype)


# ------------------------------------------------------------------------------------------------ index glue
BROKEN = ("merge_nw_nh_swapped", "merge_g_minus_1", "global_crop_plus_1", "local_first_0", "seg_attn_seg_x_swapped",
          "mixed_over_first_segment", "local_row0_zero", "stride_is_packed_rows", "ragged_lrow0_of_next_image",
          "ragged_empty_image_counts_one")


def applies(broken: str, *, n_images: int, grids, g: int, merge: bool, learnable_gated: int, padded_stride: bool) -> bool:
    """Whether the wrong glue ``broken`` can change the result at all, from the layout alone (grids: per-image (nw, nh)).
    merge_nw_nh_swapped : the raster order depends on nw only through gx = k % nw, gy = k / nw and the row pitch nw*g; with g = 1 the
                          order is k itself, with nw == nh nothing is swapped.
    merge_g_minus_1     : (gy*(g-1) + qy) differs from (gy*g + qy) only where gy > 0, i.e. nh > 1.
    crop / row0 variants: need local crops.   segment variants: need both experts (learnable_gated < 0).
    stride_is_packed_rows: needs a second image and a token buffer wider than an image's rows.
    ragged_lrow0_of_next_image: needs an image with local rows that is not the last such image.
    ragged_empty_image_counts_one: needs an image behind an empty one."""
    n = [nw * nh for nw, nh in grids]
    any_local = any(n)
    if broken == "merge_nw_nh_swapped":
        return merge and g > 1 and any(nw != nh for nw, nh in grids if nw * nh)
    if broken == "merge_g_minus_1":
        return merge and any(nh > 1 for nw, nh in grids)
    if broken in ("global_crop_plus_1", "local_first_0", "local_row0_zero"):
        return any_local
    if broken in ("seg_attn_seg_x_swapped", "mixed_over_first_segment"):
        return learnable_gated < 0
    if broken == "stride_is_packed_rows":
        return n_images > 1 and padded_stride
    if broken == "ragged_lrow0_of_next_image":
        return sum(1 for x in n if x) > 1
    if broken == "ragged_empty_image_counts_one":
        return any(x == 0 for x in n[:-1])
    raise KeyError(broken)


def global_crop_index(n_images: int, n_local: int, broken: Optional[str] = None):
    """Index in feats [n_images * (1 + n_local), P, D] of every image's global crop."""
    period = 1 + n_local
    return [i * period + (1 if broken == "global_crop_plus_1" else 0) for i in range(n_images)]


def local_crop_index(n_images: int, n_local: int, broken: Optional[str] = None):
    """Index in feats of every local crop, image after image."""
    period, first = 1 + n_local, 0 if broken == "local_first_0" else 1
    return [i * period + first + j for i in range(n_images) for j in range(n_local)]


def merged_position(n_local: int, q: int, nw: int, nh: int, merge, broken: Optional[str] = None):
    """d[rr] = position among an image's local token rows of row rr of its [n_local, g, g] compressed crops: the inverse of the
    view(nh, nw, g, g).permute(0, 2, 1, 3) raster order (merge) or rr itself (flat)."""
    rows = n_local * q
    if not merge or rows == 0:
        return list(range(rows))
    g = math.isqrt(q)
    if broken == "merge_nw_nh_swapped":
        nw, nh = nh, nw
    if broken == "merge_g_minus_1":
        out = []
        for rr in range(rows):
            qx, qy, k = rr % g, (rr // g) % g, rr // q
            out.append(((k // nw * (g - 1) + qy) * nw + k % nw) * g + qx)
        return out
    src = torch.arange(rows).reshape(nh, nw, g, g).permute(0, 2, 1, 3).reshape(-1)      # merged row j holds source row src[j]
    d = torch.empty(rows, dtype=torch.long)
    d[src] = torch.arange(rows)
    return d.tolist()


def row_map_uniform(n_images: int, P: int, n_local: int, q: int, nw: int, merge, out_image_stride: int, nh: Optional[int] = None,
                    broken: Optional[str] = None):
    """Token-buffer row of GEMM row r of projection[2]'s output [global rows of every image | local rows of every image]."""
    nh = n_local // nw if nh is None and nw else (nh or 0)
    stride = P + n_local * q if broken == "stride_is_packed_rows" else out_image_stride
    row0 = 0 if broken == "local_row0_zero" else P
    d = merged_position(n_local, q, nw, nh, merge, broken)
    rm = [i * stride + p for i in range(n_images) for p in range(P)]
    rm += [i * stride + row0 + d[rr] for i in range(n_images) for rr in range(n_local * q)]
    return rm


def ragged_crop_index(grids, broken: Optional[str] = None):
    """(global crops, local crops) in feats [sum (1 + n_i), P, D] for per-image grids (nw_i, nh_i)."""
    total = sum(1 + nw * nh for nw, nh in grids)
    gi, li, c = [], [], 0
    for nw, nh in grids:
        n = nw * nh
        gi.append(c % total)
        li += [(c + 1 + j) % total for j in range(n)]
        c += 1 + (max(n, 1) if broken == "ragged_empty_image_counts_one" else n)
    return gi, li


def ragged_row_map(grids, P: int, q: int, merge, out_row0=None, broken: Optional[str] = None):
    """ops.adapter_ragged_plan's row map as a list (the plan is restated there once; not again here)."""
    from slime_amd import ops
    row0, rows, row_map = ops.adapter_ragged_plan(grids, P, q, bool(merge), out_row0)
    B = len(grids)
    n = [nw * nh * q for nw, nh in grids]
    rm = [row_map(r) for r in range(B * P + sum(n))]
    if broken == "ragged_lrow0_of_next_image" and sum(n):
        loc, lrow0 = rm[B * P:], [0]
        for x in n:
            lrow0.append(lrow0[-1] + x)
        rm = rm[:B * P] + [loc[(lrow0[b + 1] + rr) % len(loc)] for b in range(B) for rr in range(n[b])]
    return row0, rows, rm


def segments(learnable_gated: int, rows_g: int, rows_l: int):
    """Row offsets (seg_x, seg_attn, seg_local, rows_all) of [T(x_global) | attn(x_global) | post_qformer(x_local)]; -1: dropped."""
    row, seg_x, seg_attn, seg_local = 0, -1, -1, -1
    if learnable_gated != 1:
        seg_x, row = row, row + rows_g
    if learnable_gated != 0:
        seg_attn, row = row, row + rows_g
    if rows_l:
        seg_local, row = row, row + rows_l
    return seg_x, seg_attn, seg_local, row


def mix_in_gemm(pm) -> bool:
    """api.hip's mix_in_gemm: the GatedBlock mix happens in projection[0]'s epilogue iff the descriptor has w1_frag, H % 256 == 0."""
    return pm.tensors.get("w1_frag") is not None and pm.hidden % 256 == 0 and pm.in_dim % 64 == 0


# ------------------------------------------------------------------------------------------------ backends
class TorchBackend:
    """The seven operations in float64.  dtype = None: no rounding anywhere (T and fp32 results stay float64); otherwise results
    are rounded to T / fp32 where the kernels round."""

    def __init__(self, dtype=None):
        self.dtype = dtype

    def _t(self, x):
        return x if self.dtype is None else x.to(self.dtype)

    def _f(self, x):
        return x if self.dtype is None else x.to(torch.float32)

    def out_dtype(self, dt):
        return torch.float64 if self.dtype is None else dt

    def empty_t(self, rows, cols, device):
        return torch.zeros(rows, cols, dtype=self.out_dtype(self.dtype), device=device)

    def to_f32(self, x):
        return self._f(x.double())

    def select_crops(self, crops):
        x = crops.reshape(-1, crops.shape[-1])
        return self._f(x.double()), self._t(x.double())

    def layernorm(self, x, w, b, eps, normalize, want_f32, want_t, add=None, add_period=0):
        y = x.double()
        if normalize:
            mu = y.mean(-1, keepdim=True)
            var = ((y - mu) ** 2).mean(-1, keepdim=True)
            y = (y - mu) / torch.sqrt(var + eps) * w.double() + b.double()
        t2 = None
        if add is not None:
            t2 = self._t(y + add.double().repeat(y.shape[0] // add_period, 1))
        return (self._f(y) if want_f32 else None), (self._t(y) if want_t else None), t2

    def gemm(self, A, T, name, bias, epilogue, out=None, row_map=None, A2=None, gates=None):
        w = T[name].double()
        acc = A.double() @ w.t() + bias.double()
        if epilogue == EPI_BIAS_T:
            r = self._t(acc)
        elif epilogue == EPI_BIAS_GELU_T:
            r = self._t(torch.nn.functional.gelu(acc))
        elif epilogue == EPI_BIAS_F32:
            r = self._f(acc)
        elif epilogue == EPI_BIAS_GELU_MIX_T:
            acc2 = A2.double() @ w.t() + bias.double()
            gl = torch.nn.functional.gelu
            r = self._t(gates[:, 0:1].double() * gl(acc) + gates[:, 1:2].double() * gl(acc2))
        else:
            raise KeyError(epilogue)
        if out is None:
            return r
        idx = torch.arange(r.shape[0]) if row_map is None else torch.as_tensor(row_map, dtype=torch.long)
        out[idx] = r.to(out.dtype)
        return out

    def attention(self, q_proj, k, v, heads, dh):
        n, nkv, D = k.shape
        nq = q_proj.shape[0]
        q = q_proj.double().view(nq, heads, dh).transpose(0, 1)                             # [h, nq, dh], log2 units
        kk = k.double().view(n, nkv, heads, dh).transpose(1, 2)
        vv = v.double().view(n, nkv, heads, dh).transpose(1, 2)
        p = torch.softmax((q.unsqueeze(0) @ kk.transpose(-1, -2)) * LN2, dim=-1)
        return self._t((p @ vv).transpose(1, 2).reshape(n, nq, D))

    def gate_weights(self, x, w_gate):
        p = torch.softmax(x.double() @ w_gate.double(), dim=1)
        return self._f(p / (p.sum(1, keepdim=True) + 1e-6))

    def gate_premix(self, x, w_gate, a0, a1, out):
        p = torch.softmax(x.double() @ w_gate.double(), dim=1)
        g = p / (p.sum(1, keepdim=True) + 1e-6)
        out.copy_(self._t(g[:, 0:1] * a0.double() + g[:, 1:2] * a1.double()))
        return out

    def merge_rows_batched(self, x, in_image_stride, out, out_image_stride, dst_row0, images, nw, nh, g, merge):
        """include/slime_hip.h: image b reads in + b*in_image_stride rows, writes out rows b*out_image_stride + dst_row0 + d."""
        rows = nw * nh * g * g
        for b in range(images):
            for rr in range(rows):
                d = rr
                if merge:
                    qx, qy, k = rr % g, (rr // g) % g, rr // (g * g)
                    d = ((k // nw * g + qy) * nw + k % nw) * g + qx
                out[b * out_image_stride + dst_row0 + d] = x[b * in_image_stride + rr].to(out.dtype)


class HipBackend:
    """The seven operations through the C ABI, every result in a tensor of the test's own.  ``kernels`` collects the GEMM kernel
    (slime_gemm_kernel_name) of every GEMM call in order."""

    def __init__(self, dtype, device):
        from slime_amd import _lib, ops
        self.lib, self._lib, self.dtype, self.dev = _lib.load(), _lib, dtype, device
        self.code = ops.dtype_code
        self.kernels = []

    def _s(self):
        return torch.cuda.current_stream().cuda_stream

    def _ok(self, rc, what):
        self._lib.check(rc, what)

    def out_dtype(self, dt):
        return dt

    def empty_t(self, rows, cols, device):
        return torch.empty(rows, cols, dtype=self.dtype, device=device)

    def to_f32(self, x):
        return x.float()

    def select_crops(self, crops):
        crops = crops.contiguous()
        n, P, D = crops.shape
        o32 = torch.empty(n * P, D, dtype=torch.float32, device=crops.device)
        ot = torch.empty(n * P, D, dtype=crops.dtype, device=crops.device)
        self._ok(self.lib.slime_select_crops(crops.data_ptr(), self.code(crops.dtype), P, D, 1, 0, 1, n, o32.data_ptr(), ot.data_ptr(),
                                             self._s()), "slime_select_crops")
        return o32, ot

    def layernorm(self, x, w, b, eps, normalize, want_f32, want_t, add=None, add_period=0):
        rows, D = x.shape
        assert x.dtype == torch.float32 and x.stride(1) == 1
        mk = lambda dt: torch.empty(rows, D, dtype=dt, device=x.device)
        o32 = mk(torch.float32) if want_f32 else None
        ot = mk(self.dtype) if want_t else None
        ot2 = mk(self.dtype) if add is not None else None
        p = lambda t: None if t is None else t.data_ptr()
        self._ok(self.lib.slime_layernorm(x.data_ptr(), x.stride(0), rows, D, p(w), p(b), float(eps), int(normalize), p(o32), p(ot), p(ot2),
                                          p(add), int(add_period), self.code(self.dtype), self._s()), "slime_layernorm")
        return o32, ot, ot2

    def gemm(self, A, T, name, bias, epilogue, out=None, row_map=None, A2=None, gates=None):
        w, wf = T.get(name), T.get(name + "_frag")
        M, K = A.shape
        N = (w if w is not None else wf).shape[0]
        assert A.stride(1) == 1 and (A2 is None or A2.stride(0) == A.stride(0))
        buf = C.create_string_buffer(128)
        self._ok(self.lib.slime_gemm_kernel_name(M, N, K, self.code(A.dtype), epilogue, int(wf is not None), buf, 128), "kernel_name")
        self.kernels.append((name, M, N, K, epilogue, buf.value.decode()))
        if out is None:
            out = torch.empty(M, N, dtype=torch.float32 if epilogue == EPI_BIAS_F32 else A.dtype, device=A.device)
        rm = None if row_map is None else torch.tensor(row_map, dtype=torch.int32, device=A.device)
        p = lambda t: None if t is None else t.data_ptr()
        g = self._lib.GemmArgs(A=A.data_ptr(), lda=A.stride(0), B=p(w), bias=p(bias), C=out.data_ptr(), ldc=N, M=M, N=N, K=K,
                               dtype=self.code(A.dtype), epilogue=epilogue, B_frag=p(wf), A2=p(A2), mix_gates=p(gates), row_map=p(rm))
        self._ok(self.lib.slime_gemm_ex(C.byref(g), self._s()), "slime_gemm_ex")
        return out

    def attention(self, q_proj, k, v, heads, dh):
        n, nkv, D = k.shape
        nq = q_proj.shape[0]
        o = torch.empty(n, nq, D, dtype=k.dtype, device=k.device)
        self._ok(self.lib.slime_attention(q_proj.data_ptr(), 0, D, k.data_ptr(), nkv * D, D, v.data_ptr(), nkv * D, D, o.data_ptr(), nq * D, D,
                                          n, heads, dh, nq, nkv, self.code(k.dtype), self._s()), "slime_attention")
        return o

    def gate_weights(self, x, w_gate):
        out = torch.empty(x.shape[0], 2, dtype=torch.float32, device=x.device)
        self._ok(self.lib.slime_gate_weights(x.data_ptr(), x.shape[1], w_gate.data_ptr(), out.data_ptr(), x.shape[0], self._s()),
                 "slime_gate_weights")
        return out

    def gate_premix(self, x, w_gate, a0, a1, out):
        rows, H = a0.shape
        self._ok(self.lib.slime_gate_premix(x.data_ptr(), x.shape[1], w_gate.data_ptr(), a0.data_ptr(), a1.data_ptr(), out.data_ptr(),
                                            self.code(a0.dtype), rows, H, self._s()), "slime_gate_premix")
        return out

    def merge_rows_batched(self, x, in_image_stride, out, out_image_stride, dst_row0, images, nw, nh, g, merge):
        self._ok(self.lib.slime_merge_rows_batched(x.data_ptr(), in_image_stride, out.data_ptr(), self.code(out.dtype), out_image_stride,
                                                   dst_row0, images, nw, nh, g, out.shape[-1], int(merge), self._s()),
                 "slime_merge_rows_batched")


# ------------------------------------------------------------------------------------------------ replays of csrc/api.hip
def replay_resampler(be, pr, x, n: int, want_f32: bool = True, want_t: bool = True):
    """resampler_run on fp32 rows x [n * n_kv, D] (a view with a row stride >= D is the entry's ldx) -> (out_f32, out_t)."""
    T, D, dh = pr.tensors, pr.dim, pr.dim // pr.heads
    eps = float(pr.desc.eps)
    _, xn, xk = be.layernorm(x, T["ln_kv_w"], T["ln_kv_b"], eps, True, False, True, add=T["pos_k"], add_period=pr.n_kv)
    kp = be.gemm(xk, T, "w_k", T["b_k"], EPI_BIAS_T)
    vp = be.gemm(xn, T, "w_v", T["b_v"], EPI_BIAS_T)
    ctx = be.attention(T["q_proj"], kp.view(n, pr.n_kv, D), vp.view(n, pr.n_kv, D), pr.heads, dh)
    o32 = be.gemm(ctx.view(n * pr.n_query, D), T, "w_o", T["b_o"], EPI_BIAS_F32)
    o_f32, o_t, _ = be.layernorm(o32, T["ln_post_w"], T["ln_post_b"], eps, True, want_f32, want_t)
    return o_f32, o_t


def replay_mlp(be, pm, x, x_is_t: bool):
    """slime_mlp_forward: x fp32 (rounded to T by the normalize = 0 LayerNorm) or T rows -> fp32 rows."""
    T = pm.tensors
    a = x if x_is_t else be.layernorm(x, None, None, 0.0, False, False, True)[1]
    mid = be.gemm(a, T, "w1", T["b1"], EPI_BIAS_GELU_T)
    return be.gemm(mid, T, "w2", T["b2"], EPI_BIAS_F32)


def replay_gated(be, pg, x, n: int, learnable_gated: int):
    """slime_gated_forward on fp32 rows x [n * P, D] -> fp32 [n * P, H]."""
    m, T = pg.mlp, pg.mlp.tensors
    rows = n * pg.attn.n_query
    if learnable_gated == 0:
        return replay_mlp(be, m, x, False)
    attn_t = replay_resampler(be, pg.attn, x, n, False, True)[1]
    if learnable_gated == 1:
        return replay_mlp(be, m, attn_t, True)
    xt = be.layernorm(x, None, None, 0.0, False, False, True)[1]
    if mix_in_gemm(m):
        gates = be.gate_weights(x, pg.w_gate)
        mixed = be.gemm(xt, T, "w1", T["b1"], EPI_BIAS_GELU_MIX_T, A2=attn_t, gates=gates)
    else:
        mid = be.gemm(torch.cat([xt, attn_t]), T, "w1", T["b1"], EPI_BIAS_GELU_T)
        mixed = be.gate_premix(x, pg.w_gate, mid[:rows], mid[rows:], mid[rows:])
    return be.gemm(mixed, T, "w2", T["b2"], EPI_BIAS_F32)


def _adapter_core(be, pg, post, feats, gi, li, learnable_gated, out, direct, rmap, merge_args, broken):
    """What slime_adapter_forward and slime_adapter_forward_ragged share, api.hip's ``adapter_run`` (the both-experts block is its
    ``both_experts_hidden``): gi / li = feats indices of the global / local crops (adapter_run's two crop sources), rmap =
    projection[2]'s row map (direct store) or merge_args = (out_image_stride, n_local, nw, nh, g, merge, local row0) for the fp32 rows +
    slime_merge_rows_batched path, which the uniform entry runs behind adapter_run.  ``out`` [rows, H] is written in place."""
    m, T = pg.mlp, pg.mlp.tensors
    P, D, H = pg.attn.n_kv, m.in_dim, m.hidden
    n_images = len(gi)
    rows_g = n_images * P
    rows_l = len(li) * post.n_query if li else 0
    seg_x, seg_attn, seg_local, rows_all = segments(learnable_gated, rows_g, rows_l)
    xg32, xg_t = be.select_crops(feats[gi])
    stack = be.empty_t(rows_all, D, feats.device)
    if seg_x >= 0:
        stack[seg_x:seg_x + rows_g] = xg_t
    if seg_attn >= 0:
        stack[seg_attn:seg_attn + rows_g] = replay_resampler(be, pg.attn, xg32, n_images, False, True)[1]
    if rows_l:
        xl32 = be.to_f32(feats[li]).reshape(-1, D)                   # float(T): what the LayerNorm from T features computes on
        stack[seg_local:] = replay_resampler(be, post, xl32, len(li), False, True)[1]
    if learnable_gated < 0:
        a0, a1 = (seg_attn, seg_x) if broken == "seg_attn_seg_x_swapped" else (seg_x, seg_attn)
        mixed_at = seg_x if broken == "mixed_over_first_segment" else seg_attn
        mid = be.empty_t(rows_all, H, feats.device)
        if mix_in_gemm(m):
            gates = be.gate_weights(xg32, pg.w_gate)
            mid[mixed_at:mixed_at + rows_g] = be.gemm(stack[a0:a0 + rows_g], T, "w1", T["b1"], EPI_BIAS_GELU_MIX_T,
                                                      A2=stack[a1:a1 + rows_g], gates=gates)
            if rows_l:
                mid[seg_local:] = be.gemm(stack[seg_local:], T, "w1", T["b1"], EPI_BIAS_GELU_T)
        else:
            mid = be.gemm(stack, T, "w1", T["b1"], EPI_BIAS_GELU_T)
            be.gate_premix(xg32, pg.w_gate, mid[a0:a0 + rows_g], mid[a1:a1 + rows_g], mid[mixed_at:mixed_at + rows_g])
        A = mid[seg_attn:seg_attn + rows_g + rows_l]
    else:
        A = be.gemm(stack, T, "w1", T["b1"], EPI_BIAS_GELU_T)
    if direct:
        epi = EPI_BIAS_F32 if out.dtype == be.out_dtype(torch.float32) else EPI_BIAS_T
        be.gemm(A, T, "w2", T["b2"], epi, out=out, row_map=rmap)
        return out
    stride, n_local, nw, nh, g, merge, row0 = merge_args
    e = be.gemm(A, T, "w2", T["b2"], EPI_BIAS_F32)
    be.merge_rows_batched(e, P, out, stride, 0, n_images, P, 1, 1, 0)
    if rows_l:
        be.merge_rows_batched(e[rows_g:], n_local * post.n_query, out, stride, row0, n_images, nw, nh, g, merge)
    return out


def replay_adapter(be, tiny: Tiny, feats, n_images: int, n_local: int, nw: int, nh: int, merge, learnable_gated: int, out,
                   out_image_stride: int, broken: Optional[str] = None):
    """slime_adapter_forward: feats T [n_images * (1 + n_local), P, D] -> out [n_images * out_image_stride, H] (in place; rows no
    image owns are not written).  The direct store when out is fp32 or T, fp32 rows + merge otherwise (the broken merge variants
    act on the row map, i.e. on the direct store)."""
    pg = tiny.pg
    post = tiny.post if n_local > 0 else None
    P, q = pg.attn.n_kv, (tiny.post.n_query if n_local > 0 else 0)
    gi = global_crop_index(n_images, n_local, broken)
    li = local_crop_index(n_images, n_local, broken)
    direct = out.dtype in (be.out_dtype(torch.float32), be.out_dtype(tiny.dtype))
    rmap = row_map_uniform(n_images, P, n_local, q, nw, merge, out_image_stride, nh, broken) if direct else None
    stride = P + n_local * q if broken == "stride_is_packed_rows" else out_image_stride
    margs = (stride, n_local, nw, nh, math.isqrt(q), merge, 0 if broken == "local_row0_zero" else P)
    return _adapter_core(be, pg, post, feats, gi, li, learnable_gated, out, direct, rmap, margs, broken)


def replay_adapter_ragged(be, tiny: Tiny, feats, grids, merge, learnable_gated: int, out, out_row0=None, broken: Optional[str] = None):
    """slime_adapter_forward_ragged: feats T [sum (1 + n_i), P, D], out [out_rows, H] fp32 or T (always the direct store)."""
    pg = tiny.pg
    any_local = any(nw * nh for nw, nh in grids)
    post = tiny.post if any_local else None
    gi, li = ragged_crop_index(grids, broken)
    _, _, rmap = ragged_row_map(grids, pg.attn.n_kv, post.n_query if post else 1, merge, out_row0, broken)
    return _adapter_core(be, pg, post, feats, gi, li, learnable_gated, out, True, rmap, None, broken)


# ------------------------------------------------------------------------------------------------ guarded buffers
class GuardedWorkspace:
    """A byte buffer with a 256-byte aligned window of EXACTLY ``nbytes`` bytes (plus ``misalign``), SENTINEL_BYTE in front of the
    window and behind it, ``fill`` inside."""

    GUARD = 1024

    def __init__(self, nbytes: int, device, fill: int = 0xFF, misalign: int = 0):
        self.nbytes = int(nbytes)
        self.buf = torch.empty(self.GUARD + 512 + self.nbytes + self.GUARD, dtype=torch.uint8, device=device)
        self.buf.fill_(SENTINEL_BYTE)
        base = (self.buf.data_ptr() + self.GUARD + 255) // 256 * 256 + misalign
        self.off = base - self.buf.data_ptr()
        self.window.fill_(fill)

    @property
    def window(self):
        return self.buf[self.off:self.off + self.nbytes]

    def ptr(self) -> int:
        return self.buf.data_ptr() + self.off

    def intact(self) -> bool:
        return bool((self.buf[:self.off] == SENTINEL_BYTE).all()) and bool((self.buf[self.off + self.nbytes:] == SENTINEL_BYTE).all())

    def snapshot(self):
        return self.buf.clone()

    def unchanged(self, snap) -> bool:
        return bool(torch.equal(self.buf, snap))


def guarded_input(t: torch.Tensor, rows: int, pad_cols: int = 0) -> Padded:
    """A copy of an input in a buffer of its own, NaN around it (and in the pad columns of a strided one)."""
    t = t.contiguous()
    return Padded(rows, t.numel() // rows, t.dtype, t.device, pad_cols=pad_cols, guard_rows=0, tail=TAIL).fill(t.view(rows, -1), math.nan)


def guarded_output(rows: int, H: int, dtype, device) -> Padded:
    """A contiguous [rows, H] output window, every byte SENTINEL_BYTE, guard rows and a tail behind it."""
    return Padded(rows, H, dtype, device, pad_cols=0, guard_rows=3, tail=TAIL)


def sentinel_rows(win: torch.Tensor) -> torch.Tensor:
    """bool [rows]: the row still holds SENTINEL_BYTE in every byte."""
    return (win.contiguous().view(torch.uint8).view(win.shape[0], -1) == SENTINEL_BYTE).all(dim=1)
