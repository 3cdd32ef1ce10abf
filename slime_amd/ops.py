"""Torch-tensor front end of libslime_hip: weight packing (load time) and thin call wrappers.

PyTorch is plumbing here -- device memory, streams, dtype bookkeeping.  Every arithmetic step of the
hot path runs in the HIP library; there is no eager / CPU fallback (``_lib.load()`` raises if the
library is absent).
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import math
import os
import threading
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .weights import VisionConfig, SiglipVisionConfig, Dinov2VisionConfig, AdapterConfig, strip_tower_prefix, strip_dinov2_prefix, sub_state

LOG2E = 1.4426950408889634   # slime_attention takes q pre-scaled by head_dim^-0.5 * log2(e)

_DT = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16, torch.float32: _lib.F32, torch.uint8: _lib.U8}


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise ValueError(f"unsupported dtype {dt}") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "libslime_hip needs contiguous device tensors"
    return t.data_ptr()


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _lib.SlimeHipError(f"{name} must live on the GPU: slime_amd has no CPU path")


class Workspace:
    """Grow-only scratch buffer (256-B aligned by the caching allocator's 512-B granularity)."""

    def __init__(self):
        self.buf: Optional[torch.Tensor] = None

    def get(self, nbytes: int, device) -> torch.Tensor:
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
        return self.buf

    def aligned(self, nbytes: int, device) -> Tuple[int, int]:
        """``get``, as what a C entry takes: (the 256-B aligned base address, the bytes available behind it)."""
        buf = self.get(nbytes, device)
        base = (buf.data_ptr() + 255) // 256 * 256
        return base, buf.numel() - (base - buf.data_ptr())


# ------------------------------------------------------------------------------------------------
# primitive wrappers (used by the parity tests and by the modules)
# ------------------------------------------------------------------------------------------------

def pack_b_frag(w: torch.Tensor) -> Optional[torch.Tensor]:
    """Copy of the static GEMM operand(s) w T [..., N, K] in MFMA-fragment order (slime_gemm_pack_b; layout in
    include/slime_hip.h), or None where the library cannot run from it (it is asked: slime_gemm_b_frag_usable; host tensors)."""
    if w is None or not w.is_cuda:
        return None
    N, K = w.shape[-2], w.shape[-1]
    lib = _lib.load()
    if not lib.slime_gemm_b_frag_usable(N, K):
        return None
    w = w.contiguous()
    out = torch.empty_like(w)
    per = N * K * w.element_size()
    assert lib.slime_gemm_packed_b_bytes(N, K) == per
    for i in range(w.numel() // (N * K)):
        _lib.check(lib.slime_gemm_pack_b(w.data_ptr() + i * per, N, K, out.data_ptr() + i * per, _stream()), "slime_gemm_pack_b")
    return out


def keep_row_major() -> bool:
    """Weight-memory policy.  Since ABI 5 every kernel slime_gemm_ex dispatches to can read a static operand from
    its fragment-order image alone, so by default a packed weight is resident ONCE (tower 0.58 GB, adapter 62 MB; through round 4
    every weight was held twice: row-major for the LDS-staged kernels + fragment order for the direct-B kernel).
    SLIME_KEEP_ROW_MAJOR=1 keeps the row-major copies as well (the round-4 layout; results are bit-identical either way)."""
    return os.environ.get("SLIME_KEEP_ROW_MAJOR", "0") == "1"


def pack_static(T: Dict[str, Optional[torch.Tensor]], names: Sequence[str]) -> None:
    """T[name + '_frag'] = fragment-order image of T[name]; the row-major tensor is dropped (T[name] = None) where the library can
    run from the image alone, unless keep_row_major()."""
    for name in names:
        T[name + "_frag"] = pack_b_frag(T[name])
        if T[name + "_frag"] is not None and not keep_row_major():
            T[name] = None


def packed_weight_bytes(*packs) -> int:
    """Resident bytes of the packed tensors of PackedTower / PackedResampler / PackedMlp / ... objects (each tensor once)."""
    seen, total = set(), 0
    for p in packs:
        for t in (p.tensors if hasattr(p, "tensors") else p).values():
            if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
    return total


_ksplit_ws = Workspace()


def _launch_gemm(g: "_lib.GemmArgs", splits: int, device, ws: Optional[torch.Tensor] = None) -> None:
    """slime_gemm_ex (splits == 1) or slime_gemm_ksplit with a workspace of slime_gemm_ksplit_workspace_bytes (``ws``: a uint8
    device tensor of the caller's, 256-byte aligned, or the module's grow-only buffer -- ONE per process: calls that may overlap on
    two streams each pass a ``ws`` of their own)."""
    lib = _lib.load()
    if splits == 1:
        _lib.check(lib.slime_gemm_ex(C.byref(g), _stream()), "slime_gemm_ex")
        return
    if ws is None:
        base, nbytes = _ksplit_ws.aligned(lib.slime_gemm_ksplit_workspace_bytes(g.M, g.N, splits), device)
    else:
        base, nbytes = ws.data_ptr(), ws.numel() * ws.element_size()
    _lib.check(lib.slime_gemm_ksplit(C.byref(g), int(splits), base, nbytes, _stream()), "slime_gemm_ksplit")


def gemm_ksplit(a: torch.Tensor, w: Optional[torch.Tensor], bias: Optional[torch.Tensor], epilogue: int, splits: int,
                out: Optional[torch.Tensor] = None, w_frag: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
                row_map: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gemm`` as a deterministic split-K pair of launches (slime_gemm_ksplit): K is cut into ``splits`` chunks by a rule of
    (K, splits) alone and the partial products are summed in plane order, so a result row depends on its row of ``a``, on ``w`` and
    on ``splits`` only.  splits == 1 is ``gemm``."""
    return gemm(a, w, bias, epilogue, out, w_frag, resid, row_map, splits=splits, ws=ws)


def gemm(a: torch.Tensor, w: Optional[torch.Tensor], bias: Optional[torch.Tensor], epilogue: int,
         out: Optional[torch.Tensor] = None, w_frag: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None,
         row_map: Optional[torch.Tensor] = None, splits: int = 1, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = epi(a @ w.T + bias); a [M,K] T, w [N,K] T, bias fp32 [N]; w_frag = pack_b_frag(w) (optional); resid T [M,N] for
    EPI_BIAS_RESID_T (out = T(a @ w.T + bias + resid), out may be resid); row_map int32 [M] (device): row r of the result is stored
    at out[row_map[r]] (``out`` given, with at least max(row_map) + 1 rows; plain T / fp32 epilogues).
    splits > 1: the deterministic split-K pair of launches (``gemm_ksplit``); ws: its workspace, or None for the module's buffer."""
    lib = _lib.load()
    M, K = a.shape
    if w is None and w_frag is None:
        raise ValueError("gemm: the static operand is missing (row-major w, its fragment-order image w_frag, or both)")
    N = (w if w is not None else w_frag).shape[0]        # w = None: the fragment-order image alone (slime_gemm_b_frag_usable)
    if out is None:
        odt = a.dtype if (epilogue <= _lib.EPI_BIAS_GELU_T or epilogue == _lib.EPI_BIAS_RESID_T) else torch.float32
        out = torch.empty((M, N), dtype=odt, device=a.device)
    g = _lib.GemmArgs(A=_ptr(a), lda=a.stride(0), B=_ptr(w), bias=_ptr(bias), C=_ptr(out), ldc=out.stride(0), M=M, N=N, K=K,
                      dtype=dtype_code(a.dtype), epilogue=epilogue, B_frag=_ptr(w_frag), resid=_ptr(resid),
                      ldr=resid.stride(0) if resid is not None else 0, row_map=_ptr(row_map))
    _launch_gemm(g, splits, a.device, ws)
    return out


def gemm_ln_producer(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], h: torch.Tensor,
                     w_frag: Optional[torch.Tensor] = None, splits: int = 1, ws: Optional[torch.Tensor] = None):
    """h (fp32, in place) += a @ w.T + bias; returns (x16 = T(h), stats [M, N/64, 2]): SLIME_EPI_BIAS_RESID_F32_LN."""
    lib = _lib.load()
    M, K = a.shape
    N = (w if w is not None else w_frag).shape[0]
    x16 = torch.empty((M, N), dtype=a.dtype, device=a.device)
    stats = torch.empty((M, N // 64, 2), dtype=torch.float32, device=a.device)
    g = _lib.GemmArgs(A=_ptr(a), lda=a.stride(0), B=_ptr(w), bias=_ptr(bias), C=_ptr(h), ldc=h.stride(0), M=M, N=N, K=K,
                      dtype=dtype_code(a.dtype), epilogue=_lib.EPI_BIAS_RESID_F32_LN, x16=_ptr(x16), ldx=N, stats_out=_ptr(stats),
                      B_frag=_ptr(w_frag))
    _launch_gemm(g, splits, a.device, ws)
    return x16, stats


def _resid_shift(dtype: torch.dtype) -> int:
    if dtype == torch.bfloat16:
        return 8
    if dtype == torch.float16:
        return 5
    raise ValueError(f"the split residual stream's upper part is bf16 or fp16, not {dtype}")


def resid_split(h: torch.Tensor, dtype: torch.dtype):
    """fp32 rows -> the tower's SPLIT residual stream (include/slime_hip.h, ABI 7; a torch restatement of csrc/common.h resid_delta):
    hi = T(h) (RNE) and lo8 = floor((pattern(h) - pattern(float(hi))) / 2^SH) clamped to int8, SH = 8 (bf16) / 5 (fp16)."""
    sh = _resid_shift(dtype)
    hi = h.to(dtype)
    d = (h.float().contiguous().view(torch.int32) - hi.float().view(torch.int32)) >> sh          # int32 >> is arithmetic: floor
    return hi, d.clamp(-128, 127).to(torch.int8)


def resid_join(hi: torch.Tensor, lo8: torch.Tensor) -> torch.Tensor:
    """The fp32 rows a split residual stream holds (csrc/common.h resid_join): pattern(float(hi)) + lo8 2^SH + 2^(SH-1)."""
    sh = _resid_shift(hi.dtype)
    return (hi.float().contiguous().view(torch.int32) + lo8.to(torch.int32) * (1 << sh) + (1 << (sh - 1))).view(torch.float32)


def gemm_resid_split(a: torch.Tensor, w: Optional[torch.Tensor], bias: Optional[torch.Tensor], hi: torch.Tensor, lo: torch.Tensor,
                     w_frag: Optional[torch.Tensor] = None, splits: int = 1, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SLIME_EPI_BIAS_RESID_SPLIT_LN on the split residual stream (hi: T [M, N], lo: int8 [M, N], updated in place):
    c = a @ w.T + bias + resid_join(hi, lo); hi, lo = resid_split(c).  Returns stats [M, N/64, 2] (partial sums of c)."""
    assert lo.dtype == torch.int8 and lo.stride(1) == 1, "the stream's lower part is one signed byte per element (ABI 7)"
    lib = _lib.load()
    M, K = a.shape
    N = (w if w is not None else w_frag).shape[0]
    stats = torch.empty((M, N // 64, 2), dtype=torch.float32, device=a.device)
    g = _lib.GemmArgs(A=_ptr(a), lda=a.stride(0), B=_ptr(w), bias=_ptr(bias), C=_ptr(hi), ldc=hi.stride(0), M=M, N=N, K=K,
                      dtype=dtype_code(a.dtype), epilogue=_lib.EPI_BIAS_RESID_SPLIT_LN, stats_out=_ptr(stats), B_frag=_ptr(w_frag),
                      lo8=_ptr(lo), ldlo=lo.stride(0))
    _launch_gemm(g, splits, a.device, ws)
    return stats


def patch_embed_prenorm(pixels: torch.Tensor, patch_w_frag: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, ln_w: torch.Tensor,
                        ln_b: torch.Tensor, eps: float, dtype: torch.dtype, image: int, patch: int, kpad: int, want_h=True, want_x16=True,
                        want_lo=False):
    """slime_patch_embed_prenorm: pixels [n,3,image,image] (fp32 or T) -> (h fp32 [n*(1+P), D] | None, x16 T | None, lo int8 | None,
    stats [n*(1+P), D/64, 2] | None)."""
    lib = _lib.load()
    n, D = pixels.shape[0], cls.shape[0]
    rows = n * ((image // patch) ** 2 + 1)
    dev = pixels.device
    h = torch.empty((rows, D), dtype=torch.float32, device=dev) if want_h else None
    x16 = torch.empty((rows, D), dtype=dtype, device=dev) if want_x16 else None
    lo = torch.empty((rows, D), dtype=torch.int8, device=dev) if want_lo else None
    stats = torch.empty((rows, D // 64, 2), dtype=torch.float32, device=dev) if want_x16 else None
    _lib.check(lib.slime_patch_embed_prenorm(_ptr(pixels), dtype_code(pixels.dtype), _ptr(patch_w_frag), _ptr(cls), _ptr(pos), _ptr(ln_w),
                                             _ptr(ln_b), float(eps), _ptr(h), _ptr(x16), _ptr(lo), _ptr(stats), dtype_code(dtype), n, image,
                                             patch, kpad, D, _stream()), "slime_patch_embed_prenorm")
    return h, x16, lo, stats


def gemm_ln_consumer(x16: torch.Tensor, stats: torch.Tensor, w_folded: torch.Tensor, bias_folded: torch.Tensor, colsum: torch.Tensor,
                     eps: float, epilogue: int, w_frag: Optional[torch.Tensor] = None, splits: int = 1,
                     ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """epi(LayerNorm(x16) @ W.T + b) with the LayerNorm folded: w_folded = T(W diag(gamma)), bias_folded = b + W beta,
    colsum = row sums of w_folded; stats from the producer.  Output T [M, N]."""
    lib = _lib.load()
    M, K = x16.shape
    N = (w_folded if w_folded is not None else w_frag).shape[0]
    out = torch.empty((M, N), dtype=x16.dtype, device=x16.device)
    g = _lib.GemmArgs(A=_ptr(x16), lda=x16.stride(0), B=_ptr(w_folded), bias=_ptr(bias_folded), C=_ptr(out), ldc=N, M=M, N=N, K=K,
                      dtype=dtype_code(x16.dtype), epilogue=epilogue, ln_stats=_ptr(stats), ln_groups=stats.shape[1],
                      ln_colsum=_ptr(colsum), ln_eps=float(eps), B_frag=_ptr(w_frag))
    _launch_gemm(g, splits, x16.device, ws)
    return out


def layernorm(x: torch.Tensor, w, b, eps: float, dtype: torch.dtype, want_f32=False, want_t=True,
              add: Optional[torch.Tensor] = None, normalize=True):
    lib = _lib.load()
    rows, D = x.shape
    o32 = torch.empty((rows, D), dtype=torch.float32, device=x.device) if want_f32 else None
    ot = torch.empty((rows, D), dtype=dtype, device=x.device) if want_t else None
    ot2 = torch.empty((rows, D), dtype=dtype, device=x.device) if add is not None else None
    _lib.check(lib.slime_layernorm(_ptr(x), x.stride(0), rows, D, _ptr(w), _ptr(b), float(eps), int(normalize),
                                   _ptr(o32), _ptr(ot), _ptr(ot2), _ptr(add), add.shape[0] if add is not None else 0,
                                   dtype_code(dtype), _stream()), "slime_layernorm")
    return o32, ot, ot2


def attention(q, k, v, heads: int, head_dim: int) -> torch.Tensor:
    """q [B|1, nq, H*dh] (pre-scaled by dh^-0.5 * log2 e), k/v [B, nkv, H*dh] -> [B, nq, H*dh]; all T, last dim contiguous."""
    lib = _lib.load()
    B, nkv = k.shape[0], k.shape[1]
    nq = q.shape[1]
    o = torch.empty((B, nq, heads * head_dim), dtype=k.dtype, device=k.device)
    for t in (q, k, v):
        assert t.stride(-1) == 1
    q_bs = 0 if q.shape[0] == 1 and B > 1 else q.stride(0)
    _lib.check(lib.slime_attention(q.data_ptr(), q_bs, q.stride(1), k.data_ptr(), k.stride(0), k.stride(1),
                                   v.data_ptr(), v.stride(0), v.stride(1), o.data_ptr(), o.stride(0), o.stride(1),
                                   B, heads, head_dim, nq, nkv, dtype_code(k.dtype), _stream()), "slime_attention")
    return o


# ------------------------------------------------------------------------------------------------
# weight packing (load time; plain torch)
# ------------------------------------------------------------------------------------------------

@dataclass
class PackedTower:
    """A packed CLIP, SigLIP or DINOv2 tower (``pack_tower`` / ``pack_siglip_tower`` / ``pack_dinov2_tower``)."""
    cfg: VisionConfig                    # or SiglipVisionConfig / Dinov2VisionConfig, by ``form``
    dtype: torch.dtype
    layers_run: int
    tensors: Dict[str, torch.Tensor]
    desc: _lib.VitDesc
    ws: Workspace = field(default_factory=Workspace)
    probe: Optional[tuple] = None        # (layer, kernel id, start event, stop event): in-situ kernel timing (CLIP form)
    act: int = _lib.ACT_QUICKGELU        # SLIME_ACT_* of cfg.hidden_act (CLIP form: what slime_vit_forward_opts is given)
    form: str = "clip"                   # "clip" | "siglip" | "dinov2": the C entry that runs the tower (``_tower_call``)

    @property
    def device(self):
        return self.tensors["pos"].device


def tower_act(cfg: VisionConfig) -> int:
    """SLIME_ACT_* of ``cfg.hidden_act``; a tower with another activation is refused by name (no kernel computes it)."""
    try:
        return _lib.ACT_BY_NAME[cfg.hidden_act]
    except KeyError:
        raise ValueError(f"vision tower hidden_act={cfg.hidden_act!r} is not supported: the HIP path computes "
                         f"{' and '.join(repr(k) for k in _lib.ACT_BY_NAME)} only") from None


def layers_for_select(cfg: VisionConfig, select_layer: int) -> int:
    """hidden_states has L+1 entries; index i is produced by running i layers (clip_encoder.py:36-37)."""
    L = cfg.num_hidden_layers
    idx = select_layer if select_layer >= 0 else L + 1 + select_layer
    if not 0 <= idx <= L:
        raise ValueError(f"mm_vision_select_layer {select_layer} out of range for {L} layers")
    return idx


def fold_ln(Wm, bm, gamma, beta, row_scale=None, dtype: Optional[torch.dtype] = None):
    """LayerNorm folded into the Linear that consumes it (slime_gemm_ex): W' = T(W diag(gamma) rowscale), b' = (b + W beta) rowscale,
    colsum = row sums of the ROUNDED W' (it must cancel the mean term of what the MFMA multiplies).  Host tensors: (W' T, b' fp32,
    colsum fp32); dtype = None rounds nothing (all three float64)."""
    W64 = Wm.detach().double().cpu()
    Wp = W64 * gamma.detach().double().cpu()[None, :]
    bp = bm.detach().double().cpu() + W64 @ beta.detach().double().cpu()
    if row_scale is not None:
        Wp, bp = Wp * row_scale[:, None], bp * row_scale
    if dtype is None:
        return Wp, bp, Wp.sum(1)
    Wt = Wp.float().to(dtype)
    return Wt, bp.float(), Wt.double().sum(1).float()


def tower_host_tensors(state_dict: Dict[str, torch.Tensor], cfg: VisionConfig, dtype: Optional[torch.dtype],
                       select_layer: int = -2) -> Dict[str, torch.Tensor]:
    """The pack-time algebra of ``pack_tower`` on the host (no device work; CPU tensors out): the conv weight as a zero-padded
    [D, kpad] matrix, and per layer (stacked along dim 0, ``layers_for_select`` layers) [q; k; v] with LayerNorm1 and the q scale
    dh^-0.5 log2(e) folded in (``fold_ln``), fc1 with LayerNorm2 folded in, out_proj and fc2 as they are.  Matrices in ``dtype``,
    everything else fp32; ``dtype=None``: nothing is rounded, every tensor float64."""
    _check_operand_dtype(dtype, allow_none=True)
    sd = strip_tower_prefix(state_dict)
    L = layers_for_select(cfg, select_layer)
    f32, tt = _host_casts(dtype)
    T: Dict[str, torch.Tensor] = {
        "patch_w": _conv_matrix(sd, cfg, tt), "cls": f32(sd["embeddings.class_embedding"]),
        "pos": f32(sd["embeddings.position_embedding.weight"]),
        "pre_ln_w": f32(sd["pre_layrnorm.weight"]), "pre_ln_b": f32(sd["pre_layrnorm.bias"]),
    }
    _layer_host_tensors(T, sd, cfg, dtype, L)
    return T


def _host_casts(dtype: Optional[torch.dtype]):
    """(fp32 cast, T cast) of the host packers; dtype = None: both float64 (nothing is rounded)."""
    def f32(t):
        t = t.detach().cpu()
        return (t.double() if dtype is None else t.float()).contiguous()

    def tt(t):
        t = t.detach().cpu()
        return (t.double() if dtype is None else t.float().to(dtype)).contiguous()

    return f32, tt


def _conv_matrix(sd, cfg, tt, key: str = "embeddings.patch_embedding.weight") -> torch.Tensor:
    """The patch-embed conv weight as a [D, kpad] matrix (column order Conv2d.weight.flatten(1), zero padded to a multiple of 64)."""
    D, P2 = cfg.hidden_size, 3 * cfg.patch_size * cfg.patch_size
    pw = torch.zeros((D, (P2 + 63) // 64 * 64), dtype=torch.float32)
    pw[:, :P2] = sd[key].detach().float().cpu().reshape(D, P2)
    return tt(pw)


class LayerKeys(NamedTuple):
    """A checkpoint layout's names under one encoder layer (``layer.format(i)`` + name + ".weight" / ".bias"); ``scale_o`` /
    ``scale_fc2``: the vectors that scale the outputs of out_proj / fc2 (DINOv2's LayerScale), or None."""
    layer: str
    q: str
    k: str
    v: str
    o: str
    ln1: str
    ln2: str
    fc1: str = "mlp.fc1"
    fc2: str = "mlp.fc2"
    scale_o: Optional[str] = None
    scale_fc2: Optional[str] = None


CLIP_LAYER_KEYS = LayerKeys("encoder.layers.{}.", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj",
                            "layer_norm1", "layer_norm2")        # the SigLIP layout's as well
DINOV2_LAYER_KEYS = LayerKeys("encoder.layer.{}.", "attention.attention.query", "attention.attention.key", "attention.attention.value",
                              "attention.output.dense", "norm1", "norm2", scale_o="layer_scale1.lambda1", scale_fc2="layer_scale2.lambda1")


def _layer_host_tensors(T: Dict[str, torch.Tensor], sd, cfg, dtype: Optional[torch.dtype], L: int,
                        keys: LayerKeys = CLIP_LAYER_KEYS) -> None:
    """The per-layer part of the ``*_host_tensors`` functions: adds the stacked, folded tensors of the first ``L`` layers to ``T``."""
    D = cfg.hidden_size
    f32, tt = _host_casts(dtype)
    if L == 0:
        return
    rs = torch.ones(3 * D, dtype=torch.float64)
    rs[:D] = cfg.head_dim ** -0.5 * LOG2E                      # q rows carry dh^-0.5 * log2 e: logits in log2 units (slime_attention contract)
    cols = {k: [] for k in ("w_qkv", "b_qkv", "colsum_qkv", "w_fc1", "b_fc1", "colsum_fc1", "w_o", "b_o", "w_fc2", "b_fc2")}
    for i in range(L):
        p = keys.layer.format(i)
        Wm = torch.cat([sd[p + n + ".weight"].float() for n in (keys.q, keys.k, keys.v)], 0)
        bm = torch.cat([sd[p + n + ".bias"].float() for n in (keys.q, keys.k, keys.v)], 0)
        for k, v in zip(("w_qkv", "b_qkv", "colsum_qkv"), fold_ln(Wm, bm, sd[p + keys.ln1 + ".weight"], sd[p + keys.ln1 + ".bias"], rs, dtype)):
            cols[k].append(v)
        for k, v in zip(("w_fc1", "b_fc1", "colsum_fc1"), fold_ln(sd[p + keys.fc1 + ".weight"], sd[p + keys.fc1 + ".bias"],
                                                                  sd[p + keys.ln2 + ".weight"], sd[p + keys.ln2 + ".bias"], None, dtype)):
            cols[k].append(v)
        for w, b, lin, lam in (("w_o", "b_o", keys.o, keys.scale_o), ("w_fc2", "b_fc2", keys.fc2, keys.scale_fc2)):
            Wm, bm = sd[p + lin + ".weight"], sd[p + lin + ".bias"]
            if lam is not None:                                # output feature j of the Linear is scaled by lambda[j]: row j of W, b[j]
                s = sd[p + lam].detach().double().cpu()
                Wm, bm = Wm.detach().double().cpu() * s[:, None], bm.detach().double().cpu() * s
            cols[w].append(tt(Wm))
            cols[b].append(f32(bm))
    for k, v in cols.items():
        T[k] = torch.stack(v).contiguous()


def _check_operand_dtype(dtype: Optional[torch.dtype], allow_none: bool = False) -> None:
    if dtype not in (torch.bfloat16, torch.float16) and not (allow_none and dtype is None):
        raise ValueError("tower compute dtype must be bf16 or fp16 (MFMA operand type); fp32 I/O is supported")


def _pack_tail(who: str, form: str, host: Dict[str, torch.Tensor], cfg, dtype: torch.dtype, device, L: int, check, act=_lib.ACT_QUICKGELU):
    """What the three ``pack_*`` share behind their config checks: the host tensors ``host`` on ``device``, the four layer matrices
    and the conv weight in MFMA-fragment order, the descriptor, and the driver's own validation (``check(lib, desc)``, the form's
    slime_*_check) at PACK time: a geometry the fused front end cannot run (more than 24 patches per side, image not a multiple of
    8, ...) is refused here with the limit named, not by the first forward."""
    T: Dict[str, torch.Tensor] = {k: v.to(device).contiguous() for k, v in host.items()}
    if L > 0:
        # fragment-order images (the direct-B kernel loads them straight into registers, the LDS-staged kernels DMA from them);
        # the row-major tensors are dropped unless SLIME_KEEP_ROW_MAJOR=1
        pack_static(T, ("w_qkv", "w_o", "w_fc1", "w_fc2"))
    T["patch_w_frag"] = pack_b_frag(T["patch_w"])          # the front end (slime_patch_embed_*) reads this image only
    if T["patch_w_frag"] is None:
        if not T["patch_w"].is_cuda:
            raise _lib.SlimeHipError(f"{who}: weights are packed on the GPU (slime_gemm_pack_b): slime_amd has no CPU path")
        raise ValueError(f"{who}: the patch-embed weight could not be packed (hidden size and padded patch size must be multiples of 64)")
    T["patch_w"] = None
    d = _vit_desc(T, cfg, dtype, L)
    _lib.check(check(_lib.load(), C.byref(d)), who)
    return PackedTower(cfg, dtype, L, T, d, act=act, form=form)


def pack_tower(state_dict: Dict[str, torch.Tensor], cfg: VisionConfig, dtype: torch.dtype, device,
               select_layer: int = -2) -> PackedTower:
    """HF CLIPVisionModel state dict (either key generation) -> device tensors in the kernels' layout (``tower_host_tensors`` on
    ``device``, the four layer matrices and the conv weight also in MFMA-fragment order)."""
    _check_operand_dtype(dtype)
    act = tower_act(cfg)
    L = layers_for_select(cfg, select_layer)
    return _pack_tail("pack_tower", "clip", tower_host_tensors(state_dict, cfg, dtype, select_layer), cfg, dtype, device, L,
                      lambda lib, d: lib.slime_vit_check(d), act)


def _vit_desc(T: Dict[str, Optional[torch.Tensor]], cfg, dtype: torch.dtype, L: int) -> "_lib.VitDesc":
    """slime_vit_desc over the packed device tensors ``T`` (a tensor that is absent or None leaves its field NULL)."""
    d = _lib.VitDesc()
    d.hidden, d.inter, d.heads, d.layers_run = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, L
    d.image, d.patch, d.dtype, d.eps = cfg.image_size, cfg.patch_size, dtype_code(dtype), cfg.layer_norm_eps
    d.kpad = (3 * cfg.patch_size * cfg.patch_size + 63) // 64 * 64
    for name in ("patch_w", "cls", "pos", "pre_ln_w", "pre_ln_b", "w_qkv", "b_qkv", "colsum_qkv", "w_o", "b_o",
                 "w_fc1", "b_fc1", "colsum_fc1", "w_fc2", "b_fc2", "w_qkv_frag", "w_o_frag", "w_fc1_frag", "w_fc2_frag", "patch_w_frag"):
        setattr(d, name, T[name].data_ptr() if name in T and T[name] is not None else None)
    return d


def _tower_pixels(pt: PackedTower, pixels: torch.Tensor) -> torch.Tensor:
    """pixels as the C entries take them: [N, 3, S, S] of the size the tower was packed for, fp32 or the operand dtype, contiguous."""
    _require_cuda(pixels, "pixels")
    s = pt.cfg.image_size
    if pixels.dim() != 4 or pixels.shape[1] != 3 or pixels.shape[2] != s or pixels.shape[3] != s:
        # HF raises on a size mismatch too (modeling_clip.py:204-207)
        raise ValueError(f"Input image size ({tuple(pixels.shape[2:])}) doesn't match model ({s}*{s}).")
    if pixels.dtype not in (torch.float32, pt.dtype):
        pixels = pixels.to(pt.dtype)
    return pixels.contiguous()


def _tower_call(pt: PackedTower, pixels, out, keep: bool, hidden, states, k_split) -> None:
    """One tower pass through the form's C entry (any of out / hidden / states; ``keep``: ``out`` has the rows in front of the patches
    too): slime_vit_forward_opts with the tower's activation, slime_siglip_forward or slime_dinov2_forward.  A CLIP tower with a
    timing probe set makes its out / hidden pass through slime_vit_forward_ex, the one entry that takes a probe."""
    lib = _lib.load()
    n, ks, d = pixels.shape[0], None, C.byref(pt.desc)
    if k_split is not None:
        if len(k_split) != 4:
            raise ValueError("tower_forward: k_split is (qkv, out_proj, fc1, fc2)")
        ks = _lib.VitKsplit(*(int(v) for v in k_split))
    probed = pt.form == "clip" and pt.probe is not None and states is None
    if probed and ks is not None:
        raise ValueError("tower_forward: the timing probe goes with k_split=None (slime_vit_forward_ex)")
    if probed and pt.act != _lib.ACT_QUICKGELU:
        raise ValueError("tower_forward: the timing probe (slime_vit_forward_ex) is built for quick-GELU towers")
    ksp = C.byref(ks) if ks is not None else None
    desc = (d, pt.cfg.n_prefix) if pt.form == "dinov2" else (d,)             # the DINOv2 entries take n_prefix behind the descriptor
    family = {"clip": "vit", "siglip": "siglip", "dinov2": "dinov2"}[pt.form]
    if ks is not None:
        need = getattr(lib, f"slime_{family}_ksplit_workspace_bytes")(*desc, n, ksp)
    else:
        need = getattr(lib, f"slime_{family}_workspace_bytes")(*desc, n)
    base, avail = pt.ws.aligned(need, pixels.device)
    px = (pixels.data_ptr(), dtype_code(pixels.dtype), n, _ptr(out), dtype_code(out.dtype) if out is not None else _lib.F32)
    if probed:
        layer, kernel, e0, e1 = pt.probe
        probe = C.byref(_lib.Probe(int(layer), int(kernel), e0.cuda_event, e1.cuda_event))
        _lib.check(lib.slime_vit_forward_ex(d, *px, int(keep), _ptr(hidden), base, avail, _stream(), probe), "slime_vit_forward")
    elif pt.form == "clip":
        _lib.check(lib.slime_vit_forward_opts(d, C.byref(_lib.VitOpts(pt.act)), *px, int(keep), _ptr(hidden), _ptr(states), ksp, base, avail,
                                              _stream()), "slime_vit_forward_opts")
    elif pt.form == "siglip":                                 # no rows in front of the patches: no keep flag
        _lib.check(lib.slime_siglip_forward(d, *px, _ptr(hidden), _ptr(states), ksp, base, avail, _stream()), "slime_siglip_forward")
    else:
        _lib.check(lib.slime_dinov2_forward(*desc, *px, int(keep), _ptr(hidden), _ptr(states), ksp, base, avail, _stream()),
                   "slime_dinov2_forward")


def tower_forward(pt: PackedTower, pixels: torch.Tensor, out_dtype: Optional[torch.dtype] = None,
                  keep_cls: bool = False, want_hidden: bool = False, out: Optional[torch.Tensor] = None,
                  k_split: Optional[Sequence[int]] = None):
    """pixels [N,3,S,S] (fp32 or the tower dtype) -> hidden_states[select_layer] in out_dtype (written into ``out`` if given: a
    contiguous tensor of that shape or leading-dim slice of one): the P patch rows [N, P, D], or with ``keep_cls`` all
    ``cfg.seq_len`` rows -- the class token in front for a CLIP tower, the class token and the registers for a DINOv2 tower, nothing
    more for a SigLIP tower.  ``want_hidden`` adds the fp32 state with all rows.
    k_split = (qkv, out_proj, fc1, fc2): run those layer GEMMs as deterministic split-K pairs (1 = unsplit).  None (the default) is
    the unsplit pass.  For one setting the result does not depend on how the crops are cut into calls; it is not bit-identical to
    another setting's."""
    pixels = _tower_pixels(pt, pixels)
    cfg, n = pt.cfg, pixels.shape[0]
    out_dtype = out_dtype or pixels.dtype
    rows = cfg.seq_len if keep_cls else cfg.num_patches
    if out is None:
        out = torch.empty((n, rows, cfg.hidden_size), dtype=out_dtype, device=pixels.device)
    elif tuple(out.shape) != (n, rows, cfg.hidden_size) or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError("tower_forward: out must be a contiguous [N, rows, hidden] tensor of the output dtype")
    hidden = torch.empty((n, cfg.seq_len, cfg.hidden_size), dtype=torch.float32, device=pixels.device) if want_hidden else None
    _tower_call(pt, pixels, out, keep_cls, hidden, None, k_split)
    return (out, hidden) if want_hidden else out


def tower_hidden_states(pt: PackedTower, pixels: torch.Tensor, k_split: Optional[Sequence[int]] = None) -> torch.Tensor:
    """pixels [N,3,S,S] -> fp32 [layers_run + 1, N, cfg.seq_len, D]: HF's hidden_states of ONE tower pass (entry 0 = the embeddings,
    after the pre-LayerNorm where the tower has one)."""
    pixels = _tower_pixels(pt, pixels)
    states = torch.empty((pt.layers_run + 1, pixels.shape[0], pt.cfg.seq_len, pt.cfg.hidden_size), dtype=torch.float32,
                         device=pixels.device)
    _tower_call(pt, pixels, None, True, None, states, k_split)
    return states


# The family-named calls, kept as spellings of the one path above (existing callers and the SigLIP / DINOv2 GPU tests use them).
siglip_tower_hidden_states = dinov2_tower_hidden_states = tower_hidden_states


def siglip_tower_forward(pt: PackedTower, pixels, out_dtype=None, want_hidden=False, out=None, k_split=None):
    """``tower_forward`` without ``keep_cls``: a SigLIP tower has no rows in front of its patches."""
    return tower_forward(pt, pixels, out_dtype, False, want_hidden, out, k_split)


def dinov2_tower_forward(pt: PackedTower, pixels, out_dtype=None, keep_prefix=False, want_hidden=False, out=None, k_split=None):
    """``tower_forward`` with ``keep_cls`` under its DINOv2 name."""
    return tower_forward(pt, pixels, out_dtype, keep_prefix, want_hidden, out, k_split)


# ------------------------------------------------------------------------------------------------
# SigLIP towers (HF SiglipVisionModel, patch 16, head_dim 64): slime_siglip_forward
# ------------------------------------------------------------------------------------------------
SIGLIP_ACT = "gelu_pytorch_tanh"
SIGLIP_MAX_GRID = 24


def check_siglip_config(cfg: SiglipVisionConfig) -> None:
    """The towers the SigLIP path runs, refused by name otherwise (no device work): the tanh-form GELU, head_dim 64, at most 24
    patches per side, an intermediate size that is a multiple of 128.  (so400m-patch14: head_dim 72, 4304, 27 per side;
    base-patch16-512: 32 per side.)"""
    if cfg.hidden_act != SIGLIP_ACT:
        raise ValueError(f"SigLIP vision tower hidden_act={cfg.hidden_act!r} is not supported: the HIP SigLIP path computes "
                         f"{SIGLIP_ACT!r} only")
    if cfg.num_attention_heads <= 0 or cfg.hidden_size % cfg.num_attention_heads or cfg.head_dim != 64:
        raise ValueError(f"SigLIP vision tower head_dim={cfg.hidden_size / max(cfg.num_attention_heads, 1):g} (hidden_size {cfg.hidden_size} / "
                         f"{cfg.num_attention_heads} heads) is not supported: head_dim must be 64")
    if cfg.patch_size <= 0 or cfg.image_size % cfg.patch_size or cfg.grid > SIGLIP_MAX_GRID:
        raise ValueError(f"SigLIP vision tower with {cfg.image_size / max(cfg.patch_size, 1):g} patches per side (image_size {cfg.image_size} / "
                         f"patch_size {cfg.patch_size}) is not supported: at most {SIGLIP_MAX_GRID} whole patches per side")
    if cfg.intermediate_size % 128:
        raise ValueError(f"SigLIP vision tower intermediate_size={cfg.intermediate_size} is not supported: it must be a multiple of 128")


def siglip_host_tensors(state_dict: Dict[str, torch.Tensor], cfg: SiglipVisionConfig, dtype: Optional[torch.dtype],
                        select_layer: int = -2) -> Dict[str, torch.Tensor]:
    """``tower_host_tensors`` for the SigLIP layout: the conv weight as a [D, kpad] matrix, ``pos`` = position_embedding +
    patch_embedding.bias [P, D] (one fp32 addition per element at pack time; float64 with dtype = None), and the same per-layer
    tensors.  ``post_layernorm.*`` and ``head.*`` are not read."""
    _check_operand_dtype(dtype, allow_none=True)
    sd = strip_tower_prefix(state_dict)
    L = layers_for_select(cfg, select_layer)
    f32, tt = _host_casts(dtype)
    pos = f32(sd["embeddings.position_embedding.weight"]) + f32(sd["embeddings.patch_embedding.bias"])[None, :]
    T: Dict[str, torch.Tensor] = {"patch_w": _conv_matrix(sd, cfg, tt), "pos": pos.contiguous()}
    _layer_host_tensors(T, sd, cfg, dtype, L)
    return T


def pack_siglip_tower(state_dict: Dict[str, torch.Tensor], cfg: SiglipVisionConfig, dtype: torch.dtype, device,
                      select_layer: int = -2) -> PackedTower:
    """HF SiglipVisionModel state dict (either key generation) -> device tensors in the kernels' layout, as ``pack_tower``: LayerNorm
    gamma / beta folded into q/k/v and fc1, pos', the fragment-order images, the colsums; slime_siglip_check at pack time."""
    _check_operand_dtype(dtype)
    check_siglip_config(cfg)
    L = layers_for_select(cfg, select_layer)
    return _pack_tail("pack_siglip_tower", "siglip", siglip_host_tensors(state_dict, cfg, dtype, select_layer), cfg, dtype, device, L,
                      lambda lib, d: lib.slime_siglip_check(d))


# ------------------------------------------------------------------------------------------------
# DINOv2 towers (HF Dinov2Model / Dinov2WithRegistersModel, ViT-B/14 and ViT-L/14): slime_dinov2_forward
# ------------------------------------------------------------------------------------------------
DINOV2_ACT = "gelu"
DINOV2_MAX_GRID = 24
DINOV2_MAX_REGISTERS = 16
DINOV2_WIDTHS = (128, 256, 768, 1024)


def check_dinov2_config(cfg: Dinov2VisionConfig) -> None:
    """The towers the DINOv2 path runs, refused by name otherwise (no device work): the plain MLP with the exact GELU, head_dim 64,
    a width the kernels have, a run size of at most 24 whole patches per side that is a multiple of 8, at most 16 register tokens.
    (The giant model: SwiGLU, head_dim 64 x 24 heads = 1536 wide; 518 px: 37 per side.)"""
    if cfg.use_swiglu_ffn:
        raise ValueError("DINOv2 vision tower use_swiglu_ffn=True (the giant model) is not supported: the HIP DINOv2 path runs the "
                         "fc1 / GELU / fc2 MLP only")
    if cfg.hidden_act != DINOV2_ACT:
        raise ValueError(f"DINOv2 vision tower hidden_act={cfg.hidden_act!r} is not supported: the HIP DINOv2 path computes "
                         f"{DINOV2_ACT!r} only")
    if cfg.num_attention_heads <= 0 or cfg.hidden_size % cfg.num_attention_heads or cfg.head_dim != 64:
        raise ValueError(f"DINOv2 vision tower head_dim={cfg.hidden_size / max(cfg.num_attention_heads, 1):g} (hidden_size {cfg.hidden_size} / "
                         f"{cfg.num_attention_heads} heads) is not supported: head_dim must be 64")
    if cfg.hidden_size not in DINOV2_WIDTHS:
        raise ValueError(f"DINOv2 vision tower hidden_size={cfg.hidden_size} is not supported: the widths are "
                         f"{', '.join(str(w) for w in DINOV2_WIDTHS)}")
    if cfg.intermediate_size % 128:
        raise ValueError(f"DINOv2 vision tower intermediate_size={cfg.intermediate_size} (hidden_size {cfg.hidden_size} x mlp_ratio "
                         f"{cfg.mlp_ratio}) is not supported: it must be a multiple of 128")
    if cfg.patch_size <= 0 or cfg.image_size <= 0 or cfg.image_size % cfg.patch_size or cfg.image_size % 8:
        raise ValueError(f"DINOv2 vision tower run size {cfg.image_size} is not supported: it must be a multiple of patch_size "
                         f"{cfg.patch_size} and of 8")
    if cfg.grid > DINOV2_MAX_GRID:
        raise ValueError(f"DINOv2 vision tower with {cfg.grid} patches per side (run size {cfg.image_size} / patch_size {cfg.patch_size}) "
                         f"is not supported: at most {DINOV2_MAX_GRID} patches per side")
    if not 0 <= cfg.num_register_tokens <= DINOV2_MAX_REGISTERS:
        raise ValueError(f"DINOv2 vision tower num_register_tokens={cfg.num_register_tokens} is not supported: at most "
                         f"{DINOV2_MAX_REGISTERS} register tokens")


def dinov2_pos_table(pos: torch.Tensor, grid: int, antialias: bool) -> torch.Tensor:
    """The patch rows of HF's ``interpolate_pos_encoding`` for a ``grid x grid`` input: ``pos`` [1, 1 + g0^2, D] -> fp32 [grid^2, D].
    HF's own arguments (fp32, bicubic, align_corners=False, an explicit size; ``antialias`` only in Dinov2WithRegistersModel), and
    as there no interpolation when the grids agree."""
    patch = pos.detach().cpu()[0, 1:]
    g0 = int(round(patch.shape[0] ** 0.5))
    if g0 * g0 != patch.shape[0]:
        raise ValueError(f"DINOv2 position table has {patch.shape[0]} patch rows: not a square grid")
    if g0 == grid:
        return patch.float().contiguous()
    t = patch.reshape(1, g0, g0, -1).permute(0, 3, 1, 2).to(torch.float32)
    t = torch.nn.functional.interpolate(t, size=(grid, grid), mode="bicubic", align_corners=False, antialias=antialias)
    return t.permute(0, 2, 3, 1).reshape(grid * grid, -1).contiguous()


def dinov2_host_tensors(state_dict: Dict[str, torch.Tensor], cfg: Dinov2VisionConfig, dtype: Optional[torch.dtype],
                        select_layer: int = -2, image_size: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """``tower_host_tensors`` for the DINOv2 layout (``image_size``: the run size, default ``cfg.image_size``):
      patch_w  the conv weight as a [D, kpad] matrix;
      cls      the prefix table [n_prefix, D]: row 0 = cls_token + position 0, then the register tokens as they are;
      pos      [P, D] = the position table's patch rows interpolated to the run grid (``dinov2_pos_table``) + the conv bias;
      w_qkv / w_fc1 with norm1 / norm2 folded in (``fold_ln``), q rows carrying dh^-0.5 log2(e);
      w_o = T(diag(lambda1) Wo), b_o = lambda1 * b and w_fc2 = T(diag(lambda2) W2), b_fc2 = lambda2 * b: LayerScale is linear.
    Matrices in ``dtype``, everything else fp32; ``dtype=None``: nothing is rounded, every tensor float64 (the interpolation itself
    is fp32 in HF whatever the model's dtype, and is here).  ``mask_token`` and ``layernorm.*`` are not read.

    fp16 and small lambda: a folded weight lambda * w below 2^-14 lands on the fp16 subnormal grid (spacing 2^-24), so its absolute
    rounding error is at most 2^-25 instead of 2^-11 relative; over a row of the GEMM that moves an element of h by at most
    2^-25 * sum_k |a_k|.  bf16 has fp32's exponent range and keeps its relative 2^-8."""
    _check_operand_dtype(dtype, allow_none=True)
    sd = strip_dinov2_prefix(state_dict)
    if image_size is not None and image_size != cfg.image_size:
        cfg = dataclasses.replace(cfg, image_size=int(image_size))
    L = layers_for_select(cfg, select_layer)
    f32, tt = _host_casts(dtype)
    D, R = cfg.hidden_size, cfg.num_register_tokens
    e = "embeddings."
    table = sd[e + "position_embeddings"]
    prefix = [f32(sd[e + "cls_token"]).reshape(1, D) + f32(table)[0, :1]]
    if R > 0:
        regs = f32(sd[e + "register_tokens"]).reshape(-1, D)
        if regs.shape[0] != R:
            raise ValueError(f"DINOv2 checkpoint has {regs.shape[0]} register tokens, the config says {R}")
        prefix.append(regs)
    pos = f32(dinov2_pos_table(table, cfg.grid, cfg.antialias)) + f32(sd[e + "patch_embeddings.projection.bias"])[None, :]
    T: Dict[str, torch.Tensor] = {"patch_w": _conv_matrix(sd, cfg, tt, e + "patch_embeddings.projection.weight"),
                                  "cls": torch.cat(prefix, 0).contiguous(), "pos": pos.contiguous()}
    _layer_host_tensors(T, sd, cfg, dtype, L, DINOV2_LAYER_KEYS)
    return T


def pack_dinov2_tower(state_dict: Dict[str, torch.Tensor], cfg: Dinov2VisionConfig, dtype: torch.dtype, device,
                      select_layer: int = -2, image_size: Optional[int] = None) -> PackedTower:
    """HF Dinov2Model / Dinov2WithRegistersModel state dict -> device tensors in the kernels' layout, as ``pack_tower``
    (``dinov2_host_tensors`` on ``device``, the fragment-order images); slime_dinov2_check at pack time.  In the descriptor ``image``
    is the run size, ``cls`` the prefix table, and ``pre_ln_*`` stay NULL."""
    _check_operand_dtype(dtype)
    if image_size is not None and image_size != cfg.image_size:
        cfg = dataclasses.replace(cfg, image_size=int(image_size))
    check_dinov2_config(cfg)
    L = layers_for_select(cfg, select_layer)
    return _pack_tail("pack_dinov2_tower", "dinov2", dinov2_host_tensors(state_dict, cfg, dtype, select_layer), cfg, dtype, device, L,
                      lambda lib, d: lib.slime_dinov2_check(d, cfg.n_prefix))


def gemm_kernel_name(M: int, N: int, K: int, dtype: torch.dtype, epilogue: int, has_b_frag: bool = False) -> str:
    lib = _lib.load()
    buf = C.create_string_buffer(128)
    _lib.check(lib.slime_gemm_kernel_name(M, N, K, dtype_code(dtype), epilogue, int(has_b_frag), buf, 128), "slime_gemm_kernel_name")
    return buf.value.decode()


def tower_kernel_names(pt: PackedTower, n_crops: int) -> Dict[int, str]:
    """probe kernel id (include/slime_hip.h: slime_probe) -> rocprofv3 kernel name for a tower pass over n_crops crops."""
    cfg = pt.cfg
    M, D, Fi = n_crops * cfg.seq_len, cfg.hidden_size, cfg.intermediate_size
    t = "F16" if pt.dtype == torch.float16 else "BF16"
    fr = {k: pt.tensors.get(k + "_frag") is not None for k in ("w_qkv", "w_o", "w_fc1", "w_fc2")}
    resid_epi = _lib.load().slime_vit_residual_epilogue()      # what the tower launches for out_proj / fc2
    if pt.form == "siglip":
        fc1_epi = _lib.EPI_BIAS_GELU_TANH_T
    else:
        fc1_epi = _lib.EPI_BIAS_GELU_T if pt.form == "dinov2" or pt.act == _lib.ACT_GELU else _lib.EPI_BIAS_QUICKGELU_T
    return {1: gemm_kernel_name(M, 3 * D, D, pt.dtype, _lib.EPI_BIAS_T, fr["w_qkv"]),
            2: f"attn64r_kernel<{t}, 3>" if 321 <= cfg.seq_len <= 608 and cfg.head_dim == 64 else f"attn_kernel<{t}, 64, 608, 8, 5>",
            5: gemm_kernel_name(M, Fi, D, pt.dtype, fc1_epi, fr["w_fc1"]),
            3: gemm_kernel_name(M, D, D, pt.dtype, resid_epi, fr["w_o"]),
            6: gemm_kernel_name(M, D, Fi, pt.dtype, resid_epi, fr["w_fc2"])}


@dataclass
class PackedResampler:
    dim: int
    heads: int
    n_query: int
    n_kv: int
    dtype: torch.dtype
    tensors: Dict[str, torch.Tensor]
    desc: _lib.ResamplerDesc
    ws: Workspace = field(default_factory=Workspace)


def _abs_pos(table: torch.Tensor, side: int) -> torch.Tensor:
    """get_abs_pos (sampler.py:27-36): bicubic resize of the square sincos table, rounded back to the
    table's dtype (fp16 in the reference)."""
    src = int(math.sqrt(table.shape[0]))
    dt = table.dtype
    return F.interpolate(table.float().reshape(1, src, src, -1).permute(0, 3, 1, 2), size=(side, side),
                         mode="bicubic", align_corners=False).permute(0, 2, 3, 1).flatten(0, 2).to(dt)


def pack_resampler(sd: Dict[str, torch.Tensor], dim: int, heads: int, n_kv: int, dtype: torch.dtype, device,
                   eps: float = 1e-6) -> PackedResampler:
    """Resampler state dict (keys as sampler.py:115-137) -> kernel layout.  The query side is input
    independent (sampler.py:161-163) and is folded into ``q_proj`` here, in fp32, once."""
    nq = sd["query"].shape[0]
    dh = dim // heads
    side = int(math.isqrt(n_kv))
    assert side * side == n_kv, "key grid must be square (sampler.py:146-147)"
    E = dim
    in_w, in_b = sd["attn.in_proj_weight"].float().cpu(), sd["attn.in_proj_bias"].float().cpu()
    pos_q = sd["pos_embed"].cpu()
    if torch.isnan(pos_q.float()).any():
        # sampler.py:150-154 ("some init error"): a stored table that contains NaN is regenerated from the sincos
        # formula in the stored dtype.  The reference tests this on the device at every call; here once, at pack time.
        from .weights import sincos_pos_embed_2d
        pos_q = torch.from_numpy(sincos_pos_embed_2d(dim, int(math.isqrt(nq)))).to(pos_q.dtype)
    q = F.layer_norm(sd["query"].float().cpu(), (E,), sd["ln_q.weight"].float().cpu(), sd["ln_q.bias"].float().cpu(), eps)
    q = F.linear(q + pos_q.float(), in_w[:E], in_b[:E]) * (dh ** -0.5 * LOG2E)
    pos_k = _abs_pos(pos_q, side).float()

    def f32(t):
        return t.detach().to(device=device, dtype=torch.float32).contiguous()

    def tt(t):
        return t.detach().to(device=device, dtype=torch.float32).to(dtype).contiguous()

    T = {"q_proj": tt(q), "pos_k": f32(pos_k), "ln_kv_w": f32(sd["ln_kv.weight"]), "ln_kv_b": f32(sd["ln_kv.bias"]),
         "w_k": tt(in_w[E:2 * E]), "b_k": f32(in_b[E:2 * E]), "w_v": tt(in_w[2 * E:]), "b_v": f32(in_b[2 * E:]),
         "w_o": tt(sd["attn.out_proj.weight"]), "b_o": f32(sd["attn.out_proj.bias"]),
         "ln_post_w": f32(sd["ln_post.weight"]), "ln_post_b": f32(sd["ln_post.bias"])}
    pack_static(T, ("w_k", "w_v", "w_o"))
    d = _lib.ResamplerDesc()
    d.dim, d.heads, d.n_query, d.n_kv, d.dtype, d.eps = dim, heads, nq, n_kv, dtype_code(dtype), eps
    for k, v in T.items():
        setattr(d, k, None if v is None else v.data_ptr())
    return PackedResampler(dim, heads, nq, n_kv, dtype, T, d)


def resampler_forward(pr: PackedResampler, x: torch.Tensor, want_t: bool = False):
    """x fp32 [n, n_kv, dim] -> fp32 [n, n_query, dim] (and the T copy if want_t)."""
    lib = _lib.load()
    _require_cuda(x, "x")
    x = x.float().contiguous()
    n = x.shape[0]
    assert x.shape[1] == pr.n_kv and x.shape[2] == pr.dim
    out = torch.empty((n, pr.n_query, pr.dim), dtype=torch.float32, device=x.device)
    out_t = torch.empty((n, pr.n_query, pr.dim), dtype=pr.dtype, device=x.device) if want_t else None
    need = lib.slime_resampler_workspace_bytes(C.byref(pr.desc), n)
    base, avail = pr.ws.aligned(need, x.device)
    _lib.check(lib.slime_resampler_forward(C.byref(pr.desc), x.data_ptr(), pr.dim, n, out.data_ptr(), _ptr(out_t), base,
                                           avail, _stream()), "slime_resampler_forward")
    return (out, out_t) if want_t else out


@dataclass
class PackedMlp:
    in_dim: int
    hidden: int
    dtype: torch.dtype
    tensors: Dict[str, torch.Tensor]
    desc: _lib.MlpDesc
    ws: Workspace = field(default_factory=Workspace)


def pack_mlp(w1, b1, w2, b2, dtype: torch.dtype, device) -> PackedMlp:
    T = {"w1": w1.detach().to(device=device, dtype=torch.float32).to(dtype).contiguous(),
         "b1": b1.detach().to(device=device, dtype=torch.float32).contiguous(),
         "w2": w2.detach().to(device=device, dtype=torch.float32).to(dtype).contiguous(),
         "b2": b2.detach().to(device=device, dtype=torch.float32).contiguous()}
    pack_static(T, ("w1", "w2"))
    d = _lib.MlpDesc()
    d.in_dim, d.hidden, d.dtype = w1.shape[1], w1.shape[0], dtype_code(dtype)
    for k, v in T.items():
        setattr(d, k, None if v is None else v.data_ptr())
    return PackedMlp(w1.shape[1], w1.shape[0], dtype, T, d)


def mlp_forward(pm: PackedMlp, x: torch.Tensor) -> torch.Tensor:
    """x [rows, in_dim] fp32 or T -> fp32 [rows, hidden]."""
    lib = _lib.load()
    _require_cuda(x, "x")
    x = x.contiguous()
    rows = x.shape[0]
    out = torch.empty((rows, pm.hidden), dtype=torch.float32, device=x.device)
    need = lib.slime_mlp_workspace_bytes(C.byref(pm.desc), rows)
    base, avail = pm.ws.aligned(need, x.device)
    xf = x.data_ptr() if x.dtype == torch.float32 else None
    xt = x.data_ptr() if x.dtype == pm.dtype else None
    if xf is None and xt is None:
        x = x.float()
        xf = x.data_ptr()
    _lib.check(lib.slime_mlp_forward(C.byref(pm.desc), xf, xt, rows, out.data_ptr(), base,
                                     avail, _stream()), "slime_mlp_forward")
    return out


@dataclass
class PackedGated:
    mlp: PackedMlp
    attn: PackedResampler
    w_gate: torch.Tensor
    ws: Workspace = field(default_factory=Workspace)


def pack_gated(sd: Dict[str, torch.Tensor], cfg: AdapterConfig, dtype: torch.dtype, device) -> PackedGated:
    """GatedBlock state dict (``mm_projector.`` prefix removed)."""
    mlp = pack_mlp(sd["projection.0.weight"], sd["projection.0.bias"], sd["projection.2.weight"],
                   sd["projection.2.bias"], dtype, device)
    attn = pack_resampler(sub_state(sd, "attn."), cfg.mm_hidden_size, cfg.num_heads, cfg.global_queries, dtype,
                          device, cfg.ln_eps)
    # w_gate is a bf16 Parameter cast to the activation dtype at use (projector/builder.py:148)
    wg = sd["w_gate"].detach().to(device=device, dtype=torch.float32).contiguous()
    return PackedGated(mlp, attn, wg)


def gated_forward(pg: PackedGated, x: torch.Tensor, learnable_gated: int = -1) -> torch.Tensor:
    """x fp32 [n, 576, D] -> fp32 [n, 576, H]: the full GatedBlock path."""
    lib = _lib.load()
    _require_cuda(x, "x")
    x = x.float().contiguous()
    n, Tn, D = x.shape
    assert Tn == pg.attn.n_kv and D == pg.mlp.in_dim
    out = torch.empty((n, Tn, pg.mlp.hidden), dtype=torch.float32, device=x.device)
    need = lib.slime_gated_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), n)
    base, avail = pg.ws.aligned(need, x.device)
    _lib.check(lib.slime_gated_forward(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), pg.w_gate.data_ptr(),
                                       int(learnable_gated), x.data_ptr(), n, out.data_ptr(), base,
                                       avail, _stream()), "slime_gated_forward")
    return out


def _adapter_feats(pg: PackedGated, feats: torch.Tensor) -> torch.Tensor:
    """Tower features as both fused adapter entries take them: on the GPU, in the operand dtype, contiguous."""
    _require_cuda(feats, "feats")
    return feats.to(pg.mlp.dtype).contiguous()


def _post_desc(post: Optional["PackedResampler"], any_local):
    """post_qformer's descriptor, or NULL for a batch without local crops."""
    return C.byref(post.desc) if any_local else None


def adapter_forward(pg: PackedGated, post: Optional["PackedResampler"], feats: torch.Tensor, n_images: int, n_local: int,
                    nw: int, nh: int, merge: bool = True, learnable_gated: int = -1,
                    out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused adapter for images that share one crop layout: tower features T [n_images*(1+n_local), 576, D] ->
    tokens [n_images, 576 + n_local*g*g, H] (gated global rows, then the merged local rows).  ``out`` may be a
    wider [n_images, rows, H] buffer (extra rows per image are left untouched)."""
    lib = _lib.load()
    feats = _adapter_feats(pg, feats)
    assert feats.shape[0] == n_images * (1 + n_local) and feats.shape[1] == pg.attn.n_kv and feats.shape[2] == pg.mlp.in_dim
    rows = pg.attn.n_kv + (n_local * post.n_query if n_local else 0)
    if out is None:
        out = torch.empty((n_images, rows, pg.mlp.hidden), dtype=out_dtype or feats.dtype, device=feats.device)
    assert out.dim() == 3 and out.shape[0] == n_images and out.shape[1] >= rows and out.shape[2] == pg.mlp.hidden and out.is_contiguous()
    pdesc = _post_desc(post, n_local)
    need = lib.slime_adapter_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), pdesc, n_images, n_local)
    base, avail = pg.ws.aligned(need, feats.device)
    _lib.check(lib.slime_adapter_forward(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), pg.w_gate.data_ptr(), int(learnable_gated),
                                         pdesc, feats.data_ptr(), n_images, n_local, nw, nh, int(merge), out.data_ptr(),
                                         dtype_code(out.dtype), out.shape[1], base, avail, _stream()), "slime_adapter_forward")
    return out


RAGGED_MAX_IMAGES = 64        # SLIME_ADAPTER_RAGGED_MAX_IMAGES: the per-image layout travels in the plan kernel's arguments


def adapter_ragged_plan(grids, P: int, q: int, merge: bool = True, out_row0=None):
    """Host restatement of the ragged adapter's plan (rowwise.hip: adapter_ragged_plan_kernel), pure integer logic: ``grids`` =
    per-image ``(nw, nh)`` (``(0, 0)``: no local crops), ``P`` global rows and ``q = g*g`` rows per local crop.  Returns
    ``(out_row0, rows, row_map)``: the first token-buffer row of every image (packed back to back unless given), the rows a
    packed buffer needs (the end of the last range when ``out_row0`` is given), and ``row_map(r)`` = token-buffer row of GEMM row
    r of projection[2]'s output ``[global rows of every image | local rows of every image]``."""
    n = [int(nw) * int(nh) for nw, nh in grids]
    if out_row0 is None:
        out_row0, o = [], 0
        for n_i in n:
            out_row0.append(o)
            o += P + n_i * q
    out_row0 = [int(r) for r in out_row0]
    rows = max((r + P + n_i * q for r, n_i in zip(out_row0, n)), default=0)
    lrow0 = [0]
    for n_i in n:
        lrow0.append(lrow0[-1] + n_i * q)
    B, g = len(n), math.isqrt(q)

    def row_map(r: int) -> int:
        if r < B * P:
            return out_row0[r // P] + r % P
        e = r - B * P
        b = 0
        while b < B - 1 and e >= lrow0[b + 1]:
            b += 1
        rr = e - lrow0[b]
        d = rr
        if merge:
            nw = max(int(grids[b][0]), 1)
            qx, qy, k = rr % g, (rr // g) % g, rr // (g * g)
            gx, gy = k % nw, k // nw
            d = ((gy * g + qy) * nw + gx) * g + qx
        return out_row0[b] + P + d
    return out_row0, rows, row_map


def adapter_forward_ragged(pg: PackedGated, post: Optional["PackedResampler"], feats: torch.Tensor, grids, merge: bool = True,
                           learnable_gated: int = -1, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                           out_row0=None):
    """Fused adapter for images with DIFFERENT crop layouts (``slime_adapter_forward_ragged``): tower features T
    [sum_i (1 + n_i), 576, D] in image order, ``grids[i] = (nw_i, nh_i)`` with n_i = nw_i * nh_i local crops (``(0, 0)``: none;
    ``merge=False``: ``(n_i, 1)``).  Returns ``(tokens [rows, H], out_row0)``: image i owns rows ``[out_row0[i], out_row0[i] + 576 +
    n_i*g*g)`` -- gated global rows, then its local rows in raster order of its own grid.  ``out`` may be a larger flat [rows, H]
    buffer (fp32 or T) with ``out_row0`` chosen by the caller; rows no image owns are left untouched."""
    lib = _lib.load()
    feats = _adapter_feats(pg, feats)
    grids = [(int(nw), int(nh)) for nw, nh in grids]
    B, n_crops = len(grids), sum(1 + nw * nh for nw, nh in grids)
    if feats.dim() != 3 or feats.shape[0] != n_crops or feats.shape[1] != pg.attn.n_kv or feats.shape[2] != pg.mlp.in_dim:
        raise _lib.SlimeHipError(f"adapter_forward_ragged: the grids {grids} hold {n_crops} crops of [{pg.attn.n_kv}, {pg.mlp.in_dim}], "
                                 f"feats is {tuple(feats.shape)}")
    any_local = n_crops > B
    if any_local and post is None:
        raise _lib.SlimeHipError("adapter_forward_ragged: local crops without post_qformer")
    q = post.n_query if any_local else 1
    row0, rows, _ = adapter_ragged_plan(grids, pg.attn.n_kv, q, merge, out_row0)
    if out is None:
        out = torch.empty((rows, pg.mlp.hidden), dtype=out_dtype or feats.dtype, device=feats.device)
    assert out.dim() == 2 and out.shape[1] == pg.mlp.hidden and out.is_contiguous()
    nw_a = (C.c_int * max(B, 1))(*[g[0] for g in grids])
    nh_a = (C.c_int * max(B, 1))(*[g[1] for g in grids])
    r0_a = (C.c_longlong * max(B, 1))(*row0) if out_row0 is not None else None
    pdesc = _post_desc(post, any_local)
    need = lib.slime_adapter_ragged_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), pdesc, B, nw_a, nh_a)
    base, avail = pg.ws.aligned(max(need, 256), feats.device)
    _lib.check(lib.slime_adapter_forward_ragged(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), pg.w_gate.data_ptr(), int(learnable_gated),
                                                pdesc, feats.data_ptr(), B, nw_a, nh_a, int(merge), out.data_ptr(), dtype_code(out.dtype),
                                                r0_a, out.shape[0], base, avail, _stream()), "slime_adapter_forward_ragged")
    return out, row0


def adapter_forward_precompressed(pg: PackedGated, glob: torch.Tensor, comp: torch.Tensor, n_images: int, n_local: int, nw: int, nh: int,
                                  merge: bool = True, learnable_gated: int = -1, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """Adapter for the compressed-local exchange (slime_amd.dist.sharded_tower_compressed): ``glob`` T [B, 576, D] tower
    features of the global views, ``comp`` T [B*n_local, q, D] local crops ALREADY through post_qformer.  Per-module sequence
    (GatedBlock, projection MLP, batched merge) -- the arithmetic of adapter_forward after its post_qformer stage."""
    lib = _lib.load()
    B, P, q = n_images, glob.shape[1], comp.shape[1]
    g = int(math.isqrt(q))
    H = pg.mlp.hidden
    out = torch.empty((B, P + n_local * q, H), dtype=out_dtype or glob.dtype, device=glob.device)
    gt = gated_forward(pg, glob.float(), learnable_gated)                                   # fp32 [B, P, H]
    loc = mlp_forward(pg.mlp, comp.reshape(-1, comp.shape[-1]).contiguous())               # fp32 [B*n_local*q, H]
    _lib.check(lib.slime_merge_rows_batched(gt.data_ptr(), P, out.data_ptr(), dtype_code(out.dtype), out.shape[1], 0, B, P, 1, 1, H, 0,
                                            _stream()), "slime_merge_rows_batched")
    _lib.check(lib.slime_merge_rows_batched(loc.data_ptr(), n_local * q, out.data_ptr(), dtype_code(out.dtype), out.shape[1], P, B, nw,
                                            nh, g, H, int(merge), _stream()), "slime_merge_rows_batched")
    return out


def merge_rows(local: torch.Tensor, out: torch.Tensor, dst_row0: int, nw: int, nh: int, grid: int, merge: bool):
    """Scatter [n, g*g, C] fp32 local tokens into ``out`` rows (spatial raster order or flat), casting."""
    lib = _lib.load()
    C_ = local.shape[-1]
    _lib.check(lib.slime_merge_rows(_ptr(local), _ptr(out), dtype_code(out.dtype), int(dst_row0), nw, nh, grid, C_,
                                    int(merge), _stream()), "slime_merge_rows")


def gather_rows(src: torch.Tensor, out: torch.Tensor, rows_in: int, row_off: int, groups: int, rows_out: int):
    lib = _lib.load()
    _lib.check(lib.slime_gather_rows(_ptr(src), rows_in, row_off, _ptr(out), dtype_code(out.dtype), groups, rows_out,
                                     src.shape[-1], _stream()), "slime_gather_rows")


def tile_normalize(canvas_u8: torch.Tensor, crop: int, mean, std, out_dtype: torch.dtype) -> torch.Tensor:
    """uint8 [Hc, Wc, 3] device canvas -> normalised crops [(Hc/crop)*(Wc/crop), 3, crop, crop]."""
    lib = _lib.load()
    _require_cuda(canvas_u8, "canvas")
    Hc, Wc, _ = canvas_u8.shape
    n = (Hc // crop) * (Wc // crop)
    out = torch.empty((n, 3, crop, crop), dtype=out_dtype, device=canvas_u8.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.slime_tile_normalize(_ptr(canvas_u8.contiguous()), Hc, Wc, crop, m, s, out.data_ptr(),
                                        dtype_code(out_dtype), _stream()), "slime_tile_normalize")
    return out


def resample_tables(in_size: int, out_size: int, filter: int = _lib.FILTER_BICUBIC):
    """Host-side Pillow coefficient tables (int32 numpy arrays): bounds [out, 2], kk [out, ksize].  ``filter``: ``_lib.FILTER_BICUBIC``
    (``Image.BICUBIC``) or ``_lib.FILTER_LANCZOS`` (``Image.LANCZOS``)."""
    import numpy as np
    lib = _lib.load()
    ks = lib.slime_resample_ksize_ex(in_size, out_size, filter)
    if ks <= 0:
        raise ValueError(f"resample_tables: bad sizes {in_size} -> {out_size} or filter {filter}")
    bounds = np.empty((out_size, 2), dtype=np.int32)
    kk = np.empty((out_size, ks), dtype=np.int32)
    _lib.check(lib.slime_resample_coeffs_ex(in_size, out_size, filter, bounds.ctypes.data, kk.ctypes.data), "slime_resample_coeffs_ex")
    return bounds, kk


_TABLE_CACHE = {}


def _device_tables(in_size: int, out_size: int, device: torch.device, filter: int = _lib.FILTER_BICUBIC):
    key = (in_size, out_size, str(device), filter)
    hit = _TABLE_CACHE.get(key)
    if hit is None:
        b, k = resample_tables(in_size, out_size, filter)
        hit = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), k.shape[1])
        if len(_TABLE_CACHE) > 256:
            _TABLE_CACHE.clear()
        _TABLE_CACHE[key] = hit
    return hit


def resize_bicubic_u8(img_u8: torch.Tensor, out_w: int, out_h: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bit-exact ``PIL.Image.resize((out_w, out_h))`` (default bicubic) of a uint8 [H, W, 3] device image.
    ``out`` may be a [out_h, out_w, 3] view into a larger canvas (last two dims contiguous)."""
    lib = _lib.load()
    _require_cuda(img_u8, "image")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError(f"resize_bicubic_u8 expects a uint8 [H, W, 3] image, got {img_u8.dtype} {tuple(img_u8.shape)}")
    if img_u8.stride(2) != 1 or img_u8.stride(1) != 3:
        img_u8 = img_u8.contiguous()
    H, W, _ = img_u8.shape
    if out is None:
        out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=img_u8.device)
    elif tuple(out.shape) != (out_h, out_w, 3) or out.stride(2) != 1 or out.stride(1) != 3 or out.dtype != torch.uint8:
        raise ValueError("resize_bicubic_u8: out must be a uint8 [out_h, out_w, 3] view with packed pixels")
    bh = kh = bv = kv = None
    ksh = ksv = 0
    if W != out_w:
        bh, kh, ksh = _device_tables(W, out_w, img_u8.device)
    if H != out_h:
        bv, kv, ksv = _device_tables(H, out_h, img_u8.device)
    tmp = torch.empty((H * out_w * 3,), dtype=torch.uint8, device=img_u8.device) if (bh is not None and bv is not None) else None
    _lib.check(lib.slime_resize_bicubic_u8(img_u8.data_ptr(), H, W, img_u8.stride(0), out.data_ptr(), out.stride(0), out_h, out_w,
                                           _ptr(bh), _ptr(kh), ksh, _ptr(bv), _ptr(kv), ksv, _ptr(tmp),
                                           0 if tmp is None else tmp.numel(), _stream()), "slime_resize_bicubic_u8")
    return out


def resize_bicubic_u8_batched(imgs_u8: torch.Tensor, out_w: int, out_h: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batched :func:`resize_bicubic_u8`: uint8 [B, H, W, 3] -> [B, out_h, out_w, 3], one launch per pass for the
    whole batch.  ``out`` may be the interior view canvas[:, y0:y0+out_h, x0:x0+out_w] of a [B, Hc, Wc, 3] buffer."""
    lib = _lib.load()
    _require_cuda(imgs_u8, "images")
    if imgs_u8.dtype != torch.uint8 or imgs_u8.dim() != 4 or imgs_u8.shape[3] != 3:
        raise ValueError(f"resize_bicubic_u8_batched expects uint8 [B, H, W, 3], got {imgs_u8.dtype} {tuple(imgs_u8.shape)}")
    imgs_u8 = imgs_u8.contiguous()
    B, H, W, _ = imgs_u8.shape
    if out is None:
        out = torch.empty((B, out_h, out_w, 3), dtype=torch.uint8, device=imgs_u8.device)
    elif (tuple(out.shape) != (B, out_h, out_w, 3) or out.stride(3) != 1 or out.stride(2) != 3 or out.dtype != torch.uint8):
        raise ValueError("resize_bicubic_u8_batched: out must be a uint8 [B, out_h, out_w, 3] view with packed pixels")
    bh = kh = bv = kv = None
    ksh = ksv = 0
    if W != out_w:
        bh, kh, ksh = _device_tables(W, out_w, imgs_u8.device)
    if H != out_h:
        bv, kv, ksv = _device_tables(H, out_h, imgs_u8.device)
    tmp = torch.empty((B * H * out_w * 3,), dtype=torch.uint8, device=imgs_u8.device) if (bh is not None and bv is not None) else None
    _lib.check(lib.slime_resize_bicubic_u8_batched(imgs_u8.data_ptr(), B, imgs_u8.stride(0), H, W, imgs_u8.stride(1), out.data_ptr(),
                                                   out.stride(0), out.stride(1), out_h, out_w, _ptr(bh), _ptr(kh), ksh, _ptr(bv),
                                                   _ptr(kv), ksv, _ptr(tmp), 0 if tmp is None else tmp.numel(), _stream()),
               "slime_resize_bicubic_u8_batched")
    return out


def tile_normalize_batched(canvas_u8: torch.Tensor, crop: int, mean, std, out: torch.Tensor, first_crop: int) -> None:
    """uint8 [B, Hc, Wc, 3] canvases -> normalised tiles written into out[b, first_crop + tile] of a
    [B, crops_per_image, 3, crop, crop] tensor (contiguous)."""
    lib = _lib.load()
    _require_cuda(canvas_u8, "canvas")
    canvas_u8 = canvas_u8.contiguous()
    B, Hc, Wc, _ = canvas_u8.shape
    tiles = (Hc // crop) * (Wc // crop)
    assert out.is_contiguous() and out.dim() == 5 and out.shape[0] == B and first_crop + tiles <= out.shape[1]
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    base = out.data_ptr() + first_crop * 3 * crop * crop * out.element_size()
    _lib.check(lib.slime_tile_normalize_batched(canvas_u8.data_ptr(), B, canvas_u8.stride(0), Hc, Wc, crop, m, s, base, out.shape[1],
                                                dtype_code(out.dtype), _stream()), "slime_tile_normalize_batched")


def slice_jobs(jobs, crop: int, mean, std, out: torch.Tensor) -> None:
    """The slicer for differently sized images (``slime_slice_jobs``): two launches and one table upload for the whole list.
    ``jobs``: up to 128 tuples ``(src, out_w, out_h, canvas_w, canvas_h, x0, y0, first_crop)`` -- ``src`` a uint8 [H, W, 3] device image,
    resized as ``PIL.Image.resize((out_w, out_h))`` does, pasted at (x0, y0) into a black canvas_h x canvas_w canvas whose row-major
    ``crop`` x ``crop`` tiles become the normalised crops ``out[first_crop : first_crop + tiles]``.  ``out``: contiguous
    [crops, 3, crop, crop] device tensor (fp32 / bf16 / fp16); crops no job names keep their contents."""
    lib = _lib.load()
    _require_cuda(out, "out")
    if out.dim() != 4 or tuple(out.shape[1:]) != (3, crop, crop) or not out.is_contiguous():
        raise ValueError(f"slice_jobs: out must be a contiguous [crops, 3, {crop}, {crop}] tensor, got {tuple(out.shape)}")
    n = len(jobs)
    table = (_lib.SliceJob * max(n, 1))()
    keep = []                                              # tensors the table points to
    for J, (src, out_w, out_h, canvas_w, canvas_h, x0, y0, first_crop) in zip(table, jobs):
        _require_cuda(src, "image")
        if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
            raise ValueError(f"slice_jobs expects uint8 [H, W, 3] images, got {src.dtype} {tuple(src.shape)}")
        if src.stride(2) != 1 or src.stride(1) != 3:
            src = src.contiguous()
        keep.append(src)
        H, W, _ = src.shape
        J.src, J.src_stride, J.src_h, J.src_w = src.data_ptr(), src.stride(0), H, W
        J.out_h, J.out_w, J.canvas_h, J.canvas_w, J.x0, J.y0, J.first_crop = out_h, out_w, canvas_h, canvas_w, x0, y0, first_crop
        if W != out_w:
            b, k, J.ksize_h = _device_tables(W, out_w, src.device)
            J.bounds_h, J.kk_h = b.data_ptr(), k.data_ptr()
            keep += [b, k]
        if H != out_h:
            b, k, J.ksize_v = _device_tables(H, out_h, src.device)
            J.bounds_v, J.kk_v = b.data_ptr(), k.data_ptr()
            keep += [b, k]
    tmp_bytes = C.c_size_t(0)
    _lib.check(lib.slime_slice_jobs_plan(table, n, crop, C.byref(tmp_bytes)), "slime_slice_jobs_plan")
    nbytes = n * C.sizeof(_lib.SliceJob)
    staging = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
    C.memmove(staging.data_ptr(), table, nbytes)
    table_dev = staging.to(out.device, non_blocking=True)                  # the one upload
    tmp = torch.empty((tmp_bytes.value,), dtype=torch.uint8, device=out.device) if tmp_bytes.value else None
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    _lib.check(lib.slime_slice_jobs(table, table_dev.data_ptr(), n, crop, m, s, out.data_ptr(), out.shape[0], dtype_code(out.dtype),
                                    _ptr(tmp), tmp_bytes.value, _stream()), "slime_slice_jobs")


class ViewSpec(NamedTuple):
    """One view job of :func:`view_jobs` (``slime_view_job`` without its pointers): the box ``(x0, y0, w, h)`` of the image that is
    used, the field it is pasted into at ``paste`` = (x, y) over colour ``bg``, the resize of that field to ``out`` = (w, h) with
    ``filter``, and the windows ``(x0, y0, step, nx, ny)`` of the resized image."""
    box: tuple
    field: tuple
    paste: tuple
    bg: tuple
    out: tuple
    filter: int
    windows: tuple

    @property
    def crops(self) -> int:
        return self.windows[3] * self.windows[4]


def view_jobs(jobs, crop: int, mean, std, out: torch.Tensor) -> None:
    """The slicer of the 'pad', 'pad_then_devide', 'any_res' and bare-processor modes (``slime_view_jobs``): per 128 jobs two launches
    and one table upload.  ``jobs``: tuples ``(img, spec, first_crop)`` -- ``img`` a uint8 [H, W, 3] device image, ``spec`` a
    :class:`ViewSpec`; the job's windows become the normalised crops ``out[first_crop : first_crop + spec.crops]``, bit-identical to
    materialising the padded field, ``PIL.Image.resize(spec.out, filter)``, cropping and ``ClipImageProcessor.normalize_u8``.
    ``out``: contiguous [crops, 3, crop, crop] device tensor (fp32 / bf16 / fp16); crops no job names keep their contents."""
    lib = _lib.load()
    _require_cuda(out, "out")
    if out.dim() != 4 or tuple(out.shape[1:]) != (3, crop, crop) or not out.is_contiguous():
        raise ValueError(f"view_jobs: out must be a contiguous [crops, 3, {crop}, {crop}] tensor, got {tuple(out.shape)}")
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    contiguous = {}                                        # one packed copy per image, however many jobs name it
    for i0 in range(0, max(len(jobs), 1), _lib.VIEW_MAX_JOBS):
        chunk = jobs[i0:i0 + _lib.VIEW_MAX_JOBS]
        n = len(chunk)
        table = (_lib.ViewJob * max(n, 1))()
        keep = []                                          # tensors the table points to
        for J, (img, spec, first_crop) in zip(table, chunk):
            _require_cuda(img, "image")
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError(f"view_jobs expects uint8 [H, W, 3] images, got {img.dtype} {tuple(img.shape)}")
            if img.stride(2) != 1 or img.stride(1) != 3:
                if id(img) not in contiguous:
                    contiguous[id(img)] = img.contiguous()
                img = contiguous[id(img)]
            keep.append(img)
            J.img, J.img_stride, J.img_h, J.img_w = img.data_ptr(), img.stride(0), img.shape[0], img.shape[1]
            J.box_x0, J.box_y0, J.box_w, J.box_h = spec.box
            (J.field_w, J.field_h), (J.paste_x, J.paste_y) = spec.field, spec.paste
            J.bg[0], J.bg[1], J.bg[2] = spec.bg
            (J.out_w, J.out_h), J.filter = spec.out, spec.filter
            J.win_x0, J.win_y0, J.win_step, J.win_nx, J.win_ny = spec.windows
            J.first_crop = first_crop
            if J.field_w != J.out_w:
                b, k, J.ksize_h = _device_tables(J.field_w, J.out_w, img.device, spec.filter)
                J.bounds_h, J.kk_h = b.data_ptr(), k.data_ptr()
                keep += [b, k]
            if J.field_h != J.out_h:
                b, k, J.ksize_v = _device_tables(J.field_h, J.out_h, img.device, spec.filter)
                J.bounds_v, J.kk_v = b.data_ptr(), k.data_ptr()
                keep += [b, k]
        tmp_bytes = C.c_size_t(0)
        _lib.check(lib.slime_view_jobs_plan(table, n, crop, C.byref(tmp_bytes)), "slime_view_jobs_plan")
        nbytes = n * C.sizeof(_lib.ViewJob)
        staging = torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True)
        C.memmove(staging.data_ptr(), table, nbytes)
        table_dev = staging.to(out.device, non_blocking=True)              # the one upload
        tmp = torch.empty((tmp_bytes.value,), dtype=torch.uint8, device=out.device) if tmp_bytes.value else None
        _lib.check(lib.slime_view_jobs(table, table_dev.data_ptr(), n, crop, m, s, out.data_ptr(), out.shape[0], dtype_code(out.dtype),
                                       _ptr(tmp), tmp_bytes.value, _stream()), "slime_view_jobs")


def router_scores(local_f: torch.Tensor, text: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Cosine router scores [T] (fp32) for local tokens [T,H] against text embeddings [L,H]."""
    lib = _lib.load()
    _require_cuda(local_f, "local_f")
    img = local_f.float().contiguous()
    txt = text.to(device=img.device, dtype=torch.float32).contiguous()
    T, H = img.shape
    L = txt.shape[0]
    m = None if mask is None else mask.to(device=img.device).ne(0).to(torch.uint8).contiguous()
    scores = torch.empty((T,), dtype=torch.float32, device=img.device)
    ws = torch.empty((L + H + 8,), dtype=torch.float32, device=img.device)
    _lib.check(lib.slime_router_scores(img.data_ptr(), T, txt.data_ptr(), L, _ptr(m), H, scores.data_ptr(), ws.data_ptr(),
                                       _stream()), "slime_router_scores")
    return scores


def router_select(scores: torch.Tensor, topp: float, temp: float, want_probs: bool = False):
    """Device-side top-p selection; returns (keep_idx_buffer [T] int32, count [1] int32[, probs])."""
    lib = _lib.load()
    T = scores.shape[0]
    keep = torch.empty((T,), dtype=torch.int32, device=scores.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=scores.device)
    probs = torch.empty((T,), dtype=torch.float32, device=scores.device) if want_probs else None
    _lib.check(lib.slime_router_select(scores.data_ptr(), T, float(temp), float(topp), keep.data_ptr(), cnt.data_ptr(),
                                       _ptr(probs), _stream()), "slime_router_select")
    return (keep, cnt, probs) if want_probs else (keep, cnt)


def router_topp(local_f: torch.Tensor, text: torch.Tensor, mask: Optional[torch.Tensor], topp: float, temp: float) -> torch.Tensor:
    """Indices (ascending, int64) of the local tokens the text-guided router keeps.  One D2H read of the
    count -- the output length is data dependent (the reference syncs at ``nonzero`` too)."""
    if local_f.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.long, device=local_f.device)
    keep, cnt = router_select(router_scores(local_f, text, mask), topp, temp)
    return keep[: int(cnt.item())].long()


class RouterState(NamedTuple):
    """What the batched router leaves on the device, plus the one thing the host needs: ``keep`` int32 [B, T_max] (row b: the kept
    local indices, ascending, in its first ``counts[b]`` entries), ``cnt`` int32 [B], ``off`` int64 [B] (first local row of
    every image in the token buffer), ``n_rows`` int32 [B]; ``counts`` = ``cnt`` on the host."""
    keep: torch.Tensor
    cnt: torch.Tensor
    off: torch.Tensor
    n_rows: torch.Tensor
    counts: List[int]


def router_select_batched_device(tokens: torch.Tensor, row_off: Sequence[int], n_rows: Sequence[int], text: torch.Tensor,
                                 mask: Optional[torch.Tensor], topp: float, temp: float) -> RouterState:
    """The router for the B images of a step in ONE launch pair and ONE D2H read (of the B kept counts), its results left on the
    device (``RouterState``) for ``splice_routed``.
    ``tokens`` fp32 [rows, H] (any 2-D contiguous view of the token buffer); image b owns rows
    ``row_off[b] .. row_off[b] + n_rows[b] - 1``; ``text`` [B, L, H], ``mask`` [B, L] or None."""
    lib = _lib.load()
    _require_cuda(tokens, "tokens")
    assert tokens.dim() == 2 and tokens.dtype == torch.float32 and tokens.is_contiguous()
    B, H = len(n_rows), tokens.shape[1]
    dev = tokens.device
    T_max = max(int(n) for n in n_rows) if B else 0
    if B == 0 or T_max == 0:                                        # nothing to route: no launch, no sync
        return RouterState(torch.zeros((B, 1), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
                           torch.tensor([int(o) for o in row_off], dtype=torch.int64).to(dev),
                           torch.zeros((B,), dtype=torch.int32, device=dev), [0] * B)
    txt = text.to(device=dev, dtype=torch.float32).contiguous()
    L = txt.shape[1]
    m = None if mask is None else mask.to(device=dev).ne(0).to(torch.uint8).contiguous()
    off = torch.tensor([int(o) for o in row_off], dtype=torch.int64).to(dev, non_blocking=True)
    cnt_in = torch.tensor([int(n) for n in n_rows], dtype=torch.int32).to(dev, non_blocking=True)
    scores = torch.empty((B, T_max), dtype=torch.float32, device=dev)
    keep = torch.empty((B, T_max), dtype=torch.int32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.slime_router_batched_workspace_floats(B, L, H) + 8,), dtype=torch.float32, device=dev)
    _lib.check(lib.slime_router_scores_batched(tokens.data_ptr(), off.data_ptr(), cnt_in.data_ptr(), B, T_max, txt.data_ptr(), L,
                                               _ptr(m), H, scores.data_ptr(), ws.data_ptr(), _stream()), "slime_router_scores_batched")
    _lib.check(lib.slime_router_select_batched(scores.data_ptr(), cnt_in.data_ptr(), B, T_max, float(temp), float(topp),
                                               keep.data_ptr(), cnt.data_ptr(), _stream()), "slime_router_select_batched")
    return RouterState(keep, cnt, off, cnt_in, cnt.cpu().tolist())           # the step's only host sync


def router_topp_batched(tokens: torch.Tensor, row_off: Sequence[int], n_rows: Sequence[int], text: torch.Tensor,
                        mask: Optional[torch.Tensor], topp: float, temp: float) -> List[torch.Tensor]:
    """``router_select_batched_device`` as per-image tensors: the kept LOCAL indices of every image (ascending, int64, relative to
    row_off[b])."""
    st = router_select_batched_device(tokens, row_off, n_rows, text, mask, topp, temp)
    return [st.keep[b, :st.counts[b]].long() for b in range(len(n_rows))]


# ---- the attention router (mm_resampler_type='qformer': TextGuidedRouterAttention, resampler/builder.py:94-162) ----------------------

ROUTER_MAX_T = 4096          # slime_router_select's limit (ROUTER_MAX_T in csrc/router.hip)
ROUTER_ATTN_MAX_H = 8192
ROUTER_ATTN_EPS = 1e-5       # nn.LayerNorm's default (the Resampler's partial(nn.LayerNorm, eps=1e-6) is NOT used by the router)


@dataclass
class PackedRouterAttention:
    H: int
    heads: int
    N1: int
    dtype: torch.dtype
    tensors: Dict[str, Optional[torch.Tensor]]
    desc: _lib.RouterAttnDesc
    ws: Workspace = field(default_factory=Workspace)


def router_attention_host_tensors(sd: Dict[str, torch.Tensor], H: int, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """The pack-time algebra of ``pack_router_attention`` on the host (fp32 in, CPU tensors out): ``cross_attn.in_proj_weight`` rows
    [q; k; v] become ``w_q`` = T(Wq s), ``b_q`` = bq s with s = 128^-0.5 log2(e) (slime_attention takes q pre-scaled) and ONE
    ``w_kv`` [2H, H] = [Wk; Wv] (the k|v projection is one GEMM; attention reads k and v with row stride 2H); ``prob_proj`` is zero
    padded from H / 4 to N1 = the next multiple of 128 (zero weight rows, zero bias, zero w2: the padding adds exactly 0)."""
    if H % 128 != 0 or H < 128 or H > ROUTER_ATTN_MAX_H:
        raise ValueError(f"attention router: hidden_size={H} must be a multiple of 128 (heads of 128) in 128..{ROUTER_ATTN_MAX_H}")
    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"attention router: operand dtype {dtype} is not a 16-bit MFMA type")
    f = lambda k: sd[k].detach().float().cpu()
    in_w, in_b = f("cross_attn.in_proj_weight"), f("cross_attn.in_proj_bias")
    assert in_w.shape == (3 * H, H) and in_b.shape == (3 * H,), "cross_attn.in_proj_* must be [3H, H] / [3H]"
    s = 128 ** -0.5 * LOG2E
    n1, N1 = H // 4, (H // 4 + 127) // 128 * 128
    w1 = torch.zeros((N1, H), dtype=torch.float32)
    b1 = torch.zeros((N1,), dtype=torch.float32)
    w2 = torch.zeros((N1,), dtype=torch.float32)
    w1[:n1], b1[:n1], w2[:n1] = f("prob_proj.0.weight"), f("prob_proj.0.bias"), f("prob_proj.2.weight").view(-1)
    T = {"w_q": (in_w[:H] * s).to(dtype), "b_q": in_b[:H] * s, "w_kv": in_w[H:].to(dtype), "b_kv": in_b[H:].clone(),
         "w_o": f("cross_attn.out_proj.weight").to(dtype), "b_o": f("cross_attn.out_proj.bias"),
         "w_1": w1.to(dtype), "b_1": b1, "w_2": w2, "b_2": f("prob_proj.2.bias").view(())}
    for ln in ("ln_q", "ln_kv", "ln_post"):
        T[ln + "_w"], T[ln + "_b"] = f(ln + ".weight"), f(ln + ".bias")
    return {k: v.contiguous() for k, v in T.items()}


def pack_router_attention(sd: Dict[str, torch.Tensor], H: int, dtype: torch.dtype, device) -> PackedRouterAttention:
    """``TextGuidedRouterAttention`` state dict -> kernel layout (``router_attention_host_tensors`` on ``device``, the four
    matrices also in MFMA-fragment order where ``pack_b_frag`` applies).  ``query`` and ``self_attn.*`` are not packed: they take
    no part in the forward pass."""
    host = router_attention_host_tensors(sd, H, dtype)
    b2 = float(host.pop("b_2"))
    T: Dict[str, Optional[torch.Tensor]] = {k: v.to(device) for k, v in host.items()}
    pack_static(T, ("w_q", "w_kv", "w_o", "w_1"))
    d = _lib.RouterAttnDesc()
    d.H, d.heads, d.N1, d.dtype, d.eps, d.b_2 = H, H // 128, T["w_2"].shape[0], dtype_code(dtype), ROUTER_ATTN_EPS, b2
    for k, v in T.items():
        setattr(d, k, None if v is None else v.data_ptr())
    return PackedRouterAttention(H, H // 128, int(T["w_2"].shape[0]), dtype, T, d)


def _router_attention_plan(row_off: Sequence[int], n_rows: Sequence[int], L: int, mask_host):
    """Host side of the attention router: (tok_idx, key_idx, n_keys) -- the token rows of every image and the text rows
    (b * L + l) of the valid keys of every image that has tokens, image after image.  Raises ValueError for an image with tokens
    and no valid key (the reference's softmax over an empty key set is NaN) and for more tokens than the select kernel sorts."""
    import numpy as np
    B = len(n_rows)
    T_max = max((int(n) for n in n_rows), default=0)
    if T_max > ROUTER_MAX_T:
        raise ValueError(f"attention router: {T_max} local tokens in one image, the selection sorts at most {ROUTER_MAX_T}")
    tok, keys, n_keys = [], [], []
    for b in range(B):
        n = int(n_rows[b])
        valid = np.arange(L, dtype=np.int64) if mask_host is None else np.nonzero(mask_host[b])[0].astype(np.int64)
        n_keys.append(int(valid.size))
        if n == 0:
            continue
        if valid.size == 0:
            raise ValueError(f"attention router: image {b} has {n} local tokens and no valid text key (attention mask all zero)")
        tok.append(np.arange(int(row_off[b]), int(row_off[b]) + n, dtype=np.int64))
        keys.append(b * L + valid)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros((0,), dtype=np.int64)
    return cat(tok), cat(keys), n_keys


def router_attention_scores(pra: PackedRouterAttention, tokens: torch.Tensor, row_off: Sequence[int], n_rows: Sequence[int],
                            text: torch.Tensor, mask: Optional[torch.Tensor], temp: float) -> torch.Tensor:
    """Attention-router scores for the B images of a step: fp32 [B, T_max], row b = softmax(logit / temp) over its n_rows[b] local
    tokens (the rest of the row is unspecified) -- what ``TextGuidedRouterAttention.forward`` returns.  ``tokens`` fp32 [rows, H];
    image b owns rows ``row_off[b] .. row_off[b] + n_rows[b] - 1``; ``text`` [B, L, H]; ``mask`` [B, L] or None (every key valid).
    The valid-key lists are built on the HOST from the mask: a mask that lives on the device costs one [B, L] D2H copy (the fused
    path's ``_pure_text_planned`` hands its host mask's device copy; pass a CPU mask to avoid the copy).  No other sync."""
    assert tokens.dim() == 2 and tokens.dtype == torch.float32 and tokens.is_contiguous()
    B, H = len(n_rows), tokens.shape[1]
    assert text.dim() == 3 and text.shape[0] == B and text.shape[2] == H == pra.H, "text is [B, L, H] of the router's width"
    L = text.shape[1]
    mask_host = None if mask is None else mask.detach().ne(0).cpu().numpy()
    tok_idx, key_idx, n_keys = _router_attention_plan(row_off, n_rows, L, mask_host)
    lib = _lib.load()
    _require_cuda(tokens, "tokens")
    dev = tokens.device
    T_max = max(1, max((int(n) for n in n_rows), default=0))
    scores = torch.empty((B, T_max), dtype=torch.float32, device=dev)
    if tok_idx.size == 0:
        return scores
    txt = text.to(device=dev, dtype=torch.float32).contiguous()
    idx = torch.cat([torch.from_numpy(tok_idx), torch.from_numpy(key_idx)]).to(dev, non_blocking=True)   # one upload
    sum_T, sum_L = int(tok_idx.size), int(key_idx.size)
    need = lib.slime_router_attn_workspace_bytes(C.byref(pra.desc), sum_T, sum_L)
    base, avail = pra.ws.aligned(need, dev)
    nr = (C.c_int * B)(*[int(n) for n in n_rows])
    nk = (C.c_int * B)(*n_keys)
    _lib.check(lib.slime_router_attn_scores(C.byref(pra.desc), tokens.data_ptr(), tokens.shape[0], idx.data_ptr(), nr, txt.data_ptr(),
                                            B * L, idx.data_ptr() + 8 * sum_T, nk, B, T_max, float(temp), scores.data_ptr(), base,
                                            avail, _stream()), "slime_router_attn_scores")
    return scores


def router_attention_select_batched_device(pra: PackedRouterAttention, tokens: torch.Tensor, row_off: Sequence[int],
                                           n_rows: Sequence[int], text: torch.Tensor, mask: Optional[torch.Tensor], topp: float,
                                           temp: float, want_scores: bool = False):
    """``router_select_batched_device`` with the attention router's scores: the same ``RouterState`` (kept indices on the device,
    counts on the host), so ``splice_routed`` and the callers of the cosine form take it unchanged.  The step's host syncs: the read
    of the B kept counts, and the [B, L] mask copy of ``router_attention_scores`` if the mask lives on the device."""
    B = len(n_rows)
    dev = tokens.device
    T_max = max((int(n) for n in n_rows), default=0)
    if B == 0 or T_max == 0:                                        # nothing to route: no launch, no sync
        st = RouterState(torch.zeros((B, 1), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev),
                         torch.tensor([int(o) for o in row_off], dtype=torch.int64).to(dev),
                         torch.zeros((B,), dtype=torch.int32, device=dev), [0] * B)
        return (st, None) if want_scores else st
    scores = router_attention_scores(pra, tokens, row_off, n_rows, text, mask, temp)
    lib = _lib.load()
    off = torch.tensor([int(o) for o in row_off], dtype=torch.int64).to(dev, non_blocking=True)
    cnt_in = torch.tensor([int(n) for n in n_rows], dtype=torch.int32).to(dev, non_blocking=True)
    keep = torch.empty((B, T_max), dtype=torch.int32, device=dev)
    cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(lib.slime_router_select_batched(scores.data_ptr(), cnt_in.data_ptr(), B, T_max, float(temp), float(topp),
                                               keep.data_ptr(), cnt.data_ptr(), _stream()), "slime_router_select_batched")
    st = RouterState(keep, cnt, off, cnt_in, cnt.cpu().tolist())     # the step's host sync
    return (st, scores) if want_scores else st


def ln_gather(src: torch.Tensor, idx: Optional[torch.Tensor], w: torch.Tensor, b: torch.Tensor, eps: float, out: torch.Tensor) -> torch.Tensor:
    """out[r] = T(LayerNorm(src[idx[r]])) (slime_ln_gather): src fp32 [rows_in, D], idx int64 [rows] or None (identity), out T
    [rows, D] written in place."""
    lib = _lib.load()
    _require_cuda(src, "src")
    assert src.dtype == torch.float32 and src.dim() == 2 and src.is_contiguous() and out.is_contiguous()
    assert idx is None or (idx.dtype == torch.int64 and idx.numel() == out.shape[0])
    _lib.check(lib.slime_ln_gather(src.data_ptr(), src.shape[0], _ptr(idx), out.shape[0], src.shape[1], _ptr(w), _ptr(b), float(eps),
                                   out.data_ptr(), dtype_code(out.dtype), _stream()), "slime_ln_gather")
    return out


def router_prob_head(h: torch.Tensor, w2: torch.Tensor, b2: float, n_rows: Optional[Sequence[int]], temp: float, logit: torch.Tensor,
                     scores: Optional[torch.Tensor]) -> None:
    """logit[r] = b2 + relu(h[r]) . w2 and, with ``scores`` [B, T_max], the per-image softmax(logit / temp) (slime_router_prob_head),
    both written in place."""
    lib = _lib.load()
    _require_cuda(h, "h")
    assert h.dtype == torch.float32 and h.dim() == 2 and h.is_contiguous()
    B = len(n_rows) if n_rows is not None else 0
    nr = (C.c_int * max(B, 1))(*[int(n) for n in (n_rows or [0])])
    _lib.check(lib.slime_router_prob_head(h.data_ptr(), h.shape[0], h.shape[1], _ptr(w2), float(b2), nr, B,
                                          scores.shape[1] if scores is not None else 0, float(temp), logit.data_ptr(), _ptr(scores),
                                          _stream()), "slime_router_prob_head")


# ------------------------------------------------------------------------------------------------
# after the visual tokens: splice + Llama prefill attention
# ------------------------------------------------------------------------------------------------

def splice_rows(table: Optional[torch.Tensor], feats: Optional[torch.Tensor], src: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """out[r] = table[src[r]] (src >= 0) | feats[-2 - src[r]] (src <= -2) | 0 (src == -1); src int64 [rows] on the device.
    One launch for the whole padded batch (llava_arch.py:343-459 builds it with per-sequence cat / split / stack)."""
    lib = _lib.load()
    _require_cuda(src, "src")
    H = (table if table is not None else feats).shape[-1]
    rows = src.numel()
    out = torch.empty((rows, H), dtype=out_dtype, device=src.device)
    t = None if table is None else table.contiguous()
    f = None if feats is None or feats.numel() == 0 else feats.contiguous()
    _lib.check(lib.slime_splice_rows(_ptr(t), dtype_code(t.dtype) if t is not None else 0, 0 if t is None else t.shape[0],
                                     _ptr(f), dtype_code(f.dtype) if f is not None else 0, 0 if f is None else f.shape[0],
                                     _ptr(src.contiguous()), out.data_ptr(), dtype_code(out_dtype), rows, H, _stream()),
               "slime_splice_rows")
    return out


def splice_routed(table: torch.Tensor, sep_id: int, tokens: torch.Tensor, P: int, router_state: RouterState, src: torch.Tensor,
                  mid_dtype: torch.dtype, out_dtype: torch.dtype) -> torch.Tensor:
    """``splice_rows`` without the per-image features: a ``src`` entry <= -2 names (image b, position p) of the feature
    ``[P global tokens | table[sep_id] | routed local tokens]`` (``-2 - (b << 32 | p)``, llava_arch.routed_src) and is resolved on the
    device from ``router_state`` and the fp32 token buffer ``tokens`` [rows, H]; feature rows take the value
    ``x.to(mid_dtype).to(out_dtype)``.  One launch; returns [src.numel(), H] of ``out_dtype``."""
    lib = _lib.load()
    _require_cuda(src, "src")
    _require_cuda(tokens, "tokens")
    assert tokens.dim() == 2 and tokens.dtype == torch.float32 and tokens.is_contiguous()
    assert table.device == tokens.device == src.device, "splice_routed: table, tokens and src live on one device"
    st = router_state
    B, T_max = st.keep.shape
    H = tokens.shape[1]
    assert table.shape[-1] == H, f"embedding rows of {table.shape[-1]}, token rows of {H}"
    rows = src.numel()
    out = torch.empty((rows, H), dtype=out_dtype, device=src.device)
    t = table.contiguous()
    _lib.check(lib.slime_splice_routed(_ptr(t), dtype_code(t.dtype), t.shape[0], int(sep_id), tokens.data_ptr(), tokens.shape[0],
                                       _ptr(st.off), _ptr(st.n_rows), B, int(P), T_max, _ptr(st.keep), _ptr(st.cnt),
                                       dtype_code(mid_dtype), _ptr(src.contiguous()), out.data_ptr(), dtype_code(out_dtype), rows, H,
                                       _stream()), "slime_splice_routed")
    return out


def splice_merged(table: torch.Tensor, tokens: Optional[torch.Tensor], extra: Optional[torch.Tensor], src: torch.Tensor,
                  mid_dtype: torch.dtype, out_dtype: torch.dtype) -> torch.Tensor:
    """``splice_rows`` without the merged per-image features of the un-sampled 'spatial' / 'spatial_unpad' branch: a ``src`` entry
    ``-2 - k`` names row k of the virtual concatenation ``[tokens | extra]`` -- ``tokens`` fp32 [crops * P, H], the projector's output,
    whose rows take the value ``x.to(mid_dtype).to(out_dtype)``; ``extra`` [n, H] (``image_newline[None]``), cast once or copied.
    One launch; returns [src.numel(), H] of ``out_dtype``."""
    lib = _lib.load()
    _require_cuda(src, "src")
    H = table.shape[-1]
    if tokens is not None and tokens.numel() == 0:
        tokens = None
    if extra is not None and extra.numel() == 0:
        extra = None
    if tokens is not None:
        _require_cuda(tokens, "tokens")
        assert tokens.dim() == 2 and tokens.dtype == torch.float32 and tokens.is_contiguous()
        assert table.device == tokens.device == src.device, "splice_merged: table, tokens and src live on one device"
        assert tokens.shape[1] == H, f"embedding rows of {H}, token rows of {tokens.shape[1]}"
    if extra is not None:
        _require_cuda(extra, "extra")
        assert extra.dim() == 2 and extra.shape[1] == H, f"embedding rows of {H}, extra rows of {tuple(extra.shape)}"
        assert extra.device == src.device, "splice_merged: extra and src live on one device"
        extra = extra.contiguous()
    assert table.device == src.device, "splice_merged: table and src live on one device"
    rows = src.numel()
    out = torch.empty((rows, H), dtype=out_dtype, device=src.device)
    t = table.contiguous()
    _lib.check(lib.slime_splice_merged(_ptr(t), dtype_code(t.dtype), t.shape[0], _ptr(tokens), 0 if tokens is None else tokens.shape[0],
                                       dtype_code(mid_dtype), _ptr(extra), dtype_code(extra.dtype) if extra is not None else 0,
                                       0 if extra is None else extra.shape[0], _ptr(src.contiguous()), out.data_ptr(),
                                       dtype_code(out_dtype), rows, H, _stream()), "slime_splice_merged")
    return out


@dataclass
class PackedLlamaAttention:
    hidden: int
    n_heads: int
    n_kv_heads: int
    head_dim: int
    dtype: torch.dtype
    tensors: Dict[str, torch.Tensor]
    desc: "_lib.LlamaAttnDesc"

    @property
    def ws(self) -> Workspace:
        """The layers of a language model run one after the other on one stream: they share ONE grow-only scratch buffer per
        (device, stream) (a Workspace per packed layer kept 32 x ~200 MB alive at the SliME-8B prefill shapes).  Keyed on the
        CURRENT stream: two models / requests prefilling on different streams (or devices) never write the same scratch, and a
        model split across GPUs keeps one buffer per device instead of re-allocating at every device switch."""
        return _llama_workspace()


# One grow-only Workspace per (device, stream) for the Llama attention sub-layer: ~200 MB at SliME-8B prefill shapes (8 x 1216 tokens).
# Bounded PER DEVICE: at most LLAMA_WS_MAX_STREAMS entries per device (SLIME_LLAMA_WS_MAX_STREAMS overrides the default of 4), the
# device's least recently used one evicted (a server that prefills on many torch streams would otherwise pin that much per stream
# handle forever -- the pool has ~32 handles per device; a model split across GPUs does not evict another device's buffers);
# ``release_llama_workspaces()`` drops all.  An evicted buffer goes back to the caching allocator.  It was allocated on the stream
# it served (the key's stream was current when Workspace.get grew it) and only ever used there, so the allocator's own
# allocation-stream ordering already keeps it from a new owner until that stream's queued work is done: no record_stream needed.
LLAMA_WS_MAX_STREAMS = max(1, int(os.environ.get("SLIME_LLAMA_WS_MAX_STREAMS", "4")))
_LLAMA_WS: "collections.OrderedDict[tuple, Workspace]" = collections.OrderedDict()
_LLAMA_WS_LOCK = threading.Lock()


def _llama_workspace() -> Workspace:
    st = torch.cuda.current_stream()
    key = (st.device.index, st.cuda_stream)
    with _LLAMA_WS_LOCK:
        ws = _LLAMA_WS.get(key)
        if ws is None:
            ws = _LLAMA_WS[key] = Workspace()
        _LLAMA_WS.move_to_end(key)
        mine = [k for k in _LLAMA_WS if k[0] == key[0]]            # this device's entries, least recently used first
        for k in mine[: max(0, len(mine) - LLAMA_WS_MAX_STREAMS)]:
            del _LLAMA_WS[k]
        return ws


def release_llama_workspaces() -> int:
    """Drop every cached Llama-attention workspace (returns the number of bytes released to the caching allocator)."""
    with _LLAMA_WS_LOCK:
        n = sum(w.buf.numel() for w in _LLAMA_WS.values() if w.buf is not None)
        _LLAMA_WS.clear()
    return n


def llama_inv_freq(head_dim: int, theta: float) -> torch.Tensor:
    """fp32 inverse frequencies exactly as LlamaRotaryEmbedding computes them (default rope type)."""
    return 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))


def pack_llama_attention(wq, wk, wv, wo, n_heads: int, n_kv_heads: int, dtype: torch.dtype, device,
                         rope_theta: float = 500000.0) -> PackedLlamaAttention:
    """q_proj / k_proj / v_proj / o_proj weights (nn.Linear layout, no biases) -> one fused [q|k|v] operand + o."""
    D = wq.shape[1]
    dh = wq.shape[0] // n_heads
    if dh != 128 or wk.shape[0] != n_kv_heads * dh or wv.shape[0] != n_kv_heads * dh or tuple(wo.shape) != (D, n_heads * dh):
        raise ValueError("pack_llama_attention: head_dim must be 128 and the projection shapes consistent")

    def tt(t):
        return t.detach().to(device=device, dtype=torch.float32).to(dtype).contiguous()

    T = {"w_qkv": tt(torch.cat([wq.detach().float().cpu(), wk.detach().float().cpu(), wv.detach().float().cpu()], 0)),
         "w_o": tt(wo), "inv_freq": llama_inv_freq(dh, rope_theta).to(device)}
    pack_static(T, ("w_qkv", "w_o"))
    d = _lib.LlamaAttnDesc()
    d.hidden, d.n_heads, d.n_kv_heads, d.head_dim, d.dtype = D, n_heads, n_kv_heads, dh, dtype_code(dtype)
    for k, v in T.items():
        setattr(d, k, None if v is None else v.data_ptr())
    return PackedLlamaAttention(D, n_heads, n_kv_heads, dh, dtype, T, d)


_RANGE_CACHE: Dict[str, object] = {}
_RANGE_LOCK = threading.Lock()


def token_ranges(attention_mask: Optional[torch.Tensor]):
    """Key-padding mask [B, S] -> (start, length) int32 [B] of the token run of every sequence.  Prefill masks are
    contiguous runs (right or left padding, llava_arch.py:435-455); anything else is rejected.  Host-side check: one D2H --
    per MASK TENSOR, not per layer: the 32 layers of a forward pass the same tensor object, so the last result is kept together
    with a reference to that object and reused while the caller hands in the very same object, unmodified (``is`` + the in-place
    version counter; a data pointer would not do -- the caching allocator recycles addresses)."""
    if attention_mask is None:
        return None, None
    with _RANGE_LOCK:                                    # one consistent (mask, version, start, length) record per look-up
        ref = _RANGE_CACHE.get("mask")
        if ref is not None and ref() is attention_mask and _RANGE_CACHE.get("version") == attention_mask._version:
            return _RANGE_CACHE["start"], _RANGE_CACHE["length"]
    start, length = _token_ranges(attention_mask)
    with _RANGE_LOCK:                                    # weak reference: the cache does not keep the last mask alive
        _RANGE_CACHE.update(mask=weakref.ref(attention_mask), version=attention_mask._version, start=start, length=length)
    return start, length


def _token_ranges(attention_mask: torch.Tensor):
    m = attention_mask.ne(0)
    length = m.sum(1)
    start = torch.where(length > 0, m.to(torch.int8).argmax(1), torch.zeros_like(length))
    S = m.shape[1]
    idx = torch.arange(S, device=m.device)[None]
    run = (idx >= start[:, None]) & (idx < (start + length)[:, None])
    if not bool(torch.equal(run, m)):
        raise ValueError("attention_mask must mark one contiguous run of tokens per sequence (left or right padding)")
    return start.to(torch.int32).contiguous(), length.to(torch.int32).contiguous()


def _position_ids(position_ids: Optional[torch.Tensor], B: int, S: int, device) -> torch.Tensor:
    """int32 [B, S] on the device.  HF passes position_ids of shape [1, S] (LlamaModel builds them from cache_position when
    the caller gives None, and prepare_inputs_labels_for_multimodal returns None in that case) and lets cos[position_ids]
    broadcast over the batch; the kernels index one entry per row, so the broadcast is materialised here."""
    if position_ids is None:
        position_ids = torch.arange(S, device=device)[None]
    if position_ids.dim() == 1:
        position_ids = position_ids[None]
    if position_ids.dim() != 2 or position_ids.shape[1] != S or position_ids.shape[0] not in (1, B):
        raise ValueError(f"position_ids of shape {tuple(position_ids.shape)} do not broadcast to ({B}, {S})")
    pos = position_ids.to(device=device, dtype=torch.int32).expand(B, S).contiguous()
    assert pos.shape == (B, S)
    return pos


def _llama_attention(pa: PackedLlamaAttention, hidden: torch.Tensor, position_ids, attention_mask, out_dtype, resid, out,
                     window: Optional[int]) -> torch.Tensor:
    """The one host sequence behind ``llama_attention_forward`` / ``_resid`` / ``_window``: operands, position ids, token ranges,
    output and workspace, then ONE C-ABI call -- ``window`` None: slime_llama_attn_forward or, with ``resid``, _forward_resid (the
    launches those two functions always made); an int: slime_llama_attn_forward_window."""
    lib = _lib.load()
    _require_cuda(hidden, "hidden")
    B, S, D = hidden.shape
    assert D == pa.hidden
    if resid is not None:
        assert hidden.dtype == pa.dtype and resid.dtype == pa.dtype and tuple(resid.shape) == (B, S, D) and out_dtype in (None, pa.dtype)
        x, r = hidden.contiguous(), resid.contiguous()
        out_dtype = kernel_out = pa.dtype
    else:
        x, r = hidden.to(pa.dtype).contiguous(), None
        out_dtype = out_dtype or hidden.dtype
        kernel_out = torch.float32 if out_dtype == torch.float32 else pa.dtype
    pos = _position_ids(position_ids, B, S, x.device)
    start, length = token_ranges(None if attention_mask is None else attention_mask.to(x.device))
    if out is None:
        out = torch.empty((B, S, D), dtype=kernel_out, device=x.device)
    assert out.is_contiguous() and out.dtype == kernel_out and tuple(out.shape) == (B, S, D) and out.data_ptr() != x.data_ptr()
    need = lib.slime_llama_attn_workspace_bytes(C.byref(pa.desc), B, S)
    base, avail = pa.ws.aligned(need, x.device)
    head = (C.byref(pa.desc), x.data_ptr(), pos.data_ptr(), _ptr(start), _ptr(length), B, S)
    if window is not None:
        _lib.check(lib.slime_llama_attn_forward_window(*head, None if r is None else r.data_ptr(), out.data_ptr(), dtype_code(kernel_out),
                                                       int(window), base, avail, _stream()), "slime_llama_attn_forward_window")
    elif r is not None:
        _lib.check(lib.slime_llama_attn_forward_resid(*head, r.data_ptr(), out.data_ptr(), base, avail, _stream()),
                   "slime_llama_attn_forward_resid")
    else:
        _lib.check(lib.slime_llama_attn_forward(*head, out.data_ptr(), dtype_code(kernel_out), base, avail, _stream()),
                   "slime_llama_attn_forward")
    return out if out.dtype == out_dtype else out.to(out_dtype)


def llama_attention_forward_resid(pa: PackedLlamaAttention, hidden: torch.Tensor, resid: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
                                  attention_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The attention sub-layer with the decoder layer's residual add in o_proj's epilogue (slime_llama_attn_forward_resid):
    out = T(resid + self_attn(hidden)), all T [B, S, D].  ``out`` may be ``resid`` itself (in-place stream); ``hidden`` may be
    ``resid`` (no norm in between) but not ``out``."""
    return _llama_attention(pa, hidden, position_ids, attention_mask, None, resid, out, None)


def llama_attention_forward(pa: PackedLlamaAttention, hidden: torch.Tensor, position_ids: Optional[torch.Tensor] = None,
                            attention_mask: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """hidden [B, S, D] -> [B, S, D]: q/k/v projection, RoPE, causal GQA attention over the un-padded tokens, o_proj."""
    return _llama_attention(pa, hidden, position_ids, attention_mask, out_dtype, None, None, None)


def llama_attention_forward_window(pa: PackedLlamaAttention, hidden: torch.Tensor, position_ids: Optional[torch.Tensor],
                                   attention_mask: Optional[torch.Tensor], out_dtype: Optional[torch.dtype], window: int,
                                   resid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The attention sub-layer with a sliding window (slime_llama_attn_forward_window; MistralAttention / MixtralAttention):
    query row i sees key row j iff j <= i, i - j < window and both lie in the sequence's token run; ``window`` 0 (or >= S) is
    ``llama_attention_forward`` / ``_resid`` bit for bit, a negative one is refused by the library.  ``resid`` given:
    out = T(resid + self_attn(hidden)) (``out`` may be ``resid``); else [B, S, D] of ``out_dtype`` (default: hidden's)."""
    return _llama_attention(pa, hidden, position_ids, attention_mask, out_dtype, resid, out, int(window))


def prefill_attention_window(qkv: torch.Tensor, n_heads: int, n_kv_heads: int, window: int,
                             attention_mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sliding-window causal GQA attention (slime_prefill_attention_window) on a packed [B, S, (n_heads + 2 n_kv_heads) * 128]
    buffer of q | k | v heads -- q pre-scaled by 128^-0.5 log2 e, RoPE applied, as ``slime_rope`` leaves it -> [B, S, n_heads * 128].
    ``window`` as in ``llama_attention_forward_window``."""
    lib = _lib.load()
    _require_cuda(qkv, "qkv")
    B, S, N = qkv.shape
    assert qkv.is_contiguous() and qkv.dtype in (torch.bfloat16, torch.float16) and N == (n_heads + 2 * n_kv_heads) * 128
    start, length = token_ranges(None if attention_mask is None else attention_mask.to(qkv.device))
    if out is None:
        out = torch.empty((B, S, n_heads * 128), dtype=qkv.dtype, device=qkv.device)
    assert out.is_contiguous() and out.dtype == qkv.dtype and tuple(out.shape) == (B, S, n_heads * 128)
    p = qkv.data_ptr()
    _lib.check(lib.slime_prefill_attention_window(p, S * N, N, p + n_heads * 256, S * N, N, p + (n_heads + n_kv_heads) * 256, S * N, N,
                                                  out.data_ptr(), S * n_heads * 128, n_heads * 128, B, n_heads, n_kv_heads, 128, S,
                                                  _ptr(start), _ptr(length), dtype_code(qkv.dtype), int(window), _stream()),
               "slime_prefill_attention_window")
    return out
