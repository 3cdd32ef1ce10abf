"""Head-sharded Llama attention conformance: the rank slices of ``slime_amd.dist.shard_llama_attention_weights``, the fp32 and 16-bit
partial sums of the row-parallel o_proj and their reduction -- the cases, the float64 references, the DERIVED element-wise bounds, a
torch restatement of one sharded layer (``emulate``) and its deliberately wrong variants (``MUTANTS``).  Plain module (no fixtures,
not a conftest); pure torch, works on CPU and GPU tensors, importable without a GPU and without the HIP library.  Used by
test_head_shard_bound_cpu.py, test_gpu_head_shard.py and head_shard_gpu_worker.py.

A rank's call is ``slime_llama_attn_forward`` / ``_resid`` on a descriptor with n_heads * 128 < hidden (csrc/prefill.hip:
llama_attn_run): a q/k/v GEMM with N = (hq_r + 2 hkv_r) 128, RoPE and causal GQA attention on the rank's heads, an o_proj with
K = hq_r 128 whose result [rows, hidden] is one term of a sum over the ranks.  ``GEOMS`` holds (hidden, HQ, HKV, world); a rank's slice
(hq_r, hkv_r) = (HQ / world, HKV / world) follows.  Weights are seeded N(0, k^-1/2) in fp32 (``layer_weights``), sliced in fp32 by
``shard_llama_attention_weights`` and rounded to T by the pack, once.

What is bit-exact (no bound):
 (a) the fused entry on a slice equals ``tower_conformance.replay_llama_attn`` with the slice's (hidden, hq_r, hkv_r);
 (b) rank r's packed q / k / v rows after RoPE are the column blocks ``column_blocks`` names of the full layer's rows, and its context
     rows are columns [r hq_r 128, (r + 1) hq_r 128) of the full layer's: a GEMM element depends on its A row, its B row and K alone
     and all kernels share one k order; RoPE is element-wise; an attention (sequence, head) item is independent of the others;
     sharding by kv heads preserves the GQA group, hence the kernel;
 (c) the 16-bit terms handed to the all-reduce are the roundings of the fp32 partials: t_0 = T(fp32(p_0 + resid)), t_r = T(p_r).

The bounds (e = 2^-24; u = unit roundoff of T, 2^-8 bf16 / 2^-11 fp16; g = T's subnormal half-spacing, gemm_conformance.SUBNORMAL)
--------------------------------------------------------------------------------------------------------------------------------
 (1) fp32 partials against the full layer's fp32 o_proj (``partial_sum_bound``).  p_r = the rank's fp32 o_proj, summed over r in
     float64 by the test; P = the full layer's fp32 o_proj; S = sum_k |ctx_k w_k| in float64 from the DEVICE's context rows and the
     T-rounded W_o.  By (b) both multiply the same context bits, so each lies within gemm_conformance's term (1) of the same exact
     product: sum_r e (K_r + 4) S_r = e (K_r + 4) S for the partials (all K_r are equal and sum_r S_r = S) and e (K + 4) S for the
     full layer:                                        |sum_r p_r - P| <= e (K_r + 4) S + e (K + 4) S
 (2) the reduction in T (``reduce_bound``).  sigma = sum_r t_r in float64.  Any association of world - 1 additions in T: addition i
     rounds its exact result s_i by at most u |s_i| + g, and |s_i| <= (1 + u)^(i - 1) A with A = sum_r |t_r| (every earlier rounding
     inflates a partial sum by at most 1 + u), so the total is A ((1 + u)^(world - 1) - 1) + (world - 1) g.  For world <= 8 and
     u <= 2^-8: (1 + u)^7 - 1 = 7 u (1 + 3 u + 5 u^2 + ..) < 7 u (1 + 2^-6 * 0.76); what is left of the factor covers an addition
     carried out in fp32 and rounded to T a second time (2^-16 relative):
                                                        |result - sigma| <= (world - 1) u A (1 + 2^-6) + (world - 1) g
 (3) the whole layer, element by element (``layer_bound``; the CPU test's handle on the two residual mutants, which (2) cannot see
     because it compares a sum with its own terms): the reduced result against resid + ctx W_o^T in float64 is (2), plus one rounding
     to T per term, |t_r - f_r| <= u |t_r| / (1 - u) + g, plus term (1) of every rank's fp32 value with the residual in rank 0's
     weight: e (K_r + 4) (S + |resid|).
 (4) one rel-L2 per geometry and dtype against the oracle on the FULL layer at the project's per-stage tolerance (``TOL``, the values
     of tests/test_gpu_path.py): the only number here that is not derived element by element; it is there because (a) - (c), (1) and
     (2) would all pass if the slices and the replay misread the layer in the same way.
None of these constants was fitted to a kernel's output; test_head_shard_bound_cpu.py checks that ``emulate`` stays inside every
bound and that every mutant leaves one by more than ``MARGIN``.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import tower_conformance as TC
from gemm_conformance import E32, EPI_BIAS_T, SUBNORMAL, UNIT

DH = 128
DTYPES = TC.DTYPES
DT_ID = TC.DT_ID
TOL = {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}          # tests/test_gpu_path.py TOL: the project's per-stage tolerance
MARGIN = 16.0                                                # "leaves the bound by a wide margin": worst |err| / bound above this

# (hidden, HQ, HKV, world): the smallest at which each kernel branch and each slice shape exists
#   (512, 4, 4, 2)   slice (2, 2): N_qkv 768, K of o_proj 256, GQA group 1
#   (512, 4, 4, 4)   slice (1, 1): N_qkv 384 -- no multiple of 256, so no direct-B kernel -- and one k-tile pair in o_proj (K 128)
#   (512, 4, 2, 2)   slice (2, 1): N_qkv 512, K 256, group 2
#   (1024, 8, 2, 2)  slice (4, 1): N_qkv 768, K 512, group 4: bf16 takes prefill32_kernel, fp16 the eight-wave kernel
#   (4096, 32, 8, 8) slice (4, 1): the Llama-3-8B slice on 8 ranks; bf16 at REAL_SHAPE only
GEOMS = ((512, 4, 4, 2), (512, 4, 4, 4), (512, 4, 2, 2), (1024, 8, 2, 2), (4096, 32, 8, 8))
SMALL_GEOMS = GEOMS[:4]
REAL_GEOM = GEOMS[4]
SHAPES = ((1, 1), (3, 5), (2, 65), (1, 193))                 # (batch, S): test_gpu_tower_conformance.LLAMA_SHAPES
REAL_SHAPE = (1, 65)
FORM_SHAPES = ((3, 5), (2, 65))                              # where the three weight forms are walked (the fragment form elsewhere)
ORACLE_SHAPE = (2, 65)                                       # bound (4): right padded
PADS = ("none", "right", "left")


def geom_id(geom) -> str:
    return "h%d-q%d-kv%d-w%d" % tuple(geom)


def geom_dtypes(geom):
    return (torch.bfloat16,) if tuple(geom) == REAL_GEOM else DTYPES


def geom_shapes(geom):
    return (REAL_SHAPE,) if tuple(geom) == REAL_GEOM else SHAPES


def geom_params(geoms=GEOMS):
    """[(geometry, dtype)] and their ids, for pytest.mark.parametrize."""
    params = [(g, dt) for g in geoms for dt in geom_dtypes(g)]
    return params, [f"{geom_id(g)}-{DT_ID[dt]}" for g, dt in params]


def slice_heads(geom) -> Tuple[int, int]:
    hidden, hq, hkv, world = geom
    return hq // world, hkv // world


def slice_workspace_bytes(rows: int, hq_r: int, hkv_r: int) -> int:
    """What slime_llama_attn_workspace_bytes must hold on a slice: the packed q/k/v rows and the context rows, 16-bit."""
    return rows * (hq_r + 2 * hkv_r) * 2 * DH + rows * hq_r * 2 * DH


@functools.lru_cache(maxsize=None)
def layer_weights(hidden: int, hq: int, hkv: int, seed: int = 7):
    """(wq, wk, wv, wo) of the FULL layer in fp32, N(0, k^-1/2); the slices are taken from these, never generated per rank."""
    g = torch.Generator().manual_seed(seed + hidden + 31 * hq + 977 * hkv)
    return tuple(torch.randn(n, k, generator=g) * k ** -0.5 for n, k in ((hq * DH, hidden), (hkv * DH, hidden), (hkv * DH, hidden), (hidden, hq * DH)))


def rank_slices(w, hq: int, hkv: int, world: int):
    """shard_llama_attention_weights of every rank: [(wq_r, wk_r, wv_r, wo_r, hq_r, hkv_r)]."""
    from slime_amd.dist import shard_llama_attention_weights
    return [shard_llama_attention_weights(w[0], w[1], w[2], w[3], hq, hkv, world, r) for r in range(world)]


def layer_inputs(hidden: int, batch: int, S: int, dtype, seed: int = 3):
    """(x T [batch S, hidden], resid T, pos int32 [batch S] with a per-sequence offset): test_gpu_tower_conformance._llama_inputs on the CPU."""
    g = torch.Generator().manual_seed(seed + 17 * S + batch)
    x = torch.randn(batch * S, hidden, generator=g).to(dtype)
    r = torch.randn(batch * S, hidden, generator=g).to(dtype)
    pos = (torch.arange(S)[None] + 7 * torch.arange(batch)[:, None]).reshape(-1).to(torch.int32)
    return x, r, pos


def kv_ranges(pad: str, batch: int, S: int):
    """kv_start / kv_len int32 [batch] (None: absent): sequence b holds max(1, S - 2 b - 1) tokens at the front or at the back
    (test_gpu_tower_conformance._ranges on the CPU)."""
    if pad == "none":
        return None, None
    ln = [max(1, S - 2 * b - 1) for b in range(batch)]
    st = [0 if pad == "right" else S - x for x in ln]
    return torch.tensor(st, dtype=torch.int32), torch.tensor(ln, dtype=torch.int32)


def range_mask(kv_start, kv_len, batch: int, S: int) -> Optional[torch.Tensor]:
    """The key-padding mask [batch, S] (int64) of a pair of ranges, for the oracle and for ops.llama_attention_forward*."""
    if kv_start is None:
        return None
    idx = torch.arange(S)[None]
    st, ln = kv_start.cpu().long()[:, None], kv_len.cpu().long()[:, None]
    return ((idx >= st) & (idx < st + ln)).long()


def column_blocks(hq: int, hkv: int, world: int, rank: int) -> Dict[str, Tuple[int, int]]:
    """Where rank ``rank``'s columns stand in the FULL layer's rows: its q, k and v blocks in a packed [q | k | v] row of
    (hq + 2 hkv) 128 columns, and its block of a context row of hq 128 columns.  From the definition of the shard (kv heads in
    contiguous blocks, each with its hq / hkv query heads), not from shard_llama_attention_weights."""
    hq_r, hkv_r = hq // world, hkv // world
    q0, k0, v0 = rank * hq_r * DH, (hq + rank * hkv_r) * DH, (hq + hkv + rank * hkv_r) * DH
    return {"q": (q0, q0 + hq_r * DH), "k": (k0, k0 + hkv_r * DH), "v": (v0, v0 + hkv_r * DH), "ctx": (q0, q0 + hq_r * DH)}


def rows_of_rank(qkv_full: torch.Tensor, hq: int, hkv: int, world: int, rank: int) -> torch.Tensor:
    """The [rows, (hq_r + 2 hkv_r) 128] packed rows rank ``rank`` must hold, cut from the full layer's."""
    b = column_blocks(hq, hkv, world, rank)
    return torch.cat([qkv_full[:, b[k][0]:b[k][1]] for k in "qkv"], dim=1)


class Recorder:
    """A backend of tower_conformance.replay_llama_attn that also keeps the packed q/k/v rows as RoPE left them (``qkv``) and the
    context rows (``ctx``); everything else is the wrapped backend's."""

    def __init__(self, be):
        self._be, self.qkv, self.ctx = be, None, None

    def __getattr__(self, name):
        return getattr(self._be, name)

    def rope(self, qkv, *a, **kw):
        self._be.rope(qkv, *a, **kw)
        self.qkv = qkv.clone()

    def prefill_attention(self, *a, **kw):
        self.ctx = self._be.prefill_attention(*a, **kw)
        return self.ctx


# ------------------------------------------------------------------------------------------------ bounds
def abs_products(ctx: torch.Tensor, wo_t: torch.Tensor) -> torch.Tensor:
    """S = sum_k |ctx_k w_k| per element in float64: ctx the context rows as they are (T), wo_t the T-rounded W_o [hidden, K]."""
    return ctx.double().abs() @ wo_t.double().abs().t()


def gemm_term1(S: torch.Tensor, K: int) -> torch.Tensor:
    """gemm_conformance's term (1): e (K + 4) S."""
    return E32 * (K + 4) * S


def partial_sum_bound(S: torch.Tensor, K_r: int, K: int) -> torch.Tensor:
    """Bound (1) of |sum_r p_r - P|."""
    return gemm_term1(S, K_r) + gemm_term1(S, K)


def reduce_bound(terms: Sequence[torch.Tensor], dtype) -> torch.Tensor:
    """Bound (2) of |any association of the terms summed in T - their float64 sum|."""
    world = len(terms)
    A = sum(t.double().abs() for t in terms)
    return (world - 1) * UNIT[dtype] * A * (1 + 2.0 ** -6) + (world - 1) * SUBNORMAL[dtype]


def layer_bound(terms: Sequence[torch.Tensor], S: torch.Tensor, K_r: int, resid: torch.Tensor, dtype) -> torch.Tensor:
    """Bound (3) of |reduced result - (resid + ctx W_o^T in float64)|."""
    u, g = UNIT[dtype], SUBNORMAL[dtype]
    rounding = sum(u * t.double().abs() / (1 - u) + g for t in terms)
    return reduce_bound(terms, dtype) + rounding + gemm_term1(S + resid.double().abs(), K_r)


def reduce_orders(world: int, seed: int = 5) -> List[Tuple[int, ...]]:
    """Every order for world <= 4; 0..7, 7..0 and one seeded shuffle for more."""
    if world <= 4:
        return list(itertools.permutations(range(world)))
    g = torch.Generator().manual_seed(seed)
    return [tuple(range(world)), tuple(reversed(range(world))), tuple(torch.randperm(world, generator=g).tolist())]


def reduce_in_T(terms: Sequence[torch.Tensor], order: Sequence[int]) -> torch.Tensor:
    """The terms (all T) added one after the other in ``order``, every addition in T."""
    acc = terms[order[0]]
    for r in order[1:]:
        acc = acc + terms[r]
    assert acc.dtype == terms[0].dtype
    return acc


def float64_sum(terms: Sequence[torch.Tensor]) -> torch.Tensor:
    return sum(t.double() for t in terms)


def worst_ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max |err| / bound over the elements (0 / 0 counts as 0, anything non-finite as inf)."""
    err, bound = err.double().abs(), bound.double()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def check_terms_are_roundings(terms, partials, resid, dtype) -> List[str]:
    """(c): t_0 == T(fp32(p_0 + resid)) and t_r == T(p_r) bit for bit; returns what differs."""
    bad = []
    for r, (t, p) in enumerate(zip(terms, partials)):
        want = (p + resid.float()).to(dtype) if r == 0 else p.to(dtype)
        if not bool(torch.equal(t.view(torch.int16), want.view(torch.int16))):
            bad.append(f"rank {r}: {int((t.view(torch.int16) != want.view(torch.int16)).sum())} elements differ from the rounding of the fp32 partial")
    return bad


def check_reduce(terms, dtype, seed: int = 5) -> float:
    """Worst |reduce_in_T - float64 sum| / bound (2) over the orders of ``reduce_orders``."""
    sigma, bd = float64_sum(terms), reduce_bound(terms, dtype)
    return max(worst_ratio(reduce_in_T(terms, o).double() - sigma, bd) for o in reduce_orders(len(terms), seed))


def oracle_layer(w, hq: int, hkv: int, x, resid, pos, kv_start, kv_len, batch: int, S: int) -> torch.Tensor:
    """resid + oracle.prefill_oracle.llama_attention_forward of the FULL layer in float64 (unrounded fp32 weights, the T input as it
    is) -> [batch S, hidden]."""
    from oracle import prefill_oracle as P
    hidden = x.shape[-1]
    y = P.llama_attention_forward(x.cpu().double().view(batch, S, hidden), *(t.double() for t in w), hq, hkv,
                                  pos.cpu().view(batch, S).long(), range_mask(kv_start, kv_len, batch, S), head_dim=DH)
    return resid.cpu().double().view(batch * S, hidden) + y.reshape(batch * S, hidden)


# ------------------------------------------------------------------------------------------------ the emulation and its mutants
MUTANTS = ("resid_on_every_rank", "resid_dropped", "wo_rows_for_columns", "kv_block_plus_1_head", "query_heads_round_robin",
           "kv_columns_swapped")
SLICE_MUTANTS = MUTANTS[2:]                                  # wrong slices: they leave bound (1); the first two leave bound (3)


def mutant_applies(mutant: str, hq: int, hkv: int, world: int) -> bool:
    """Whether a wrong variant can change anything, from the geometry alone.
    query_heads_round_robin : r::world is the contiguous block when a rank owns one query head.
    kv_block_plus_1_head    : needs a second kv head to move to.
    wo_rows_for_columns     : needs hidden == hq 128, which every full layer here has."""
    if mutant == "query_heads_round_robin":
        return hq // world > 1
    if mutant == "kv_block_plus_1_head":
        return hkv > 1
    return True


def honest_heads(hq: int, hkv: int, world: int, rank: int):
    """(query heads, kv heads) of a rank as global head numbers, read off shard_llama_attention_weights itself (applied to matrices
    whose rows hold their own row number), so that the emulation slices as the product does."""
    from slime_amd.dist import shard_llama_attention_weights
    rq, rk = torch.arange(hq * DH)[:, None].float(), torch.arange(hkv * DH)[:, None].float()
    wo = torch.arange(hq * DH)[None, :].float()
    q, k, v, o, hq_r, hkv_r = shard_llama_attention_weights(rq, rk, rk, wo, hq, hkv, world, rank)
    qh, kh = (q[::DH, 0] / DH).long().tolist(), (k[::DH, 0] / DH).long().tolist()
    assert torch.equal(k, v) and torch.equal(o[0], q[:, 0]) and len(qh) == hq_r and len(kh) == hkv_r
    assert torch.equal(q[:, 0], torch.cat([torch.arange(h * DH, (h + 1) * DH) for h in qh]).float())
    return qh, kh


@dataclass
class Emulated:
    terms: List[torch.Tensor]             # T [rows, hidden] per rank: what the all-reduce is handed
    partials: List[torch.Tensor]          # fp32 [rows, hidden] per rank: o_proj over the rank's heads
    full: torch.Tensor                    # fp32 [rows, hidden]: the full layer's o_proj
    S: torch.Tensor                       # float64: sum_k |ctx_k w_k| of the full layer
    ctx_full: torch.Tensor                # T [rows, hq 128]
    ctx: List[torch.Tensor]               # T [rows, hq_r 128] per rank
    resid: torch.Tensor


def emulate(geom, dtype, x, resid, pos, kv_start, kv_len, batch: int, S: int, mutant: Optional[str] = None) -> Emulated:
    """One head-sharded layer in torch.  The q/k/v GEMM and RoPE of the full layer are tower_conformance.TorchBackend(T) (float64,
    rounded where the kernels round); attention is that backend's causal GQA on one (query head, kv head) pair at a time, so that a
    rank's context columns are the full layer's by construction (statement (b) of the header); o_proj is a matmul in fp32 (torch's
    order, any order is inside term (1)), the residual is added in fp32 and the terms are rounded to T.  ``mutant`` changes what a
    rank takes from the layer."""
    hidden, hq, hkv, world = geom
    grp = hq // hkv
    w = layer_weights(hidden, hq, hkv)
    from slime_amd import ops
    be = TC.TorchBackend(dtype)
    T = {"w_qkv": torch.cat(w[:3]).to(dtype), "inv_freq": ops.llama_inv_freq(DH, 500000.0)}
    qkv = be.gemm(x, T, "w_qkv", None, EPI_BIAS_T)
    be.rope(qkv, pos, hq + hkv, hq, DH, T["inv_freq"], TC.llama_q_scale())
    wo_t = w[3].to(dtype)
    swap = mutant == "kv_columns_swapped"

    @functools.lru_cache(maxsize=None)
    def pair(qh: int, kh: int, swapped: bool) -> torch.Tensor:
        col = lambda c: qkv[:, c * DH:(c + 1) * DH]
        k, v = col(hq + kh), col(hq + hkv + kh)
        three = torch.cat([col(qh), v, k] if swapped else [col(qh), k, v], dim=1)
        return be.prefill_attention(three, 0, DH, 2 * DH, batch, S, 1, 1, DH, kv_start, kv_len).to(dtype)

    ctx_full = torch.cat([pair(h, h // grp, False) for h in range(hq)], dim=1)
    full = ctx_full.float() @ wo_t.float().t()
    ctxs, partials, terms = [], [], []
    for r in range(world):
        qh, kh = honest_heads(hq, hkv, world, r)
        if mutant == "kv_block_plus_1_head":
            kh = [(h + 1) % hkv for h in kh]
        if mutant == "query_heads_round_robin":
            qh = list(range(hq))[r::world]
        cols = torch.cat([torch.arange(h * DH, (h + 1) * DH) for h in qh])
        wo_r = wo_t[cols, :].t() if mutant == "wo_rows_for_columns" else wo_t[:, cols]
        ctx = torch.cat([pair(h, kh[j // grp], swap) for j, h in enumerate(qh)], dim=1)      # local head j reads local kv head j / grp
        p = ctx.float() @ wo_r.float().t()
        carries = (r == 0 or mutant == "resid_on_every_rank") and mutant != "resid_dropped"
        t = (p + resid.float()).to(dtype) if carries else p.to(dtype)
        ctxs.append(ctx), partials.append(p), terms.append(t)
    return Emulated(terms, partials, full, abs_products(ctx_full, wo_t), ctx_full, ctxs, resid)
