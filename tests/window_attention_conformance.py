"""Sliding-window prefill attention (``slime_prefill_attention_window``): the float64 reference with the window, a 16-bit
emulation of the kernel's arithmetic with the window mask and its deliberately wrong variants, and the case builder.  Plain
module (no fixtures, not a conftest); pure torch, CPU and GPU tensors.  Used by test_window_attention_cpu.py and
test_gpu_window_attention.py.

Semantics (include/slime_hip.h): query row i of a sequence sees key row j iff  j <= i,  i - j < W,  and both rows lie in the
sequence's token range [start, start + length).  Rows are indices into the [B, S] layout.

The bound is attention_conformance's, unchanged: it is derived per element from the arithmetic (P rounded to T, fp32
accumulation, one final rounding), and a window only removes terms from the sums it speaks about -- ``reference`` here computes
ref, A, e32 and under over the windowed key set with the same formulas.

Inputs.  attention_conformance.make_case("random") gives every key a weight of about 1 / (number of live keys): at W = 256 a key
wrongly admitted or dropped at the window's edge would move an element by less than the bf16 bound.  ``make_window_case``
therefore makes both edge keys heavy on chosen rows of every 16-row query block (``heavy_rows``): such a row's query is
aligned with key i - W (the first EXCLUDED key, logit +40 log2 units -- admitted, it takes the whole row) and with key
i - W + 1 (the last INCLUDED key, +20 -- it carries the row; dropped, the row falls back to the spread of the others).  Rows
are chosen off the tile's first row and off the 32-key grid where the block leaves the choice, so that an edge counted from the
tile or rounded to a step shows.  All other rows keep their random queries, so ordinary many-key rows stay covered.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

import attention_conformance as AC

POS_OFFSET = 5                      # the "position-id units" mutant: ids = row + 5
EXCLUDED_LOGIT, INCLUDED_LOGIT = 40.0, 20.0

# shapes walked on the GPU (test_gpu_window_attention.py); test_window_attention_cpu.py takes its cases from here
EIGHT_WAVE_S = (1, 31, 33, 200, 257, 449)           # straddling 32, QB = 256 / group and the 192-key chunk
EIGHT_WAVE_W = (1, 2, 31, 32, 33, 64, 191, 192, 193, 256)        # and S - 1
EIGHT_WAVE_GROUPS = {torch.bfloat16: (1, 2, 8, 16), torch.float16: (1, 2, 4, 8, 16)}     # bf16 group 4: the PREFILL32 list below
PREFILL32_S = (64, 65, 300, 600)
PREFILL32_W = (1, 17, 32, 33, 64, 65, 96, 97, 255, 256, 257, 300)
RANGE_KINDS = ("none", "left", "right", "ragged3")


def windows_for(S: int, table) -> List[int]:
    """The windows of ``table`` (and S - 1) that hide a key at length S -- 0 < W < S, the windowed kernel -- plus one W >= S (the
    smallest of the table, else S), which the dispatch hands to the unwindowed kernel."""
    w = sorted({x for x in tuple(table) + (S - 1,) if 0 < x < S})
    over = [x for x in table if x >= S]
    return w + [min(over) if over else S]


def ranges_for(kind: str, S: int):
    """(start list, length list) or None.  left / right: one sequence, padding off a 32-key step and off a 16-row block where S
    leaves room (attention_conformance.prefill_ranges' numbers); ragged3: a left-padded, a right-padded and a short sequence in
    the middle of the rows."""
    if kind == "none":
        return None
    st, ln = AC.prefill_ranges(S)                  # [left, 0, one, 0], [S - left, right, 1, S]
    if kind == "left":
        return [st[0]], [ln[0]]
    if kind == "right":
        return [0], [ln[1]]
    if kind == "ragged3":
        mid = S // 5
        return [st[0], 0, mid], [ln[0], ln[1], max(1, S - 2 * mid - 1)]
    raise ValueError(kind)


def _bounds(ranges, B: int, S: int):
    lo = [0] * B if ranges is None else [int(x) for x in ranges[0]]
    hi = [S] * B if ranges is None else [min(S, int(a) + int(b)) for a, b in zip(ranges[0], ranges[1])]
    return lo, hi


def heavy_rows(S: int, W: int, lo: int, hi: int) -> List[int]:
    """Per 16-row block the rows whose query is aligned with the window's edge keys: among the block's live rows that have an
    excluded key inside the token range (i - W >= lo) the first, the last, and the first one off the tile's first row and off
    the 32-key grid ((i - W + 1) % 32 != 0); in blocks without such a row, the last live row whose included edge key i - W + 1
    is not cut off by the range's start (one key fewer shows there), else the block's middle live row."""
    rows = []
    for blk in range((S + 15) // 16):
        live = [i for i in range(blk * 16, min(S, blk * 16 + 16)) if lo <= i < hi]
        cand = [i for i in live if i - W >= lo]
        if cand:
            pick = {cand[0], cand[-1]}
            off = [i for i in cand if i % 16 != 0 and (i - W + 1) % 32 != 0]
            if off:
                pick.add(off[0])
            rows += sorted(pick)
        elif live:
            edge = [i for i in live if i - W + 1 >= lo]          # rows whose last included key is not cut by the range's start
            rows.append(edge[-1] if edge else live[len(live) // 2])
    return rows


def make_window_case(dtype, *, B: int, H: int, HKV: int, S: int, W: int, ranges=None, guard="nan", gain=1.0, seed=0,
                     device="cpu") -> AC.Case:
    """attention_conformance.make_case("random", causal) with the edge keys of window W made heavy on ``heavy_rows`` (module
    docstring).  Built on the CPU, then moved."""
    c = AC.make_case("random", dtype, B=B, H=H, HKV=HKV, dh=128, n_q=S, n_kv=S, gain=gain, causal=True, ranges=ranges, guard=guard,
                     seed=seed, device="cpu")
    group = H // HKV
    lo, hi = _bounds(ranges, B, S)
    qv = c.view(c.qbuf, H)                          # [B, S + 3, H, dh] views of the padded buffers
    kv = c.view(c.kbuf, HKV)
    for b in range(B):
        for i in heavy_rows(S, W, lo[b], hi[b]):
            q = torch.zeros(H, 128)
            for j, logit in ((i - W, EXCLUDED_LOGIT), (max(lo[b], i - W + 1), INCLUDED_LOGIT)):
                if j >= lo[b]:
                    kk = kv[b, j].float().repeat_interleave(group, 0)              # [H, dh], the 16-bit key as stored
                    q = q + kk * (logit / (kk * kk).sum(-1, keepdim=True).clamp_min(1e-6))
            qv[b, i] = q.to(dtype)
    rg = None if c.ranges is None else (c.ranges[0].to(device), c.ranges[1].to(device))
    return AC.Case(dtype, B, H, HKV, 128, S, S, True, False, c.qbuf.to(device), c.kbuf.to(device), c.vbuf.to(device), rg)


# ------------------------------------------------------------------------------------------------ masks
def window_live(i, j, W: int, rule: str = "right"):
    """The window's part of the key mask (the causal part and the token range are applied by the callers).  ``rule`` "right" is
    the specification; the others are the mutants of test_window_attention_cpu.py."""
    if rule == "right":
        return i - j < W
    if rule == "le":                                # i - j <= W: one key more
        return i - j <= W
    if rule == "minus1":                            # i - j < W - 1: one key fewer
        return i - j < W - 1
    if rule == "tile_first_row":                    # counted from the 16-row query tile's first row
        return (i // 16) * 16 - j < W
    if rule == "edge_rounded_to_32":                # the first visible key rounded down to a 32-key step
        return j >= torch.div(i - W + 1, 32, rounding_mode="floor") * 32
    if rule == "position_id_units":                 # the query's position id (row + 5) against the key's row
        return (i + POS_OFFSET) - j < W
    if rule == "no_window":
        return torch.ones_like(i - j, dtype=torch.bool)
    raise ValueError(rule)


MUTANT_RULES = ("le", "minus1", "tile_first_row", "edge_rounded_to_32", "position_id_units", "no_window")


def live_mask(B: int, S: int, W: int, ranges, device, rule: str = "right"):
    """(live [B, 1, S, S] bool, row_live [B, 1, S, 1] bool): causal & window(rule) & token range, rows outside the range dead."""
    i = torch.arange(S, device=device).view(1, 1, S, 1)
    j = torch.arange(S, device=device).view(1, 1, 1, S)
    live = (j <= i) & window_live(i, j, W, rule)
    if ranges is not None:
        lo = ranges[0].to(device).long().view(-1, 1, 1, 1)
        hi = torch.clamp(lo + ranges[1].to(device).long().view(-1, 1, 1, 1), max=S)
        row_live = (i >= lo) & (i < hi)
        live = live & (j >= lo) & (j < hi) & row_live
    else:
        row_live = torch.ones((B, 1, S, 1), dtype=torch.bool, device=device)
    return live.expand(B, 1, S, S), row_live.expand(B, 1, S, 1)


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(c: AC.Case, W: int) -> AC.Ref:
    """attention_conformance.reference restated with the window (that one has none): float64 on the 16-bit operands as they are,
    and the bound's ingredients A, e32, under over the windowed key set, by the same formulas."""
    q, k, v = c.logical()
    B, S, HKV, dh = k.shape
    H = q.shape[2]
    dev = k.device
    idx = torch.arange(H, device=dev) // (H // HKV)
    outs = []
    for b in range(B):
        rg = None if c.ranges is None else (c.ranges[0][b:b + 1], c.ranges[1][b:b + 1])
        live, row_live = live_mask(1, S, W, rg, dev)
        qd = q[b:b + 1].double().permute(0, 2, 1, 3)
        kd = k[b:b + 1].double().permute(0, 2, 1, 3)[:, idx]
        vd = v[b:b + 1].double().permute(0, 2, 1, 3)[:, idx]
        s = (qd @ kd.transpose(-1, -2)).masked_fill(~live, -math.inf)
        m = s.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.exp2(s - m)
        l = p.sum(-1, keepdim=True)
        w = p / l.clamp_min(1e-300)
        out = w @ vd
        A = w @ vd.abs()
        L = (qd.abs() @ kd.abs().transpose(-1, -2)).masked_fill(~live, 0.0).amax(-1, keepdim=True)
        n = live.sum(-1, keepdim=True).double()
        e32 = 2.0 ** -24 * (math.log(2.0) * (2 * dh + 8) * L + 4.0 + n + 3.0 * torch.ceil(n / 32) + 16.0)
        under = (live.double() @ vd.abs() + n * out.abs()) / l.clamp_min(1.0)
        z = torch.zeros((), dtype=torch.float64, device=dev)
        outs.append(tuple(torch.where(row_live, t, z).permute(0, 2, 1, 3) for t in (out, A, e32, under)))
    return AC.Ref(*(torch.cat([o[t] for o in outs]) for t in range(4)))


# ------------------------------------------------------------------------------------------------ 16-bit emulation
def raw_scores(c: AC.Case) -> torch.Tensor:
    """fp32 logits [B, H, S, S] of a case, unmasked: ``emulate`` takes them so that a walk over the mutants computes them once."""
    q, k, _ = c.logical()
    idx = torch.arange(q.shape[2], device=k.device) // (q.shape[2] // k.shape[2])
    return q.float().permute(0, 2, 1, 3) @ k.float().permute(0, 2, 1, 3)[:, idx].transpose(-1, -2)


def emulate(c: AC.Case, W: int, rule: str = "right", scores: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention_conformance.emulate's arithmetic (style "exact": the eight-wave kernel) with the window mask ``rule``: fp32
    logits, 32-key steps from key 0 with the running maximum floored at -1e30 (rows meet steps without a live key first, as
    in the kernel), p rounded to T for the PV product, fp32 accumulation, one final rounding.  [B, S, H, dh] of dtype T."""
    q, k, v = c.logical()
    B, S, HKV, dh = k.shape
    H = q.shape[2]
    dev = k.device
    idx = torch.arange(H, device=dev) // (H // HKV)
    live, row_live = live_mask(B, S, W, c.ranges, dev, rule)
    vf = v.float().permute(0, 2, 1, 3)[:, idx]
    s = (raw_scores(c) if scores is None else scores).masked_fill(~live, -math.inf)
    m = torch.full((B, H, S, 1), -math.inf, device=dev)
    l = torch.zeros((B, H, S, 1), device=dev)
    acc = torch.zeros((B, H, S, dh), device=dev)
    for j0 in range(0, S, 32):
        sc = s[..., j0:j0 + 32]
        m_new = torch.clamp(torch.maximum(m, sc.amax(-1, keepdim=True)), min=-1e30)
        alpha = torch.exp2(m - m_new)
        l, acc, m = l * alpha, acc * alpha, m_new
        p = torch.exp2(sc - m)
        l = l + p.sum(-1, keepdim=True)
        acc = acc + p.to(c.dtype).float() @ vf[..., j0:j0 + 32, :]
    inv = torch.where(row_live & (l > 0), 1.0 / l, torch.zeros_like(l))
    return (acc * inv).to(c.dtype).permute(0, 2, 1, 3).contiguous()


def excess(got, r: AC.Ref, dtype) -> torch.Tensor:
    return AC.elementwise_excess(got, r.out, r.A, dtype, r.e32, r.under)


def blocks_with_excluded_key(S: int, W: int, lo: int, hi: int) -> List[int]:
    """16-row query blocks that have a live row whose key i - W lies in the token range (without ranges: a row >= W)."""
    return [blk for blk in range((S + 15) // 16)
            if any(lo <= i < hi and i - W >= lo for i in range(blk * 16, min(S, blk * 16 + 16)))]


# ------------------------------------------------------------------------------------------------ the case lists
def eight_wave_cases(dtype, group: int, S: int):
    """(W, range kind, B, seed) of every eight-wave case at one (dtype, group, S)."""
    for W in windows_for(S, EIGHT_WAVE_W):
        for kind in RANGE_KINDS:
            yield W, kind, (3 if kind == "ragged3" else 1), 7919 * group + 31 * S + W


def prefill32_cases(S: int):
    for W in windows_for(S, PREFILL32_W):
        for kind in RANGE_KINDS:
            yield W, kind, (3 if kind == "ragged3" else 1), 104729 + 31 * S + W


MANY_ITEMS = ((97, False), (256, True))     # (W, token ranges?) of the 8 kv heads x batch 4 x S = 600 case: 320 64-row items


def build_many_items(W: int, ranged: bool, device="cpu") -> AC.Case:
    return make_window_case(torch.bfloat16, B=4, H=32, HKV=8, S=600, W=W, ranges=AC.prefill_ranges(600) if ranged else None,
                            guard="attract", gain=6.0, seed=W, device=device)


def build(dtype, group: int, S: int, W: int, kind: str, B: int, seed: int, device="cpu", guard="nan", HKV: int = 2) -> AC.Case:
    gain = AC.GAINS[(S + W + group) % 3]
    return make_window_case(dtype, B=B, H=HKV * group, HKV=HKV, S=S, W=W, ranges=ranges_for(kind, S), guard=guard, gain=gain,
                            seed=seed, device=device)


# ------------------------------------------------------------------------------------------------ the whole sub-layer, float64
def attention_layer_reference(hidden, wq, wk, wv, wo, n_heads: int, n_kv_heads: int, position_ids=None, attention_mask=None,
                              theta: float = 10000.0, window: int = 0, dtype=torch.float64):
    """MistralAttention.forward restated (q/k/v projections without biases, default rotary embedding in the rotate_half
    convention, repeat_kv, softmax(q k^T / sqrt(dh)) over the keys of ``live_mask``, o_proj) in ``dtype`` on the CPU.  hidden
    [B, S, D]; ``attention_mask`` the [B, S] key-padding mask (one run of tokens per sequence); ``window`` 0: causal only.
    Rows outside the token run are zero.  Compared against HF itself in test_window_attention_cpu.py."""
    B, S, D = hidden.shape
    x = hidden.to(dtype)
    dh = wq.shape[0] // n_heads
    q = (x @ wq.to(dtype).t()).view(B, S, n_heads, dh).transpose(1, 2)
    k = (x @ wk.to(dtype).t()).view(B, S, n_kv_heads, dh).transpose(1, 2)
    v = (x @ wv.to(dtype).t()).view(B, S, n_kv_heads, dh).transpose(1, 2)
    pos = torch.arange(S)[None] if position_ids is None else position_ids
    pos = pos.expand(B, S) if pos.dim() == 2 else pos[None].expand(B, S)
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))           # fp32, as the rotary module holds it
    ang = pos.to(dtype)[:, None, :, None] * inv_freq.to(dtype)[None, None, None, :]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)

    def rot(t):
        return t * cos + torch.cat([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin

    q, k = rot(q), rot(k)
    g = n_heads // n_kv_heads
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    rg = None
    if attention_mask is not None:
        m = attention_mask.ne(0)
        length = m.sum(1)
        start = torch.where(length > 0, m.to(torch.int8).argmax(1), torch.zeros_like(length))
        rg = (start, length)
    live, row_live = live_mask(B, S, window if window > 0 else S, rg, hidden.device)
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    s = s.masked_fill(~live, -math.inf)
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
    w = p / p.sum(-1, keepdim=True).clamp_min(1e-300)
    ctx = torch.where(row_live, w @ v, torch.zeros((), dtype=dtype)).transpose(1, 2).reshape(B, S, n_heads * dh)
    return torch.where(row_live.view(B, S, 1), ctx @ wo.to(dtype).t(), torch.zeros((), dtype=dtype))
