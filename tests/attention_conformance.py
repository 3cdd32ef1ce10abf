"""Element-wise conformance of the two attention entry points (``slime_attention``, ``slime_prefill_attention``): a float64
reference, a DERIVED per-element error bound, a torch restatement of the kernels' arithmetic, deliberately broken variants
of that restatement, and the input generator with padded / poisoned buffers.  Plain module (no fixtures, not a conftest);
pure torch, works on CPU and GPU tensors.  Used by test_attention_bound_cpu.py and test_gpu_attention_conformance.py.

The bound (``elementwise_excess``), derived from the arithmetic documented in csrc/attention.hip / prefill.hip
--------------------------------------------------------------------------------------------------------------------------
Exact (float64, on the 16-bit operands): o_d = sum_j p_j v_jd / l, p_j = 2^(s_j - m), l = sum_j p_j; w_j = p_j / l,
A_d = sum_j w_j |v_jd|.  u = unit roundoff of T (2^-8 bf16, 2^-11 fp16; every conversion is round-to-nearest-even).

 (a) P is rounded to T before the PV MFMA: p^_j = p_j (1 + d_j), |d_j| <= u.  The numerator moves by at most
     u sum_j p_j |v_jd| = u l A_d                                                            ->  u * A          (c2 = 1)
 (b) the denominator: the generic and the eight-wave prefill kernel sum the UNROUNDED fp32 p (no u term); attn64r / prefill32
     sum the ROUNDED p with a ones-row MFMA: l^ = l (1 + e), |e| <= u, which moves o by u |o| ->  u * |ref|
 (c) one final rounding of o to T: u |o^|, o^ within the other terms of ref                  ->  u * |ref|      (c1 = 1 + 1 = 2)
     and the whole bound times (1 + 2u) for the second-order products of (a)-(c).
 (d) fp32 arithmetic, as a relative weight e32 on (|ref| + A) (a relative perturbation e_j of every weight moves
     o by at most max|e_j| (A + |ref|)):
       logits: dh products (exact in fp32 for 16-bit operands) accumulated one rounding each on partial sums of magnitude
       <= |c0| + L, L_i = max_j sum_d |q_id| |k_jd| >= |s_ij|, |m|; attn64r starts the accumulator at c0 = -reference
       (|c0| <= L), and a few more roundings follow (s - m, the reference refresh).  The logit error
       2^-24 (2 dh + 8) L enters through 2^x: relative ln2 * that; v_exp_f32 itself is good to 1 ulp (2 * 2^-24, and the
       same again for the second-order slack);
       accumulation: n PV products, the running rescale (one rounding per 32-key step), the fp32 sum of p (8 per step, one
       per step, 2 across lanes), reciprocal and scaling: n + 3 ceil(n / 32) + 16 roundings of 2^-24.
 (e) fp16 only: a p below 2^-14 falls on the subnormal grid of spacing 2^-24 (below 2^-25 it is flushed to zero): absolute
     error 2^-25 per key, relative to the reference the kernel holds WHEN THE KEY IS PROCESSED.  That reference never
     exceeds the final maximum, and later rescales (<= 1) are fp32, so in final units the numerator moves by at most
     2^-25 sum_j |v_jd| and the rounded-p denominator by 2^-25 n; with l >= 1 (the maximal key has p = 1):
     2^-25 (sum_j |v_jd| + n |ref|) / l.  The final rounding of a subnormal output adds 2^-25.
Rows outside the token range have ref = A = 0: the bound is 0 and the kernel must store exact zeros.
None of these constants was fitted to a kernel's output; test_attention_bound_cpu.py checks that ``emulate`` stays inside
and that every mutant leaves it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch

LOG2E = 1.4426950408889634
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
C1, C2 = 2.0, 1.0                       # see (b) + (c) and (a) above
PAD_COLS, PAD_ROWS = 64, 3              # guard columns per row, guard rows per batch entry
ATTRACT_V, ATTRACT_K_OVER = 1000.0, 64.0
SENTINEL = 0x7B7B                       # o is pre-filled with this 16-bit pattern (a finite number in both formats)

# shapes walked on the GPU (test_gpu_attention_conformance.py); test_attention_bound_cpu.py takes its subset from here
ATTN64_NKV = (1, 15, 16, 17, 31, 32, 33, 257, 320, 321, 336, 337, 352, 353, 576, 577, 592, 593, 607, 608, 609, 640, 1216, 1217)
ATTN64_NQ = (1, 15, 16, 17, 320, 577, 640, 641)
ATTN128_NKV = (1, 31, 32, 33, 64, 287, 288, 289, 576, 577)
ATTN128_NQ = (1, 16, 17, 144, 256, 257, 576)
GROUPS = (1, 2, 4, 8, 16)
GAINS = (1.0, 6.0, 12.0)


def prefill_lengths(group: int, prefill32: bool = False):
    qb = 256 // group
    s = {qb - 1, qb, qb + 1, 2 * qb + 17, 1, 31, 32, 33, 191, 192, 193, 600}
    if prefill32:
        s |= {63, 64, 65, 1300}
    return sorted(x for x in s if x > 0)


def prefill_ranges(S: int):
    """(start, length) of four sequences: left padding, right padding, a length-1 sequence, the whole S -- starts and ends
    off a 32-key step and off a 16-row block wherever S leaves room."""
    left = min(S - 1, 37) if S > 40 else S // 3
    right = max(1, S - 21) if S > 40 else max(1, S - S // 3)
    one = min(S - 1, 19 if S > 40 else S // 2)
    return [left, 0, one, 0], [S - left, right, 1, S]


class Ref(NamedTuple):
    out: torch.Tensor       # [B, n_q, H, dh] float64
    A: torch.Tensor         # [B, n_q, H, dh]  sum_j w_j |v_jd|
    e32: torch.Tensor       # [B, n_q, H, 1]   term (d): relative weight on (|ref| + A)
    under: torch.Tensor     # [B, n_q, H, dh]  term (e) without its 2^-25: (sum_j |v_jd| + n |ref|) / l


def _kv_index(H: int, HKV: int, head_mod: bool = False, device=None) -> torch.Tensor:
    h = torch.arange(H, device=device)
    return h % HKV if head_mod else h // (H // HKV)


def reference(q, k, v, *, causal: bool = False, group: int = 1, ranges: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
              batch_chunk: int = 4) -> Ref:
    """float64 attention on the 16-bit operands as they are.  q [B or 1, n_q, H, dh] PRE-SCALED by dh^-0.5 log2 e (logits in
    log2 units), k / v [B, n_kv, H / group, dh]; query head h uses kv head h // group (repeat_kv); ``ranges`` =
    (start [B], length [B]): sequence b lives in [start, start + length), rows outside it are exactly zero."""
    B, n_kv, HKV, dh = k.shape
    n_q, H = q.shape[1], q.shape[2]
    assert H == HKV * group
    dev = k.device
    idx = _kv_index(H, HKV, device=dev)
    i = torch.arange(n_q, device=dev)[:, None]
    j = torch.arange(n_kv, device=dev)[None, :]
    outs = []
    for b0 in range(0, B, batch_chunk):
        b1 = min(B, b0 + batch_chunk)
        qd = (q[b0:b1] if q.shape[0] == B else q.expand(B, -1, -1, -1)[b0:b1]).double().permute(0, 2, 1, 3)    # [b, H, n_q, dh]
        kd = k[b0:b1].double().permute(0, 2, 1, 3)[:, idx]
        vd = v[b0:b1].double().permute(0, 2, 1, 3)[:, idx]
        live = torch.ones((b1 - b0, 1, n_q, n_kv), dtype=torch.bool, device=dev)
        row_live = torch.ones((b1 - b0, 1, n_q, 1), dtype=torch.bool, device=dev)
        if causal:
            live = live & (j <= i)
        if ranges is not None:
            lo = ranges[0][b0:b1].to(dev).long().view(-1, 1, 1, 1)
            hi = torch.clamp(lo + ranges[1][b0:b1].to(dev).long().view(-1, 1, 1, 1), max=n_kv)
            live = live & (j >= lo) & (j < hi)
            row_live = (i >= lo) & (i < hi)
        live = live & row_live
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
    return Ref(*(torch.cat([o[t] for o in outs]) for t in range(4)))


def bound(ref: torch.Tensor, A: torch.Tensor, dtype, e32=None, under=None) -> torch.Tensor:
    u = UNIT[dtype]
    b = C1 * u * ref.abs() + C2 * u * A
    if e32 is not None:
        b = b + e32 * (ref.abs() + A)
    if dtype == torch.float16:
        if under is not None:
            b = b + 2.0 ** -25 * under
        b = b + 2.0 ** -25 * (ref != 0)
    return b * (1 + 2 * u)


def elementwise_excess(got, ref, A, dtype, e32=None, under=None) -> torch.Tensor:
    """|got - ref| - bound, float64; <= 0 everywhere for a conforming kernel.  A NaN / inf in ``got`` gives +inf."""
    ref = ref.double()
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return err - bound(ref, A.double(), dtype, e32, under)


def worst(got, r: Ref, dtype):
    """(max |err| / bound -- inf where the bound is 0 and the element is not exact --, max excess, its index, got, want)."""
    ex = elementwise_excess(got, r.out, r.A, dtype, r.e32, r.under)
    bd = bound(r.out, r.A, dtype, r.e32, r.under)
    ratio = torch.where(bd > 0, (ex + bd) / bd.clamp_min(1e-300), torch.where(ex > 0, torch.full_like(bd, math.inf), torch.zeros_like(bd)))
    flat = int(ex.argmax())
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(flat), ex.shape))
    return float(ratio.max()), float(ex.max()), idx, float(got.double().reshape(-1)[flat]), float(r.out.reshape(-1)[flat])


def describe_failure(name: str, got, r: Ref, dtype) -> str:
    ratio, ex, (b, i, h, d), g, w = worst(got, r, dtype)
    return (f"{name}: worst element (batch {b}, head {h}, row {i}, column {d}): got {g!r}, want {w!r}, "
            f"excess over the bound {ex:.3e}, worst |err| / bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------ emulation and mutants
@dataclass(frozen=True)
class Defect:
    """One deliberate defect of ``emulate``.  ``confine`` = (batch, head, 16-row block): the key-mask defects (admit / drop)
    then hold in that sub-block only."""
    admit_next: bool = False          # the key after the last live one is admitted (past n_kv: the row that follows in memory)
    drop_last: bool = False           # the last live key is dropped
    confine: Optional[Tuple[int, int, int]] = None
    causal_shift: int = 0             # key j is live iff j <= i + causal_shift
    start_shift: int = 0              # token range [start + start_shift, end + end_shift)
    end_shift: int = 0
    head_mod: bool = False            # kv head h % n_kv_heads instead of h // group
    swap_blocks: Optional[Tuple[int, int, int]] = None     # (batch, head, block): output blocks `block` and `block + 1` swapped
    dirty_outside: bool = False       # rows outside the token range keep a non-zero value


NO_DEFECT = Defect()
MUTANTS = {
    "admit_key_past_n_kv": Defect(admit_next=True),
    "drop_last_live_key": Defect(drop_last=True),
    "admit_key_past_n_kv_one_subblock": Defect(admit_next=True, confine=(0, 1, 1)),
    "drop_last_live_key_one_subblock": Defect(drop_last=True, confine=(0, 1, 1)),
    "causal_mask_one_key_more": Defect(causal_shift=1),
    "causal_mask_one_key_less": Defect(causal_shift=-1),
    "range_start_one_early": Defect(start_shift=-1),
    "range_start_one_late": Defect(start_shift=1),
    "range_end_one_early": Defect(end_shift=-1),
    "range_end_one_late": Defect(end_shift=1),
    "kv_head_modulo": Defect(head_mod=True),
    "swap_neighbouring_query_blocks": Defect(swap_blocks=(0, 1, 0)),
    "rows_outside_range_not_zeroed": Defect(dirty_outside=True),
}
CONFINED = ("admit_key_past_n_kv_one_subblock", "drop_last_live_key_one_subblock")


def emulate(q, k, v, n_q: int, n_kv: int, dtype, *, causal: bool = False, group: int = 1, ranges=None, style: str = "exact",
            defect: Defect = NO_DEFECT) -> torch.Tensor:
    """The kernels' arithmetic in torch: fp32 logits, 32-key steps with a running reference, p rounded to T for the PV product,
    fp32 accumulation, one final rounding.  q [B or 1, >= n_q, H, dh], k / v [B, >= n_kv (+ guard rows), HKV, dh] are views of
    the padded buffers (a defect may read the guard row that follows the last key).  style "exact": the reference is the
    running row maximum and the denominator sums the unrounded p (generic kernel, prefill_attn_kernel); "lazy": the reference
    is the row maximum of the first step with a live key and moves only when a score exceeds it by more than 8, and the
    denominator sums the rounded p (attn64r, prefill32).  Returns [B, n_q, H, dh] of dtype T."""
    B, rows_k, HKV, dh = k.shape
    H = q.shape[2]
    dev = k.device
    d = defect
    extra = 1 if (d.admit_next or d.end_shift > 0 or d.causal_shift > 0) and rows_k > n_kv else 0
    nk = n_kv + extra
    idx = _kv_index(H, HKV, d.head_mod, dev)
    qf = q[:, :n_q].float().expand(B, -1, -1, -1).permute(0, 2, 1, 3)
    kf = k[:, :nk].float().permute(0, 2, 1, 3)[:, idx]
    vf = v[:, :nk].float().permute(0, 2, 1, 3)[:, idx]
    i = torch.arange(n_q, device=dev).view(1, 1, -1, 1)
    j = torch.arange(nk, device=dev).view(1, 1, 1, -1)
    if ranges is not None:
        lo = ranges[0].to(dev).long().view(-1, 1, 1, 1)
        hi = torch.clamp(lo + ranges[1].to(dev).long().view(-1, 1, 1, 1), max=n_kv)
    else:
        lo = torch.zeros((B, 1, 1, 1), dtype=torch.long, device=dev)
        hi = torch.full((B, 1, 1, 1), n_kv, dtype=torch.long, device=dev)
    lo, hi = lo + d.start_shift, hi + d.end_shift
    last = (torch.minimum(i + d.causal_shift, hi - 1) if causal else hi - 1).expand(B, 1, n_q, 1)     # last live key per row
    live = (j >= lo) & (j <= last)
    live = live.expand(B, H, n_q, nk).clone()
    where = torch.ones((B, H, n_q, 1), dtype=torch.bool, device=dev)
    if d.confine is not None:
        cb, ch, blk = d.confine
        where = torch.zeros_like(where)
        where[cb % B, ch % H, blk * 16:blk * 16 + 16] = True
    if d.admit_next:
        live |= where & (j == last + 1)
    if d.drop_last:
        live &= ~(where & (j == last))
    row_live = ((i >= lo) & (i < hi)) if ranges is not None else (i >= 0)          # without token ranges every query row is live
    row_live = row_live.expand(B, 1, n_q, 1)
    live &= row_live

    s = (qf @ kf.transpose(-1, -2)).masked_fill(~live, -math.inf)                    # fp32
    m = torch.full((B, H, n_q, 1), -math.inf if style == "exact" else 0.0, device=dev)
    started = torch.zeros((B, H, n_q, 1), dtype=torch.bool, device=dev)
    l = torch.zeros((B, H, n_q, 1), device=dev)
    acc = torch.zeros((B, H, n_q, dh), device=dev)
    zero = torch.zeros((), device=dev)
    for j0 in range(0, nk, 32):
        sc = s[..., j0:j0 + 32]
        mx = sc.amax(-1, keepdim=True)
        if style == "exact":
            m_new = torch.clamp(torch.maximum(m, mx), min=-1e30)
            alpha = torch.exp2(m - m_new)
        else:
            fin = torch.isfinite(mx)
            rel = torch.where(fin, mx - m, zero)
            dlt = torch.where(fin & ~started, rel, torch.where(rel > 8.0, rel, zero))
            started = started | fin
            m_new = m + dlt
            alpha = torch.exp2(-dlt)
        l, acc, m = l * alpha, acc * alpha, m_new
        p = torch.exp2(sc - m)
        pt = p.to(dtype).float()
        l = l + (pt if style == "lazy" else p).sum(-1, keepdim=True)
        acc = acc + pt @ vf[..., j0:j0 + 32, :]
    inv = torch.where(row_live & (l > 0), 1.0 / l, torch.zeros_like(l))
    out = (acc * inv).to(dtype)
    if d.dirty_outside:
        out = torch.where(row_live, out, torch.full_like(out, 2.0 ** -6))
    if d.swap_blocks is not None:
        sb, sh, blk = d.swap_blocks
        sb, sh = sb % B, sh % H
        if (blk + 2) * 16 <= n_q:
            a, b_ = out[sb, sh, blk * 16:blk * 16 + 16].clone(), out[sb, sh, blk * 16 + 16:blk * 16 + 32].clone()
            out[sb, sh, blk * 16:blk * 16 + 16], out[sb, sh, blk * 16 + 16:blk * 16 + 32] = b_, a
    return out.permute(0, 2, 1, 3).contiguous()


# ------------------------------------------------------------------------------------------------ inputs in padded buffers
@dataclass
class Case:
    """q / k / v / o in padded buffers: row stride = heads * dh + 64 elements, batch stride = (rows + 3) row strides."""
    dtype: torch.dtype
    B: int
    H: int
    HKV: int
    dh: int
    n_q: int
    n_kv: int
    causal: bool
    shared_q: bool
    qbuf: torch.Tensor
    kbuf: torch.Tensor
    vbuf: torch.Tensor
    ranges: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    @property
    def group(self):
        return self.H // self.HKV

    def view(self, buf, heads):
        """[B, rows + 3, heads, dh] view of a padded buffer (guard rows included, guard columns not)."""
        return buf[..., :heads * self.dh].unflatten(-1, (heads, self.dh))

    def window(self, buf, heads, rows):
        return self.view(buf, heads)[:, :rows]

    def logical(self):
        return self.window(self.qbuf, self.H, self.n_q), self.window(self.kbuf, self.HKV, self.n_kv), self.window(self.vbuf, self.HKV, self.n_kv)

    def reference(self) -> Ref:
        q, k, v = self.logical()
        return reference(q, k, v, causal=self.causal, group=self.group, ranges=self.ranges)

    def emulate(self, style="exact", defect=NO_DEFECT):
        return emulate(self.view(self.qbuf, self.H), self.view(self.kbuf, self.HKV), self.view(self.vbuf, self.HKV), self.n_q, self.n_kv,
                       self.dtype, causal=self.causal, group=self.group, ranges=self.ranges, style=style, defect=defect)

    def batch_slice(self, b0, b1):
        rg = None if self.ranges is None else (self.ranges[0][b0:b1], self.ranges[1][b0:b1])
        return Case(self.dtype, b1 - b0, self.H, self.HKV, self.dh, self.n_q, self.n_kv, self.causal, self.shared_q,
                    self.qbuf if self.shared_q else self.qbuf[b0:b1], self.kbuf[b0:b1], self.vbuf[b0:b1], rg)

    def new_output(self):
        o = torch.full((self.B, self.n_q + PAD_ROWS, self.H * self.dh + PAD_COLS), SENTINEL, dtype=torch.int16, device=self.kbuf.device)
        return o.view(self.dtype)

    def check_output(self, obuf):
        """(the n_q x E window [B, n_q, H, dh], True iff every element of o outside the window still holds the sentinel)."""
        bits = obuf.view(torch.int16).clone()
        win = self.window(obuf, self.H, self.n_q).clone()
        bits[:, :self.n_q, :self.H * self.dh] = SENTINEL
        return win, bool((bits == SENTINEL).all())


def make_case(kind: str, dtype, *, B, H, dh, n_q, n_kv, HKV=None, gain=1.0, causal=False, shared_q=False, ranges=None, guard="nan",
              boost=None, seed=0, device="cpu") -> Case:
    """kind "random" (logit std = gain, log2 units), "onehot" (gain 1 + one query per 16-row block aligned with a key late in
    the sweep), "uniform" (q = 0: the output is the mean of v over the live keys; the first and last live key carry -+64).
    In "random" / "onehot", column 0 of every head is reserved: q = 1 there, k = 0 except the LAST LIVE key of the
    sequence, which holds a boost (default 3 gain + log2(n_kv) / 2; 0 = plain random data) that gives it a weight of tens of
    percent in every row that sees it (dropping it is a gross error), and the guard rows, which hold boost + 64 (admitting one
    is a gross error: their v is 1000).
    guard "nan": guard rows (>= n_q, >= n_kv) and guard columns of q / k / v are NaN; "attract": the finite attractors above;
    "neighbour": guard rows are plain random rows, as the next batch entry's are in an unpadded layout.
    Rows inside [0, n_kv) but outside a sequence's token range are ordinary (padding-token) rows of the model, not guards:
    they hold the attractors in every pass."""
    HKV = HKV or H
    g = torch.Generator().manual_seed(seed)
    Bq = 1 if shared_q else B
    amp = math.sqrt(gain) / dh ** 0.25
    q = torch.randn(Bq, n_q, H, dh, generator=g) * amp
    k = torch.randn(B, n_kv + PAD_ROWS, HKV, dh, generator=g) * amp
    v = torch.randn(B, n_kv + PAD_ROWS, HKV, dh, generator=g)
    lo = [0] * B if ranges is None else [int(x) for x in ranges[0]]
    hi = [n_kv] * B if ranges is None else [min(n_kv, int(a) + int(b)) for a, b in zip(ranges[0], ranges[1])]
    if boost is None:
        boost = float(round(3.0 * gain + 0.5 * math.log2(max(n_kv, 2))))
    if kind == "uniform":
        q.zero_()
        for b in range(B):
            v[b, hi[b] - 1] = 64.0
            if hi[b] - lo[b] > 1:
                v[b, lo[b]] = -64.0
    else:
        q[..., 0] = 1.0
        k[..., 0] = 0.0
        for b in range(B):
            k[b, hi[b] - 1, :, 0] = boost
        if kind == "onehot":
            group = H // HKV
            for blk in range((n_q + 15) // 16):
                i = min(n_q - 1, blk * 16 + (5 * blk + 3) % 16)
                for b in range(Bq):
                    j = max(lo[b], min(i, hi[b] - 1) - blk % 3) if causal else (n_kv - 1 - blk) % n_kv
                    kk = k[b, j].repeat_interleave(group, 0)                       # [H, dh]
                    q[b, i] = kk * (40.0 / (kk * kk).sum(-1, keepdim=True).clamp_min(1e-6))
        elif kind != "random":
            raise ValueError(kind)
    pad = math.nan if guard == "nan" else ATTRACT_V

    def padded(x, rows, heads):
        buf = torch.full((x.shape[0], rows + PAD_ROWS, heads * dh + PAD_COLS), pad, dtype=torch.float32)
        n = rows + PAD_ROWS if (guard == "neighbour" and x.shape[1] > rows) else rows
        buf[:, :n, :heads * dh] = x[:, :n].reshape(x.shape[0], n, heads * dh)
        return buf

    qb, kb, vb = padded(q, n_q, H), padded(k, n_kv, HKV), padded(v, n_kv, HKV)
    kview = kb[..., :HKV * dh].unflatten(-1, (HKV, dh))
    vview = vb[..., :HKV * dh].unflatten(-1, (HKV, dh))
    if guard == "attract":                                       # guard key rows: a large multiple of the common query direction
        kview[:, n_kv:] = 0.0
        kview[:, n_kv:, :, 0] = boost + ATTRACT_K_OVER
    for b in range(B):                                           # padding-token rows of the sequence: attractors in every pass
        for r in list(range(0, lo[b])) + list(range(hi[b], n_kv)):
            kview[b, r] = 0.0
            kview[b, r, :, 0] = boost + ATTRACT_K_OVER
            vview[b, r] = ATTRACT_V
    rg = None if ranges is None else (torch.as_tensor(ranges[0], dtype=torch.int32).to(device), torch.as_tensor(ranges[1], dtype=torch.int32).to(device))
    return Case(dtype, B, H, HKV, dh, n_q, n_kv, causal, shared_q, qb.to(dtype).to(device), kb.to(dtype).to(device), vb.to(dtype).to(device), rg)


def rel_l2(a, b) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
