"""Element-wise conformance of the cosine text-guided router (csrc/router.hip: ``slime_router_scores``, ``slime_router_scores_batched``
and the softmax ``slime_router_select`` writes to ``probs_out``): the cases, float64 references, DERIVED per-element bounds, torch fp32
restatements of the kernels' arithmetic (``emulate_*``) with switchable defects, and the construction of inputs whose kept set is
decided with a margin.  Plain module (no fixtures, not a conftest); pure torch, works on CPU and GPU tensors.  Used by
test_router_bound_cpu.py and test_gpu_router_conformance.py.

Conventions are those of rowwise_conformance.py: e = 2^-24, a sum whose terms pass through at most n additions carries e n sum|terms|,
every bound carries SLACK = 1 + 2^-10 for second-order products, and the one allowance for sqrtf followed by a division is
A_RSQRT e (both are correctly rounded in a build without fast-math: 1.5 e would do; the constant is rowwise_conformance's, not a new one).
EPS is the fp32 number 1e-8f the kernels (and torch's fp32 cosine_similarity) clamp with, widened to float64.

(1) Scores.  Reference (unfactorised, float64 on the fp32 operands): c_tl = (x_t / max(|x_t|, EPS)) . (y_l / max(|y_l|, EPS)),
    score_t = sum_l m_l c_tl with a mask (masked terms are zeroed, whatever finite values the row holds), mean_l c_tl without.
    The kernels compute score_t = (x_t . u) / max(|x_t|, EPS), u_h = sum_l w_l y_lh, w_l = m_l / max(|y_l|, EPS)  (m_l = fl(1 / L) with no mask).
    n(H) = ceil(H / 256) float4 steps per lane; a term of a row sum passes through at most 4 n(H) additions in its lane (three
    inside a step and one into the accumulator, whatever the compiler contracts into fma) and six butterfly levels:
      C = 4 n(H) + 6,   one more e for the product:       |fl(sum a_h b_h) - sum a_h b_h| <= (C + 1) e sum|a_h b_h|
    w_l:  the sum of squares is relative (C + 1) e, its root half of that; max(., EPS) is 1-Lipschitz in the relative sense
          (max(a (1 + d), EPS) is inside (1 +- d) max(a, EPS)), so the clamp needs no case of its own:
            eps_w = (C + 1) e / 2 + A_RSQRT e            (+ e for fl(1 / L) without a mask);    a masked row: w_l = 0 exactly
    u_h:  L sequential multiply-adds from 0 (one product rounding, at most L additions), w exact in float64:
            A_h = sum_l |w_l y_lh|,          du_h = (eps_w + (L + 1) e) A_h
    score: d = x . u^ with the computed u^ (|u^_h| <= |u_h| + du_h), the norm as for w:
            dd      = (C + 1) e sum_h |x_h| (|u_h| + du_h) + sum_h |x_h| du_h
            eps_n   = (C + 1) e / 2 + A_RSQRT e
            dscore  = (dd / N + (|score| + dd / N) eps_n) SLACK,       N = max(|x|, EPS)
    The bound is ABSOLUTE: where the text rows cancel (u ~ 0) it is e-sized against sum_l |c_tl| and nothing is relative to the
    score.  It is exactly 0 -- the score must be the reference's bits, 0.0 -- for an all-zero image row and for a fully masked text.
    The float64 reference's own rounding (2^-53 per operation) is eight orders below e and is not carried.
(2) probs_out, against the float64 softmax of the DEVICE's fp32 scores and the fp32 temperature: z_i = s_i / temp (one division, e |z_i|),
    mx = the largest computed z (its own rounding is common to all elements and drops out of a softmax), a_i = z_i - mx (e |a_i|):
            da_i = e (|z_i| + |a_i|)
    e_i = expf(a_i): relative rho_i = expm1(da_i) + A_EXP e, and an absolute 2^-126 (results below fp32's normal range may be flushed;
    below 2^-150, i.e. a_i < -104, the result is exactly 0 either way).  The sum: ceil(P / 1024) terms per thread (P = T rounded up
    to a power of two), six butterfly levels, 16 partials in turn, all terms >= 0 and the largest exactly 1:
            D = ceil(P / 1024) + 22,     eps_S = sum_j p_j rho_j + D e + T 2^-126
            dp_i = (p_i (rho_i + eps_S + e) + 2 * 2^-126) SLACK
(3) The kept set.  Given float64 scores with a bound ds on every one, every z moves by at most dz = max ds / temp, and the
    probabilities the selection sorts differ from the float64 ones by at most  DP_i = p_i expm1(2 dz) + dp_i  (e^z_i and the sum each
    move by a factor inside e^+-dz).  A cumulative sum c of the k largest moves less: with the kept terms scaled up and the others
    down, c' <= c / (c + (1 - c) e^-2dz), so  |c' - c| <= c (1 - c) expm1(2 dz).
    The fp32 kept set equals the float64 one if every gap between neighbouring sorted probabilities exceeds DP_i + DP_i+1 (the order
    is then the same) and every cumulative sum c_i stays away from top-p by more than
            dc_i = c_i (1 - c_i) expm1(2 dz) + sum_j<=i dp_j + i e c_i + |topp - fl32(topp)|
    (the sequential fp32 cumulative sum of i + 1 terms and the fp32 top-p).  ``selection_margin`` returns the smallest ratio of the
    two kinds; the cases of ``SEP_CASES`` hold it above 16 (test_router_bound_cpu.py asserts it for every one).
None of these constants was fitted to a kernel's output; test_router_bound_cpu.py checks that every ``emulate_*`` stays inside and that
every defect leaves its bound on the case named for it.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

import rowwise_conformance as RC
from rowwise_conformance import A_EXP, A_RSQRT, E32, FLUSH32, SLACK, Padded, SENTINEL_BYTE   # noqa: F401  (re-exported for the tests)

EPS = float(torch.tensor(1e-8, dtype=torch.float32))          # the kernels' 1e-8f
SENTINEL_F32 = float(torch.tensor([SENTINEL_BYTE] * 4, dtype=torch.uint8).view(torch.float32)[0])
ROUTER_MAX_T = 4096


def f32(v: float) -> float:
    """The fp32 number a ``float`` argument of the C ABI becomes."""
    return float(torch.tensor(v, dtype=torch.float32))


def ceil4(n: int) -> int:
    return (n + 3) // 4 * 4


def single_workspace_floats(L: int, H: int) -> int:
    """include/slime_hip.h: the single entry's scratch."""
    return L + H + 4


def batched_workspace_floats(B: int, L: int, H: int) -> int:
    """slime_router_batched_workspace_floats: one stride for the w [L] and the u [H] table of an image, both tables B times."""
    return 0 if min(B, L, H) <= 0 else 2 * max(ceil4(L), H) * B


def chain(H: int) -> int:
    return 4 * ((H + 255) // 256) + 6


# ================================================================================================ (1) score cases
SCORE_KINDS = ("random", "aligned", "cancelling", "zero_row", "tiny", "zero_text_row", "all_masked")
# (T, L, H): T on both sides of the four-row workgroup, H = one float4 / one trip / one lane into the second trip / four trips,
# every L of the issue, L > H (the batched stride comes from L), ceil4(L) == H
SCORE_SHAPES = ((1, 1, 4), (4, 3, 128), (5, 4, 256), (7, 5, 260), (37, 12, 1024), (5, 12, 4), (37, 3, 260), (7, 1, 1024), (1, 5, 128),
                (4, 12, 256), (37, 260, 256), (5, 125, 128))
PRODUCT_SHAPE = (1008, 300, 4096)
BIG = 1.0e17                    # what a masked-out row may hold (H BIG^2 stays finite in fp32 up to H = 4096)


@dataclass
class ScoreCase:
    T: int
    L: int
    H: int
    kind: str
    img: torch.Tensor                   # [T, H] fp32
    text: torch.Tensor                  # [L, H] fp32
    mask: Optional[torch.Tensor]        # [L] uint8 or None

    def what(self):
        return f"scores T={self.T} L={self.L} H={self.H} {self.kind} mask={'yes' if self.mask is not None else 'no'}"


def make_mask(L: int, seed: int, g=None) -> torch.Tensor:
    """uint8 [L]: at least one valid row, and from L = 2 on at least one masked-out row."""
    g = g or torch.Generator().manual_seed(977 * seed + L)
    m = (torch.rand(L, generator=g) < 0.6).to(torch.uint8)
    m[seed % L] = 1
    if L >= 2:
        m[(seed + 1) % L] = 0
    return m


def make_score_case(T: int, L: int, H: int, kind: str, masked: bool, seed: int = 0, device="cpu") -> ScoreCase:
    """"aligned": every text row a positive multiple of one direction (|u| = the number of valid rows); "cancelling": the second half
    of the rows is the first half negated, NOT next to their partners, so u is rounding residue (an odd row out stays random);
    "zero_row": image row T / 2 all zero; "tiny": image rows of norm 1e-9, 1e-6 and O(1) in turn, the first valid text row at norm
    1e-9 and the last at 1e-6; "zero_text_row": the last valid text row all zero; "all_masked": no valid row.  Masked-out rows hold
    ordinary random values."""
    assert kind in SCORE_KINDS and (masked or kind != "all_masked")
    g = torch.Generator().manual_seed(15485863 * seed + 7919 * T + 131 * L + H + 17 * SCORE_KINDS.index(kind) + int(masked))
    img = torch.randn(T, H, generator=g, dtype=torch.float64) * (0.5 + 1.5 * torch.rand(T, 1, generator=g, dtype=torch.float64))
    text = torch.randn(L, H, generator=g, dtype=torch.float64) * (0.5 + 1.5 * torch.rand(L, 1, generator=g, dtype=torch.float64))
    mask = make_mask(L, seed, g) if masked else None
    valid = torch.arange(L) if mask is None else mask.nonzero().view(-1)
    if kind == "aligned":
        text = torch.randn(1, H, generator=g, dtype=torch.float64) * (0.5 + 1.5 * torch.rand(L, 1, generator=g, dtype=torch.float64))
    elif kind == "cancelling":
        half = L // 2
        text[half:2 * half] = -text[:half]
        if mask is not None:                         # partners share their validity, and one pair is valid
            mask[half:2 * half] = mask[:half]
            if half:
                mask[0] = mask[half] = 1
    elif kind == "zero_row":
        img[T // 2] = 0.0
    elif kind == "tiny":
        r = torch.arange(T)
        nrm = img.norm(dim=1, keepdim=True)
        img = torch.where((r % 3 == 0)[:, None], img / nrm * 1e-9, torch.where((r % 3 == 1)[:, None], img / nrm * 1e-6, img))
        text[valid[-1]] *= 1e-6 / text[valid[-1]].norm()
        text[valid[0]] *= 1e-9 / text[valid[0]].norm()
    elif kind == "zero_text_row":
        text[valid[-1]] = 0.0
    elif kind == "all_masked":
        mask = torch.zeros(L, dtype=torch.uint8)
    return ScoreCase(T, L, H, kind, img.float().to(device), text.float().to(device), None if mask is None else mask.to(device))


def score_cases(seed: int = 0, shapes: Sequence[Tuple[int, int, int]] = SCORE_SHAPES, device="cpu"):
    for i, (T, L, H) in enumerate(shapes):
        for kind in SCORE_KINDS:
            for masked in (True, False):
                if masked or kind != "all_masked":
                    yield make_score_case(T, L, H, kind, masked, seed=100 * seed + i, device=device)


def score_reference(img, text, mask):
    """(float64 scores [T], bound [T]) of part (1): the oracle's ``router_cosine_scores`` in float64, operands normalised one by one."""
    x, y = img.double(), text.double()
    T, H = x.shape
    L = y.shape[0]
    nx, ny = x.norm(dim=1).clamp_min(EPS), y.norm(dim=1).clamp_min(EPS)
    cos = (x / nx[:, None]) @ (y / ny[:, None]).T                                  # [T, L], every pair on its own
    if mask is not None:
        m = mask.ne(0)
        score = cos.masked_fill(~m[None, :], 0.0).sum(1)
        w = m.double() / ny
    else:
        score = cos.mean(1)
        w = torch.full_like(ny, 1.0 / L) / ny
    C = chain(H)
    eps_w = (C + 1) * E32 / 2 + A_RSQRT * E32 + (E32 if mask is None else 0.0)
    wy = w[:, None] * y
    if mask is not None:
        wy = torch.where(m[:, None], wy, torch.zeros_like(wy))                     # 0 times a finite number: exactly nothing
    u = wy.sum(0)
    du = (eps_w + (L + 1) * E32) * wy.abs().sum(0)
    dd = (C + 1) * E32 * (x.abs() @ (u.abs() + du)) + x.abs() @ du
    eps_n = (C + 1) * E32 / 2 + A_RSQRT * E32
    return score, (dd / nx + (score.abs() + dd / nx) * eps_n) * SLACK


@dataclass(frozen=True)
class ScoreDefect:
    eps_on_product: bool = False          # x . y / max(|x| |y|, eps), the clamp of old torch
    eps_under_sqrt: bool = False          # sqrt(max(s, eps)): the clamp on the squared norm, the root taken outside it
    eps_added: bool = False               # sqrt(s) + eps
    mean_over_valid: bool = False         # with a mask: the sum divided by the number of valid rows
    sum_without_mask: bool = False        # without a mask: no 1 / L
    mask_ignored: bool = False
    drop_row_tail: bool = False           # the last T % 4 rows are never written
    drop_col_tail: bool = False           # the columns behind the last whole 256 are never read
    u_at_L: bool = False                  # u written at ws + L and read at ws + ceil4(L): a read shifted by ceil4(L) - L
    u_of_image_0: bool = False            # batched: every image reads the first image's u


SCORE_MUTANTS = {"eps_on_the_product_of_the_norms": ScoreDefect(eps_on_product=True),
                 "eps_on_the_squared_norm_root_outside": ScoreDefect(eps_under_sqrt=True),
                 "eps_added_to_the_norm": ScoreDefect(eps_added=True),
                 "mean_over_the_valid_count": ScoreDefect(mean_over_valid=True),
                 "sum_instead_of_mean_without_mask": ScoreDefect(sum_without_mask=True),
                 "mask_ignored": ScoreDefect(mask_ignored=True),
                 "last_T_mod_4_rows_dropped": ScoreDefect(drop_row_tail=True),
                 "column_tail_H_mod_256_dropped": ScoreDefect(drop_col_tail=True),
                 "u_at_ws_plus_L": ScoreDefect(u_at_L=True)}
BATCH_MUTANTS = {"image_b_reads_u_of_image_0": ScoreDefect(u_of_image_0=True)}


def _lane_dot(a, b, cols: int):
    """sum_h a_h b_h over the first ``cols`` columns in the kernels' order: lane = (h / 4) % 64 takes its float4 of every 256 columns
    in turn, ((p0 + p1) + p2) + p3 into its accumulator, then the xor butterfly 32 .. 1; lane 0's value.  a, b [R, H] fp32 -> [R]."""
    R = a.shape[0]
    n = max(1, (cols + 255) // 256)
    pa, pb = a.new_zeros(R, n * 256), a.new_zeros(R, n * 256)
    pa[:, :cols], pb[:, :cols] = a[:, :cols], b[:, :cols]
    p = (pa * pb).view(R, n, 64, 4)
    q = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    v = a.new_zeros(R, 64)
    for k in range(n):
        v = v + q[:, k]
    lane = torch.arange(64, device=a.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def _norm32(s, eps, d: ScoreDefect):
    if d.eps_under_sqrt:
        return torch.sqrt(torch.maximum(s, eps))
    if d.eps_added:
        return torch.sqrt(s) + eps
    return torch.maximum(torch.sqrt(s), eps)


def emulate_text_dir(text, mask, defect: ScoreDefect = ScoreDefect()):
    """router_text_weight_kernel and router_text_dir_kernel in torch fp32 -> u [H]."""
    d = defect
    L, H = text.shape
    cols = H - H % 256 if d.drop_col_tail else H
    eps = torch.tensor(1e-8, dtype=torch.float32, device=text.device)
    one = torch.ones((), dtype=torch.float32, device=text.device)
    use_mask = mask is not None and not d.mask_ignored
    if use_mask:
        m = mask.ne(0).float()
        if d.mean_over_valid:
            m = m / m.sum().clamp_min(1.0)
    else:
        m = (one if (d.sum_without_mask or mask is not None) else one / torch.tensor(float(L), dtype=torch.float32, device=text.device)).expand(L)
    w = m / _norm32(_lane_dot(text, text, cols), eps, d)
    u = torch.zeros(H, dtype=torch.float32, device=text.device)
    for l in range(L):
        u = u + w[l] * text[l]
    if d.u_at_L and ceil4(L) != L:
        sh = ceil4(L) - L
        u = torch.cat([u[sh:], u.new_zeros(sh)])
    return u


def emulate_scores(img, text, mask, defect: ScoreDefect = ScoreDefect(), u=None):
    """slime_router_scores in torch fp32 -> [T] fp32; a row the (defective) kernel never writes holds the sentinel."""
    d = defect
    T, H = img.shape
    eps = torch.tensor(1e-8, dtype=torch.float32, device=img.device)
    if d.eps_on_product:                                  # unfactorised, as the clamp on the product cannot be factorised
        nx, ny = torch.sqrt(_lane_dot(img, img, H)), torch.sqrt(_lane_dot(text, text, H))
        cos = (img @ text.T) / torch.maximum(nx[:, None] * ny[None, :], eps)
        return (cos * mask.ne(0).float()[None, :]).sum(1) if mask is not None else cos.mean(1)
    if u is None:
        u = emulate_text_dir(text, mask, d)
    cols = H - H % 256 if d.drop_col_tail else H
    out = _lane_dot(img, u[None, :].expand(T, H), cols) / _norm32(_lane_dot(img, img, cols), eps, d)
    if d.drop_row_tail and T % 4:
        out[T - T % 4:] = SENTINEL_F32
    return out


def emulate_scores_batched(tokens, row_off, n_rows, text, mask, defect: ScoreDefect = ScoreDefect()) -> List[torch.Tensor]:
    """slime_router_scores_batched: image b = rows row_off[b] .. + n_rows[b] of ``tokens`` against text[b] (and mask[b])."""
    out = []
    u0 = emulate_text_dir(text[0], None if mask is None else mask[0], defect)
    for b, (o, n) in enumerate(zip(row_off, n_rows)):
        if n == 0:
            out.append(tokens.new_zeros(0))
            continue
        out.append(emulate_scores(tokens[o:o + n], text[b], None if mask is None else mask[b], defect, u=u0 if defect.u_of_image_0 else None))
    return out


def check_scores(c: ScoreCase, got, ref=None):
    """-> (worst |err| / bound, message or None); the exact cases (zero image row, no valid text row) are held to 0.0."""
    want, bd = ref if ref is not None else score_reference(c.img, c.text, c.mask)
    ratio, msg = RC.check(c.what(), got, want, bd)
    if msg is None and c.kind == "zero_row" and float(got[c.T // 2]) != 0.0:
        msg = f"{c.what()}: the all-zero image row {c.T // 2} scored {float(got[c.T // 2])!r}, not 0.0"
    if msg is None and c.kind == "all_masked" and not bool((got == 0).all()):
        msg = f"{c.what()}: no valid text row, yet a score is not 0.0"
    return ratio, msg


# ---- the batch of part 2 of the issue ---------------------------------------------------------------------------------------------
@dataclass
class BatchCase:
    name: str
    tokens: torch.Tensor               # [rows, H] fp32
    row_off: List[int]
    n_rows: List[int]
    text: torch.Tensor                 # [B, L, H]
    mask: Optional[torch.Tensor]       # [B, L] uint8 or None

    @property
    def B(self):
        return len(self.n_rows)

    @property
    def T_max(self):
        return max(self.n_rows)


BATCH_LAYOUTS = ("fused", "ragged")


def make_batch_case(layout: str, L: int, H: int, masked: bool, B: int = 4, seed: int = 0, device="cpu") -> BatchCase:
    """B = 4: image 0 starts at row 0, image 1 has no rows, images 2 and 3 overlap in the token buffer and image 3 ends at its last
    row.  "fused": P = 3 rows in front of every image but the first (which must start at row 0); "ragged": the images back to back.
    Every image has its own valid count.  B = 1: one image of 6 rows from row 0 to the end."""
    assert layout in BATCH_LAYOUTS and B in (1, 4)
    g = torch.Generator().manual_seed(32452843 * seed + 1009 * L + H + BATCH_LAYOUTS.index(layout))
    P = 3 if layout == "fused" else 0
    if B == 1:
        off, n = [0], [6]
    else:
        n = [5, 0, 9, 6]
        off = [0, 5 + P, 5 + 2 * P, 5 + 2 * P + 9 - 2]                            # image 3 begins two rows before image 2 ends
    rows = off[-1] + n[-1]
    tokens = torch.randn(rows, H, generator=g)
    text = torch.randn(B, L, H, generator=g)
    mask = None
    if masked:
        mask = torch.stack([make_mask(L, seed + 3 * b + 1) for b in range(B)])
        for b in range(B):                                                         # a different valid count per image where L allows it
            want = min(L, 1 + b)
            idx = torch.randperm(L, generator=g)
            mask[b] = 0
            mask[b, idx[:want]] = 1
    return BatchCase(f"{layout} B={B} L={L} H={H} mask={'yes' if masked else 'no'}", tokens.to(device), off, n, text.to(device),
                     None if mask is None else mask.to(device))


# ================================================================================================ (2) probs_out
PROB_T = (1, 2, 1023, 1025, 4096)
PROB_TEMP = (0.3, 1.0, 2.0)
PROB_KINDS = ("cosine", "spread")
SPREAD = 200.0                           # scores over [-200, 200]: max z > 88.8 (expf overflows without the max subtraction) and
                                         # (max - min) / temp > 104 at every temperature of PROB_TEMP
TOPP_ALMOST_ONE = 1.0 - 2.0 ** -20


def prob_scores(T: int, kind: str, seed: int = 0) -> torch.Tensor:
    """"cosine": what the score kernel can produce for a dozen text rows; "spread": a shuffled linspace over [-SPREAD, SPREAD]."""
    assert kind in PROB_KINDS
    g = torch.Generator().manual_seed(104729 * seed + T + PROB_KINDS.index(kind))
    if kind == "cosine":
        return (12.0 * (2 * torch.rand(T, generator=g) - 1)).contiguous()
    return torch.linspace(-SPREAD, SPREAD, T)[torch.randperm(T, generator=g)].contiguous()


def _prob_terms(z):
    """z float64 [T] -> (p, bound dp, a = z - max z) of part (2), on the HOST: the float64 softmax of torch's GPU build was measured
    6e-6 (relative) away from the host's at z - max z = -65, which is the size of the bound there."""
    z = z.detach().double().cpu()
    T = z.numel()
    a = z - z.max()
    p = torch.softmax(z, 0)
    P = 1
    while P < T:
        P <<= 1
    rho = torch.expm1(E32 * (z.abs() + a.abs())) + A_EXP * E32
    eps_S = float((p * rho).sum()) + ((P + 1023) // 1024 + 22) * E32 + T * FLUSH32
    return p, (p * (rho + eps_S + E32) + 2 * FLUSH32) * SLACK, a


def probs_reference(scores32, temp: float):
    """float64 softmax of the fp32 scores over the fp32 temperature -> (p, bound, z - max z)."""
    return _prob_terms(scores32.double() / f32(temp))


@dataclass(frozen=True)
class ProbDefect:
    no_max_subtraction: bool = False
    temp_after_exp: bool = False          # expf(s - max s) / temp: the temperature cancels in the normalisation


PROB_MUTANTS = {"softmax_without_the_max_subtraction": ProbDefect(no_max_subtraction=True),
                "temperature_after_the_exponent": ProbDefect(temp_after_exp=True)}


def emulate_probs(scores32, temp: float, defect: ProbDefect = ProbDefect()):
    """router_select_kernel's softmax in torch fp32: thread tid sums elements tid, tid + 1024, ..., butterfly per wave, 16 partials in turn."""
    d = defect
    T = scores32.numel()
    t = torch.tensor(temp, dtype=torch.float32, device=scores32.device)
    if d.temp_after_exp:
        e = torch.exp(scores32 - scores32.max()) / t
    else:
        z = scores32 / t
        e = torch.exp(z if d.no_max_subtraction else z - z.max())
    n = max(1, (T + 1023) // 1024)
    pad = e.new_zeros(n * 1024)
    pad[:T] = e
    pad = pad.view(n, 1024)
    v = e.new_zeros(1024)
    for k in range(n):
        v = v + pad[k]
    v = v.view(16, 64)
    lane = torch.arange(64, device=e.device)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    sm = e.new_zeros(())
    for wv in range(16):
        sm = sm + v[wv, 0]
    return e / sm


def check_probs(name: str, got, scores32, temp: float):
    """-> (ratio, message or None): inside the bound everywhere, and exactly 0.0 wherever z - max z < -104."""
    p, bd, a = probs_reference(scores32, temp)
    got = got.detach().cpu()
    ratio, msg = RC.check(name, got, p, bd)
    if msg is None and not bool((got[a < -104.0] == 0).all()):
        msg = f"{name}: an element with z - max z < -104 is not exactly 0.0"
    return ratio, msg


def router_expected(probs, topp: float) -> torch.Tensor:
    """The kept set (ascending) from the device's own probabilities, in router_select_kernel's arithmetic: a STABLE descending sort,
    the cumulative sum taken in turn with every partial sum rounded to fp32, compared with the fp32 top-p, one more.
    rowwise_conformance.router_expected takes torch.cumsum, which on the CPU carries a double and rounds each output: the two differ
    by an ulp of the partial sum, which decides the count where a sum lands on top-p (the spread kind at top-p = 1 - 2^-20 does)."""
    import numpy as np
    p = probs.detach().float().cpu()
    T = p.numel()
    sp, si = torch.sort(p, descending=True, stable=True)
    c = torch.from_numpy(np.cumsum(sp.numpy(), dtype=np.float32))
    k = int((c <= torch.tensor(topp, dtype=torch.float32)).sum())
    return (si[:k + 1] if k < T else torch.arange(T)).sort()[0]


def kept_zeros_are_the_lowest(probs, kept) -> bool:
    """Among the elements of probability exactly 0.0, the kept ones are the lowest-indexed."""
    zeros = (probs == 0).nonzero().view(-1)
    kz = kept[(probs[kept] == 0)]
    return bool(torch.equal(kz, zeros[:kz.numel()]))


# ================================================================================================ (3) a kept set decided with a margin
SEP_T = (37, 288, 1008)
SEP_PT = ((0.95, 1.0), (0.5, 0.3), (1e-4, 1.0))
SEP_H = 128
MARGIN = 16.0
# (T, top-p, temp) -> (half-width of the a_t linspace, number of valid text rows U: the scores span [-U span, U span]).  U makes the
# distribution peaked enough that the cut falls after few terms (the sequential cumulative sum costs e per term) at a step of the
# cumulative sum far above its error, and small enough that no probability underflows at temp = 0.3.  Chosen by walking the span in
# steps of 0.01 until selection_margin exceeded 2 MARGIN; test_router_bound_cpu.py asserts MARGIN for every entry, so a change of
# the construction or of a bound that spoils one fails there.
SEP_CASES = {(37, 0.95, 1.0): (0.3, 24), (37, 0.5, 0.3): (0.3, 4), (37, 1e-4, 1.0): (0.3, 24),
             (288, 0.95, 1.0): (0.3, 24), (288, 0.5, 0.3): (0.3, 4), (288, 1e-4, 1.0): (0.3, 24),
             (1008, 0.95, 1.0): (0.88, 24), (1008, 0.5, 0.3): (0.3, 4), (1008, 1e-4, 1.0): (0.3, 24)}


def make_separated(T: int, span: float, U: int, seed: int = 0, device="cpu"):
    """(img [T, H], text [U + 1, H], mask [U + 1]): the U valid text rows are positive multiples of one unit vector v (u = U v), the
    masked-out row (the second) is random; image row t = r_t (a_t v + sqrt(1 - a_t^2) n_t), n_t a unit vector orthogonal to v, a_t a
    shuffled linspace over [-span, span], r_t in [0.5, 2].  The float64 score of row t is U a_t up to the fp32 rounding of the inputs."""
    g = torch.Generator().manual_seed(49979687 * seed + T)
    H = SEP_H
    v = torch.randn(H, generator=g, dtype=torch.float64)
    v = v / v.norm()
    text = v[None, :] * (0.5 + 1.5 * torch.rand(U + 1, 1, generator=g, dtype=torch.float64))
    text[1] = torch.randn(H, generator=g, dtype=torch.float64)
    mask = torch.ones(U + 1, dtype=torch.uint8)
    mask[1] = 0
    a = torch.linspace(-span, span, T, dtype=torch.float64)[torch.randperm(T, generator=g)]
    n = torch.randn(T, H, generator=g, dtype=torch.float64)
    n = n - (n @ v)[:, None] * v
    n = n / n.norm(dim=1, keepdim=True)
    img = (a[:, None] * v + torch.sqrt(1 - a * a)[:, None] * n) * (0.5 + 1.5 * torch.rand(T, 1, generator=g, dtype=torch.float64))
    return img.float().to(device), text.float().to(device), mask.to(device)


def selection_margin(scores64, ds, topp: float, temp: float) -> float:
    """Part (3): the smallest of (gap of neighbouring sorted probabilities) / (DP_i + DP_i+1) and |c_i - topp| / dc_i."""
    t = f32(temp)
    p, dp, _ = _prob_terms(scores64 / t)
    g2 = math.expm1(2 * float(ds.max()) / t)
    DP = p * g2 + dp
    sp, si = torch.sort(p, descending=True, stable=True)
    ratio = math.inf
    if p.numel() > 1:
        D = DP[si]
        ratio = float(((sp[:-1] - sp[1:]) / (D[:-1] + D[1:])).min())
    c = torch.cumsum(sp, 0)
    i = torch.arange(p.numel(), dtype=torch.float64)
    dc = c * (1 - c).clamp_min(0.0) * g2 + torch.cumsum(dp[si], 0) + i * E32 * c + abs(topp - f32(topp))
    return min(ratio, float(((c - topp).abs() / dc).min()))


def separated_case(T: int, topp: float, temp: float, device="cpu"):
    """-> (img, text, mask, float64 kept set of the oracle's router_select on the float64 scores, margin)."""
    from oracle import slime_oracle as O
    img, text, mask = make_separated(T, *SEP_CASES[(T, topp, temp)], device=device)
    s64, ds = (t.cpu() for t in score_reference(img, text, mask))                  # the selection's float64 side runs on the host
    return img, text, mask, O.router_select(s64, topp, temp), selection_margin(s64, ds, topp, temp)
