"""Element-wise conformance of ``slime_gemm_ex``: a float64 reference of every epilogue of include/slime_hip.h, a DERIVED
per-element error bound, a torch fp32 restatement of the kernels' arithmetic, deliberately broken variants of that restatement,
and the input generator with padded / poisoned buffers.  Plain module (no fixtures, not a conftest); pure torch, works on CPU and
GPU tensors.  Used by test_gemm_bound_cpu.py and test_gpu_gemm_conformance.py.

The bound, derived from the arithmetic of csrc/gemm.hip (``epilogue_wave``, ``epilogue_mix``, ``gelu_erf``) and gemm_shared.h
--------------------------------------------------------------------------------------------------------------------------------
Exact (float64, on the 16-bit operands as they are): acc = sum_k a_k b_k, Sacc = sum_k |a_k b_k|, x = acc + bias (+ residual h),
S = Sacc + |bias| + |h|.  e = 2^-24 (fp32 unit roundoff), u = unit roundoff of T (2^-8 bf16, 2^-11 fp16; every conversion is RNE).

 (1) fp32 accumulation: a product of two 16-bit operands is exact in fp32; one rounding per accumulated product and the epilogue's
     own additions (at most 3: bias, residual, the bracket of the split form), as a relative weight on S -- the convention of term
     (d) of the attention bound:                                                   dx = e (K + 4) S
     fp32 outputs (BIAS_F32, BIAS_RESID_F32, the C of BIAS_RESID_F32_LN) stop here.  Kind "integer" (below): the accumulation is exact
     in any order, so K drops out and dx = 4 e S -- which is what pins lo8 to its cell in fp16, where a cell of the byte is
     2^-18 |c| and e (K + 4) S never is below it.
 (2) one final RNE to T where the output is T (BIAS_T, BIAS_RESID_T, x16, and behind every activation):
                                                                                   dy + u (|y| + dy) + g
     g = fp16's subnormal grid, 2^-25 (half of the spacing 2^-24 below 2^-14); bf16's (2^-134) is kept for form's sake.  The fp32 part
     dy carries a factor (1 + 2^-10) for the second-order products of everything below.
 (3) quick-GELU y = x / (1 + 2^(C x)), C = -1.702f * log2e in fp32: C carries 3 roundings (two constants, their product), C x one more:
     the exponent moves by 4 e |C x|, i.e. the power by ln2 * that, plus v_exp_f32's 1 ulp (2 e): epsE.  s = 1 / (1 + E) moves
     by (1 - s) epsE relatively, then 1 + E (e), v_rcp_f32 at 1 ulp (2 e) and the product (e):
                                                        dy = |y'(x)| dx + |y| ((1 - s) epsE + 4 e),   y' = s + 1.702 x s (1 - s)
     Both activations: + |x| 2^-126, absolute -- v_exp_f32 overflows to inf (x < -51: s = 0 where the true s is a denormal) and
     v_exp_f32 / v_rcp_f32 flush results below fp32's normal range to zero.
 (4) erf-GELU is the Abramowitz-Stegun 7.1.26 form, documented ABSOLUTE erf error 1.5e-7, which enters as 0.5 |x| 1.5e-7 -- at
     x = -5 that is a quarter of the value, and exactly that much is allowed.  The fp32 evaluation: z = |x| c (2 e), t = rcp(fma) (4 e
     + 1 ulp = 6 e), a five-level Horner form (term i: 2 i + 2 roundings and i t-errors: <= 42 e on sum_i |a_i| t^i, taken per element
     against the polynomial's value), -z z and the scaling inside __expf (7 e z^2 on the power), v_exp_f32 (2 e), the product (e):
         eps_tail = 42 e sum|a_i| t^i / poly + (7 z^2 + 3) e,     d(1 + erf) = 1.5e-7 + tail eps_tail (+ 2 e for 2 - tail, x >= 0)
                                                        dy = |y'(x)| dx + 0.5 |x| d(1 + erf) + 2 e |y|,    y' = Phi(x) + x phi(x)
 (5) the gate mix g0 gelu(x0) + g1 gelu(x1): the two terms of (4) weighted by |g0|, |g1|, and 3 e (|g0 y0| + |g1 y1|) for the two
     products and the sum.
 (6) the LayerNorm-fold consumer fma(rstd, acc, fma(-mu rstd, colsum, bias)); mu, rstd in float64 from the SAME partial sums the
     kernel is handed.  ln_finalize in fp32 (G = ln_groups): d_sx = G e sum|sx_g|, d_mu = d_sx / K + 2 e |mu|, d_sq = G e sq,
     d_var = d_sq / K + 2 e sq / K + 2 |mu| d_mu + e mu^2 (var = E[x^2] - mu^2: the cancellation at |mu| >> sigma is in this
     term), eps_r = d_var / (2 (var + eps - d_var)) + e / 2 + 4 e (rsqrtf at 2 ulp), d_nmr = rstd d_mu + |mu| rstd (eps_r + e):
         dx = rstd e K Sacc + eps_r rstd |acc| + d_nmr |colsum| + 2 e (rstd Sacc + |mu| rstd |colsum| + |bias|)
     i.e. the weight rstd (S + |mu| |colsum|) + |bias| of the fold, plus the fp32 error of the statistics.
 (7) the split residual (BIAS_RESID_SPLIT_LN): h = join(hi, lo8) is exact integer arithmetic; c = acc + (bias + h) by (1).  The
     kernel's fp32 c^ lies in [c - dx, c + dx].  hi' must be T(c^) for SOME such c^: T(c - dx) <= hi' <= T(c + dx) (where c sits
     within dx of a rounding boundary either neighbour is admissible); lo8' must be the byte of the header's integer definition
     for some c^ of that interval GIVEN the hi' that was stored (the definition is monotonic in c^); and
     |join(hi', lo8') - c| <= dx + ulp(hi') / 512 (+ 2^-25 below fp16's normal range, where hi's spacing is fixed).
 (8) stats_out per 64-column group, of the UNROUNDED c: each partial sum by its own accumulation, 64 terms, plus the per-element
     error of c:   d_sum = sum dx + 64 e sum |c|,    d_sumsq = sum (2 |c| dx + dx^2) + 65 e sum c^2.
Kind "integer" (small integers, at most 32 non-zero products per element): every partial sum in ANY order is an integer below 2^24
and the result an integer that T holds exactly, so fp32 / BIAS_T / BIAS_RESID_T outputs must be bit-equal to the reference.
None of these constants was fitted to a kernel's output; test_gemm_bound_cpu.py checks that ``emulate`` stays inside and that every
mutant leaves the bound.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

LOG2E = 1.4426950408889634
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
E32 = 2.0 ** -24
SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
RESID_SH = {torch.bfloat16: 8, torch.float16: 5}
MANT = {torch.bfloat16: 8, torch.float16: 11}            # significand bits, hidden one included
EMIN = {torch.bfloat16: -126, torch.float16: -14}
HALF_MAX = {torch.bfloat16: 0.5 * 3.3895313892515355e38, torch.float16: 0.5 * 65504.0}
FLUSH32 = 2.0 ** -126                                     # below it v_exp_f32 / v_rcp_f32 flush to zero
ERF_ABS = 1.5e-7                                          # Abramowitz-Stegun 7.1.26
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
PAD_COLS, PAD_ROWS, TAIL = 64, 3, 64
SENTINEL_BYTE = 0x7B          # every output byte beforehand: 0x7B7B (16-bit) and 0x7B7B7B7B (fp32) are finite numbers, 123 as a byte

# epilogue codes of include/slime_hip.h
(EPI_BIAS_T, EPI_BIAS_QUICKGELU_T, EPI_BIAS_GELU_T, EPI_BIAS_F32, EPI_BIAS_RESID_F32, EPI_BIAS_RESID_F32_LN, EPI_BIAS_RESID_T,
 EPI_BIAS_GELU_MIX_T, EPI_BIAS_RESID_SPLIT_LN) = range(9)
# form -> (epilogue, LayerNorm-fold consumer)
FORMS = {
    "bias_t": (EPI_BIAS_T, False), "quickgelu_t": (EPI_BIAS_QUICKGELU_T, False), "gelu_t": (EPI_BIAS_GELU_T, False),
    "bias_f32": (EPI_BIAS_F32, False), "resid_f32": (EPI_BIAS_RESID_F32, False), "resid_f32_ln": (EPI_BIAS_RESID_F32_LN, False),
    "resid_t": (EPI_BIAS_RESID_T, False), "gelu_mix_t": (EPI_BIAS_GELU_MIX_T, False), "resid_split_ln": (EPI_BIAS_RESID_SPLIT_LN, False),
    "fold_bias_t": (EPI_BIAS_T, True), "fold_quickgelu_t": (EPI_BIAS_QUICKGELU_T, True),
}
WAVE_FORMS = tuple(f for f in FORMS if f != "gelu_mix_t")             # what every kernel family instantiates (epilogue_wave)
ROW_MAP_FORMS = ("bias_t", "quickgelu_t", "gelu_t", "bias_f32")
EXACT_FORMS = ("bias_t", "bias_f32", "resid_f32", "resid_f32_ln", "resid_t")   # kind "integer": C bit-equal to the reference
OUT_T_FORMS = ("bias_t", "quickgelu_t", "gelu_t", "resid_t", "gelu_mix_t", "resid_split_ln", "fold_bias_t", "fold_quickgelu_t")
KINDS = ("random", "integer", "tails")

# ---- the shape tables, from the kernels' own constants (csrc/gemm.hip: launch_epi, launch_*_k) -----------------------------------
TILE_BM = {3: 128, 15: 128, 18: 64, 4: 256, 10: 192, 11: 256, 12: 128}        # forced tile id -> rows per workgroup
TILE_FAMILY = {3: "gemm_kernel 128x128 two-stage", 15: "gemm_kernel 128x128 ring", 18: "gemm_kernel 64x64 ring", 4: "gemm_pp_kernel",
               10: "gemm_w4_kernel 192", 11: "gemm_w4_kernel 256", 12: "gemm_db_kernel"}
TILE_N = {3: (256, 128, 384), 15: (256, 128, 384), 18: (256, 128, 384), 4: (256, 512), 10: (256, 512), 11: (256, 512), 12: (256, 512)}
K_SMALL = (64, 128, 192, 256)         # fewer k-tiles than ring stages / than the direct-B kernel's fragment flight, and just enough
K_TAG = (1984, 2048, 2112)            # both sides of KTAG (K >= 2048) and of the fc2 direct-B rule (K > 2048)
MIX_TOKENS = 64                       # tokens per workgroup of the mix epilogue
MIX_M = (1, 63, 64, 65, 145)
PP_TILES_M = (7, 8, 9)                # xcd_rows_tile: quotient 0 with remainder 7, quotient 1 with remainder 0 / 1


def m_table(bm: int):
    return tuple(sorted({1, 15, 16, 17, bm - 1, bm, bm + 1, 2 * bm + 17}))


def pp_tile_ms():
    """One M per tiles_m of PP_TILES_M, each with a ragged last 256-row tile."""
    return tuple((t - 1) * 256 + 37 for t in PP_TILES_M)


# ------------------------------------------------------------------------------------------------ padded buffers
class Padded:
    """rows x width window inside an allocation of its own: the window starts 16 bytes into it (16-byte, not 128-byte aligned),
    the row stride is width + pad_cols elements, guard_rows rows follow the window and ``tail`` elements the last row.  Every byte
    is SENTINEL_BYTE until something else is written."""

    def __init__(self, rows, width, dtype, device, pad_cols=PAD_COLS, guard_rows=PAD_ROWS, tail=0):
        self.rows, self.width, self.dtype = rows, width, dtype
        self.ld = width + pad_cols
        self.off = 16 // torch.empty((), dtype=dtype).element_size()
        self.flat = torch.empty(self.off + (rows + guard_rows) * self.ld + tail, dtype=dtype, device=device)
        self.flat.view(torch.uint8).fill_(SENTINEL_BYTE)
        self.full = self.flat[self.off:self.off + (rows + guard_rows) * self.ld].view(rows + guard_rows, self.ld)

    @property
    def win(self):
        return self.full[:self.rows, :self.width]

    def ptr(self):
        return self.full.data_ptr()

    def fill(self, window, guard=None):
        """window values (any float / int tensor of the window's shape); ``guard``: every element outside it."""
        if guard is not None:
            self.flat.fill_(guard)
        self.win.copy_(window.to(self.dtype))
        return self

    def snapshot(self):
        return self.flat.clone()

    def restore(self, snap):
        self.flat.copy_(snap)

    def window_of(self, snap):
        return snap[self.off:self.off + self.full.numel()].view(self.full.shape)[:self.rows, :self.width]

    def intact(self, snap) -> bool:
        """True iff every byte outside the window still is what ``snap`` holds."""
        cur = self.flat.clone()
        keep = cur[self.off:self.off + self.full.numel()].view(self.full.shape)
        keep[:self.rows, :self.width] = self.window_of(snap)
        return bool(torch.equal(cur.view(torch.uint8), snap.view(torch.uint8)))


# ------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    kind: str
    dtype: torch.dtype
    form: str
    M: int
    N: int
    K: int
    guard: str
    buf: Dict[str, Padded]                       # A, B, bias, C and what the form adds (A2, gates, resid, x16, lo8, stats_out, ln_stats, colsum, row_map)
    has_bias: bool = True
    alias: bool = False                          # resid_t: resid is C
    ln_eps: float = 1e-5
    out_rows: int = 0                            # rows of the C window (M, or 2 M + 5 behind a row map)
    snaps: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def epilogue(self):
        return FORMS[self.form][0]

    @property
    def fold(self):
        return FORMS[self.form][1]

    @property
    def outputs(self):
        o = ["C"]
        if self.form == "resid_f32_ln":
            o += ["x16", "stats_out"]
        if self.form == "resid_split_ln":
            o += ["lo8", "stats_out"]
        return o

    def snapshot(self):
        self.snaps = {k: self.buf[k].snapshot() for k in self.outputs}

    def restore(self):
        for k in self.outputs:
            self.buf[k].restore(self.snaps[k])

    def windows(self):
        """The outputs' windows as they are now (clones)."""
        return {k: self.buf[k].win.clone() for k in self.outputs}

    def intact(self):
        """name of the first output whose bytes outside the window changed since ``snapshot``, or None."""
        for k in self.outputs:
            if not self.buf[k].intact(self.snaps[k]):
                return k
        return None

    def arg_fields(self, operand="B", b_frag: Optional[int] = None):
        """Field values of slime_gemm_args (ctypes: _lib.GemmArgs(**fields)).  operand "B": row-major only; "B+frag"; "frag":
        the fragment-order image alone (``b_frag`` = its device pointer)."""
        b = self.buf
        f = dict(A=b["A"].ptr(), lda=b["A"].ld, B=b["B"].ptr() if operand != "frag" else None, bias=b["bias"].ptr() if self.has_bias else None,
                 C=b["C"].ptr(), ldc=b["C"].ld, M=self.M, N=self.N, K=self.K, dtype={torch.bfloat16: 0, torch.float16: 1}[self.dtype],
                 epilogue=self.epilogue, B_frag=b_frag if operand != "B" else None)
        if self.fold:
            f.update(ln_stats=b["ln_stats"].ptr(), ln_groups=self.K // 64, ln_colsum=b["colsum"].ptr(), ln_eps=self.ln_eps)
        if self.form == "resid_f32_ln":
            f.update(x16=b["x16"].ptr(), ldx=b["x16"].ld, stats_out=b["stats_out"].ptr())
        if self.form == "resid_split_ln":
            f.update(lo8=b["lo8"].ptr(), ldlo=b["lo8"].ld, stats_out=b["stats_out"].ptr())
        if self.form == "resid_t":
            r = b["C"] if self.alias else b["resid"]
            f.update(resid=r.ptr(), ldr=r.ld)
        if self.form == "gelu_mix_t":
            f.update(A2=b["A2"].ptr(), mix_gates=b["gates"].ptr())
        if "row_map" in b:
            f.update(row_map=b["row_map"].ptr())
        return f


def _attract(dtype):
    return 1.0e6 if dtype != torch.float16 else 6.0e4


def make_case(kind: str, dtype, form: str, M: int, N: int, K: int, *, guard="nan", alias=True, row_map=False, bias=True, gates=None,
              outlier_row=True, outliers=True, seed=0, device="cpu") -> Case:
    """Padded, poisoned buffers for one call (class Padded: row stride width + 64, 3 guard rows, window 16 bytes into the allocation;
    B, bias and colsum are followed by 64 poisoned elements, stats_out / gates / ln_stats / row_map by 3 extra rows).
    kind "random": A ~ N(0, 1), B ~ N(0, 1) K^-1/2, a per-column bias of distinct magnitudes (0.01 * 1.5^(n mod 16), alternating sign),
    one 50x outlier column in A and another in B (``outliers``); "integer": A in -2 .. 2, B = +-1 at 32 k positions (8 in the first 32-wide k-step, 8
    in the last, 16 between) and 0 elsewhere, bias / residual in -8 .. 8; "tails": a bias that spreads the pre-activations over
    [-9, 9] under a small product (both GELUs are judged in their negative tails).
    guard "nan": every input guard is NaN; "attract": A's guards hold 1e4-scale values and the residual's 1e6 (6e4 where it is
    fp16), so a kernel that reads one column or row too far is grossly wrong.  Outputs that are not read keep SENTINEL_BYTE; outputs
    updated in place (the residual forms) carry the input guard, and ``Case.intact`` compares every byte outside the window."""
    assert form in FORMS and kind in KINDS and guard in ("nan", "attract")
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 7919 * M + 31 * N + K)
    fold = FORMS[form][1]

    def randn(*s):
        return torch.randn(*s, generator=g, device=device)

    def randint(lo, hi, *s):
        return torch.randint(lo, hi, s, generator=g, device=device).float()

    if kind == "integer":
        A, A2 = randint(-2, 3, M, K), randint(-2, 3, M, K)
        mask = torch.zeros(K, device=device)
        mid = torch.randperm(K - 64, generator=g, device=device)[:16] + 32 if K > 64 else torch.arange(8, 24, device=device) + 8
        mask[:8], mask[K - 8:] = 1.0, 1.0
        mask[mid] = 1.0
        B = (randint(0, 2, N, K) * 2 - 1) * mask
        bias_v, h = randint(-8, 9, N), randint(-8, 9, M, N)
    else:
        sa = 0.25 if kind == "tails" else 1.0
        A, A2, B = randn(M, K) * sa, randn(M, K) * sa, randn(N, K) * K ** -0.5
        h = randn(M, N)
        n = torch.arange(N, device=device)
        if kind == "tails":
            bias_v = (torch.linspace(-9.0, 9.0, N, device=device))[torch.randperm(N, generator=g, device=device)]
        else:
            bias_v = 0.01 * 1.5 ** (n % 16).float() * (1 - 2 * ((n // 16) % 2)).float()
            if outliers:
                A[:, K // 3] *= 50.0
                A2[:, K // 3] *= 50.0
                B[:, (2 * K) // 3] *= 50.0
    if fold and kind != "integer":                       # un-normalised rows: a mean per row, one row at |mu| = 10 sigma
        A = A + 0.5 * randn(M, 1)
        if outlier_row:
            A[min(3, M - 1)] += 10.0 * (0.25 if kind == "tails" else 1.0)
    nan = math.nan
    ga = nan if guard == "nan" else 1.0e4
    gr = nan if guard == "nan" else _attract(dtype)
    buf: Dict[str, Padded] = {}
    buf["A"] = Padded(M, K, dtype, device).fill(A, ga)
    buf["B"] = Padded(N, K, dtype, device, pad_cols=0, guard_rows=0, tail=TAIL).fill(B, ga)
    buf["bias"] = Padded(1, N, torch.float32, device, pad_cols=0, guard_rows=0, tail=TAIL).fill(bias_v.view(1, N), ga)
    out_t = form in OUT_T_FORMS
    R = 2 * M + 5 if row_map else M
    cdt = dtype if out_t else torch.float32
    buf["C"] = Padded(R, N, cdt, device)
    if form in ("resid_f32", "resid_f32_ln"):
        buf["C"].fill(h, nan if guard == "nan" else 1.0e6)
    if form == "resid_f32_ln":
        buf["x16"] = Padded(M, N, dtype, device)
    if form in ("resid_f32_ln", "resid_split_ln"):
        buf["stats_out"] = Padded(M, 2 * (N // 64), torch.float32, device, pad_cols=0)
    if form == "resid_split_ln":
        hi = h.to(dtype)
        sh = RESID_SH[dtype]
        lo = ((h.contiguous().view(torch.int32) - hi.float().view(torch.int32)) >> sh).clamp(-128, 127)
        if kind == "integer":                            # the stream's lower part exercised over its whole range
            lo = torch.where(hi.float() != 0, torch.randint(-128, 128, (M, N), generator=g, device=device, dtype=torch.int32), lo)
        buf["C"].fill(hi, gr)
        buf["lo8"] = Padded(M, N, torch.int8, device).fill(lo)
    if form == "resid_t":
        if alias:
            buf["C"].fill(h, gr)
        else:
            buf["resid"] = Padded(M, N, dtype, device).fill(h, gr)
    if form == "gelu_mix_t":
        buf["A2"] = Padded(M, K, dtype, device).fill(A2, ga)
        if gates is None:
            pairs = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.3, 0.7]], device=device)
            gates = pairs[torch.arange(M, device=device) % 3]
        buf["gates"] = Padded(M, 2, torch.float32, device, pad_cols=0).fill(gates, ga)
    if fold:
        a16 = buf["A"].win.double().view(M, K // 64, 64)
        st = torch.stack([a16.sum(-1), (a16 * a16).sum(-1)], -1).float().view(M, 2 * (K // 64))
        buf["ln_stats"] = Padded(M, 2 * (K // 64), torch.float32, device, pad_cols=0).fill(st, ga)
        buf["colsum"] = Padded(1, N, torch.float32, device, pad_cols=0, guard_rows=0, tail=TAIL).fill(
            buf["B"].win.double().sum(1).float().view(1, N), ga)
    if row_map:
        assert form in ROW_MAP_FORMS
        p = torch.randperm(M, generator=g, device=device)
        rm = (2 * p + (torch.arange(M, device=device) % 3 == 0).long()).to(torch.int32)     # non-monotone, with gaps, injective
        buf["row_map"] = Padded(M, 1, torch.int32, device, pad_cols=0).fill(rm.view(M, 1), R)   # entries past M point at a guard row
    c = Case(kind, dtype, form, M, N, K, guard, buf, has_bias=bias, alias=alias, out_rows=R)
    c.snapshot()
    return c


# ------------------------------------------------------------------------------------------------ float64 reference
@dataclass
class Ref:
    """float64 results and what the bound needs (all [M, N] unless noted)."""
    out: torch.Tensor                         # C (for the split form: the unrounded c)
    S: torch.Tensor                           # sum_k |a_k b_k| + |bias| + |residual|
    dx: torch.Tensor                          # term (1) / (6): bound of the fp32 pre-activation (or of c)
    x: Optional[torch.Tensor] = None          # pre-activation (non-linear forms); [2, M, N] for the mix
    gates: Optional[torch.Tensor] = None      # [M, 2]
    stats: Optional[torch.Tensor] = None      # [M, N / 64, 2]
    row_map: Optional[torch.Tensor] = None    # [M] int64


def join64(hi: torch.Tensor, lo8: torch.Tensor, dtype) -> torch.Tensor:
    """The header's join(hi, lo8): the fp32 number with pattern(float(hi)) + lo8 2^SH + 2^(SH - 1), exact; returned in float64."""
    sh = RESID_SH[dtype]
    p = hi.float().contiguous().view(torch.int32) + lo8.to(torch.int32) * (1 << sh) + (1 << (sh - 1))
    return p.view(torch.float32).double()


def delta8(c32: torch.Tensor, hi: torch.Tensor, dtype) -> torch.Tensor:
    """The header's lo8 = clamp((pattern(c) - pattern(float(hi))) >> SH, -128, 127), int32."""
    d = (c32.float().contiguous().view(torch.int32) - hi.float().contiguous().view(torch.int32)) >> RESID_SH[dtype]
    return d.clamp(-128, 127)


def _quickgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def _gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def reference(c: Case) -> Ref:
    """float64 on the 16-bit operands as they are (the buffers' windows), for the case's form.  Call before the launch: the
    residual forms update their inputs in place (Case.restore puts them back)."""
    b = c.buf
    A, B = b["A"].win.double(), b["B"].win.double()
    acc, Sacc = A @ B.T, A.abs() @ B.abs().T
    bias = b["bias"].win.double().view(1, -1) if c.has_bias else torch.zeros((1, c.N), dtype=torch.float64, device=A.device)
    K = c.K
    nacc = 0 if c.kind == "integer" else K              # kind "integer": the accumulation is exact, only the epilogue rounds
    rm = b["row_map"].win.view(-1).long() if "row_map" in b else None
    if c.fold:
        G = K // 64
        st = b["ln_stats"].win.double().view(c.M, G, 2)
        sx, sq = st[..., 0].sum(1, keepdim=True), st[..., 1].sum(1, keepdim=True)
        asx = st[..., 0].abs().sum(1, keepdim=True)
        mu = sx / K
        var = (sq / K - mu * mu).clamp_min(0.0)
        rstd = (var + c.ln_eps).rsqrt()
        cs = b["colsum"].win.double().view(1, -1)
        x = rstd * (acc - mu * cs) + bias
        d_mu = G * E32 * asx / K + 2 * E32 * mu.abs()
        d_var = G * E32 * sq / K + 2 * E32 * sq / K + 2 * mu.abs() * d_mu + E32 * mu * mu
        eps_r = d_var / (2 * (var + c.ln_eps - d_var).clamp_min(1e-300)) + 4.5 * E32
        d_nmr = rstd * d_mu + mu.abs() * rstd * (eps_r + E32)
        W = rstd * Sacc + mu.abs() * rstd * cs.abs() + bias.abs()
        dx = rstd * E32 * nacc * Sacc + eps_r * rstd * acc.abs() + d_nmr * cs.abs() + 2 * E32 * W
        return Ref(out=_activate(c.form, x), S=W, dx=dx, x=x)
    if c.form == "gelu_mix_t":
        A2 = b["A2"].win.double()
        x = torch.stack([acc + bias, A2 @ B.T + bias])
        S = torch.stack([Sacc, A2.abs() @ B.abs().T]) + bias.abs()
        gt = b["gates"].win.double()
        y = _gelu64(x)
        return Ref(out=gt[:, 0:1] * y[0] + gt[:, 1:2] * y[1], S=S, dx=E32 * (nacc + 4) * S, x=x, gates=gt)
    h = None
    if c.form in ("resid_f32", "resid_f32_ln"):
        h = b["C"].win.double()
    elif c.form == "resid_t":
        h = (b["C"] if c.alias else b["resid"]).win.double()
    elif c.form == "resid_split_ln":
        h = join64(b["C"].win, b["lo8"].win, c.dtype)
    x = acc + bias + (h if h is not None else 0.0)
    S = Sacc + bias.abs() + (h.abs() if h is not None else 0.0)
    dx = E32 * (nacc + 4) * S
    r = Ref(out=_activate(c.form, x), S=S, dx=dx, x=x, row_map=rm)
    if c.form in ("resid_f32_ln", "resid_split_ln"):
        xg = x.view(c.M, c.N // 64, 64)
        r.stats = torch.stack([xg.sum(-1), (xg * xg).sum(-1)], -1)
    return r


def _activate(form, x):
    if form.endswith("quickgelu_t"):
        return _quickgelu64(x)
    if form == "gelu_t":
        return _gelu64(x)
    return x


# ------------------------------------------------------------------------------------------------ the bound
def _round_T(y, dy, dtype):
    """term (2): the fp32 error dy followed by one RNE to T."""
    return dy * (1 + 2.0 ** -10) + UNIT[dtype] * (y.abs() + dy) + SUBNORMAL[dtype]


def _d_quickgelu(x, dx):
    s = torch.sigmoid(1.702 * x)
    y = x * s
    dydx = (s + 1.702 * x * s * (1 - s)).abs()
    epsE = math.log(2.0) * (1.702 * LOG2E * x.abs()) * 4 * E32 + 2 * E32
    return dydx * dx + y.abs() * ((1 - s) * epsE + 4 * E32) + x.abs() * FLUSH32


def _d_gelu(x, dx):
    z = x.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + AS_P * z)
    poly, spoly, tp = torch.zeros_like(x), torch.zeros_like(x), t.clone()
    for a in AS_A:
        poly, spoly, tp = poly + a * tp, spoly + abs(a) * tp, tp * t
    tail = torch.special.erfc(z)
    eps_tail = 42 * E32 * spoly / poly + (7 * z * z + 3) * E32
    d_ope = ERF_ABS + tail * eps_tail + 2 * E32 * (x >= 0)
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    dydx = (0.5 * torch.special.erfc(-z * torch.sign(x)) + x * phi).abs()
    y = _gelu64(x)
    return dydx * dx + 0.5 * x.abs() * d_ope + 2 * E32 * y.abs() + x.abs() * FLUSH32


def bound(c: Case, r: Ref) -> Dict[str, torch.Tensor]:
    """Per-element bounds of every output of the case but the split form's pair (``check_split``): "C", and "x16" / "stats_out"."""
    out: Dict[str, torch.Tensor] = {}
    f = c.form
    if f in ("bias_f32", "resid_f32", "resid_f32_ln"):
        out["C"] = r.dx * (1 + 2.0 ** -10)
    elif f in ("bias_t", "resid_t", "fold_bias_t"):
        out["C"] = _round_T(r.out, r.dx, c.dtype)
    elif f in ("quickgelu_t", "fold_quickgelu_t"):
        out["C"] = _round_T(r.out, _d_quickgelu(r.x, r.dx), c.dtype)
    elif f == "gelu_t":
        out["C"] = _round_T(r.out, _d_gelu(r.x, r.dx), c.dtype)
    elif f == "gelu_mix_t":
        g0, g1 = r.gates[:, 0:1].abs(), r.gates[:, 1:2].abs()
        y = _gelu64(r.x)
        d = g0 * _d_gelu(r.x[0], r.dx[0]) + g1 * _d_gelu(r.x[1], r.dx[1]) + 3 * E32 * (g0 * y[0].abs() + g1 * y[1].abs())
        out["C"] = _round_T(r.out, d, c.dtype)
    if f == "resid_f32_ln":
        out["x16"] = _round_T(r.out, r.dx, c.dtype)
    if f in ("resid_f32_ln", "resid_split_ln"):
        xg, dg = r.x.view(c.M, c.N // 64, 64), r.dx.view(c.M, c.N // 64, 64)
        d_sum = dg.sum(-1) + 64 * E32 * xg.abs().sum(-1)
        d_sq = (2 * xg.abs() * dg + dg * dg).sum(-1) + 65 * E32 * (xg * xg).sum(-1)
        out["stats_out"] = torch.stack([d_sum, d_sq], -1) * (1 + 2.0 ** -10)
    return out


def elementwise_excess(got, want, bd) -> torch.Tensor:
    """|got - want| - bound, float64; <= 0 everywhere for a conforming kernel.  A NaN / inf in ``got`` gives +inf."""
    err = (got.double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    return err - bd


def worst(got, want, bd):
    """(max |err| / bound -- inf where the bound is 0 and the element is not exact --, max excess, its index, got, want, bound there)."""
    ex = elementwise_excess(got, want, bd)
    ratio = torch.where(bd > 0, (ex + bd) / bd.clamp_min(1e-300), torch.where(ex > 0, torch.full_like(bd, math.inf), torch.zeros_like(bd)))
    flat = int(ex.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ex.shape))
    return (float(ratio.max()), float(ex.max()), idx, float(got.double().reshape(-1)[flat]), float(want.reshape(-1)[flat]),
            float(bd.reshape(-1)[flat]))


def describe_failure(name: str, got, want, bd, bm: int = 128, what: str = "C") -> str:
    ratio, ex, idx, g, w, b = worst(got, want, bd)
    row, col = idx[0], idx[1] if len(idx) > 1 else 0
    return (f"{name}: worst element of {what} at (row {row}, column {col}) = row {row % bm} of row tile {row // bm} (BM = {bm}), column "
            f"{col % 8} of store group {col // 8}: got {g!r}, want {w!r}, bound {b:.3e}, excess {ex:.3e}, worst |err| / bound {ratio:.3f}")


def _ulp_T(v, dtype):
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** EMIN[dtype]))).clamp_min(EMIN[dtype])
    return torch.exp2(e - (MANT[dtype] - 1))


def check_split(c: Case, r: Ref, hi, lo8):
    """Term (7).  hi / lo8: the windows after the call.  Returns (worst ratio of |join(hi', lo8') - c| to its bound, message or None)."""
    cref, dx = r.out, r.dx * (1 + 2.0 ** -10)
    lo32 = torch.nextafter((cref - dx).float(), torch.full_like(cref, -math.inf).float())      # fp32 values that enclose [c - dx, c + dx]
    hi32 = torch.nextafter((cref + dx).float(), torch.full_like(cref, math.inf).float())
    hf = hi.float()
    if not bool(torch.isfinite(hf).all()):
        return math.inf, "hi' holds a non-finite value"
    bad = (hf < lo32.to(c.dtype).float()) | (hf > hi32.to(c.dtype).float())
    if bool(bad.any()):
        i, j = (int(v) for v in bad.nonzero()[0])
        return math.inf, (f"hi' at (row {i}, column {j}) = {float(hf[i, j])!r} is not T(c) for any c within the bound of "
                          f"{float(cref[i, j])!r} (+- {float(dx[i, j]):.3e})")
    # the byte, given the hi' that was stored: c^ has the sign of hi' (RNE keeps it), and the definition is monotonic in c^
    neg = torch.signbit(hf)
    zero = torch.zeros_like(lo32)
    lo_c = torch.where(neg, lo32, torch.maximum(lo32, zero))
    hi_c = torch.where(neg, torch.minimum(hi32, -zero), hi32)
    d_a, d_b = delta8(lo_c, hi, c.dtype), delta8(hi_c, hi, c.dtype)
    l8 = lo8.to(torch.int32)
    badl = (l8 < torch.minimum(d_a, d_b)) | (l8 > torch.maximum(d_a, d_b))
    if bool(badl.any()):
        i, j = (int(v) for v in badl.nonzero()[0])
        return math.inf, (f"lo8' at (row {i}, column {j}) = {int(l8[i, j])} but the header's definition gives {int(d_a[i, j])} .. "
                          f"{int(d_b[i, j])} for hi' = {float(hf[i, j])!r}, c = {float(cref[i, j])!r} (+- {float(dx[i, j]):.3e})")
    bd = dx + _ulp_T(hf.double(), c.dtype) / 512 + (SUBNORMAL[c.dtype] if c.dtype == torch.float16 else 0.0) * (hf.abs() < 2.0 ** -14)
    got = join64(hi, lo8, c.dtype)
    ratio, ex, idx, g, w, b = worst(got, cref, bd)
    return ratio, (None if ex <= 0 else describe_failure("join(hi', lo8')", got, cref, bd, what="the split stream"))


def check(c: Case, r: Ref, outs: Dict[str, torch.Tensor], bm: int = 128):
    """Every output window of the case against the reference: (worst |err| / bound over all of them, message or None).
    ``outs``: name -> window after the call (Case.windows() or emulate()).  Behind a row map the rows no entry names must still
    hold what they held at the snapshot, compared as bytes."""
    worst_ratio, bds = 0.0, bound(c, r)
    C = outs["C"]
    if r.row_map is not None:
        before = c.buf["C"].window_of(c.snaps["C"])
        gap = torch.ones(c.out_rows, dtype=torch.bool, device=C.device)
        gap[r.row_map] = False
        if not torch.equal(C[gap].contiguous().view(torch.uint8), before[gap].contiguous().view(torch.uint8)):
            rows = (C[gap].float() != before[gap].float()).any(1).nonzero().view(-1)
            return math.inf, f"row_map: a row no entry names was written (gap row #{int(rows[0]) if len(rows) else -1})"
        C = C[r.row_map]
    if c.form == "resid_split_ln":
        ratio, msg = check_split(c, r, C, outs["lo8"])
        if msg:
            return ratio, msg
        worst_ratio = ratio
    else:
        if c.kind == "integer" and c.form in EXACT_FORMS:
            if not torch.equal(C.double(), r.out):
                return math.inf, describe_failure("integer operands: C must be bit-equal to the reference", C, r.out, torch.zeros_like(r.out), bm)
        ratio, ex, *_ = worst(C, r.out, bds["C"])
        if ex > 0:
            return ratio, describe_failure(c.form, C, r.out, bds["C"], bm)
        worst_ratio = ratio
    for name, want in (("x16", r.out), ("stats_out", r.stats)):
        if name in bds:
            got = outs[name] if name != "stats_out" else outs[name].view(c.M, c.N // 64, 2)
            ratio, ex, *_ = worst(got, want, bds[name])
            if ex > 0:
                return ratio, describe_failure(c.form, got, want, bds[name], bm, what=name)
            worst_ratio = max(worst_ratio, ratio)
    return worst_ratio, None


def rel_l2(a, b) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ emulation and mutants
@dataclass(frozen=True)
class Defect:
    """One deliberate defect of ``emulate``."""
    drop_last_kstep: bool = False
    first_kstep_twice: bool = False
    bias_other_half: bool = False          # bias[p][j] for bias[p][4 + j]
    no_bias_on_ragged_tile: bool = False
    tail_row_stored_twice: bool = False    # row M - 1 also lands on row M - 2
    last_row_group_unwritten: bool = False
    one_group: bool = False                # the two store defects above and row_map_next: one 8-column store group (one lane's store) only
    truncate: bool = False
    tanh_gelu: bool = False
    quickgelu_17: bool = False
    gates_swapped: bool = False
    a2_is_a: bool = False
    resid_twice: bool = False              # h enters twice on one 16-row step
    lo8_plus_one: bool = False
    lo8_unsigned: bool = False
    mu_sign: bool = False
    colsum_next: bool = False
    stats_rounded: bool = False
    stats_neighbour_group: bool = False
    row_map_next: bool = False


NO_DEFECT = Defect()
MUTANTS = {
    "last_kstep_dropped": Defect(drop_last_kstep=True),
    "first_kstep_twice": Defect(first_kstep_twice=True),
    "bias_of_the_other_half": Defect(bias_other_half=True),
    "no_bias_on_ragged_tile": Defect(no_bias_on_ragged_tile=True),
    "tail_row_stored_twice": Defect(tail_row_stored_twice=True),
    "last_row_group_unwritten": Defect(last_row_group_unwritten=True),
    "truncation_for_rne": Defect(truncate=True),
    "tanh_gelu_for_erf_gelu": Defect(tanh_gelu=True),
    "quickgelu_1.7": Defect(quickgelu_17=True),
    "gates_swapped": Defect(gates_swapped=True),
    "a2_is_a": Defect(a2_is_a=True),
    "residual_read_after_store": Defect(resid_twice=True),
    "lo8_off_by_one": Defect(lo8_plus_one=True),
    "lo8_not_sign_extended": Defect(lo8_unsigned=True),
    "fold_mu_sign": Defect(mu_sign=True),
    "fold_colsum_of_next_column": Defect(colsum_next=True),
    "stats_of_the_rounded_values": Defect(stats_rounded=True),
    "stats_of_the_neighbouring_group": Defect(stats_neighbour_group=True),
    "row_map_of_next_row": Defect(row_map_next=True),
    "tail_row_stored_twice_one_group": Defect(tail_row_stored_twice=True, one_group=True),
    "row_map_of_next_row_one_group": Defect(row_map_next=True, one_group=True),
}
# what touches at most one 8-column store group of one or two rows.  (The whole-row forms of the same defects are in MUTANTS too, but a
# whole wrong row of 1731 is sqrt(2 / 1731) = 3.4e-2 in rel-L2: the whole-tensor check does see those.)
CONFINED = ("last_row_group_unwritten", "tail_row_stored_twice_one_group", "row_map_of_next_row_one_group")


def _to_T(x, dtype, truncate=False):
    t = x.to(dtype)
    if truncate:                                      # toward zero: one pattern back where RNE went up in magnitude
        over = t.float().abs() > x.abs()
        t = (t.view(torch.int16) - over.to(torch.int16)).view(dtype)
    return t


def _gelu_erf32(x):
    """gelu_erf of csrc/gemm.hip, operation by operation in fp32."""
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    poly = t * (t * (t * (t * (t * 1.061405429 + -1.453152027) + 1.421413741) + -0.284496736) + 0.254829592)
    tail = poly * torch.exp2(-z * z * 1.4426950408889634)
    return 0.5 * x * torch.where(x >= 0, 2.0 - tail, tail)


def _act32(form, x, d: Defect):
    if form.endswith("quickgelu_t"):
        cc = torch.tensor(-1.7 if d.quickgelu_17 else -1.702, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        return x * (1.0 / (1.0 + torch.exp2(cc.to(x.device) * x)))
    if form in ("gelu_t", "gelu_mix_t"):
        if d.tanh_gelu:
            return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
        return _gelu_erf32(x)
    return x


def emulate(c: Case, defect: Defect = NO_DEFECT, bm: int = 128) -> Dict[str, torch.Tensor]:
    """The kernels' arithmetic in torch fp32: accumulation in 32-wide k-steps, the epilogues as written (the A-S polynomial, the exp2 /
    reciprocal forms, ln_finalize, the integer join / delta), RNE packing; returns the output windows (fresh tensors, starting from
    what the buffers hold now: a row or group that is not stored keeps it)."""
    d, b = defect, c.buf
    M, N, K = c.M, c.N, c.K
    dev = b["A"].win.device
    Bw = b["B"].win.float()

    def accumulate(Aw):
        acc = torch.zeros((M, N), dtype=torch.float32, device=dev)
        steps = list(range(0, K, 32))
        if d.drop_last_kstep:
            steps = steps[:-1]
        if d.first_kstep_twice:
            steps = [0] + steps
        for k0 in steps:
            acc = acc + Aw[:, k0:k0 + 32] @ Bw[:, k0:k0 + 32].T
        return acc

    acc = accumulate(b["A"].win.float())
    bias = b["bias"].win.view(-1).clone() if c.has_bias else torch.zeros(N, device=dev)
    if d.bias_other_half:
        n = torch.arange(N, device=dev)
        bias = bias[torch.where(n % 8 >= 4, n - 4, n)]
    bias = bias.view(1, N).expand(M, N).clone()
    if d.no_bias_on_ragged_tile and M % bm:
        bias[(M // bm) * bm:] = 0.0
    outs = c.windows()
    stats = None
    if c.fold:
        G = K // 64
        st = b["ln_stats"].win.view(M, G, 2)
        sx, sq = torch.zeros(M, device=dev), torch.zeros(M, device=dev)
        for i in range(G):
            sx, sq = sx + st[:, i, 0], sq + st[:, i, 1]
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
        mu = sx * inv
        var = (sq * inv - mu * mu).clamp_min(0.0)
        rstd = torch.rsqrt(var + c.ln_eps)
        nmr = (mu if d.mu_sign else -mu) * rstd
        cs = b["colsum"].win.view(-1)
        if d.colsum_next:
            cs = torch.roll(cs, -1)
        y = _act32(c.form, rstd[:, None] * acc + (nmr[:, None] * cs[None, :] + bias), d)
        res = _to_T(y, c.dtype, d.truncate)
    elif c.form == "gelu_mix_t":
        acc2 = acc if d.a2_is_a else accumulate(b["A2"].win.float())
        gt = b["gates"].win
        g0, g1 = (gt[:, 1:2], gt[:, 0:1]) if d.gates_swapped else (gt[:, 0:1], gt[:, 1:2])
        res = _to_T(g0 * _act32(c.form, acc + bias, d) + g1 * _act32(c.form, acc2 + bias, d), c.dtype, d.truncate)
    else:
        h = None
        if c.form in ("resid_f32", "resid_f32_ln"):
            h = b["C"].win.clone()
        elif c.form == "resid_t":
            h = (b["C"] if c.alias else b["resid"]).win.float()
        elif c.form == "resid_split_ln":
            lo = b["lo8"].win.to(torch.int32)
            if d.lo8_unsigned:
                lo = lo & 0xFF
            h = join64(b["C"].win, lo, c.dtype).float()
        if h is not None and d.resid_twice:
            r0 = 16 if M > 16 else 0
            h = h.clone()
            h[r0:r0 + 16] *= 2.0
        if c.form == "resid_split_ln":
            x = acc + (bias + h)
        elif h is not None:
            x = acc + (bias + h) if c.form != "resid_t" else acc + bias + h
        else:
            x = acc + bias
        y = _act32(c.form, x, d)
        res = _to_T(y, c.dtype, d.truncate) if c.form in OUT_T_FORMS else y
        if c.form in ("resid_f32_ln", "resid_split_ln"):
            src = _to_T(y, c.dtype).float() if d.stats_rounded else y
            sg = src.view(M, N // 64, 64)
            stats = torch.stack([sg.sum(-1), (sg * sg).sum(-1)], -1)
            if d.stats_neighbour_group and N // 64 >= 2:
                stats = stats[:, torch.arange(N // 64, device=dev) ^ 1]
            outs["stats_out"] = stats.view(M, 2 * (N // 64))
        if c.form == "resid_f32_ln":
            outs["x16"] = _to_T(y, c.dtype, d.truncate)
        if c.form == "resid_split_ln":
            l8 = delta8(y, res, c.dtype)
            if d.lo8_plus_one:
                l8 = (l8 + 1).clamp(-128, 127)
            outs["lo8"] = l8.to(torch.int8)
    # ---- the stores
    before = outs["C"]
    C = before.clone()
    cols = slice(0, 8) if d.one_group else slice(0, N)
    rm = b["row_map"].win.view(-1).long() if "row_map" in b else torch.arange(M, device=dev)
    C[rm] = res.to(C.dtype)
    if d.row_map_next and "row_map" in b and M >= 2:
        r = min(5, M - 2)                                   # row r goes where row r + 1 belongs; its own place is not written
        C[rm[r], cols] = before[rm[r], cols]
        C[rm[r + 1], cols] = res[r, cols].to(C.dtype)
    if d.tail_row_stored_twice and M >= 2:
        C[rm[M - 2], cols] = res[M - 1, cols].to(C.dtype)
    if d.last_row_group_unwritten:
        C[rm[M - 1], 0:8] = before[rm[M - 1], 0:8]
    outs["C"] = C
    return outs
