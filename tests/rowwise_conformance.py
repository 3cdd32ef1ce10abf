"""Element-wise conformance of the front end (``slime_patch_embed_prenorm``), the row kernels (``slime_layernorm``, the three gate
kernels) and ``slime_rope``: float64 references on the operands as the kernels receive them, DERIVED per-element bounds, torch fp32
restatements of the kernels' arithmetic (``emulate_*``), deliberately broken variants of those restatements, and the padded /
poisoned buffers of the cases (``Padded`` of gemm_conformance.py).  Plain module (no fixtures, not a conftest); pure torch, works on
CPU and GPU tensors.  Used by test_rowwise_bound_cpu.py and test_gpu_rowwise_conformance.py.

Conventions (those of gemm_conformance.py): e = 2^-24 (fp32 unit roundoff), u = unit roundoff of T (2^-8 bf16, 2^-11 fp16), every
conversion to T is RNE.  A sum whose terms pass through at most L additions carries e L sum|terms|.  Every fp32 bound carries a
factor (1 + 2^-10) for second-order products.  A T output of an fp32 value y with bound dy:
                                                                     round_T = dy + u (|y| + dy) + g      (g: the subnormal grid)
Division and 1 / D are exact-rounded: the library is built without fast-math (hipcc divides fp32 correctly rounded by default) and
every supported D is a power of two.  ASSUMPTIONS (no document on hand states them; each is marked where it enters): rsqrtf, expf,
cosf and sinf are taken at 2 ulp -- a relative 4 e for rsqrtf / expf, an ABSOLUTE 4 e for cosf / sinf (|cos|, |sin| <= 1):
A_RSQRT = A_EXP = A_TRIG = 4, as the GEMM bound does for v_exp_f32.  For RoPE that allowance is three orders below u either way.

(A) Two-pass LayerNorm of a row x (exact, float64) that the kernel holds with a per-element error dx (0 for slime_layernorm, the
    accumulation term for the front end), sums of depth L:  mu = mean x, d = x - mu, var = mean d^2, v = var + eps, rstd = v^-1/2,
    z = d rstd, y = z w + b.
      d_mu  = mean dx + e L mean|x|
      a_i   = dx_i + d_mu                      (error of x_i - mean before the subtraction's own rounding),   dd_i = a_i + e |d_i|
      var   : sum (d_i + a_i)^2 / D - var = 2 mean(d_i dx_i) + mean a_i^2  (the mean's error drops out of the first order: sum d_i = 0)
              A = 2 mean(|d| dx) + mean a^2;  roundings: 2 e per square, e L for the chain, e for the fma with eps:
      d_var = A + e (L + 3) (var + A) + e v
      eps_r = d_var / (2 (v - d_var)) + A_RSQRT e                                   (relative error of rstd)
      dz    = rstd dd + |z| (eps_r + e),       dy = |w| dz + e |y|                   (product, then the fma with w and b)
    A one-pass variance E[x^2] - mu^2 carries e mu^2 instead and leaves this bound once |mu| >> sigma.
    slime_layernorm: L = D / 64 + 6 (D / 64 values per lane, six butterfly levels).  out_f32: dy.  out_t: round_T(y, dy).
    out_t2 = T(y + add[row % add_period]): one fp32 addition, dy2 = dy + e |y + add|, then round_T.  normalize = 0: bit-equal casts
    (out_t2: T of the single fp32 sum).
(B) Front end, patch rows: x = sum_k px_k w_k + pos, the kreal = 3 patch^2 products of two T operands exact in fp32, one rounding
    per accumulated product and one for the position row: dx = e (kreal + 1) (sum|px_k w_k| + |pos|); then (A) with
    L = CW / 4 + 2 + NW (a lane's CW / 4 values in turn, two lane swaps, NW waves in order; CW = D / NW columns per wave).
    Class-token row (the simpler one): x = cls + pos[0], dx = e |x|, L = D / 64 + 6.
    x16 must be T(h) and lo8 the byte of the header's definition for the h the kernel stored, both bit for bit.
    stats: per 64 columns the sum and the sum of squares of the ROUNDED row (the stored x16, exact in float64); 16 values per lane in
    turn and two lane swaps (the class row: at most 4 values and 5 butterfly levels): depth 18, and one rounding per fma:
      d_sum = 18 e sum|r|,   d_sumsq = 19 e sum r^2
(C) Gates: l_j = sum_c x_c w_cj in fp32: dl_j = e (D + 2) sum|x_c w_cj| (product, chain, butterfly).  Delta = |l_0 - l_1|,
    d_Delta = dl_0 + dl_1 + e Delta.  p_big = expf(0), p_small = expf(-Delta): the ratio p_small / p_big carries
    eps_p = expm1(d_Delta) + 2 A_EXP e -- and nothing where Delta = 0 and d_Delta = 0 (both logits exact, e.g. a zero row: the same
    function of the same argument twice) -- plus an absolute 2^-126 (expf flushes below fp32's normal range; the fully saturated
    case Delta > 104, where one expf is exactly 0, is this term).  s_j = p_j / (p_0 + p_1):
      ds_j  = s_0 s_1 eps_p + 2^-126 + 2 e s_j                                       (sum and division)
    s_0 + s_1 is (p_0 + p_1) / fl(p_0 + p_1) up to the two divisions: 1 +- 3 e whatever the p are; its own sum and the + 1e-6f:
      d_den = 5 e den,  den = 1 + 1e-6f;     g_j = s_j / den:   dg_j = ds_j / den + g_j (d_den / den + e)
    slime_gate_weights stores g (bound dg).  The mixes y = g_0 a + g_1 b: dy = dg_0 |a| + dg_1 |b| + 3 e (|g_0 a| + |g_1 b|); fp32 out:
    dy, T out: round_T(y, dy).
(D) RoPE.  The angle is DEFINED as the fp32 product float(pos) * inv_freq[i] (HF's arithmetic; torch's fp32 multiply gives the same
    bits); the reference takes cos / sin of that fp32 number in float64.  out = (x c -+ y s) sc: the two table values (A_TRIG e
    each, absolute), two products, the difference, the scale:
      d = |sc| (A_TRIG + 3) e (|x| + |y|),   then round_T.   pos = 0: cos = 1 and sin = 0 exactly: q = T(x sc), k = x bit for bit.
None of these constants was fitted to a kernel's output; test_rowwise_bound_cpu.py checks that every ``emulate_*`` stays inside and
that every mutant leaves its bound.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

import gemm_conformance as GC
from gemm_conformance import E32, FLUSH32, SUBNORMAL, UNIT, Padded, SENTINEL_BYTE   # noqa: F401  (re-exported for the tests)

A_RSQRT = A_EXP = A_TRIG = 4.0            # ASSUMED: 2 ulp (module docstring)
SLACK = 1 + 2.0 ** -10
C6 = float(torch.tensor(1e-6, dtype=torch.float32))        # the kernels' 1e-6f
STATS_DEPTH = 18
DTYPES = (torch.bfloat16, torch.float16)
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "f32"}
PE_ROWS = 48                              # csrc/patch_embed.hip: rows per workgroup
LDS_LIMIT = 160 * 1024


def round_T(y, dy, dtype):
    return dy * SLACK + UNIT[dtype] * (y.abs() + dy) + SUBNORMAL[dtype]


def check(name: str, got, want, bd) -> Tuple[float, Optional[str]]:
    """(worst |err| / bound, message or None) of one output against its reference, element by element."""
    ratio, ex, idx, g, w, b = GC.worst(got, want, bd)
    if ex > 0:
        return ratio, f"{name}: worst element at {idx}: got {g!r}, want {w!r}, bound {b:.3e}, excess {ex:.3e}, |err| / bound {ratio:.3f}"
    return ratio, None


def bits_equal(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def first_diff(a, b):
    d = (a.contiguous().view(torch.uint8).view(a.shape + (-1,)) != b.contiguous().view(torch.uint8).view(b.shape + (-1,))).any(-1).nonzero()
    return tuple(int(v) for v in d[0]) if len(d) else None


# ================================================================================================ (A) two-pass LayerNorm
def ln_bound(x, dx, L: int, w, b, eps: float):
    """Term (A): x [.., D] float64, dx its per-element error (tensor or 0.0), sums of depth L -> (y, dy), float64."""
    dx = dx if torch.is_tensor(dx) else torch.full_like(x, float(dx))
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).mean(-1, keepdim=True)
    d_mu = dx.mean(-1, keepdim=True) + E32 * L * x.abs().mean(-1, keepdim=True)
    a = dx + d_mu
    A = 2 * (d.abs() * dx).mean(-1, keepdim=True) + (a * a).mean(-1, keepdim=True)
    v = var + eps
    d_var = A + E32 * (L + 3) * (var + A) + E32 * v
    eps_r = d_var / (2 * (v - d_var).clamp_min(1e-300)) + A_RSQRT * E32
    rstd = v.rsqrt()
    z = d * rstd
    y = z * w + b
    dz = rstd * (a + E32 * d.abs()) + z.abs() * (eps_r + E32)
    return y, (w.abs() * dz + E32 * y.abs()) * SLACK


def ln32(x, w, b, eps, one_pass=False, eps_outside=False):
    """The kernels' LayerNorm in torch fp32: mean, d = x - mean, rsqrt(mean d^2 + eps), (d rstd) w + b."""
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) * (1.0 / D)
    d = x - mean
    var = ((x * x).sum(-1, keepdim=True) * (1.0 / D) - mean * mean).clamp_min(0.0) if one_pass else (d * d).sum(-1, keepdim=True) * (1.0 / D)
    rstd = 1.0 / (var.sqrt() + eps) if eps_outside else torch.rsqrt(var + eps)
    return (d * rstd) * w + b


# ================================================================================================ (B) the front end
@dataclass(frozen=True)
class Geom:
    image: int
    patch: int
    D: int

    @property
    def g(self):
        return self.image // self.patch

    @property
    def P(self):
        return self.g * self.g

    @property
    def S(self):
        return self.P + 1

    @property
    def kreal(self):
        return 3 * self.patch * self.patch

    @property
    def kpad(self):
        return (self.kreal + 63) // 64 * 64

    @property
    def nw(self):
        return {128: 2, 256: 4, 1024: 8}[self.D]

    @property
    def name(self):
        return f"{self.image}/{self.patch}/{self.D}"

    def config(self, layers: int = 3):
        from slime_amd.weights import VisionConfig
        return VisionConfig(hidden_size=self.D, intermediate_size=4 * self.D, num_hidden_layers=layers, num_attention_heads=self.D // 64,
                            image_size=self.image, patch_size=self.patch)


def fe_lds_bytes(image: int, patch: int, kpad: int, D: int) -> int:
    """slime_patch_embed_geometry's formula: staged image rows + X[48][kpad + 8] + the offset table + the cross-wave sums."""
    a16 = lambda n: (n + 15) // 16 * 16
    nw = {128: 2, 256: 4, 1024: 8}[D]
    return a16(6 * patch * image * 2) + PE_ROWS * (kpad + 8) * 2 + a16(kpad * 2) + nw * PE_ROWS * 4


# geometry -> LDS bytes (the issue's table; test_rowwise_bound_cpu.py checks the formula against it)
GEOMETRIES = {Geom(336, 14, 1024): 121472, Geom(224, 14, 1024): 102656, Geom(168, 14, 256): 92480, Geom(112, 14, 128): 82688,
              Geom(56, 14, 128): 73280, Geom(112, 16, 256): 98304, Geom(120, 8, 128): 31488, Geom(384, 16, 1024): 151296}
SMALL_GEOMETRIES = (Geom(56, 14, 128), Geom(112, 16, 256), Geom(120, 8, 128), Geom(112, 14, 128))
FE_KINDS = ("random", "offset", "constant")
_PRE = "vision_model."


def fe_inputs(geom: Geom, kind: str, n: int, seed: int):
    """(state dict of W.make_tower_state_dict, fp32 pixels [n, 3, image, image]).  "offset": the position table + 60 and the pixels
    + 0.5, so that every row has |mu| >= 10 sigma (about 100: fe_reference's caller asserts it); "constant": the LAST crop is one
    value, so its patch rows differ by the position table alone."""
    from slime_amd import weights as W
    assert kind in FE_KINDS
    sd = W.make_tower_state_dict(geom.config(layers=1), seed=seed)
    px = W.synthetic_pixels(n, seed=seed + 1, image_size=geom.image)
    if kind == "offset":
        sd[_PRE + "embeddings.position_embedding.weight"] = sd[_PRE + "embeddings.position_embedding.weight"] + 60.0
        px = px + 0.5
    if kind == "constant":
        px[-1] = 0.75
    return sd, px


def _fe_operands(sd, geom: Geom, dtype, dev):
    g = lambda k: sd[_PRE + k].detach().to(dev)
    w = g("embeddings.patch_embedding.weight").float().reshape(geom.D, geom.kreal).to(dtype)
    return (w, g("embeddings.class_embedding").float(), g("embeddings.position_embedding.weight").float(), g("pre_layrnorm.weight").float(),
            g("pre_layrnorm.bias").float())


def _patches(px, geom: Geom):
    """[n, P, kreal], k = (c, ky, kx): the order of Conv2d.weight.flatten(1)."""
    return F.unfold(px, geom.patch, stride=geom.patch).transpose(1, 2).contiguous()


@dataclass
class FeRef:
    h: torch.Tensor                 # [n S, D] float64
    dh: torch.Tensor
    x: torch.Tensor                 # the LayerNorm's input rows (float64)
    n: int
    geom: Geom


def fe_reference(sd, geom: Geom, px, dtype, eps: float = 1e-5) -> FeRef:
    """float64 on the T pixels (fp32 pixels are rounded to T on the way in: that rounding is part of the definition) and the T weight."""
    dev = px.device
    w, cls, pos, lw, lb = _fe_operands(sd, geom, dtype, dev)
    A = _patches(px.to(dtype).double(), geom)
    w, cls, pos, lw, lb = w.double(), cls.double(), pos.double(), lw.double(), lb.double()
    n, D = px.shape[0], geom.D
    conv, Sabs = A @ w.T, A.abs() @ w.abs().T
    xp = conv + pos[1:]
    dxp = E32 * (geom.kreal + 1) * (Sabs + pos[1:].abs())
    xc = (cls + pos[0]).view(1, 1, D).expand(n, 1, D)
    yp, dyp = ln_bound(xp, dxp, geom.D // geom.nw // 4 + 2 + geom.nw, lw, lb, eps)
    yc, dyc = ln_bound(xc, E32 * xc.abs(), D // 64 + 6, lw, lb, eps)
    S = geom.S
    return FeRef(torch.cat([yc, yp], 1).reshape(n * S, D), torch.cat([dyc, dyp], 1).reshape(n * S, D), torch.cat([xc, xp], 1).reshape(n * S, D), n, geom)


@dataclass(frozen=True)
class FeDefect:
    k_kx_ky: bool = False              # k ordered (c, kx, ky)
    patch_row_16: bool = False         # patch row of workgroup row r taken as r / 16 instead of r / g
    pos_prev: bool = False             # position row t - 1
    cls_no_pos: bool = False           # class row without position 0
    one_pass: bool = False             # variance as E[x^2] - mu^2
    stats_unrounded: bool = False
    pixels_unrounded: bool = False     # fp32 pixels enter the product as they are


FE_MUTANTS = {"k_ordered_c_kx_ky": FeDefect(k_kx_ky=True), "patch_row_r_over_16": FeDefect(patch_row_16=True),
              "position_row_t_minus_1": FeDefect(pos_prev=True), "class_row_without_position_0": FeDefect(cls_no_pos=True),
              "one_pass_variance": FeDefect(one_pass=True), "stats_of_the_unrounded_row": FeDefect(stats_unrounded=True),
              "pixels_not_rounded_to_T": FeDefect(pixels_unrounded=True)}


def stats_of(rows32, D):
    r = rows32.view(-1, D // 64, 64)
    return torch.stack([r.sum(-1), (r * r).sum(-1)], -1)


def emulate_fe(sd, geom: Geom, px, dtype, eps: float = 1e-5, defect: FeDefect = FeDefect()) -> Dict[str, torch.Tensor]:
    """The kernel's arithmetic in torch fp32: T pixels x T weight accumulated in 32-wide k-steps, + position row, two-pass LayerNorm,
    T(h), the byte, the partial sums of the rounded row."""
    d, dev = defect, px.device
    w, cls, pos, lw, lb = _fe_operands(sd, geom, dtype, dev)
    w = w.float()
    n, D, g, p = px.shape[0], geom.D, geom.g, geom.patch
    A = _patches(px.float() if d.pixels_unrounded else px.to(dtype).float(), geom)
    if d.k_kx_ky:
        A = A.view(n, geom.P, 3, p, p).transpose(-1, -2).reshape(n, geom.P, geom.kreal)
    if d.patch_row_16:
        py, pxx = torch.arange(geom.P, device=dev) // g, torch.arange(geom.P, device=dev) % g
        prow0 = py // 2 * 2
        nprow = (g - prow0).clamp_max(2)
        pr = torch.minimum(((py - prow0) * g + pxx) // 16, nprow - 1)
        A = A[:, (prow0 + pr) * g + pxx]
    acc = torch.zeros((n, geom.P, D), dtype=torch.float32, device=dev)
    for k0 in range(0, geom.kreal, 32):
        acc = acc + A[..., k0:k0 + 32] @ w[:, k0:k0 + 32].T
    xp = acc + (pos[:-1] if d.pos_prev else pos[1:])
    xc = (cls if d.cls_no_pos else cls + pos[0]).view(1, 1, D).expand(n, 1, D)
    h = torch.cat([ln32(xc, lw, lb, eps, d.one_pass), ln32(xp, lw, lb, eps, d.one_pass)], 1).reshape(n * geom.S, D).contiguous()
    x16 = h.to(dtype)
    return {"h": h, "x16": x16, "lo8": GC.delta8(h, x16, dtype).to(torch.int8), "stats": stats_of(h if d.stats_unrounded else x16.float(), D)}


def fe_check(ref: FeRef, outs: Dict[str, torch.Tensor], dtype):
    """h inside the bound (class rows and patch rows reported apart), x16 = T(h) and lo8 = the header's byte for the stored h bit for
    bit, stats inside their own bound.  -> ({"h": ratio, "h_cls": ratio, "stats": ratio}, message or None)"""
    S, D = ref.geom.S, ref.geom.D
    h = outs["h"]
    is_cls = torch.zeros(ref.n * S, dtype=torch.bool, device=h.device)
    is_cls[::S] = True
    ratios = {}
    for key, sel in (("h_cls", is_cls), ("h", ~is_cls)):
        ratios[key], msg = check(f"{key} ({ref.geom.name})", h[sel], ref.h[sel], ref.dh[sel])
        if msg:
            return ratios, msg + f" [row index within the selected rows; S = {S}]"
    if "x16" in outs and outs["x16"] is not None:
        if not bits_equal(outs["x16"], h.to(dtype)):
            return ratios, f"x16 is not T(h) bit for bit, first at {first_diff(outs['x16'], h.to(dtype))}"
    if outs.get("lo8") is not None:
        want = GC.delta8(h, h.to(dtype), dtype).to(torch.int8)
        if not bits_equal(outs["lo8"], want):
            return ratios, f"lo8 is not the header's byte of the stored h, first at {first_diff(outs['lo8'], want)}"
    if outs.get("stats") is not None:
        r = outs["x16"].double().view(ref.n * S, D // 64, 64)
        want = torch.stack([r.sum(-1), (r * r).sum(-1)], -1)
        bd = torch.stack([STATS_DEPTH * E32 * r.abs().sum(-1), (STATS_DEPTH + 1) * E32 * (r * r).sum(-1)], -1) * SLACK
        ratios["stats"], msg = check(f"stats ({ref.geom.name})", outs["stats"].view(ref.n * S, D // 64, 2), want, bd)
        if msg:
            return ratios, msg
    return ratios, None


def fe_mu_over_sigma(ref: FeRef) -> float:
    """min over the rows of |mu| / sigma of the LayerNorm's input."""
    return float((ref.x.mean(-1).abs() / ref.x.std(-1, unbiased=False).clamp_min(1e-300)).min())


# ================================================================================================ slime_layernorm
LN_KINDS = ("random", "offset", "constant", "spike")
LN_SUBSETS = (("out_f32",), ("out_t",), ("out_t", "out_t2"), ("out_f32", "out_t", "out_t2"))


@dataclass
class LnCase:
    D: int
    dtype: torch.dtype
    rows: int
    ldx: int
    kind: str
    outputs: Tuple[str, ...]
    add_period: int
    normalize: bool
    eps: float
    buf: Dict[str, Padded]
    snaps: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def has_add(self):
        return "add" in self.buf

    def what(self):
        return (f"layernorm {DT_ID[self.dtype]} D={self.D} rows={self.rows} ldx={self.ldx} {self.kind} outputs={'+'.join(self.outputs)} "
                f"add_period={self.add_period if self.has_add else None} normalize={int(self.normalize)}")

    def snapshot(self):
        self.snaps = {k: self.buf[k].snapshot() for k in self.outputs}

    def windows(self):
        return {k: self.buf[k].win.clone() for k in self.outputs}

    def intact(self):
        for k in self.outputs:
            if not self.buf[k].intact(self.snaps[k]):
                return k
        return None

    def add_rows(self):
        return self.buf["add"].win[torch.arange(self.rows, device=self.buf["x"].win.device) % self.add_period]


def make_ln_case(D, dtype, rows, ldx, kind="random", outputs=("out_f32", "out_t", "out_t2"), add_period=1, normalize=True, with_add=None,
                 eps=1e-5, seed=0, device="cpu") -> LnCase:
    """Padded, poisoned buffers for one slime_layernorm call: x with row stride ldx (NaN between the rows, behind them and in front),
    w / b / add followed by NaN, every output all sentinel bytes with three guard rows.  "offset": |mu| = 100 sigma; "constant":
    every row one value (variance 0: rstd = eps^-1/2); "spike": one element 1e4 per row."""
    assert kind in LN_KINDS and ldx >= D
    g = torch.Generator(device=device).manual_seed(7919 * seed + 31 * rows + D)
    x = torch.randn(rows, D, generator=g, device=device)
    if kind == "random":
        x = 3.0 * x + 0.7
    elif kind == "offset":
        x = x + 100.0 * (1 - 2 * (torch.arange(rows, device=device) % 2)).float()[:, None]
    elif kind == "constant":
        x = (1.5 + torch.arange(rows, device=device).float())[:, None].expand(rows, D) * (1 - 2 * (torch.arange(rows, device=device) % 2)).float()[:, None]
    else:
        x[torch.arange(rows, device=device), (torch.arange(rows, device=device) * 37 + 5) % D] = 1.0e4
    nan = math.nan
    buf = {"x": Padded(rows, D, torch.float32, device, pad_cols=ldx - D).fill(x, nan),
           "w": Padded(1, D, torch.float32, device, pad_cols=0, guard_rows=0, tail=GC.TAIL).fill((1 + 0.1 * torch.randn(D, generator=g, device=device)).view(1, D), nan),
           "b": Padded(1, D, torch.float32, device, pad_cols=0, guard_rows=0, tail=GC.TAIL).fill((0.1 * torch.randn(D, generator=g, device=device)).view(1, D), nan)}
    if with_add is None:
        with_add = "out_t2" in outputs
    if with_add:
        buf["add"] = Padded(add_period, D, torch.float32, device, pad_cols=0).fill(torch.randn(add_period, D, generator=g, device=device), nan)
    for k in outputs:
        buf[k] = Padded(rows, D, torch.float32 if k == "out_f32" else dtype, device, pad_cols=0)
    c = LnCase(D, dtype, rows, ldx, kind, tuple(outputs), add_period, normalize, eps, buf)
    c.snapshot()
    return c


def ln_reference(c: LnCase):
    """-> {output: (float64 reference, bound)}; normalize = 0: the bounds are 0 (bit-equal casts, ln_check compares the bits)."""
    x = c.buf["x"].win.double()
    if c.normalize:
        y, dy = ln_bound(x, 0.0, c.D // 64 + 6, c.buf["w"].win.double(), c.buf["b"].win.double(), c.eps)
    else:
        y, dy = x, torch.zeros_like(x)
    out = {"out_f32": (y, dy), "out_t": (y, round_T(y, dy, c.dtype) if c.normalize else dy)}
    if c.has_add:
        y2 = y + c.add_rows().double()
        out["out_t2"] = (y2, round_T(y2, dy + E32 * y2.abs(), c.dtype) if c.normalize else dy)
    return {k: out[k] for k in c.outputs}


@dataclass(frozen=True)
class LnDefect:
    one_pass: bool = False
    add_row_not_wrapped: bool = False      # add row taken row % rows: past add_period the last row is what a flat table gives
    eps_outside: bool = False              # 1 / (sqrt(var) + eps)


LN_MUTANTS = {"one_pass_variance": LnDefect(one_pass=True), "add_row_modulo_rows": LnDefect(add_row_not_wrapped=True),
              "eps_outside_the_square_root": LnDefect(eps_outside=True)}


def emulate_ln(c: LnCase, defect: LnDefect = LnDefect()) -> Dict[str, torch.Tensor]:
    x = c.buf["x"].win.clone()
    y = ln32(x, c.buf["w"].win, c.buf["b"].win, c.eps, defect.one_pass, defect.eps_outside) if c.normalize else x
    outs = {"out_f32": y, "out_t": y.to(c.dtype)}
    if c.has_add:
        r = torch.arange(c.rows, device=x.device)
        idx = (r % c.rows).clamp_max(c.add_period - 1) if defect.add_row_not_wrapped else r % c.add_period
        outs["out_t2"] = (y + c.buf["add"].win[idx]).to(c.dtype)
    return {k: outs[k] for k in c.outputs}


def ln_check(c: LnCase, ref, outs):
    """-> ({output: ratio}, message or None)"""
    ratios = {}
    for k in c.outputs:
        want, bd = ref[k]
        if not c.normalize:
            exp = want.float() if k == "out_f32" else (c.buf["x"].win + c.add_rows()).to(c.dtype) if k == "out_t2" else c.buf["x"].win.to(c.dtype)
            if not bits_equal(outs[k], exp):
                return ratios, f"{k}: normalize = 0 is a cast, bit for bit; first difference at {first_diff(outs[k], exp)}"
            ratios[k] = 0.0
            continue
        ratios[k], msg = check(k, outs[k], want, bd)
        if msg:
            return ratios, msg
    return ratios, None


# ================================================================================================ (C) gates
GATE_KINDS = ("random", "equal", "saturated")
SCATTER = (3, 7, 2)                       # rows_per_group, group_stride, row0 of the scatter form


def gate_inputs(D, rows, kind, seed, device):
    """x [rows, D], w_gate [D, 2].  "equal": the two columns of w_gate identical, and row 0 of x zero (both logits exactly 0);
    "saturated": |l_0 - l_1| > 200 on every row, the sign alternating by row."""
    assert kind in GATE_KINDS
    g = torch.Generator(device=device).manual_seed(104729 * seed + 131 * D + rows)
    x = torch.randn(rows, D, generator=g, device=device)
    wg = 0.2 * torch.randn(D, 2, generator=g, device=device)
    if kind == "equal":
        wg[:, 1] = wg[:, 0]
        x[0] = 0.0
    if kind == "saturated":
        sg = (1 - 2 * (torch.arange(D, device=device) % 2)).float()
        wg = torch.stack([sg, -sg], 1)
        x = (2.0 + x.abs()) * sg[None, :] * (1 - 2 * (torch.arange(rows, device=device) % 2)).float()[:, None]
    return x, wg


def gate_reference(x, wg):
    """float64 gates [rows, 2] and their bound dg (term C)."""
    D = x.shape[1]
    x, wg = x.double(), wg.double()
    l = x @ wg
    dl = E32 * (D + 2) * (x.abs() @ wg.abs())
    delta = (l[:, 0] - l[:, 1]).abs()
    d_delta = dl.sum(1) + E32 * delta
    eps_p = torch.where((delta == 0) & (d_delta == 0), torch.zeros_like(delta), torch.expm1(d_delta) + 2 * A_EXP * E32)
    p = torch.exp(-delta)
    s_big, s_small = 1 / (1 + p), p / (1 + p)
    first_big = (l[:, 0] >= l[:, 1])
    s = torch.stack([torch.where(first_big, s_big, s_small), torch.where(first_big, s_small, s_big)], 1)
    ds = (s_big * s_small * eps_p)[:, None] + FLUSH32 + 2 * E32 * s
    den = 1.0 + C6
    gts = s / den
    dg = (ds / den + gts * (5 * E32 + E32)) * SLACK
    assert float(delta.max()) < 1e30
    return gts, dg, delta


def mix_reference(gts, dg, a, b, out_dtype):
    """y = g_0 a + g_1 b and its bound (fp32 or T output)."""
    a, b = a.double(), b.double()
    t0, t1 = gts[:, :1] * a, gts[:, 1:] * b
    y = t0 + t1
    dy = (dg[:, :1] * a.abs() + dg[:, 1:] * b.abs() + 3 * E32 * (t0.abs() + t1.abs())) * SLACK
    return y, (dy if out_dtype == torch.float32 else round_T(y, dy, out_dtype))


@dataclass(frozen=True)
class GateDefect:
    no_renorm: bool = False
    swapped: bool = False
    eps_in_softmax: bool = False          # g_j = p_j / (p_0 + p_1 + 1e-6): the 1e-6 inside the softmax's denominator


GATE_MUTANTS = {"renormalisation_dropped": GateDefect(no_renorm=True), "gates_swapped": GateDefect(swapped=True),
                "1e-6_inside_the_softmax_denominator": GateDefect(eps_in_softmax=True)}


def emulate_gates(x, wg, defect: GateDefect = GateDefect()):
    """gate_mix_kernel's gate arithmetic in torch fp32 -> [rows, 2]."""
    l = x.float() @ wg.float()
    m = l.max(1, keepdim=True).values
    p = torch.exp(l - m)
    ps = p[:, :1] + p[:, 1:]
    c6 = torch.tensor(1e-6, dtype=torch.float32, device=x.device)
    if defect.eps_in_softmax:
        g = p / (ps + c6)
    else:
        s = p / ps
        g = s if defect.no_renorm else s / (s[:, :1] + s[:, 1:] + c6)
    return g.flip(1) if defect.swapped else g


def emulate_mix(g32, a, b, out_dtype):
    return (g32[:, :1] * a.float() + g32[:, 1:] * b.float()).to(out_dtype)


def scatter_rows(rows, form=SCATTER):
    """(output row of every input row, number of output rows) of slime_gate_mix_ex's grouped scatter."""
    rpg, stride, row0 = form
    r = torch.arange(rows)
    return (r // rpg) * stride + row0 + r % rpg, ((rows - 1) // rpg) * stride + row0 + rpg + 2


# ================================================================================================ copies (index arithmetic only)
def merge_dst(nw: int, nh: int, g: int, merge: bool) -> torch.Tensor:
    """Output row of input row r = (crop k, qy, qx) of slime_merge_rows_batched (llava_arch's spatial merge)."""
    r = torch.arange(nw * nh * g * g)
    if not merge:
        return r
    qx, qy, k = r % g, (r // g) % g, r // (g * g)
    return ((k // nw * g + qy) * nw + k % nw) * g + qx


def select_crops_index(period, first, per_image, images) -> torch.Tensor:
    j = torch.arange(images * per_image)
    return (j // per_image) * period + first + j % per_image


# ================================================================================================ (D) RoPE
ROPE_POS = (0, 1, 4095, 4096, 8191, 131071)
ROPE_THETA = 5.0e5


def rope_inv_freq(theta: float = ROPE_THETA, device="cpu"):
    return (1.0 / (theta ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128))).to(device)


@dataclass
class RopeCase:
    dtype: torch.dtype
    n_rot: int
    n_q: int
    rows: int
    row_stride: int
    q_scale: float
    buf: Dict[str, Padded]
    before: torch.Tensor               # the qkv window beforehand
    snap: torch.Tensor

    def what(self):
        return f"rope {DT_ID[self.dtype]} n_rot={self.n_rot} n_q={self.n_q} rows={self.rows} row_stride={self.row_stride} pos={self.buf['pos'].win.view(-1).tolist()}"


def make_rope_case(dtype, n_rot, n_q, rows, extra, pos, q_scale=0.08838834764831845 * 1.4426950408889634, seed=0, device="cpu") -> RopeCase:
    """qkv rows of n_rot * 128 rotated elements followed by ``extra`` elements of v / padding (row_stride = n_rot * 128 + extra): the
    whole window random, everything around it sentinel; pos int32 per row; inv_freq followed by NaN."""
    g = torch.Generator(device=device).manual_seed(1543 * seed + 17 * n_rot + rows)
    stride = n_rot * 128 + extra
    assert len(pos) == rows
    buf = {"qkv": Padded(rows, stride, dtype, device, pad_cols=0).fill(torch.randn(rows, stride, generator=g, device=device)),
           "pos": Padded(rows, 1, torch.int32, device, pad_cols=0).fill(torch.tensor(pos, dtype=torch.int32, device=device).view(rows, 1)),
           "inv_freq": Padded(1, 64, torch.float32, device, pad_cols=0, guard_rows=0, tail=GC.TAIL).fill(rope_inv_freq(device=device).view(1, 64), math.nan)}
    q32 = float(torch.tensor(q_scale, dtype=torch.float32))
    return RopeCase(dtype, n_rot, n_q, rows, stride, q32, buf, buf["qkv"].win.clone(), buf["qkv"].snapshot())


def _rope_tables64(c: RopeCase):
    ang32 = c.buf["pos"].win.view(-1, 1).float() * c.buf["inv_freq"].win.view(1, 64)       # the DEFINED angle: an fp32 product
    return torch.cos(ang32.double()), torch.sin(ang32.double())


def rope_reference(c: RopeCase):
    """-> (float64 rotated part [rows, n_rot, 128], bound)."""
    x = c.before[:, :c.n_rot * 128].double().view(c.rows, c.n_rot, 2, 64)
    cs, sn = (t.view(c.rows, 1, 64) for t in _rope_tables64(c))
    sc = torch.ones(c.n_rot, dtype=torch.float64, device=x.device)
    sc[:c.n_q] = c.q_scale
    sc = sc.view(1, c.n_rot, 1)
    lo, hi = x[:, :, 0], x[:, :, 1]
    out = torch.stack([(lo * cs - hi * sn) * sc, (hi * cs + lo * sn) * sc], 2).reshape(c.rows, c.n_rot, 128)
    d = (sc.abs() * (A_TRIG + 3) * E32 * (lo.abs() + hi.abs())).repeat(1, 1, 2)
    return out, round_T(out, d, c.dtype)


@dataclass(frozen=True)
class RopeDefect:
    cs_prev: bool = False              # cs[i] used for element i + 1
    scale_k: bool = False              # q_scale applied to the k heads
    sign: bool = False                 # rotate-half sign flipped
    freq_half: bool = False            # frequency index i >> 1
    revolutions: bool = False          # the angle reduced as fp32 revolutions (the fast-math form)


ROPE_MUTANTS = {"cs_of_i_for_element_i_plus_1": RopeDefect(cs_prev=True), "q_scale_on_the_k_heads": RopeDefect(scale_k=True),
                "rotate_half_sign_flipped": RopeDefect(sign=True), "frequency_index_i_over_2": RopeDefect(freq_half=True),
                "angle_reduced_as_fp32_revolutions": RopeDefect(revolutions=True)}


def emulate_rope(c: RopeCase, defect: RopeDefect = RopeDefect()):
    """rope_kernel in torch fp32 -> the rotated part [rows, n_rot, 128] in T."""
    d = defect
    inv = c.buf["inv_freq"].win.view(64)
    i = torch.arange(64, device=inv.device)
    if d.freq_half:
        inv = inv[i >> 1]
    ang = c.buf["pos"].win.view(-1, 1).float() * inv.view(1, 64)
    if d.revolutions:
        r = ang * torch.tensor(0.15915494309189535, dtype=torch.float32, device=ang.device)
        ang = (r - torch.floor(r)) * torch.tensor(6.283185307179586, dtype=torch.float32, device=ang.device)
    cs, sn = torch.cos(ang), torch.sin(ang)
    if d.cs_prev:
        j = torch.where(i % 2 == 1, i - 1, i)
        cs, sn = cs[:, j], sn[:, j]
    cs, sn = cs.view(c.rows, 1, 64), sn.view(c.rows, 1, 64)
    if d.sign:
        sn = -sn
    x = c.before[:, :c.n_rot * 128].float().view(c.rows, c.n_rot, 2, 64)
    sc = torch.ones(c.n_rot, dtype=torch.float32, device=x.device)
    sc[:c.n_rot if d.scale_k else c.n_q] = c.q_scale
    sc = sc.view(1, c.n_rot, 1)
    lo, hi = x[:, :, 0], x[:, :, 1]
    return torch.stack([(lo * cs - hi * sn) * sc, (hi * cs + lo * sn) * sc], 2).reshape(c.rows, c.n_rot, 128).to(c.dtype)


def rope_check(c: RopeCase, got_rot):
    """got_rot: the rotated part after the call [rows, n_rot, 128] T.  Inside the bound everywhere; rows at pos = 0: q = T(x q_scale) and
    k = x, bit for bit.  -> (ratio, message or None)"""
    want, bd = rope_reference(c)
    ratio, msg = check("rope", got_rot, want, bd)
    if msg:
        return ratio, msg
    zero = (c.buf["pos"].win.view(-1) == 0)
    if bool(zero.any()):
        x = c.before[:, :c.n_rot * 128].view(c.rows, c.n_rot, 128)[zero]
        exp = x.clone()
        exp[:, :c.n_q] = (x[:, :c.n_q].float() * torch.tensor(c.q_scale, dtype=torch.float32, device=x.device)).to(c.dtype)
        if not bits_equal(got_rot[zero], exp):
            return ratio, f"pos = 0: q must be T(x q_scale) and k must be x bit for bit; first difference at {first_diff(got_rot[zero], exp)}"
    return ratio, None


# ================================================================================================ router scores (selection is exact)
ROUTER_T = (1, 2, 1023, 1024, 1025, 2048, 2049, 3073, 4096)
ROUTER_KINDS = ("tied", "blocks_of_7", "separated")
ROUTER_TOPP = (1e-4, 0.5, 0.95)


def router_scores(T: int, kind: str, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed * 7 + T)
    if kind == "tied":
        return torch.full((T,), 0.25)
    if kind == "blocks_of_7":
        levels = torch.linspace(-2, 2, (T + 6) // 7)[torch.randperm((T + 6) // 7, generator=g)]
        return levels.repeat_interleave(7)[:T][torch.randperm(T, generator=g)].contiguous()
    return torch.linspace(-4, 4, T)[torch.randperm(T, generator=g)].contiguous()


def router_expected(probs: torch.Tensor, topp: float) -> torch.Tensor:
    """The kept set (ascending) from the device's own probabilities: torch's STABLE descending sort, cumulative sum <= top-p, one more."""
    T = probs.numel()
    sp, si = torch.sort(probs, descending=True, stable=True)
    k = int((torch.cumsum(sp, 0) <= topp).sum())
    return (si[:k + 1] if k < T else torch.arange(T)).sort()[0]
