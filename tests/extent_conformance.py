"""Address-extent conformance: the same values handed to an entry point once in compact buffers and once laid out FAR -- strides,
row counts and tables whose byte extent passes 2^31 and 2^32 -- must give bit-equal outputs, and nothing outside the operands may be
written.  Plain module (no fixtures, not a conftest); pure torch.  Used by test_extent_bound_cpu.py (which proves, without a GPU,
that every case can see a truncated offset) and test_gpu_extent_conformance.py.

The placement rule
------------------
Every far operand of a call lives in ONE ``Arena``: a single uint8 device allocation filled with SENTINEL_BYTE (0x7B: 0x7B7B and
0x7B7B7B7B are finite numbers in every type used).  A window is a pointer into the arena plus the byte offsets of the operand's rows
from that pointer, as include/slime_hip.h's addressing formulas give them.
  * every pointer handed to the library sits at least LEAD = 2 GiB inside the arena, and the arena extends at least WRAP = 4 GiB
    (and past the operand's true extent) behind it: a byte offset truncated to 32 bits -- unsigned: offset mod 2^32, in [0, 2^32);
    signed: in [-2^31, 2^31) -- still lands inside the allocation.  Nothing here can leave it;
  * a wrapped READ then finds the sentinel or another row of the operand, whose values differ (the rows of every operand are random,
    hence distinct): wrong bits in the output, which is compared bit for bit with the compact run;
  * a wrapped WRITE lands on a guard byte or on another window: ``Arena.check_untouched`` copies the output windows out, overwrites
    every window with the sentinel and requires the WHOLE arena to equal the sentinel again.
The operands of one call are interleaved in the same address range (operand i starts SLOT bytes further into each 16 MiB row), so one
arena of about 11 GiB serves a call whose A, C, x16, resid and lo8 each span more than 4 GiB.

``cases()`` is the table: one row per (entry, operand, mechanism) with the shape, the strides and the byte offset of the last element
touched as a sum of products of Python ints.  ``truncations`` re-evaluates that sum with 32-bit products.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

SENTINEL_BYTE = 0x7B
GiB = 1 << 30
MiB = 1 << 20
LEAD = 2 * GiB                 # every pointer handed to the library: at least this far inside its arena
WRAP = 4 * GiB                 # ... and the arena goes on for at least this much behind it
TAIL = 64 * MiB                # what follows the farthest true extent
SLOT = 1 * MiB                 # operand i of a call starts i * SLOT bytes into the shared rows

GEMM_LD = 1 << 23              # the largest leading dimension slime_gemm_ex accepts for every K < lda (include/slime_hip.h)
GEMM_LD_REFUSED = 1 << 24      # 255 rows x 2^25 bytes: the 256-row tiles' 32-bit A offsets would wrap
GEMM_MAX_TILE_ROWS = 256


# ------------------------------------------------------------------------------------------------ layout of one operand
@dataclass
class Layout:
    """One operand of one call: ``ptr_off`` = the pointer handed to the library, as a byte offset from the arena's start; ``rows`` =
    byte offset of every row from that pointer (Python ints, from the header's formula); ``row_bytes`` = contiguous bytes per row.
    ``last`` = the formula of the last row's byte offset as a sum of products (tuple of factor tuples), for the CPU proof; ``far`` =
    the operand is one the case reaches the extent with; ``bulk`` = the rows are contiguous from the pointer on (row i at i * row_bytes)
    and too many to index one by one: the arena treats them as one span."""
    name: str
    ptr_off: int
    rows: List[int]
    row_bytes: int
    dtype: torch.dtype
    output: bool = False
    last: Tuple[Tuple[int, ...], ...] = ()
    far: bool = True
    bulk: bool = False

    @property
    def extent(self) -> int:
        """one past the farthest byte of the operand, from its pointer"""
        return max(self.rows) + self.row_bytes

    def row_at(self, off: int) -> Optional[int]:
        """index of the row whose bytes hold pointer-relative byte ``off``, or None"""
        for i, r in enumerate(self.rows):
            if r <= off < r + self.row_bytes:
                return i
        return None


def strided_rows(n: int, stride_bytes: int, first: int = 0) -> List[int]:
    return [first + i * stride_bytes for i in range(n)]


def _prod(factors: Sequence[int]) -> int:
    p = 1
    for f in factors:
        p *= f
    return p


def _wrap_u32(x: int) -> int:
    return x & 0xFFFFFFFF


def _wrap_i32(x: int) -> int:
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def true_offset(terms) -> int:
    return sum(_prod(t) for t in terms)


def truncations(terms) -> Dict[str, int]:
    """The byte offset ``sum of products`` as 32-bit code would compute it: every running product cut to 32 bits (unsigned / signed) and
    the sum kept wide ("u32 products", "i32 products"), or the sum cut as well ("u32", "i32")."""
    out = {}
    for name, cut in (("u32", _wrap_u32), ("i32", _wrap_i32)):
        total = 0
        for t in terms:
            p = 1
            for f in t:
                p = cut(p * f)
            total += p
        out[name + " products"] = total
        out[name] = cut(total)
    return out


# ------------------------------------------------------------------------------------------------ the arena
class Arena:
    """One uint8 allocation filled with the sentinel; windows are placed by ``Layout``; ``check_untouched`` returns the outputs and
    requires every byte outside the windows to be the sentinel still."""

    CHUNK = 1 * GiB

    def __init__(self, nbytes: int, device, lead: int = LEAD, wrap: int = WRAP):
        """``lead`` / ``wrap``: the placement rule's margins (smaller only in the CPU self-test of this class)"""
        assert nbytes % 16 == 0
        self.nbytes, self.lead, self.wrap = nbytes, lead, wrap
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.buf.fill_(SENTINEL_BYTE)
        self.windows: Dict[str, Layout] = {}

    def base(self) -> int:
        return self.buf.data_ptr()

    def ptr(self, name: str) -> int:
        return self.base() + self.windows[name].ptr_off

    def _span(self, lay: Layout) -> slice:
        assert lay.bulk and lay.rows[0] == 0 and lay.rows[-1] == (len(lay.rows) - 1) * lay.row_bytes
        return slice(lay.ptr_off, lay.ptr_off + lay.extent)

    def _index(self, lay: Layout):
        if lay.bulk:
            return self._span(lay)
        rows = torch.tensor([lay.ptr_off + r for r in lay.rows], dtype=torch.int64, device=self.buf.device)
        return (rows[:, None] + torch.arange(lay.row_bytes, dtype=torch.int64, device=self.buf.device)[None, :]).reshape(-1)

    def place(self, lay: Layout, values: Optional[torch.Tensor] = None) -> Layout:
        """Register the window (inside the arena, LEAD / WRAP respected, disjoint from every other window) and write ``values``
        ([rows, width] of lay.dtype) into it; without values the window keeps the sentinel (a pure output)."""
        assert lay.name not in self.windows
        assert lay.ptr_off >= self.lead and lay.ptr_off + max(self.wrap, lay.extent) <= self.nbytes, f"{lay.name}: placement rule"
        assert min(lay.rows) >= 0 and lay.ptr_off % 16 == 0
        self.windows[lay.name] = lay
        spans = sorted((w.ptr_off + r, w.ptr_off + r + (w.extent if w.bulk else w.row_bytes)) for w in self.windows.values()
                       for r in (w.rows[:1] if w.bulk else w.rows))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), f"{lay.name}: windows overlap"
        if values is not None:
            v = values.contiguous()                   # the bits as they are: lay.dtype only names the element size
            assert v.element_size() == lay.dtype.itemsize, (lay.name, v.dtype)
            assert v.shape[0] == len(lay.rows) and v[0].numel() * v.element_size() == lay.row_bytes, (lay.name, tuple(v.shape))
            self.buf[self._index(lay)] = v.view(torch.uint8).reshape(-1)
        return lay

    def read(self, name: str) -> torch.Tensor:
        """The window's rows as they are now: [rows, width] of the operand's dtype (a copy)."""
        lay = self.windows[name]
        got = self.buf[self._index(lay)]
        if lay.bulk:
            got = got.clone()                         # a slice is a view: the copy must survive the wipe of check_untouched
        return got.view(len(lay.rows), lay.row_bytes).view(lay.dtype)

    def view_bulk(self, name: str) -> torch.Tensor:
        """A bulk window IN PLACE ([rows, width], no copy: gone after check_untouched) -- for outputs of several GiB, which the caller
        compares first and then has wiped with ``check_untouched(copy_outputs=False)``."""
        lay = self.windows[name]
        return self.buf[self._span(lay)].view(len(lay.rows), lay.row_bytes).view(lay.dtype)

    def all_sentinel(self) -> bool:
        want = int.from_bytes(bytes([SENTINEL_BYTE]) * 8, "little")
        for lo in range(0, self.nbytes, self.CHUNK):
            hi = min(lo + self.CHUNK, self.nbytes)
            n8 = (hi - lo) // 8 * 8
            if not bool((self.buf[lo:lo + n8].view(torch.int64) == want).all()):
                return False
            if n8 != hi - lo and not bool((self.buf[lo + n8:hi] == SENTINEL_BYTE).all()):
                return False
        return True

    def check_untouched(self, copy_outputs: bool = True) -> Dict[str, torch.Tensor]:
        """Copy the output windows out, overwrite every window with the sentinel, and require the whole arena to equal the sentinel:
        every byte outside the windows is what it was.  The arena is clean again afterwards (reusable)."""
        outs = {n: self.read(n) for n, w in self.windows.items() if w.output} if copy_outputs else {}
        for w in self.windows.values():
            self.buf[self._index(w)] = SENTINEL_BYTE
        self.windows = {}
        assert self.all_sentinel(), "a byte of the arena outside every operand window was written"
        return outs


# ------------------------------------------------------------------------------------------------ the case table
@dataclass
class ExtentCase:
    """One far call.  ``params``: what the GPU test needs to build it; ``layout``: name -> Layout of every operand that lives in the
    arena; ``arena_bytes``: the allocation; ``band``: "4G" (the far operands' last byte offset passes 2^32) or "2G" (between 2^31
    and 2^32: only a signed 32-bit offset wraps)."""
    entry: str
    ident: str
    params: dict
    layout: Dict[str, Layout]
    arena_bytes: int
    band: str = "4G"

    @property
    def id(self):
        return f"{self.entry}-{self.ident}"


def arena_bytes_for(layouts: Sequence[Layout]) -> int:
    n = max(l.ptr_off + max(WRAP, l.extent) for l in layouts) + TAIL
    return (n + 15) // 16 * 16


def gemm_m(bm: int, need_lo8: bool) -> int:
    """Two row tiles and a ragged third one, never fewer than 257 rows (row 256 x 16 MiB = 4 GiB); 529 rows where the byte plane
    (ldlo = 2^23 BYTES per row) has to pass 2^32 as well (M >= 513)."""
    return 529 if need_lo8 else max(273, 2 * bm + 17)


def gemm_layout(form: str, M: int, N: int, K: int, out_elem: int, *, lda=GEMM_LD, ldc=GEMM_LD, ldx=GEMM_LD, ldr=GEMM_LD, ldlo=GEMM_LD,
                row_map: Optional[Sequence[int]] = None, alias=True, t_dtype=torch.bfloat16) -> Dict[str, Layout]:
    """The far operands of one slime_gemm_ex / slime_gemm_ksplit call by the header's formulas: A / A2 [M, lda] T, C [M or rows of the
    map, ldc] T or fp32, x16 [M, ldx] T, resid [M, ldr] T, lo8 [M, ldlo] bytes.  Operand i starts i * SLOT bytes into the rows."""
    cdt = t_dtype if out_elem == 2 else torch.float32
    lay: Dict[str, Layout] = {}

    def add(name, slot, nrows, ld_bytes, width_bytes, dtype, output, rows=None):
        rows = list(rows) if rows is not None else list(range(nrows))
        last = max(rows)
        lay[name] = Layout(name, LEAD + slot * SLOT, [r * ld_bytes for r in rows], width_bytes, dtype, output,
                           last=((last, ld_bytes // dtype.itemsize, dtype.itemsize), (width_bytes - 1,)))

    add("A", 0, M, lda * 2, K * 2, t_dtype, False)
    if form == "gelu_mix_t":
        add("A2", 1, M, lda * 2, K * 2, t_dtype, False)
    add("C", 2, M, ldc * out_elem, N * out_elem, cdt, True, rows=row_map)
    if form == "resid_f32_ln":
        add("x16", 3, M, ldx * 2, N * 2, t_dtype, True)
    if form == "resid_t" and not alias:
        add("resid", 4, M, ldr * 2, N * 2, t_dtype, False)
    if form == "resid_split_ln":
        add("lo8", 5, M, ldlo, N, torch.int8, True)
    return lay


# forced tile id -> rows per workgroup and the smallest N of the family (gemm_conformance.TILE_BM / TILE_N; restated here so that the
# table needs no GPU-side import; test_extent_bound_cpu.py holds the two together)
GEMM_TILES = {3: (128, 128), 15: (128, 128), 18: (64, 128), 4: (256, 256), 10: (192, 256), 11: (256, 256), 12: (128, 256)}
GEMM_FORMS = ("bias_t", "quickgelu_t", "gelu_t", "bias_f32", "resid_f32", "resid_f32_ln", "resid_t", "resid_split_ln", "fold_bias_t",
              "fold_quickgelu_t")
GEMM_F32_OUT = ("bias_f32", "resid_f32", "resid_f32_ln")
GEMM_K = 64
KSPLIT_FORMS = ("bias_t", "bias_f32", "resid_t", "resid_split_ln", "fold_quickgelu_t")
OPERAND_FORMS = ("B", "B+frag", "frag")


def _far_row_map(M: int, R: int) -> List[int]:
    """M distinct rows of an R-row buffer: the last rows, a few early ones, the rest spread; non-monotone."""
    step = 2 if R - (M + 1) // 2 >= 2 * (M // 2) else 1
    rows = list(range(R - 1, R - 1 - (M + 1) // 2, -1)) + list(range(0, step * (M // 2), step))
    assert len(rows) == M and len(set(rows)) == M and max(rows) == R - 1
    return rows


def gemm_cases() -> List[ExtentCase]:
    out: List[ExtentCase] = []
    n = 0
    for tile, (bm, N) in GEMM_TILES.items():
        for form in GEMM_FORMS:
            n += 1
            f32 = form in GEMM_F32_OUT
            M = gemm_m(bm, form == "resid_split_ln")
            if f32:
                M = 273          # fp32 rows of 2^23 elements are 32 MiB: 273 of them reach 8.5 GiB
            alias = bool(n % 2)
            p = dict(tile=tile, bm=bm, form=form, M=M, N=N, K=GEMM_K, dtype=("bf16", "fp16")[n % 2], operand=OPERAND_FORMS[n % 3], alias=alias,
                     lda=GEMM_LD, ldc=GEMM_LD, ldx=GEMM_LD, ldr=GEMM_LD, ldlo=GEMM_LD, splits=1, row_map=None)
            lay = gemm_layout(form, M, N, GEMM_K, 4 if f32 else 2, alias=alias)
            out.append(ExtentCase("slime_gemm_ex", f"tile{tile}-{form}", p, lay, arena_bytes_for(list(lay.values()))))
        # the row map: M rows scattered over 529 rows of C, the last one among them
        for form in ("bias_t", "bias_f32"):
            n += 1
            f32 = form == "bias_f32"
            M, R = 273, (529 if not f32 else 273)
            rm = _far_row_map(M, R)                  # fp32 rows are 32 MiB: the map is a permutation of 273 rows there
            p = dict(tile=tile, bm=bm, form=form, M=M, N=N, K=GEMM_K, dtype=("bf16", "fp16")[n % 2], operand=OPERAND_FORMS[n % 3], alias=True,
                     lda=GEMM_LD, ldc=GEMM_LD, ldx=GEMM_LD, ldr=GEMM_LD, ldlo=GEMM_LD, splits=1, row_map=rm)
            lay = gemm_layout(form, M, N, GEMM_K, 4 if f32 else 2, row_map=rm)
            lay["A"].far = M > 256
            out.append(ExtentCase("slime_gemm_ex", f"tile{tile}-{form}-rowmap", p, lay, arena_bytes_for(list(lay.values()))))
    # the mix epilogue: direct-B kernel only, A2 far as A
    p = dict(tile=12, bm=128, form="gelu_mix_t", M=273, N=256, K=GEMM_K, dtype="bf16", operand="B+frag", alias=True,
             lda=GEMM_LD, ldc=GEMM_LD, ldx=GEMM_LD, ldr=GEMM_LD, ldlo=GEMM_LD, splits=1, row_map=None)
    lay = gemm_layout("gelu_mix_t", 273, 256, GEMM_K, 2)
    out.append(ExtentCase("slime_gemm_ex", "tile12-gelu_mix_t", p, lay, arena_bytes_for(list(lay.values()))))
    # the k-split pair of launches (product dispatch: either tile the library picks), two k-tiles per split
    for form in KSPLIT_FORMS:
        n += 1
        f32 = form in GEMM_F32_OUT
        M = 273 if f32 else 529
        p = dict(tile=0, bm=128, form=form, M=M, N=128, K=256, dtype=("bf16", "fp16")[n % 2], operand=OPERAND_FORMS[n % 3], alias=bool(n % 2),
                 lda=GEMM_LD, ldc=GEMM_LD, ldx=GEMM_LD, ldr=GEMM_LD, ldlo=GEMM_LD, splits=2, row_map=None)
        lay = gemm_layout(form, M, 128, 256, 4 if f32 else 2, alias=bool(n % 2))
        out.append(ExtentCase("slime_gemm_ksplit", form, p, lay, arena_bytes_for(list(lay.values()))))
    # the band between 2^31 and 2^32: 2^22-element rows, 273 of them end at 2.13 GiB (T) -- a signed offset wraps, an unsigned one does not
    for tile, form in ((15, "bias_t"), (4, "resid_t"), (11, "resid_split_ln"), (12, "fold_bias_t")):
        n += 1
        bm, N = GEMM_TILES[tile]
        M, ld = 273, 1 << 22
        p = dict(tile=tile, bm=bm, form=form, M=M, N=N, K=GEMM_K, dtype=("bf16", "fp16")[n % 2], operand=OPERAND_FORMS[n % 3], alias=True,
                 lda=ld, ldc=ld, ldx=ld, ldr=ld, ldlo=2 * ld, splits=1, row_map=None)
        lay = gemm_layout(form, M, N, GEMM_K, 2, lda=ld, ldc=ld, ldx=ld, ldr=ld, ldlo=2 * ld)
        out.append(ExtentCase("slime_gemm_ex", f"tile{tile}-{form}-2G", p, lay, arena_bytes_for(list(lay.values())), band="2G"))
    return out


def cases() -> List[ExtentCase]:
    """Every far call of test_gpu_extent_conformance.py, in the order it runs them."""
    return gemm_cases() + row_cases() + attention_cases()


# ------------------------------------------------------------------------------------------------ row kernels
def row_cases() -> List[ExtentCase]:
    """slime_layernorm (x [rows, ldx] fp32), slime_rope (x [rows, row_stride] T, in place), slime_gather_rows / _split (in
    [groups * rows_in, C], group 1 past 2^32 bytes, row_off near the end), slime_select_crops (feats [images * period, P, C] T, `first`
    near the end of a large period), slime_ln_gather (src [src_rows, D] fp32, idx past 2^32 bytes), and further down the batched
    merge, the gate mix, the batched router scores, the splice (far table / features, and an `out` of 4 GiB), the batched resize and
    the batched tile-normalise.  Every mechanism has a "4G" row and, but for the 4 GiB output, a "2G" twin."""
    out: List[ExtentCase] = []

    def one(entry, ident, params, lays, band="4G"):
        lay = {l.name: l for l in lays}
        out.append(ExtentCase(entry, ident, params, lay, arena_bytes_for(lays), band))

    # slime_layernorm: rows of 128 floats, 2^22 floats (16 MiB) apart, 273 rows: the last one starts at 4.25 GiB
    for band, ldx, rows in (("4G", 1 << 22, 273), ("2G", 1 << 21, 273)):
        D = 128
        one("slime_layernorm", f"ldx-{band}", dict(D=D, ldx=ldx, rows=rows),
            [Layout("x", LEAD, strided_rows(rows, ldx * 4), D * 4, torch.float32, False, last=((rows - 1, ldx, 4), (D * 4 - 1,)))], band)
    # slime_rope: x[r * row_stride + h * head_dim + d] T, in place
    for band, rs, rows in (("4G", 1 << 23, 273), ("2G", 1 << 22, 273)):
        heads, hd = 2, 128
        one("slime_rope", f"row_stride-{band}", dict(row_stride=rs, rows=rows, heads=heads, head_dim=hd),
            [Layout("x", LEAD, strided_rows(rows, rs * 2), heads * hd * 2, torch.bfloat16, True, last=((rows - 1, rs, 2), (heads * hd * 2 - 1,)))],
            band)
    # slime_gather_rows: in[(g * rows_in + row_off + r) * C], fp32, C = 128: rows_in = 2^23 + 11 puts group 1 past 2^32 bytes
    C_, rows_out = 128, 37
    for band, rows_in in (("4G", (1 << 23) + 11), ("2G", 3 * (1 << 20) + 11)):
        row_off = rows_in - rows_out - 3
        src_rows = [(g * rows_in + row_off + r) * C_ * 4 for g in range(2) for r in range(rows_out)]
        one("slime_gather_rows", f"rows_in-{band}", dict(C=C_, rows_in=rows_in, row_off=row_off, rows_out=rows_out, groups=2),
            [Layout("in", LEAD, src_rows, C_ * 4, torch.float32, False, last=((rows_in + row_off + rows_out - 1, C_, 4), (C_ * 4 - 1,)))], band)
    # slime_gather_rows_split: hi T and lo8 int8 [groups * rows_in, C], interleaved in one range (lo starts SLOT bytes further in): with
    # rows_in = 2^24 + 11 group 1 of hi starts at 4 GiB and group 1 of the byte plane at 2 GiB, its last rows just past 2^32
    for band, rows_in in (("4G", (1 << 24) + 11), ("2G", 3 * (1 << 21) + 11)):
        row_off = rows_in - rows_out - 3
        idx = [(g * rows_in + row_off + r) for g in range(2) for r in range(rows_out)]
        last = rows_in + row_off + rows_out - 1
        hi = Layout("hi", LEAD, [i * C_ * 2 for i in idx], C_ * 2, torch.bfloat16, False, last=((last, C_, 2), (C_ * 2 - 1,)))
        lo = Layout("lo", LEAD + SLOT, [i * C_ for i in idx], C_, torch.int8, False, last=((last, C_, 1), (C_ - 1,)), far=band == "4G")
        one("slime_gather_rows_split", f"rows_in-{band}", dict(C=C_, rows_in=rows_in, row_off=row_off, rows_out=rows_out, groups=2), [hi, lo], band)
    # slime_select_crops: crop (image * period + first + j) of feats T [images * period, P, C]
    P, Cc = 16, 256
    crop_bytes = P * Cc * 2
    for band, period in (("4G", (1 << 19) + 5), ("2G", 3 * (1 << 16) + 5)):
        per_image, images = 2, 2
        first = period - per_image - 1
        crops = [i * period + first + j for i in range(images) for j in range(per_image)]
        one("slime_select_crops", f"period-{band}", dict(P=P, C=Cc, period=period, first=first, per_image=per_image, images=images),
            [Layout("feats", LEAD, [c * crop_bytes for c in crops], crop_bytes, torch.bfloat16, False,
                    last=((period + first + per_image - 1, P * Cc, 2), (crop_bytes - 1,)))], band)
    # slime_ln_gather: src fp32 [src_rows, D], idx int64
    D = 128
    for band, src_rows in (("4G", (1 << 23) + 64), ("2G", (1 << 22) + 64)):
        idx = [3, src_rows - 1, 0, src_rows - 17, 1 << 21, src_rows - 2, 5]
        one("slime_ln_gather", f"idx-{band}", dict(D=D, src_rows=src_rows, idx=idx),
            [Layout("src", LEAD, [i * D * 4 for i in sorted(set(idx))], D * 4, torch.float32, False, last=((src_rows - 1, D, 4), (D * 4 - 1,)))], band)
    # slime_merge_rows_batched: image b reads in rows b * in_image_stride + r and writes out rows b * out_image_stride + dst_row0 + dst
    C_, per = 128, 8                                   # nw = 2, nh = 1, g = 2: 8 rows per image
    for band, iis, ois in (("4G", (1 << 23) + 8, (1 << 22) + 16), ("2G", 3 * (1 << 21) + 8, 3 * (1 << 20) + 16)):
        row0 = ois - per - 3
        one("slime_merge_rows_batched", f"image-strides-{band}", dict(C=C_, nw=2, nh=1, g=2, images=2, in_image_stride=iis, out_image_stride=ois, dst_row0=row0),
            [Layout("in", LEAD, [(b * iis + r) * C_ * 4 for b in range(2) for r in range(per)], C_ * 4, torch.float32, False,
                    last=((iis + per - 1, C_, 4), (C_ * 4 - 1,))),
             Layout("out", LEAD + SLOT, [(b * ois + row0 + d) * C_ * 4 for b in range(2) for d in range(per)], C_ * 4, torch.float32, True,
                    last=((ois + row0 + per - 1, C_, 4), (C_ * 4 - 1,)))], band)
    # slime_gate_mix_ex: out row (r / rows_per_group) * group_stride + row0 + r % rows_per_group
    H_, rpg = 128, 6
    for band, gs in (("4G", (1 << 22) + 16), ("2G", 3 * (1 << 20) + 16)):
        row0 = gs - rpg - 3
        one("slime_gate_mix_ex", f"group_stride-{band}", dict(H=H_, D=64, rows=2 * rpg, rows_per_group=rpg, group_stride=gs, row0=row0),
            [Layout("out", LEAD, [(grp * gs + row0 + i) * H_ * 4 for grp in range(2) for i in range(rpg)], H_ * 4, torch.float32, True,
                    last=((gs + row0 + rpg - 1, H_, 4), (H_ * 4 - 1,)))], band)
    # slime_router_scores_batched: image b owns img rows row_off[b] .. + n_rows[b] - 1 (fp32, H = 128)
    for band, off1 in (("4G", (1 << 23) + 5), ("2G", 3 * (1 << 21) + 5)):
        row_off, n_rows = [3, off1], [5, 7]
        one("slime_router_scores_batched", f"row_off-{band}", dict(H=128, L=3, T_max=8, row_off=row_off, n_rows=n_rows),
            [Layout("img", LEAD, [(o + t) * 128 * 4 for o, n in zip(row_off, n_rows) for t in range(n)], 128 * 4, torch.float32, False,
                    last=((off1 + n_rows[1] - 1, 128, 4), (128 * 4 - 1,)))], band)
    # slime_splice_rows: an fp32 table and fp32 features of more than 2^32 bytes (H = 256), of which src names the last rows and a few early ones
    Hs = 256
    for band, n_src in (("4G", (1 << 22) + 64), ("2G", 3 * (1 << 20) + 64)):
        t_rows, f_rows = [0, 5, n_src - 3, n_src - 1], [1, 7, n_src - 2, n_src - 1]
        src = [0, -1, n_src - 1, -2 - (n_src - 1), 5, -2 - 1, n_src - 3, -2 - 7, -2 - (n_src - 2), -1, n_src + 5, 0, -2 - (n_src + 9)]
        one("slime_splice_rows", f"table-and-feats-{band}", dict(H=Hs, table_rows=n_src, feat_rows=n_src, src=src, t_rows=t_rows, f_rows=f_rows),
            [Layout("table", LEAD, [r * Hs * 4 for r in t_rows], Hs * 4, torch.float32, False, last=((n_src - 1, Hs, 4), (Hs * 4 - 1,))),
             Layout("feats", LEAD + SLOT, [r * Hs * 4 for r in f_rows], Hs * 4, torch.float32, False, last=((n_src - 1, Hs, 4), (Hs * 4 - 1,)))], band)
    # slime_splice_merged: fp32 tokens [token_rows, H] and fp32 extra rows [extra_rows, H] behind them (k = -2 - src: k < token_rows a token
    # row, else row k - token_rows of extra), both of more than 2^32 bytes; the table is small and compact
    for band, n_src in (("4G", (1 << 22) + 64), ("2G", 3 * (1 << 20) + 64)):
        k_rows, e_rows = [0, 6, n_src - 2, n_src - 1], [2, n_src - 3, n_src - 1]
        src = [1, -2 - (n_src - 1), -1, -2 - 6, -2 - (n_src + n_src - 1), 3, -2 - 0, -2 - (n_src + 2), -2 - (n_src - 2), -2 - (n_src + n_src - 3),
               -2 - (2 * n_src + 4), 17]
        one("slime_splice_merged", f"tokens-and-extra-{band}", dict(H=Hs, token_rows=n_src, extra_rows=n_src, table_rows=4, src=src, k_rows=k_rows, e_rows=e_rows),
            [Layout("tokens", LEAD, [r * Hs * 4 for r in k_rows], Hs * 4, torch.float32, False, last=((n_src - 1, Hs, 4), (Hs * 4 - 1,))),
             Layout("extra", LEAD + SLOT, [r * Hs * 4 for r in e_rows], Hs * 4, torch.float32, False, last=((n_src - 1, Hs, 4), (Hs * 4 - 1,)))], band)
    # slime_router_attn_scores: tok_idx (built by ops.router_attention_scores from row_off / n_rows) names token rows past 2^32 bytes
    for band, off1 in (("4G", (1 << 23) + 5), ("2G", 3 * (1 << 21) + 5)):
        row_off, n_rows = [3, off1], [5, 7]
        one("slime_router_attn_scores", f"tok_idx-{band}", dict(H=128, L=3, row_off=row_off, n_rows=n_rows, token_rows=off1 + n_rows[1]),
            [Layout("tokens", LEAD, [(o + t) * 128 * 4 for o, n in zip(row_off, n_rows) for t in range(n)], 128 * 4, torch.float32, False,
                    last=((off1 + n_rows[1] - 1, 128, 4), (128 * 4 - 1,)))], band)
    # slime_splice_routed: image b's local tokens at rows local_row_off[b] .. of the fp32 token buffer, its P global tokens right before
    # them; image 1's rows past 2^32 bytes.  far_rows: the token rows placed (compact row i of the 11 holds far row far_rows[i])
    for band, off1 in (("4G", (1 << 22) + 64), ("2G", 3 * (1 << 20) + 64)):
        P_, n_loc = 2, [3, 4]
        far_rows = list(range(0, 2 + n_loc[0])) + list(range(off1 - P_, off1 + n_loc[1]))
        one("slime_splice_routed", f"local_row_off-{band}",
            dict(H=Hs, P=P_, T_max=4, local_row_off=[2, off1], compact_row_off=[2, 2 + n_loc[0] + P_], n_rows=n_loc, keep_idx=[[2, 0, 0, 0], [3, 1, 0, 0]],
                 keep_count=[2, 3], token_rows=off1 + n_loc[1], far_rows=far_rows, table_rows=8, sep_id=5),
            [Layout("tokens", LEAD, [r * Hs * 4 for r in far_rows], Hs * 4, torch.float32, False, last=((off1 + n_loc[1] - 1, Hs, 4), (Hs * 4 - 1,)))], band)
    # slime_splice_rows whose OUT passes 2^32 bytes: H = 4096, fp32, 262 160 rows of 16 KiB, src mostly -1 (zeros); the first, a few middle
    # and the last rows name table rows, so a store at a wrapped offset leaves the sentinel where values belong
    Ho, n_out = 4096, 262160
    named = {r: r % 16 for r in list(range(8)) + list(range(131072, 131076)) + list(range(n_out - 8, n_out))}
    one("slime_splice_rows", "out-4G", dict(H=Ho, rows=n_out, named=named, table_rows=16),
        [Layout("out", LEAD, strided_rows(n_out, Ho * 4), Ho * 4, torch.float32, True, last=((n_out - 1, Ho, 4), (Ho * 4 - 1,)), bulk=True)])
    # slime_resize_bicubic_u8_batched: image b at b * image stride, row y at y * row stride (bytes); "staged": both passes (the horizontal one
    # into tmp), "direct": equal heights, the horizontal pass writes dst itself
    sh, sw, ow = 12, 20, 14
    for path, oh in (("staged", 9), ("direct", 12)):
        for band, ss, sis_extra, ds, dis in (("4G", (1 << 28) + 64, 1 << 31, (1 << 28) + 128, (1 << 32) + (1 << 20)),
                                             ("2G", (1 << 27) + 64, 1 << 29, (1 << 27) + 128, (1 << 30) + (1 << 20))):
            sis = sh * ss + sis_extra
            one("slime_resize_bicubic_u8_batched", f"{path}-{band}",
                dict(src_h=sh, src_w=sw, out_h=oh, out_w=ow, images=2, src_stride=ss, src_image_stride=sis, dst_stride=ds, dst_image_stride=dis),
                [Layout("src", LEAD, [b * sis + y * ss for b in range(2) for y in range(sh)], sw * 3, torch.uint8, False,
                        last=((1, sis, 1), (sh - 1, ss, 1), (sw * 3 - 1,))),
                 Layout("dst", LEAD + SLOT, [b * dis + y * ds for b in range(2) for y in range(oh)], ow * 3, torch.uint8, True,
                        last=((1, dis, 1), (oh - 1, ds, 1), (ow * 3 - 1,)))], band)
    # slime_slice_jobs: two jobs that run both passes (so the second one's tmp_offset > 0); job 0's src rows src_stride bytes apart and its one
    # tile at crop first_crop with first_crop * 3 * crop^2 * 4 > 2^32 (crop 16: 3 KiB crops); job 1's two tiles at crops 3 and 4
    crop = 16
    obytes = 3 * crop * crop * 4
    for band, ss, first in (("4G", 1 << 29, 1398112), ("2G", 1 << 28, 699056)):
        jobs = [dict(src_h=12, src_w=20, out_h=9, out_w=14, canvas_h=16, canvas_w=16, x0=1, y0=2, first_crop=first, src_stride=ss),
                dict(src_h=10, src_w=24, out_h=13, out_w=30, canvas_h=16, canvas_w=32, x0=1, y0=1, first_crop=3, src_stride=ss + 64)]
        one("slime_slice_jobs", f"src_stride-first_crop-{band}", dict(crop=crop, jobs=jobs, out_crops=first + 1, out_order=[3, 4, first]),
            [Layout("src0", LEAD, strided_rows(12, ss), 20 * 3, torch.uint8, False, last=((11, ss, 1), (20 * 3 - 1,))),
             Layout("src1", LEAD + SLOT, strided_rows(10, ss + 64), 24 * 3, torch.uint8, False, last=((9, ss + 64, 1), (24 * 3 - 1,))),
             Layout("out", LEAD + 2 * SLOT, [c * obytes for c in (3, 4, first)], obytes, torch.float32, True,
                    last=((first, 3 * crop * crop, 4), (obytes - 1,)))], band)
    # slime_view_jobs: one job, a 16 x 10 box of a 12 x 20 image pasted into a 20 x 14 field, resized to 24 x 18 (both passes), two
    # overlapping 16 x 16 windows -> crops [first_crop, first_crop + 2); image rows img_stride bytes apart
    for band, ss, first in (("4G", 1 << 29, 1398112), ("2G", 1 << 28, 699056)):
        job = dict(img_h=12, img_w=20, box=(2, 2, 16, 10),      # the box ends in the image's last row
                   field=(20, 14), paste=(2, 2), bg=(124, 116, 104), out=(24, 18), windows=(1, 1, 4, 2, 1), img_stride=ss, first_crop=first)
        one("slime_view_jobs", f"img_stride-first_crop-{band}", dict(crop=crop, job=job, out_crops=first + 2),
            [Layout("img", LEAD, strided_rows(12, ss), 20 * 3, torch.uint8, False, last=((11, ss, 1), (20 * 3 - 1,))),
             Layout("out", LEAD + SLOT, [c * obytes for c in (first, first + 1)], obytes, torch.float32, True,
                    last=((first + 1, 3 * crop * crop, 4), (obytes - 1,)))], band)
    # slime_tile_normalize_batched: canvas b at b * canvas_image_stride BYTES, its tiles -> crops [b * out_image_crops + tile] of out fp32
    crop, Hc, Wc = 16, 16, 32
    cbytes, obytes = Hc * Wc * 3, 3 * crop * crop * 4
    for band, cis, oic in (("4G", (1 << 32) + 64, 1398112), ("2G", (1 << 31) + 64, 699056)):
        one("slime_tile_normalize_batched", f"image-strides-{band}", dict(crop=crop, Hc=Hc, Wc=Wc, images=2, canvas_image_stride=cis, out_image_crops=oic),
            [Layout("canvas", LEAD, [0, cis], cbytes, torch.uint8, False, last=((1, cis, 1), (cbytes - 1,))),
             Layout("out", LEAD + SLOT, [(b * oic + t) * obytes for b in range(2) for t in range(2)], obytes, torch.float32, True,
                    last=((oic + 1, 3 * crop * crop, 4), (obytes - 1,)))], band)
    return out


# ------------------------------------------------------------------------------------------------ attention
# (branch, entry, dtype, head_dim, heads, kv heads, n_q, n_kv): the smallest shapes that select each dispatch branch named in
# tests/attention_conformance.py -- slime_attention: attn64r is head_dim 64 with 321 <= n_kv <= 608, the generic kernel everything
# else; slime_prefill_attention: prefill32 is bf16 with 4 query heads per kv head (S = 70: two of its 64-row items), the eight-wave
# kernel every other group / dtype
ATTENTION_BRANCHES = (
    ("generic64", "slime_attention", "bf16", 64, 2, 2, 17, 33),
    ("attn64r", "slime_attention", "fp16", 64, 2, 2, 33, 321),
    ("generic128", "slime_attention", "bf16", 128, 1, 1, 17, 33),
    ("eight-wave", "slime_prefill_attention", "fp16", 128, 4, 2, 70, 70),
    ("prefill32", "slime_prefill_attention", "bf16", 128, 4, 1, 70, 70),
)


def _stride_for(n_rows: int, reach: int) -> int:
    """smallest power-of-two row stride (elements of 2 bytes) that puts row n_rows - 1 at or past byte ``reach``"""
    s = 8
    while (n_rows - 1) * s * 2 < reach:
        s *= 2
    return s


def attention_layout(B, n_q, n_kv, Eq, Ekv, q_bs, q_rs, k_bs, k_rs, o_bs, o_rs) -> Dict[str, Layout]:
    """q / o [B, n_q, Eq], k / v [B, n_kv, Ekv] T by the header's formula: element (b, i, h, d) at (b * bs + i * rs + h * head_dim + d);
    v shares k's strides.  Operand i starts i * SLOT bytes into the shared range."""
    lay = {}
    for slot, (name, n, E, bs, rs, out) in enumerate((("q", n_q, Eq, q_bs, q_rs, False), ("k", n_kv, Ekv, k_bs, k_rs, False),
                                                      ("v", n_kv, Ekv, k_bs, k_rs, False), ("o", n_q, Eq, o_bs, o_rs, True))):
        nb = B if bs else 1                               # q_bs = 0: one set of rows shared by every batch entry
        rows = [(b * bs + i * rs) * 2 for b in range(nb) for i in range(n)]
        lay[name] = Layout(name, LEAD + slot * SLOT, rows, E * 2, torch.bfloat16, out,
                           last=((nb - 1, bs, 2), (n - 1, rs, 2), (E * 2 - 1,)), far=max(rows) + E * 2 > 1 << 31)
    return lay


def attention_cases() -> List[ExtentCase]:
    out: List[ExtentCase] = []
    for branch, entry, dt, dh, H, HKV, n_q, n_kv in ATTENTION_BRANCHES:
        Eq, Ekv = H * dh, HKV * dh
        prefill = entry == "slime_prefill_attention"
        for band, reach in (("4G", 1 << 32), ("2G", 1 << 31)):
            # row strides, one batch entry
            q_rs, k_rs = _stride_for(n_q, reach), _stride_for(n_kv, reach)
            p = dict(branch=branch, dtype=dt, dh=dh, H=H, HKV=HKV, n_q=n_q, n_kv=n_kv, B=1, q_bs=8 * q_rs, q_rs=q_rs, k_bs=8 * k_rs, k_rs=k_rs,
                     o_bs=8 * q_rs, o_rs=q_rs, ranges=([5], [n_kv - 9]) if prefill else None)
            lay = attention_layout(1, n_q, n_kv, Eq, Ekv, p["q_bs"], q_rs, p["k_bs"], k_rs, p["o_bs"], q_rs)
            out.append(ExtentCase(entry, f"{branch}-row-strides-{band}", p, lay, arena_bytes_for(list(lay.values())), band))
            # batch strides, two batch entries of compact rows; the head_dim 128 branch of slime_attention shares its queries (q_bs = 0)
            bs = reach // 2 + 64
            shared = branch == "generic128"
            p = dict(branch=branch, dtype=dt, dh=dh, H=H, HKV=HKV, n_q=n_q, n_kv=n_kv, B=2, q_bs=0 if shared else bs, q_rs=Eq, k_bs=bs, k_rs=Ekv,
                     o_bs=bs, o_rs=Eq, ranges=([3, 0], [n_kv - 10, n_kv]) if prefill else None)
            lay = attention_layout(2, n_q, n_kv, Eq, Ekv, p["q_bs"], Eq, bs, Ekv, bs, Eq)
            out.append(ExtentCase(entry, f"{branch}-batch-strides-{band}", p, lay, arena_bytes_for(list(lay.values())), band))
    return out


# ------------------------------------------------------------------------------------------------ entries without strides: the reach comes from n
# The front end, the tower and the Llama attention layer take no stride: their buffers are compact and pass 2^32 bytes only through the
# crop / token count.  They do not live in an Arena (a compact buffer has no room for a wrapped access to be told from a right one by
# placement); what a truncated offset does there is overwrite or read the rows of EARLY crops, so the far call's first and last crops
# are compared bit for bit with a small call of the same crops, and a sentinel tail behind every output and the workspace is checked.
# The sizes are bounded by two limits: ~16 GiB allocated at a time, and batch <= 65535 in both attention entries (grid.y).
def _up(x: int, a: int = 256) -> int:
    return (x + a - 1) // a * a


def vit_plan(n: int, S: int, D: int, F: int) -> Dict[str, int]:
    """Byte offsets of the tower's workspace regions from ``ws`` (csrc/api.hip vit_plan; include/slime_hip.h slime_vit_workspace_bytes):
    lo, xn, the region ff / qkv / ctx share, stats; every region 256-byte aligned."""
    M = n * S
    p, off = {}, 0

    def take(name, nbytes):
        nonlocal off
        p[name] = _up(off)
        off = p[name] + nbytes

    take("lo", M * D)
    take("xn", M * D * 2)
    qkv = _up(M * 3 * D * 2)
    take("ff", max(M * F * 2, qkv + M * D * 2))
    p["qkv"], p["ctx"] = p["ff"], p["ff"] + qkv
    take("stats", M * (D // 64) * 2 * 4)
    p["total"] = _up(off)
    return p


def tower_extent_case() -> dict:
    """One slime_vit_forward pass, layers_run = 1, bf16 pixels: the geometry (112 / 16, D = 256, S = 50, inter = 1024) of the tower
    conformance tests -- at S = 17 the crop count for 2^32 bytes of workspace is past the attention's batch limit -- with the largest
    round n that keeps pixels + workspace + out under ~14 GiB.  Reached: pixels 4.5 GB, the workspace 8.5 GB with the tail of qkv, ctx,
    most of ff and stats past 2^32; lo, xn and out (1.5 GB) stay below it."""
    image, patch, D, F, n = 112, 16, 256, 1024, 60000
    S = (image // patch) ** 2 + 1
    plan = vit_plan(n, S, D, F)
    return dict(image=image, patch=patch, D=D, inter=F, n=n, S=S, plan=plan, pixel_bytes=n * 3 * image * image * 2,
                out_bytes=n * (S - 1) * D * 2)


def llama_extent_case() -> dict:
    """One slime_llama_attn_forward call on the smallest head-shard slice (hidden 512, one query and one kv head: geometry (512, 4, 4, 4)
    of head_shard_conformance): batch 43750 x S = 128 = 5.6 M tokens put the end of qkv, all of ctx, and the ends of x and out past 2^32."""
    hidden, hq, hkv, batch, S = 512, 1, 1, 43750, 128
    rows = batch * S
    qkv = rows * (hq + 2 * hkv) * 128 * 2
    return dict(hidden=hidden, hq=hq, hkv=hkv, batch=batch, S=S, rows=rows, qkv_bytes=qkv, ctx_off=_up(qkv), ctx_bytes=rows * hq * 128 * 2,
                x_bytes=rows * hidden * 2, out_bytes=rows * hidden * 2)


def front_end_extent_case() -> dict:
    """slime_patch_embed_prenorm / _plain / _prefix: 224 / 14, D = 1024 (rowwise_conformance.GEOMETRIES) -- the smallest geometry of that
    table whose x16 rows pass 2^32 within the memory limit at all (at 56 / 14, D = 128 a crop has 8.6 times more pixel than x16 bytes:
    2^32 bytes of x16 would need 37 GB of pixels).  n = 8200: fp32 pixels 4.9 GB, x16 4.3 GB, lo8 2.2 GB, stats 0.27 GB."""
    image, patch, D, n, n_prefix = 224, 14, 1024, 8200, 5
    P = (image // patch) ** 2
    return dict(image=image, patch=patch, D=D, n=n, P=P, n_prefix=n_prefix, kpad=_up(3 * patch * patch, 64), pixel_bytes=n * 3 * image * image * 4,
                rows={"prenorm": n * (P + 1), "plain": n * P, "prefix": n * (P + n_prefix)})
