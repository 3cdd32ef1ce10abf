"""Element-wise conformance of ``slime_gemm_ex`` on the GPU, through the C ABI (ctypes ``_lib.GemmArgs``), against the float64
reference and the DERIVED bound of tests/gemm_conformance.py (its docstring holds the derivation; the test of the bound itself is
tests/test_gemm_bound_cpu.py).

Every case lives in padded buffers (gemm_conformance.Padded): row stride = width + 64 elements, 3 guard rows, the window 16 bytes into
its allocation; B, B_frag, bias and colsum are followed by 64 poisoned elements, stats_out / mix_gates / ln_stats / row_map by 3 rows.
Each case runs twice: the input guards are NaN in the first pass and finite attractors in the second (1e4 around A, 1e6 around the
residual: a kernel that reads one column or row too far is grossly wrong).  Outputs start as the sentinel byte 0x7B (0x7B7B and
0x7B7B7B7B are finite numbers); outputs updated in place carry the input guard.  After the call every window must be inside the bound
element by element -- kind "integer": bit-equal -- and every byte outside every output window must be what it was.  All guards are
inside the test's own allocations; nothing here provokes a fault.

What is walked: (A) every kernel the product dispatch can reach, forced in the diagnostic library (tiles 3 / 15 / 18 / 4 / 10 / 11 /
12), x every epilogue form it instantiates (the eight of epilogue_wave and the two LayerNorm-fold consumers) x both dtypes x M on both
sides of every tile height x K = 64 / 128 / 192 / 256 x both guard passes, the operand taken three ways (row-major, both, fragment
image alone: bit-equal); K = 1984 / 2048 / 2112 at M = 600; tiles_m = 7 / 8 / 9 on the ping-pong kernel's XCD deal.  (B) the product
library on the smallest shapes that reach each branch of auto_tile on a 256-CU device, each proven by slime_gemm_kernel_name.  (C) the
operands no other test guards: resid (aliasing C or not), x16 / ldx, lo8 / ldlo, stats_out, mix_gates, row_map into 2 M + 5 rows, the
fold consumer on a real producer's statistics and on a row at |mu| = 10 sigma, bias = NULL.  (D) the refusals.

Worst |err| / bound observed on an MI355X, bf16 / fp16 (the module prints this table at the end of a run and writes it to the file
SLIME_GEMM_CONFORMANCE_REPORT names).  Columns: gemm_kernel 128x128 two-stage | 128x128 ring | 64x64 ring |
gemm_pp_kernel | gemm_w4_kernel 192 rows | 256 rows | gemm_db_kernel; forced tiles and the product-dispatch cases together.
    bias_t            0.994/0.990  0.994/0.989  0.995/0.986  0.995/0.989  0.994/0.987  0.994/0.988  0.994/0.986
    quickgelu_t       0.994/0.999  0.994/0.999  0.994/0.999  0.994/0.999  0.995/0.999  0.994/0.999  0.994/0.999
    gelu_t            0.995/0.989  0.995/0.989  0.995/0.989  0.994/0.984  0.994/0.985  0.994/0.984  0.994/0.985
    bias_f32          0.059/0.068  0.059/0.068  0.056/0.064  0.071/0.080  0.076/0.085  0.077/0.091  0.060/0.068
    resid_f32         0.059/0.057  0.059/0.057  0.053/0.061  0.078/0.065  0.050/0.070  0.078/0.065  0.059/0.064
    resid_f32_ln      0.994/0.988  0.994/0.988  0.995/0.988  0.994/0.987  0.995/0.988  0.994/0.987  0.994/0.988
    resid_t           0.994/0.989  0.994/0.989  0.995/0.983  0.995/0.987  0.994/0.987  0.995/0.987  0.994/0.988
    resid_split_ln    0.981/0.865  0.981/0.865  0.978/0.845  0.983/0.880  0.983/0.889  0.984/0.889  0.983/0.898
    fold_bias_t       0.996/0.997  0.996/0.997  0.995/0.997  0.996/0.998  0.996/0.998  0.996/0.998  0.996/0.997
    fold_quickgelu_t  0.995/0.999  0.995/0.999  0.995/0.999  0.996/0.999  0.995/0.999  0.996/0.999  0.995/0.999
    gelu_mix_t (direct-B only) 0.994/0.987; row map 0.994/0.999 (T), 0.057/0.071 (fp32); fold consumer on producer statistics 0.989/0.998.
These are measurements against the float64 reference, not targets.  Wherever the output is T the ratio sits just below 1 on any large
sample: the final RNE is nearly the whole error and u |y| is its sharp bound (0.999 in fp16 is a subnormal result half a grid step
off: the quick-GELU tail); what the table shows is that nothing comes on top of it.  The fp32 outputs show the accumulation term alone:
0.05 - 0.09 of a worst case that is linear in K.  All 256 cases passed on the kernels as they were: every element inside the bound,
every "integer" case bit-equal, the three operand forms bit-equal, every byte outside every output window untouched.
"""
import ctypes as C
import json
import os

import pytest
import torch

import gemm_conformance as GC

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}
T_NAME = {torch.bfloat16: "BF16", torch.float16: "F16"}
TILES = (3, 15, 18, 4, 10, 11, 12)
GUARDS = ("nan", "attract")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    """worst |err| / bound per (kernel family, form, dtype), printed when the module is done (and written to the file
    SLIME_GEMM_CONFORMANCE_REPORT names, if set)."""
    table = {}
    yield table
    lines = [f"    {k:64s} {v:.3f}" for k, v in sorted(table.items())]
    print("\nGEMM conformance, worst |err| / bound per kernel family, form and dtype:\n" + "\n".join(lines))
    path = os.environ.get("SLIME_GEMM_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(lib, c):
    """B's fragment-order image in a buffer of its own, 64 poisoned elements behind it."""
    from slime_amd import _lib
    f = GC.Padded(c.N, c.K, c.dtype, c.buf["B"].flat.device, pad_cols=0, guard_rows=0, tail=GC.TAIL)
    if c.guard == "nan":
        f.flat.fill_(float("nan"))
    _lib.check(lib.slime_gemm_pack_b(c.buf["B"].ptr(), c.N, c.K, f.ptr(), _stream()), "slime_gemm_pack_b")
    return f


def _call(lib, c, operand, frag, **override):
    from slime_amd import _lib
    fields = c.arg_fields(operand, frag.ptr() if frag is not None else None)
    fields.update(override)
    g = _lib.GemmArgs(**fields)
    rc = lib.slime_gemm_ex(C.byref(g), _stream())
    torch.cuda.synchronize()
    return rc


def _run(lib, c, what, key, ratios, bm=128, operands=("B+frag", "B", "frag")):
    """reference -> one launch per operand form (inputs restored in between) -> the first inside the bound, the others bit-equal to
    it, every byte outside the windows untouched."""
    r = GC.reference(c)
    frag = _pack(lib, c) if any(o != "B" for o in operands) else None
    first = None
    for op in operands:
        c.restore()
        rc = _call(lib, c, op, frag)
        assert rc == 0, f"{what} [{op}]: slime_gemm_ex returned {rc}: {lib.slime_last_error().decode()}"
        touched = c.intact()
        assert touched is None, f"{what} [{op}]: a byte of {touched} outside its window was written"
        outs = c.windows()
        if first is None:
            first = outs
            ratio, msg = GC.check(c, r, outs, bm)
            assert msg is None, f"{what} [{op}]: {msg}"
            k = f"{key} {c.form} {DT_ID[c.dtype]}"
            ratios[k] = max(ratios.get(k, 0.0), ratio)
        else:
            for name, t in outs.items():
                assert torch.equal(t.contiguous().view(torch.uint8), first[name].contiguous().view(torch.uint8)), \
                    f"{what}: {name} with operand form {op} differs in bits from the form {operands[0]}"
    return ratio


def _what(c, extra=""):
    return f"{c.form} {c.kind} {DT_ID[c.dtype]} M={c.M} N={c.N} K={c.K} guard={c.guard} {extra}"


class _forced:
    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        from slime_amd import _lib
        self.ctx = _lib.diag()
        self.lib = self.ctx.__enter__()
        self.lib.slime_gemm_force_tile(self.tile)
        return self.lib

    def __exit__(self, *exc):
        self.lib.slime_gemm_force_tile(0)
        return self.ctx.__exit__(*exc)


# ------------------------------------------------------------------------------------------------ A. forced tiles
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", GC.WAVE_FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_forced_tile(dev, ratios, tile, form, dtype):
    """One kernel family x one epilogue form x one dtype: M on both sides of the tile height (1, 15, 16, 17, BM - 1, BM, BM + 1,
    2 BM + 17), K with fewer k-tiles than pipeline stages and just enough, every N of the family, both guard passes, the kinds in
    turn, the operand three ways (a forced direct-B tile without a fragment image runs the stream kernel: bit-equal all the same)."""
    bm = GC.TILE_BM[tile]
    n = 0
    with _forced(tile) as lib:
        for N in GC.TILE_N[tile]:
            for M in GC.m_table(bm):
                for K in GC.K_SMALL:
                    kind = GC.KINDS[n % 3]
                    n += 1
                    for guard in GUARDS:
                        c = GC.make_case(kind, dtype, form, M, N, K, guard=guard, alias=bool(n % 2), seed=n, device=dev)
                        _run(lib, c, _what(c, f"tile {tile}"), GC.TILE_FAMILY[tile], ratios, bm)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", ["bias_t", "resid_split_ln", "bias_f32"])
def test_ping_pong_xcd_row_deal(dev, ratios, form, dtype):
    """xcd_rows_tile deals row tiles over 8 XCDs with a quotient and a remainder: tiles_m = 7 (0 r 7), 8 (1 r 0), 9 (1 r 1), the
    last tile ragged, two column tiles."""
    with _forced(4) as lib:
        for n, M in enumerate(GC.pp_tile_ms()):
            for guard in GUARDS:
                c = GC.make_case(GC.KINDS[n % 3], dtype, form, M, 512, 64, guard=guard, seed=n, device=dev)
                _run(lib, c, _what(c, "tile 4"), GC.TILE_FAMILY[4], ratios, 256)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("K", GC.K_TAG)
@pytest.mark.parametrize("tile", [4, 10, 11, 12])
def test_forced_tile_long_k(dev, ratios, tile, K, dtype):
    """Both KTAG instantiations (K >= 2048) of each family that has them, M = 600: integer operands (bit-equal: a dropped or doubled
    k-step cannot hide in a bound that is linear in K) and random ones."""
    with _forced(tile) as lib:
        for kind, form in (("integer", "bias_t"), ("integer", "bias_f32"), ("random", "bias_f32"), ("random", "resid_split_ln")):
            c = GC.make_case(kind, dtype, form, 600, 256, K, guard="nan", seed=K, device=dev)
            _run(lib, c, _what(c, f"tile {tile}"), GC.TILE_FAMILY[tile], ratios, GC.TILE_BM[tile])


# ------------------------------------------------------------------------------------------------ B. product dispatch
RING_FORMS = ("bias_t", "gelu_t", "resid_t", "fold_quickgelu_t", "resid_split_ln", "bias_f32")
TOWER_FORMS = ("fold_bias_t", "fold_quickgelu_t", "resid_split_ln", "bias_f32")
LONG_K_FORMS = ("bias_t", "bias_f32")
# (branch, M, N, K, fragment image, kernel name with {T} = dtype and {E} = epilogue, family, BM, forms): auto_tile on a 256-CU device
BRANCHES = [
    ("64x64 ring", 100, 256, 64, False, "gemm_kernel<{T}, 64, 64, 4, 1, {E}, 2>", 18, RING_FORMS),
    ("64x64 ring (M >= 512, grid below half the CUs twice over)", 700, 1024, 64, False, "gemm_kernel<{T}, 64, 64, 4, 1, {E}, 2>", 18, RING_FORMS[:2]),
    ("128x128 ring", 2200, 1024, 64, False, "gemm_kernel<{T}, 128, 128, 2, 2, {E}, 2>", 15, RING_FORMS),
    ("128x128 two-stage", 2200, 2048, 64, False, "gemm_kernel<{T}, 128, 128, 2, 2, {E}, 1>", 3, RING_FORMS),
    ("ping-pong", 2049, 4096, 128, False, "gemm_pp_kernel<{T}, {E}, 0, 0, 4>", 4, TOWER_FORMS),
    ("ping-pong, long K", 2049, 4096, 2048, False, "gemm_pp_kernel<{T}, {E}, 1, 0, 4>", 4, LONG_K_FORMS),
    ("stream 256 rows", 3841, 4096, 64, False, "gemm_w4_kernel<{T}, {E}, 0, 8, 0>", 11, TOWER_FORMS),
    ("stream 256 rows, long K", 3841, 4096, 2048, False, "gemm_w4_kernel<{T}, {E}, 1, 8, 0>", 11, LONG_K_FORMS),
    ("stream 192 rows", 4353, 4096, 64, False, "gemm_w4_kernel<{T}, {E}, 0, 6, 0>", 10, TOWER_FORMS),
    ("direct-B, K <= 2048 rule", 2049, 4096, 128, True, "gemm_db_kernel<{T}, {E}, 0, 8>", 12, TOWER_FORMS + ("gelu_t", "resid_t")),
    ("direct-B, K <= 2048 rule at K = 2048", 2049, 4096, 2048, True, "gemm_db_kernel<{T}, {E}, 1, 8>", 12, LONG_K_FORMS),
    ("direct-B, K > 2048 small-grid rule", 1025, 4096, 2112, True, "gemm_db_kernel<{T}, {E}, 1, 8>", 12, LONG_K_FORMS + ("resid_split_ln",)),
    ("K = 2048 does not take the K > 2048 rule", 1025, 4096, 2048, True, "gemm_kernel<{T}, 128, 128, 2, 2, {E}, 1>", 3, LONG_K_FORMS),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("branch", BRANCHES, ids=[b[0].replace(" ", "_") for b in BRANCHES])
def test_product_dispatch_branch(dev, ratios, branch, dtype):
    """The product library, no hooks: each case first proves its branch through slime_gemm_kernel_name (a later dispatch change
    fails here instead of silently moving the walk), then runs the forms production uses on that branch, and BIAS_F32."""
    from slime_amd import _lib, ops
    name, M, N, K, has_frag, template, tile, forms = branch
    lib = _lib.load()
    for n, form in enumerate(forms):
        want = template.format(T=T_NAME[dtype], E=GC.FORMS[form][0])
        assert ops.gemm_kernel_name(M, N, K, dtype, GC.FORMS[form][0], has_frag) == want, f"{name}: the dispatch moved"
        kind = "integer" if (K >= 1984 and form == "bias_t") else GC.KINDS[(2 * n) % 3]
        c = GC.make_case(kind, dtype, form, M, N, K, guard=GUARDS[n % 2], seed=n, device=dev)
        _run(lib, c, _what(c, name), "product " + GC.TILE_FAMILY[tile], ratios, GC.TILE_BM[tile], operands=("B+frag", "frag") if has_frag else ("B",))
        del c
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ C. the operands
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("alias", [True, False], ids=["resid-is-C", "resid-apart"])
def test_resid_t_aliasing(dev, ratios, dtype, alias):
    from slime_amd import _lib
    lib = _lib.load()
    for n, M in enumerate((1, 65, 145, 529)):
        for guard in GUARDS:
            c = GC.make_case(GC.KINDS[n % 3], dtype, "resid_t", M, 256, 128, guard=guard, alias=alias, seed=n, device=dev)
            before = None if alias else c.buf["resid"].snapshot()
            _run(lib, c, _what(c, f"alias={alias}"), "operands", ratios)
            if not alias:
                assert torch.equal(c.buf["resid"].flat.view(torch.uint8), before.view(torch.uint8)), "resid is an input"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", ["resid_f32_ln", "resid_split_ln"])
def test_producer_outputs(dev, ratios, dtype, form):
    """x16 with ldx > N, lo8 with ldlo > N (and its guard bytes), stats_out followed by three poisoned rows."""
    from slime_amd import _lib
    lib = _lib.load()
    for n, (M, N) in enumerate(((1, 128), (63, 256), (145, 384), (300, 1024))):
        for guard in GUARDS:
            c = GC.make_case(GC.KINDS[n % 3], dtype, form, M, N, 128, guard=guard, seed=n, device=dev)
            assert c.buf["C"].ld > N and c.buf["stats_out"].full.shape[0] == M + 3
            _run(lib, c, _what(c), "operands", ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("gates", ["per-row", "1,0", "0,1", "0.3,0.7"])
def test_gelu_mix(dev, ratios, dtype, gates):
    """BIAS_GELU_MIX_T (direct-B kernel, 64 tokens per workgroup): M on both sides of 64, gate rows past M poisoned."""
    from slime_amd import _lib
    lib = _lib.load()
    n = 0
    for M in GC.MIX_M:
        for K in GC.K_SMALL:
            n += 1
            gt = None if gates == "per-row" else torch.tensor([float(v) for v in gates.split(",")], device=dev).expand(M, 2)
            for guard in GUARDS:
                c = GC.make_case(GC.KINDS[n % 3], dtype, "gelu_mix_t", M, (256, 512)[n % 2], K, guard=guard, gates=gt, seed=n, device=dev)
                _run(lib, c, _what(c, f"gates {gates}"), GC.TILE_FAMILY[12], ratios, GC.MIX_TOKENS, operands=("B+frag", "frag"))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", GC.ROW_MAP_FORMS)
def test_row_map_scatter(dev, ratios, form, dtype):
    """row_map scatters into 2 M + 5 rows, non-monotone and with gaps; M on a ragged tile of every family; the gap rows and the
    guard rows keep the sentinel."""
    for n, tile in enumerate(TILES):
        M = GC.TILE_BM[tile] + 17
        with _forced(tile) as lib:
            for guard in GUARDS:
                c = GC.make_case(GC.KINDS[n % 3], dtype, form, M, 256, 64, guard=guard, row_map=True, seed=n, device=dev)
                assert c.out_rows == 2 * M + 5
                _run(lib, c, _what(c, f"row map, tile {tile}"), "row map", ratios, GC.TILE_BM[tile])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", ["fold_bias_t", "fold_quickgelu_t"])
def test_fold_consumer_on_producer_statistics(dev, ratios, form, dtype):
    """The consumer's statistics from a real BIAS_RESID_F32_LN launch (sums of the unrounded rows, A = their rounded copy), and a
    synthetic set with one row at |mu| = 10 sigma; statistics rows past M poisoned."""
    from slime_amd import _lib
    lib = _lib.load()
    for n, M in enumerate((1, 130, 300)):
        D = 256
        p = GC.make_case("random", dtype, "resid_f32_ln", M, D, 128, guard="nan", seed=n, device=dev)
        assert _call(lib, p, "B", None) == 0
        for guard in GUARDS:
            c = GC.make_case("random", dtype, form, M, 384, D, guard=guard, seed=n + 10, device=dev)
            c.buf["A"].win.copy_(p.buf["x16"].win)
            c.buf["ln_stats"].win.copy_(p.buf["stats_out"].win)
            _run(lib, c, _what(c, "producer statistics"), "fold consumer", ratios)
            s = GC.make_case("tails", dtype, form, M, 384, D, guard=guard, outlier_row=True, seed=n + 20, device=dev)
            _run(lib, s, _what(s, "synthetic statistics, a row at 10 sigma"), "fold consumer", ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", list(GC.FORMS))
def test_null_bias(dev, ratios, form, dtype):
    from slime_amd import _lib
    lib = _lib.load()
    for guard in GUARDS:
        c = GC.make_case("tails", dtype, form, 145, 256, 128, guard=guard, bias=False, seed=3, device=dev)
        _run(lib, c, _what(c, "bias = NULL"), "bias = NULL", ratios, operands=("B+frag", "frag") if form == "gelu_mix_t" else ("B+frag", "B", "frag"))


# ------------------------------------------------------------------------------------------------ D. refusals
def _refusals():
    yield "lda < K", "bias_t", 256, lambda c, f: dict(lda=c.K - 8), "leading dims"
    yield "ldc % 8 != 0", "bias_t", 256, lambda c, f: dict(ldc=c.N + 4), "leading dims"
    yield "lda past the tiles' 32-bit A offsets", "bias_t", 256, lambda c, f: dict(lda=1 << 24), "lda=16777216 is too large"
    yield "A off 16-byte alignment", "bias_t", 256, lambda c, f: dict(A=c.buf["A"].ptr() + 2), "16-byte aligned"
    yield "C off 16-byte alignment", "bias_f32", 256, lambda c, f: dict(C=c.buf["C"].ptr() + 4), "16-byte aligned"
    yield "row_map with a residual epilogue", "resid_t", 256, lambda c, f: dict(row_map=c.buf["A"].ptr()), "row_map goes with"
    yield "mix without B_frag", "gelu_mix_t", 256, lambda c, f: dict(B_frag=None), "BIAS_GELU_MIX_T runs on the direct-B kernel only"
    yield "mix with N % 256 != 0", "gelu_mix_t", 384, lambda c, f: dict(), "BIAS_GELU_MIX_T runs on the direct-B kernel only"
    yield "ln_groups * 64 != K", "fold_bias_t", 256, lambda c, f: dict(ln_groups=c.K // 64 + 1), "ln_groups"
    yield "lo8 == C", "resid_split_ln", 256, lambda c, f: dict(lo8=c.buf["C"].ptr()), "BIAS_RESID_SPLIT_LN needs"
    yield "BIAS_RESID_T without resid", "resid_t", 256, lambda c, f: dict(resid=None), "BIAS_RESID_T needs resid"


@pytest.mark.parametrize("case", list(_refusals()), ids=[r[0].replace(" ", "_") for r in _refusals()])
def test_refusals(dev, case):
    """SLIME_EINVAL with a message that names the cause, and nothing is launched: every output byte keeps what it held."""
    from slime_amd import _lib
    lib = _lib.load()
    name, form, N, override, needle = case
    c = GC.make_case("random", torch.bfloat16, form, 70, N, 128, guard="nan", seed=1, device=dev)
    frag = _pack(lib, c)
    rc = _call(lib, c, "B+frag", frag, **override(c, frag))
    assert rc == -1, f"{name}: SLIME_EINVAL expected, got {rc}"
    assert needle in lib.slime_last_error().decode(), f"{name}: {lib.slime_last_error().decode()}"
    for k in c.outputs:
        assert torch.equal(c.buf[k].flat.view(torch.uint8), c.snaps[k].view(torch.uint8)), f"{name}: {k} was written"
