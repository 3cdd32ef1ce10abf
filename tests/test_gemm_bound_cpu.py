"""The test of the GEMM conformance test (tests/gemm_conformance.py), without a GPU.

(1) ``emulate`` -- the torch fp32 restatement of the kernels' arithmetic, the stand-in for a correct kernel -- stays inside the
    derived element-wise bound for every epilogue form x dtype x kind on a sample of the GPU file's shape tables (the M table of the
    64- and 128-row tiles, K = 64 / 192 and one K = 2048, N = 128 / 256), and no reference value exceeds half of T's largest finite
    number.  The worst |err| / bound is printed per form.  For T outputs it sits near 1 (0.97 - 0.99): the final RNE is the whole
    error there and u |y| is its sharp bound; the fp32 forms sit far below (the accumulation term is a worst case, linear in K).
(2) kind "integer": all operands are small integers, the sum of the products' magnitudes stays below 2^24 and within what T holds
    exactly, and the fp32 / BIAS_T / BIAS_RESID_T results of ``emulate`` are bit-equal to the float64 reference, up to K = 4096.
(3) every mutant of MUTANTS leaves the bound (or the bit-equality, or the row-map gaps) on at least one case of the walked set.
(4) the reason the element-wise test exists: at (M, N) = (1731, 1024), bf16, plain random data, each CONFINED mutant -- one 8-column
    store group of one or two rows wrong by about the data's size -- stays BELOW the whole-tensor tolerance of tests/test_gpu_kernels.py
    (TOL_T, rel-L2 4e-3; measured 2.1e-3 - 2.5e-3 against a clean 1.7e-3), while the element-wise check names the group.  This is a
    statement about the mutants, not about a kernel.  In fp16 (TOL_T 6e-4) the whole-tensor check does see such a group at this
    shape (sqrt(8 / M N) = 2.1e-3; measured 1.3e-3 - 1.8e-3): those figures are printed, not asserted.
(5) ``_lib.GemmArgs`` has the field order, offsets and size of ``slime_gemm_args``.
"""
import ctypes as C
import subprocess

import pytest
import torch

import gemm_conformance as GC

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}
TOL_T = {torch.bfloat16: 4e-3, torch.float16: 6e-4}            # tests/test_gpu_kernels.py


def _sample_shapes(form):
    if form == "gelu_mix_t":
        return [(m, 256, k) for m, k in zip(GC.MIX_M, (64, 128, 192, 256, 64))]
    ms = sorted(set(GC.m_table(64)) | set(GC.m_table(128)))
    shapes = [(m, (128, 256)[i % 2], (64, 192)[(i // 2) % 2]) for i, m in enumerate(ms)]
    return shapes + [(17, 128, 2048)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", list(GC.FORMS))
def test_emulation_inside_bound(form, dtype):
    worst = 0.0
    for kind in GC.KINDS:
        for n, (M, N, K) in enumerate(_sample_shapes(form)):
            c = GC.make_case(kind, dtype, form, M, N, K, guard=("nan", "attract")[n % 2], alias=bool(n % 2), seed=n)
            r = GC.reference(c)
            assert float(r.out.abs().max()) < GC.HALF_MAX[dtype], "a reference value exceeds half of T's largest finite number"
            ratio, msg = GC.check(c, r, GC.emulate(c))
            assert msg is None, f"{kind} M={M} N={N} K={K}: {msg}"
            worst = max(worst, ratio)
    print(f"\nemulate {form} {DT_ID[dtype]}: worst |err| / bound = {worst:.3f}")
    assert worst < 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_emulation_inside_bound_row_map_and_no_bias(dtype):
    for form in GC.ROW_MAP_FORMS:
        for M in (1, 37, 145):
            c = GC.make_case("random", dtype, form, M, 128, 64, row_map=True, seed=M)
            ratio, msg = GC.check(c, GC.reference(c), GC.emulate(c))
            assert msg is None and ratio < 1.0, msg
    for form in GC.FORMS:
        c = GC.make_case("tails", dtype, form, 65, 256, 128, bias=False, seed=5)
        ratio, msg = GC.check(c, GC.reference(c), GC.emulate(c))
        assert msg is None and ratio < 1.0, msg


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("K", [64, 256, 4096])
def test_integer_kind_is_exact(dtype, K):
    for form in GC.EXACT_FORMS:
        c = GC.make_case("integer", dtype, form, 33, 128, K, seed=K)
        for name in ("A", "B", "bias"):
            w = c.buf[name].win.double()
            assert torch.equal(w, w.round()), name
        r = GC.reference(c)
        # sum of the magnitudes bounds every partial sum in every order: exact in fp32, and the result exact in T
        assert float(r.S.max()) <= 2.0 ** GC.MANT[dtype] < 2.0 ** 24
        assert torch.equal(r.out, r.out.round())
        got = GC.emulate(c)["C"]
        assert torch.equal(got.double(), r.out), form
        assert GC.check(c, r, GC.emulate(c))[1] is None


def _mutant_cases(dtype):
    mk = GC.make_case
    kw = dict(guard="attract")
    yield "bias_t random 145x256x128", mk("random", dtype, "bias_t", 145, 256, 128, seed=1, **kw)
    yield "bias_t integer 17x128x4096", mk("integer", dtype, "bias_t", 17, 128, 4096, seed=2, **kw)
    yield "bias_f32 row map 37x128x64", mk("random", dtype, "bias_f32", 37, 128, 64, row_map=True, seed=3, **kw)
    yield "gelu_t tails 65x128x64", mk("tails", dtype, "gelu_t", 65, 128, 64, seed=4, **kw)
    yield "quickgelu_t tails 65x128x64", mk("tails", dtype, "quickgelu_t", 65, 128, 64, seed=5, **kw)
    yield "gelu_mix_t random 65x256x64", mk("random", dtype, "gelu_mix_t", 65, 256, 64, seed=6, **kw)
    yield "resid_t random 33x128x64", mk("random", dtype, "resid_t", 33, 128, 64, seed=7, **kw)
    yield "resid_f32_ln random 33x256x64", mk("random", dtype, "resid_f32_ln", 33, 256, 64, seed=8, **kw)
    yield "resid_split_ln random 33x128x64", mk("random", dtype, "resid_split_ln", 33, 128, 64, seed=9, **kw)
    yield "resid_split_ln integer 33x128x64", mk("integer", dtype, "resid_split_ln", 33, 128, 64, seed=10, **kw)
    yield "fold_bias_t random 33x128x128", mk("random", dtype, "fold_bias_t", 33, 128, 128, seed=11, **kw)
    yield "fold_quickgelu_t tails 33x128x64", mk("tails", dtype, "fold_quickgelu_t", 33, 128, 64, seed=12, **kw)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_every_mutant_leaves_the_bound(dtype):
    cases = [(name, c, GC.reference(c)) for name, c in _mutant_cases(dtype)]
    for name, c, r in cases:                                      # the cases themselves are clean
        assert GC.check(c, r, GC.emulate(c))[1] is None, name
    print()
    for mname, defect in GC.MUTANTS.items():
        caught = [(name, msg) for name, c, r in cases for msg in [GC.check(c, r, GC.emulate(c, defect))[1]] if msg]
        assert caught, f"mutant {mname} stays inside the bound on every case ({dtype})"
        print(f"{DT_ID[dtype]} {mname:36s} caught by [{caught[0][0]}] (+ {len(caught) - 1} more cases): {caught[0][1][:150]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_confined_mutants_against_the_whole_tensor_tolerance(dtype):
    """One 8-column store group wrong at (1731, 1024): below TOL_T in bf16 (asserted); fp16's figures are printed (module docstring)."""
    M, N, K = 1731, 1024, 64
    setup = {"last_row_group_unwritten": ("resid_t", False),            # the stale group of an in-place residual stream
             "tail_row_stored_twice_one_group": ("bias_t", False),
             "row_map_of_next_row_one_group": ("bias_t", True)}
    assert set(setup) == set(GC.CONFINED)
    print()
    for mname in GC.CONFINED:
        form, rm = setup[mname]
        c = GC.make_case("random", dtype, form, M, N, K, guard="attract", row_map=rm, outliers=False, seed=3)
        if rm:                                                          # a zeroed target, as the row-map tests of test_gpu_kernels.py use
            c.buf["C"].flat.zero_()
            c.snapshot()
        r = GC.reference(c)
        sel = (lambda t: t[r.row_map]) if rm else (lambda t: t)
        clean, bad = GC.emulate(c), GC.emulate(c, GC.MUTANTS[mname])
        base, whole = GC.rel_l2(sel(clean["C"]), r.out), GC.rel_l2(sel(bad["C"]), r.out)
        ratio, msg = GC.check(c, r, bad)
        print(f"{DT_ID[dtype]} {mname:34s} whole-tensor rel-L2 {whole:.2e} (clean {base:.2e}, TOL_T {TOL_T[dtype]:.1e}); element-wise: {msg[:140]}")
        assert GC.check(c, r, clean)[1] is None
        assert msg is not None and ratio > 1.0, "the element-wise check points at it"
        assert whole > base, "the defect is there"
        if dtype == torch.bfloat16:
            assert whole < TOL_T[dtype], "the whole-tensor check was expected to miss this mutant"


def test_shape_tables_come_from_the_tile_heights():
    for tile, bm in GC.TILE_BM.items():
        ms = GC.m_table(bm)
        assert {1, 15, 16, 17, bm - 1, bm, bm + 1, 2 * bm + 17} == set(ms)
    assert [(m + 255) // 256 for m in GC.pp_tile_ms()] == list(GC.PP_TILES_M) and all(m % 256 for m in GC.pp_tile_ms())
    assert set(GC.MIX_M) == {1, GC.MIX_TOKENS - 1, GC.MIX_TOKENS, GC.MIX_TOKENS + 1, 145}


def test_gemm_args_mirror_matches_the_header_layout(tmp_path):
    """_lib.GemmArgs against slime_gemm_args: sizeof / offsetof printed by a C program compiled against the header, field by field,
    and every field the GPU conformance test sets (Case.arg_fields) is one of them."""
    import re
    import shutil
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"}\s*slime_gemm_args\s*;", text)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(slime_gemm_args));']
    for fname, _ in _lib.GemmArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(slime_gemm_args, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.GemmArgs)
    body = text[:text.index("} slime_gemm_args")]
    body = body[body.rindex("typedef struct"):]
    declared = [f for f in re.findall(r"\b([A-Za-z_0-9]+)\s*[,;]", body)]
    assert declared == [f for f, _ in _lib.GemmArgs._fields_]                     # every field, in the header's order
    for fname, _ in _lib.GemmArgs._fields_:
        assert int(got[fname]) == getattr(_lib.GemmArgs, fname).offset, fname
    used = set()
    for form in GC.FORMS:
        c = GC.make_case("random", torch.bfloat16, form, 5, 256, 64, row_map=form in GC.ROW_MAP_FORMS, alias=False)
        used |= set(c.arg_fields("B+frag", b_frag=16))
    assert used == {f for f, _ in _lib.GemmArgs._fields_}, "the conformance test sets every field of the argument block"
