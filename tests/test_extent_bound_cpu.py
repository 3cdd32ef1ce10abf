"""No GPU: (1) every row of extent_conformance.cases() can SEE a truncated address -- its farthest byte offset passes 2^32 (or lies
between 2^31 and 2^32 for the rows of the "2G" band, where only a signed offset wraps), and the same formula with 32-bit products
lands inside the arena, outside the operand's own data or on a row with other values; (2) slime_amd._lib._SIGNATURES and the ctypes
mirrors of the job structs agree with include/slime_hip.h in argument count and width for EVERY entry point; (3) the lda limit of
slime_gemm_ex / slime_gemm_ksplit (gemm_check_args touches no device) is refused with the limit named, and the largest accepted
value passes the check."""
import ctypes as C
import re

import pytest
import torch

import extent_conformance as XC
import gemm_conformance as GC

from slime_amd import _lib

CASES = XC.cases()
FAKE = 0x10000          # a 256-byte aligned address that no refusal path reads


# ------------------------------------------------------------------------------------------------ (1) the case table
def test_the_table_covers_both_bands_and_every_gemm_family():
    assert {c.band for c in CASES} == {"4G", "2G"}
    assert len({c.id for c in CASES}) == len(CASES)
    gemm = [c for c in CASES if c.entry == "slime_gemm_ex" and c.band == "4G"]
    assert {c.params["tile"] for c in gemm} == set(GC.TILE_BM) == set(XC.GEMM_TILES)
    for tile, (bm, n) in XC.GEMM_TILES.items():
        assert bm == GC.TILE_BM[tile] and n == min(GC.TILE_N[tile])
        assert {c.params["form"] for c in gemm if c.params["tile"] == tile} >= set(GC.WAVE_FORMS)
    assert set(XC.GEMM_FORMS) == set(GC.WAVE_FORMS)
    assert {c.params["operand"] for c in gemm} == set(XC.OPERAND_FORMS)
    assert any(c.entry == "slime_gemm_ksplit" for c in CASES) and any(c.params["form"] == "gelu_mix_t" for c in gemm)
    for c in gemm:
        assert 257 <= c.params["M"] <= 529 and c.params["lda"] == c.params["ldc"] == 1 << 23


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_a_truncated_offset_is_seen_and_stays_inside_the_arena(case):
    assert case.arena_bytes <= 16 * XC.GiB, "at most ~16 GiB at a time"
    far = [l for l in case.layout.values() if l.far]
    assert far
    for lay in case.layout.values():
        # the placement rule, for every pointer
        assert lay.ptr_off >= XC.LEAD and lay.ptr_off + max(XC.WRAP, lay.extent) <= case.arena_bytes
    for lay in far:
        true = XC.true_offset(lay.last)
        assert true == lay.extent - 1, f"{lay.name}: the formula does not give the last byte of the layout"
        if case.band == "4G":
            assert true >= 1 << 32, f"{lay.name}: farthest byte offset {true} does not pass 2^32"
        else:
            assert (1 << 31) <= true < (1 << 32), f"{lay.name}: farthest byte offset {true} is not between 2^31 and 2^32"
        true_row = lay.row_at(true)
        assert true_row is not None
        for how, off in XC.truncations(lay.last).items():
            if case.band == "2G" and how.startswith("u32"):
                assert off == true                     # an unsigned 32-bit offset still reaches: only the signed forms are judged
                continue
            if how.endswith("products") and off == true:
                continue                               # a sum of several strides: no single product passes 32 bits, only the sum does
            assert off != true, f"{lay.name}: {how} does not truncate"
            assert 0 <= lay.ptr_off + off < case.arena_bytes, f"{lay.name}: {how} leaves the arena"
            hit = lay.row_at(off)
            assert hit is None or hit != true_row, f"{lay.name}: {how} lands on the row it should have reached"


def test_the_entries_without_strides_reach_past_4_gib_within_their_limits():
    """The front end, the tower pass and the Llama attention call take no stride: n carries them past 2^32.  Held here: which buffers
    and workspace regions pass 2^32 bytes (and which, named in the cases' docstrings, do not), the limits that bound n (batch <= 65535
    in both attention entries, ~16 GiB of buffers), that an offset of the last rows cut to 32 bits lands elsewhere inside the same
    workspace -- so the last crops, which are compared, miss their data --, and the workspace formulas against the library's queries."""
    lib = _lib.load()
    G32 = 1 << 32
    # tower
    t = XC.tower_extent_case()
    plan, M = t["plan"], t["n"] * t["S"]
    assert t["n"] <= 65535 and M < 1 << 31                     # slime_attention's grid.y; api.hip keeps n * S in an int
    assert plan["lo"] == 0 and plan["xn"] < G32 and plan["qkv"] < G32 < plan["qkv"] + M * 3 * t["D"] * 2          # the tail of qkv
    assert plan["ctx"] > G32 and plan["stats"] > G32 and plan["ff"] + M * t["inter"] * 2 > G32 and t["pixel_bytes"] > G32
    assert t["out_bytes"] < G32                                # stated: out stays below 2^32 at this n
    assert t["pixel_bytes"] + plan["total"] + t["out_bytes"] + XC.LEAD <= 16 * XC.GiB
    d = _lib.VitDesc(hidden=t["D"], inter=t["inter"], heads=t["D"] // 64, layers_run=1, image=t["image"], patch=t["patch"],
                     kpad=(3 * t["patch"] ** 2 + 63) // 64 * 64, dtype=_lib.BF16, eps=1e-5)
    for name, _ in _lib.VitDesc._fields_[9:]:
        setattr(d, name, FAKE)
    assert lib.slime_vit_check(C.byref(d)) == 0, lib.slime_last_error().decode()
    for n in (1, 4, 777, t["n"]):
        assert lib.slime_vit_workspace_bytes(C.byref(d), n) == XC.vit_plan(n, t["S"], t["D"], t["inter"])["total"]
    last_stat = plan["stats"] + (M - 1) * (t["D"] // 64) * 8
    # cut to 32 bits, the last statistics row lands elsewhere INSIDE the workspace: the right place keeps the sentinel, which the last
    # crops (the ones compared) then read
    assert (last_stat & (G32 - 1)) != last_stat and (last_stat & (G32 - 1)) < plan["total"]
    # llama
    a = XC.llama_extent_case()
    assert a["batch"] <= 65535 and a["rows"] == a["batch"] * a["S"]
    assert a["qkv_bytes"] > G32 and a["ctx_off"] > G32 and a["x_bytes"] > G32 and a["out_bytes"] > G32
    la = _lib.LlamaAttnDesc(hidden=a["hidden"], n_heads=a["hq"], n_kv_heads=a["hkv"], head_dim=128, dtype=_lib.BF16)
    for name, _ in _lib.LlamaAttnDesc._fields_[5:]:
        setattr(la, name, FAKE)
    need = lib.slime_llama_attn_workspace_bytes(C.byref(la), a["batch"], a["S"])
    assert a["ctx_off"] + a["ctx_bytes"] <= need <= a["ctx_off"] + a["ctx_bytes"] + 512
    assert a["x_bytes"] + a["out_bytes"] + need + XC.LEAD <= 18.1 * XC.GiB       # the one case above ~16 GiB: three buffers of 5.3 GiB
    last_ctx = a["ctx_off"] + (a["rows"] - 1) * a["hq"] * 256
    assert (last_ctx & (G32 - 1)) != last_ctx and (last_ctx & (G32 - 1)) < a["qkv_bytes"]      # ... in the q/k/v rows of early sequences
    # front end
    f = XC.front_end_extent_case()
    assert f["pixel_bytes"] > G32 and all(r * f["D"] * 2 > G32 for r in f["rows"].values())
    assert all(r * f["D"] < G32 for r in f["rows"].values())   # stated: the byte plane lo8 and stats stay below 2^32
    assert f["pixel_bytes"] + max(f["rows"].values()) * (f["D"] * 3 + f["D"] // 64 * 8) + XC.LEAD <= 16 * XC.GiB
    assert (f["image"] // f["patch"]) ** 2 == f["P"] and 1 <= f["n_prefix"] <= 17 and f["kpad"] == 640


def test_truncations_are_what_32_bit_registers_hold():
    t = ((255, 1 << 24, 2), (127,))
    got = XC.truncations(t)
    assert XC.true_offset(t) == 255 * (1 << 25) + 127
    assert got["u32"] == (255 * (1 << 25) + 127) % (1 << 32) == (127 << 25) + 127
    assert got["i32"] == got["u32"] - (1 << 32)
    assert got["u32 products"] == got["u32"] and got["i32 products"] == got["i32"]
    # the defect of the issue: row 128 of a 256-row tile at lda = 2^24 reads row 0
    assert XC.truncations(((128, 1 << 24, 2),))["u32"] == 0


def test_the_arena_sees_a_stray_write_and_a_wrapped_read():
    """The Arena at 1 / 2^16 of its scale, on the CPU: a write one byte past a window, a write into a guard row and a write on another
    operand's window are all seen; a read at a wrapped offset returns other bits than the row it should have reached."""
    lead, wrap, stride = 1 << 15, 1 << 16, 1 << 8                  # 2 GiB, 4 GiB and the 16 MiB rows, each / 2^16
    rows, width = 273, 16
    vals = torch.randn(rows, width, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert len({bytes(r) for r in vals.view(torch.uint8).numpy()}) == rows, "distinct rows"

    def fresh():
        a = XC.Arena(lead + rows * stride + 1024, "cpu", lead=lead, wrap=wrap)
        a.place(XC.Layout("x", lead, XC.strided_rows(rows, stride), width * 2, torch.bfloat16, False), vals)
        a.place(XC.Layout("y", lead + 64, XC.strided_rows(rows, stride), width * 2, torch.bfloat16, True))
        return a

    a = fresh()
    assert torch.equal(a.read("x").view(torch.uint8), vals.view(torch.uint8))
    a.buf[lead + 64 + 5 * stride:lead + 64 + 5 * stride + 32] = 1            # row 5 of the output, as a kernel would write it
    outs = a.check_untouched()
    assert set(outs) == {"y"} and bool((outs["y"][5].view(torch.uint8) == 1).all()) and bool((outs["y"][4].view(torch.uint8) == 0x7B).all())
    assert a.all_sentinel() and not a.windows                       # clean and reusable
    for stray in (lead + 64 + 5 * stride + 32,                      # one byte past a row of y
                  lead + 7 * stride + 128,                          # a guard byte between two rows
                  lead - 1, 0, a.nbytes - 1):                       # in front of the first pointer, the arena's first and last byte
        a = fresh()
        a.buf[stray] = 0
        with pytest.raises(AssertionError, match="outside every operand window"):
            a.check_untouched()
    # a row offset cut to 16 bits (the scaled 32): row 256 of x reads row 0
    off = (256 * stride) & 0xFFFF
    assert off == 0 and not torch.equal(fresh().read("x")[0], vals[256])
    with pytest.raises(AssertionError, match="placement rule"):
        XC.Arena(1 << 20, "cpu", lead=lead, wrap=wrap).place(XC.Layout("z", lead - 16, [0], 16, torch.uint8))
    with pytest.raises(AssertionError, match="overlap"):
        fresh().place(XC.Layout("z", lead + 32, [0], 64, torch.uint8))


# ------------------------------------------------------------------------------------------------ (2) the header against _SIGNATURES
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)


def _declarations():
    """name -> (return type, [argument types]) of every function the header declares, as normalised C type strings."""
    text = re.sub(r"^\s*#.*$", "", _header_text(), flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r"enum\s*\{.*?\}\s*;", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(slime_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        out[name] = (_norm(ret, False), [] if args.strip() in ("", "void") else [_norm(a, True) for a in args.split(",")])
    return out


def _norm(decl: str, has_name: bool) -> str:
    """'const long long* row_off' -> 'long long*'; 'int64_t* src' -> 'int64_t*'; 'long q_bs' -> 'long'."""
    d = re.sub(r"\bconst\b|\bextern\b|\"C\"", " ", decl)
    d = d.replace("*", " * ")
    toks = d.split()
    if has_name and toks[-1] != "*" and len(toks) > 1:
        toks = toks[:-1]
    return " ".join(toks).replace(" *", "*")


EIGHT_BYTE = {"long", "long long", "size_t", "int64_t", "unsigned long", "unsigned long long", "uint64_t"}
FOUR_BYTE_INT = {"int", "int32_t", "unsigned", "unsigned int", "uint32_t"}


def _is_pointer(ct) -> bool:
    return ct in (C.c_void_p, C.c_char_p) or (isinstance(ct, type) and issubclass(ct, C._Pointer))


def _matches(ctype_decl: str, ct) -> bool:
    if ctype_decl.endswith("*"):
        return ct is not None and _is_pointer(ct)
    if ctype_decl == "void":
        return ct is None
    if ct is None or _is_pointer(ct):
        return False
    if ctype_decl in FOUR_BYTE_INT:
        return ct in (C.c_int, C.c_uint, C.c_int32, C.c_uint32) and C.sizeof(ct) == 4
    if ctype_decl == "float":
        return ct is C.c_float
    if ctype_decl == "double":
        return ct is C.c_double
    if ctype_decl in EIGHT_BYTE:
        return issubclass(ct, C._SimpleCData) and ct not in (C.c_float, C.c_double) and C.sizeof(ct) == 8
    raise AssertionError(f"a C type this test does not know: {ctype_decl!r}")


def test_every_signature_has_the_headers_count_and_widths():
    decls = _declarations()
    assert sorted(decls) == _lib.header_symbols(), "the declaration parser and header_symbols() disagree"
    assert set(decls) == set(_lib._SIGNATURES), set(decls) ^ set(_lib._SIGNATURES)
    assert len(decls) >= 70
    bad = []
    for name, (ret, args) in sorted(decls.items()):
        res, argtypes = _lib._SIGNATURES[name]
        if not _matches(ret, res):
            bad.append(f"{name}: returns {ret}, bound as {res}")
        if len(args) != len(argtypes):
            bad.append(f"{name}: {len(args)} arguments in the header, {len(argtypes)} bound")
            continue
        for i, (a, ct) in enumerate(zip(args, argtypes)):
            if not _matches(a, ct):
                bad.append(f"{name}: argument {i} is {a}, bound as {ct}")
    assert not bad, "\n".join(bad)


def test_the_parser_reads_widths():
    d = _declarations()
    assert d["slime_attention"][1][:3] == ["void*", "long", "long"] and d["slime_attention"][0] == "int"
    assert d["slime_router_scores_batched"][1][1] == "long long*"
    assert d["slime_splice_rows"][1][6] == "int64_t*" and d["slime_splice_rows"][1][2] == "long"
    assert d["slime_gemm_packed_b_bytes"] == ("size_t", ["int", "int"])
    assert d["slime_last_error"] == ("char*", []) and d["slime_abi_version"] == ("int", [])
    assert not _matches("long", C.c_int) and not _matches("int", C.c_long) and not _matches("long", C.c_double)
    assert _matches("long", C.c_long) and _matches("long long", C.c_longlong) and _matches("size_t", C.c_size_t)
    assert not _matches("void*", C.c_long) and not _matches("long", C.c_void_p)


def _struct_fields(struct_name: str):
    """[(field name, normalised type)] of a typedef struct of the header, in order (array fields as 'uint8_t[3]')."""
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + struct_name + r"\s*;", _header_text())
    assert m, struct_name
    out = []
    for stmt in m.group(1).split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        parts = [p.strip() for p in stmt.split(",")]
        head = parts[0]
        arr = re.search(r"\[(\d+)\]$", head)
        base = _norm(re.sub(r"\[\d+\]$", "", head), True)
        first = re.sub(r"\[\d+\]$", "", head).replace("*", " ").split()[-1]
        out.append((first, base + (f"[{arr.group(1)}]" if arr else "")))
        for extra in parts[1:]:                      # `int src_h, src_w;`: further declarators share a non-pointer type
            assert "*" not in base and "*" not in extra and "[" not in extra, stmt
            out.append((extra, base))
    return out


@pytest.mark.parametrize("struct_name, mirror", [("slime_slice_job", _lib.SliceJob), ("slime_view_job", _lib.ViewJob)])
def test_job_struct_mirrors_have_the_headers_widths(struct_name, mirror):
    fields = _struct_fields(struct_name)
    assert [f for f, _ in fields] == [f for f, _ in mirror._fields_], "field order"
    for (fname, ctype_decl), (_, ct) in zip(fields, mirror._fields_):
        if ctype_decl.endswith("]"):
            n = int(ctype_decl[ctype_decl.index("[") + 1:-1])
            assert C.sizeof(ct) == n and ct._length_ == n, fname
        else:
            assert _matches(ctype_decl, ct), f"{struct_name}.{fname} is {ctype_decl}, mirrored as {ct}"
    longs = [f for f, t in fields if t == "long"]
    assert longs and all(C.sizeof(dict(mirror._fields_)[f]) == 8 for f in longs)


# ------------------------------------------------------------------------------------------------ (3) the lda limit
def _args(M=256, N=256, K=64, **kw):
    f = dict(A=FAKE, lda=K, B=FAKE, bias=FAKE, C=FAKE, ldc=N, M=M, N=N, K=K, dtype=_lib.BF16, epilogue=_lib.EPI_BIAS_T)
    f.update(kw)
    return _lib.GemmArgs(**f)


def test_gemm_lda_limit_is_refused_with_the_limit_named():
    lib = _lib.load()
    EINVAL, EWORKSPACE = -1, -2
    # "accepted" is read off slime_gemm_ksplit returning SLIME_EWORKSPACE for a 256-byte workspace at made-up pointers.  THIS DEPENDS
    # ON THE ORDER of the checks in slime_gemm_ksplit: gemm_check_args (all of slime_gemm_ex's argument checks, the lda limit among
    # them) first, the workspace check after it, and both before any device call -- the order include/slime_hip.h documents ("every
    # check precedes the first launch").  A reordering would show here as EWORKSPACE for the refused values, or as a device call.
    short_ws = lambda g: lib.slime_gemm_ksplit(C.byref(g), 2, FAKE, 256, None)
    for lda in (XC.GEMM_LD_REFUSED, 8421512, (1 << 31) - 8):
        g = _args(lda=lda, K=128)
        assert lib.slime_gemm_ex(C.byref(g), None) == EINVAL
        msg = lib.slime_last_error().decode()
        assert f"lda={lda}" in msg and "4294967296" in msg and "8388608" in msg and "(256 - 1) * lda * 2 + K * 2" in msg, msg
        assert short_ws(g) == EINVAL and lib.slime_last_error().decode() == msg
    # the refusal is the formula's: (256 - 1) * lda * 2 + K * 2 <= 2^32
    for lda, K, ok in ((1 << 23, 128, True), (1 << 23, 1 << 23, True), ((1 << 23) + 8, 1 << 23, False), (8421504, 128, True), (8421512, 128, False)):     # 8421504: the sum is 2^32 exactly
        assert ((XC.GEMM_MAX_TILE_ROWS - 1) * lda * 2 + K * 2 <= 1 << 32) == ok
        rc = short_ws(_args(lda=lda, K=K, M=273, N=128))
        assert rc == (EWORKSPACE if ok else EINVAL), (lda, K, rc, lib.slime_last_error().decode())
    # with the limit in force the direct-B kernel's 128-row tile needs no rule of its own: a fragment image stays usable at 2^23
    assert short_ws(_args(lda=1 << 23, K=128, B_frag=FAKE, epilogue=_lib.EPI_BIAS_F32)) == EWORKSPACE
