"""Address-extent conformance on the GPU (tests/extent_conformance.py holds the placement rule and the case table;
tests/test_extent_bound_cpu.py proves that every case can see a truncated offset).  Every case runs its entry point once on compact
buffers -- calls the element-wise conformance tests already bound against float64 -- and once with the same values laid out far, in
an arena of sentinel bytes: row strides of 16 MiB, row counts and tables whose byte extent passes 2^32 (and, for the "2G" rows, lies
between 2^31 and 2^32).  The outputs must be BIT-EQUAL and every byte of the arena outside the operands' windows untouched.  Calls go
through ``_lib.load()`` with its declared argtypes, so a wrong width in ``_lib._SIGNATURES`` fails here too.  Compute stays tiny: only
the extent is large.  One arena (about 11 GiB) is allocated for the module and is clean again after every case.

The entries that take no stride (the three front-end forms, one tower layer, one Llama attention call) come first: their crop / token
count carries pixels, output rows and workspace regions past 2^32, their buffers are cut from one sentinel pool by the same placement
rule, and the first and last crops must equal a small call of the same inputs bit for bit.

A case skips only when the device has less free memory than the arena (or the pool) needs.
"""
import ctypes as C

import pytest
import torch

import extent_conformance as XC
import gemm_conformance as GC

pytestmark = pytest.mark.gpu

CASES = XC.cases()
BY_ENTRY = {}
for _c in CASES:
    BY_ENTRY.setdefault(_c.entry, []).append(_c)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ARENA_BYTES = max(c.arena_bytes for c in CASES)


def _ids(entry):
    return [c.ident for c in BY_ENTRY[entry]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena(dev):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < ARENA_BYTES + 2 * XC.GiB:
        pytest.skip(f"{free >> 30} GiB free on the device, the arena needs {ARENA_BYTES >> 30} GiB and 2 GiB beside it")
    a = XC.Arena(ARENA_BYTES, dev)
    yield a
    print(f"\nextent conformance: arena {ARENA_BYTES / XC.GiB:.2f} GiB, peak device memory {torch.cuda.max_memory_allocated() / XC.GiB:.2f} GiB")
    del a.buf
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(far, compact, what):
    assert far.shape[0] == compact.shape[0], what
    a, b = _bits(far).reshape(far.shape[0], -1), _bits(compact).reshape(compact.shape[0], -1)
    if not torch.equal(a, b):
        rows = (a != b).any(1).nonzero().view(-1)
        raise AssertionError(f"{what}: the far run differs in bits from the compact run in {len(rows)} of {a.shape[0]} rows, first row {int(rows[0])}")


def _code(dtype):
    return {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}[dtype]


class _forced:
    """the diagnostic library with one kernel family forced (tile 0: the product library and its own dispatch)"""

    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        from slime_amd import _lib
        if not self.tile:
            return _lib.load()
        self.ctx = _lib.diag()
        self.lib = self.ctx.__enter__()
        self.lib.slime_gemm_force_tile(self.tile)
        return self.lib

    def __exit__(self, *exc):
        if not self.tile:
            return False
        self.lib.slime_gemm_force_tile(0)
        return self.ctx.__exit__(*exc)


# ------------------------------------------------------------------------------------------------ entries without strides (n is the reach)
# These run BEFORE the first test that asks for the arena (a module fixture, created on first use), so that their buffers and the
# arena never exist together.  The buffers of a far call are cut from ONE pool of sentinel bytes by the arena's placement rule: the
# first one starts LEAD = 2 GiB inside the pool, GUARD bytes separate them, and the last one is the largest (more than 4 GiB), so an
# offset cut to 32 bits, signed or unsigned, stays inside the allocation; afterwards every byte of the pool outside the buffers must
# be the sentinel still.
GUARD = 1 << 20


class Pool:
    def __init__(self, dev, parts):
        """parts: [(name, nbytes)], laid out in this order behind the lead; the last one must hold XC.WRAP bytes or more"""
        self.span, off = {}, XC.LEAD
        for name, nbytes in parts:
            self.span[name] = (off, nbytes)
            off = (off + nbytes + GUARD + 255) // 256 * 256
        assert parts[-1][1] >= XC.WRAP, "the last buffer is what a wrapped offset from any pointer falls into"
        self.nbytes = off
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free < self.nbytes + 2 * XC.GiB:
            pytest.skip(f"{free >> 30} GiB free on the device, the case needs {self.nbytes >> 30} GiB and 2 GiB beside it")
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.buf.fill_(XC.SENTINEL_BYTE)

    def ptr(self, name):
        return self.buf.data_ptr() + self.span[name][0]

    def view(self, name, dtype=torch.uint8):
        off, nbytes = self.span[name]
        return self.buf[off:off + nbytes].view(dtype)

    def guards_intact(self) -> bool:
        edges = [0] + [e for off, nbytes in sorted(self.span.values()) for e in (off, off + nbytes)] + [self.nbytes]
        step = 1 << 28                                       # in pieces: no mask of the lead's size
        return all(bool((self.buf[a:min(a + step, hi)] == XC.SENTINEL_BYTE).all())
                   for lo, hi in zip(edges[0::2], edges[1::2]) for a in range(lo, hi, step))


def _sentinel_row(rows2d, chunk=1 << 18):
    """True iff some row of the uint8 [rows, width] tensor still is all sentinel bytes (in chunks: no mask of the tensor's size)"""
    return any(bool((rows2d[lo:lo + chunk] == XC.SENTINEL_BYTE).all(1).any()) for lo in range(0, rows2d.shape[0], chunk))


def _fill_normal(t, seed, scale=1.0, chunk=1 << 28):
    """t ~ N(0, scale^2) in place, in chunks (no second tensor of t's size)"""
    g, flat = _gen(t.device, seed), t.view(-1)
    for lo in range(0, flat.numel(), chunk):
        flat[lo:lo + chunk].normal_(0.0, scale, generator=g)


def _small(nbytes, dev):
    return _sentinel((nbytes + GUARD,), torch.uint8, dev)


def test_front_end_with_pixels_and_rows_past_4_gib(dev):
    """slime_patch_embed_prenorm / _plain / _prefix at 224 / 14, D = 1024, n = 8200: the fp32 pixel buffer (4.9 GB) and the x16 rows
    (4.3 GB) pass 2^32 bytes.  The first and the last three crops of x16, lo8 and stats must equal a six-crop call of the same pixels
    bit for bit, no row may keep the sentinel, and every byte of the pool outside the buffers stays."""
    from slime_amd import _lib
    lib, c = _lib.load(), XC.front_end_extent_case()
    n, I, patch, D, P, kpad, npre = c["n"], c["image"], c["patch"], c["D"], c["P"], c["kpad"], c["n_prefix"]
    assert c["pixel_bytes"] > 1 << 32 and min(c["rows"].values()) * D * 2 > 1 << 32
    g = _gen(dev, 20)
    w = torch.zeros(D, kpad, device=dev)
    w[:, :3 * patch * patch] = torch.randn(D, 3 * patch * patch, generator=g, device=dev) * (3 * patch * patch) ** -0.5
    wf = torch.empty(D * kpad, dtype=torch.bfloat16, device=dev)
    wb = w.to(torch.bfloat16).contiguous()
    assert lib.slime_gemm_pack_b(wb.data_ptr(), D, kpad, wf.data_ptr(), _stream()) == 0, lib.slime_last_error().decode()
    cls, ln_w, ln_b = (torch.randn(D, generator=g, device=dev) for _ in range(3))
    pos = torch.randn(P + 1, D, generator=g, device=dev)
    pos_p = pos[1:].contiguous()
    prefix = torch.randn(npre, D, generator=g, device=dev)

    def call(form, pixels, m, x16, lo8, stats):
        a = (pixels, _lib.F32, wf.data_ptr())
        z = (None, x16, lo8, stats, _lib.BF16, m, I, patch, kpad, D, _stream())
        if form == "prenorm":
            rc = lib.slime_patch_embed_prenorm(*a, cls.data_ptr(), pos.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), 1e-5, *z)
        elif form == "plain":
            rc = lib.slime_patch_embed_plain(*a, pos_p.data_ptr(), *z)
        else:
            rc = lib.slime_patch_embed_prefix(*a, prefix.data_ptr(), npre, pos_p.data_ptr(), *z)
        torch.cuda.synchronize()
        assert rc == 0, f"{form}: {lib.slime_last_error().decode()}"

    for form, rows in c["rows"].items():
        sizes = {"stats": rows * (D // 64) * 8, "lo8": rows * D, "px": c["pixel_bytes"], "x16": rows * D * 2}
        pool = Pool(dev, list(sizes.items()))
        px = pool.view("px", torch.float32).view(n, 3 * I * I)
        _fill_normal(px, 21)
        six = torch.cat([px[:3], px[-3:]]).contiguous()
        call(form, pool.ptr("px"), n, pool.ptr("x16"), pool.ptr("lo8"), pool.ptr("stats"))
        assert pool.guards_intact(), f"{form}: a byte of the pool outside the buffers was written"
        small = {k: _small(sizes[k] // n * 6, dev) for k in ("x16", "lo8", "stats")}
        call(form, six.data_ptr(), 6, small["x16"].data_ptr(), small["lo8"].data_ptr(), small["stats"].data_ptr())
        for name in ("x16", "lo8", "stats"):
            crop_bytes = sizes[name] // n
            assert bool((small[name][crop_bytes * 6:] == XC.SENTINEL_BYTE).all()), f"{form}: bytes behind the six-crop {name} were written"
            fr = pool.view(name).view(n, crop_bytes)
            assert torch.equal(torch.cat([fr[:3], fr[-3:]]), small[name][:crop_bytes * 6].view(6, crop_bytes)), \
                f"{form}: {name} of the first / last three of {n} crops differs in bits from the six-crop call"
        assert not _sentinel_row(pool.view("x16").view(rows, D * 2)), f"{form}: a row of x16 was not written"
        del pool, px, fr, small


def test_tower_pass_with_workspace_past_4_gib(dev):
    """slime_vit_forward, one layer, 60 000 crops of the 112 / 16, D = 256 tower: the workspace is 8.5 GB, with the tail of qkv, ctx, most
    of ff and stats past 2^32 bytes from ws (offsets derived here from the plan's formula and held to slime_vit_workspace_bytes), and
    4.5 GB of bf16 pixels.  The first and last two crops must equal a four-crop pass of the same crops bit for bit (shard invariance
    is an existing guarantee); no output row keeps the sentinel; every byte of the pool outside out, pixels and ws stays."""
    import tower_conformance as TC
    from slime_amd import _lib, ops
    lib, c = _lib.load(), XC.tower_extent_case()
    n, I, D, S, plan = c["n"], c["image"], c["D"], c["S"], c["plan"]
    cfg = TC.tower_config(I, c["patch"], D, c["inter"], 1)
    pt = ops.pack_tower(TC.tower_state(cfg), cfg, torch.bfloat16, dev, select_layer=1)
    assert pt.desc.layers_run == 1 and cfg.seq_len == S and n <= 65535
    need = lib.slime_vit_workspace_bytes(C.byref(pt.desc), n)
    assert need == plan["total"], "the plan's formula (extent_conformance.vit_plan) is not the library's"
    assert plan["stats"] > 1 << 32 and plan["qkv"] < 1 << 32 < plan["ctx"] and c["pixel_bytes"] > 1 << 32
    pool = Pool(dev, [("out", c["out_bytes"]), ("px", c["pixel_bytes"]), ("ws", need)])
    px = pool.view("px", torch.bfloat16).view(n, 3 * I * I)
    _fill_normal(px, 22)
    four = torch.cat([px[:2], px[-2:]]).contiguous()
    rc = lib.slime_vit_forward(C.byref(pt.desc), pool.ptr("px"), _lib.BF16, n, pool.ptr("out"), _lib.BF16, 0, None, pool.ptr("ws"), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert pool.guards_intact(), "the tower wrote outside out and its workspace"
    far = pool.view("out").view(n, (S - 1) * D * 2)
    assert not _sentinel_row(far.view(n * (S - 1), D * 2)), "an output row was not written"
    nb_out, nb_ws = 4 * (S - 1) * D * 2, lib.slime_vit_workspace_bytes(C.byref(pt.desc), 4)
    out, ws = _small(nb_out, dev), _small(nb_ws, dev)
    rc = lib.slime_vit_forward(C.byref(pt.desc), four.data_ptr(), _lib.BF16, 4, out.data_ptr(), _lib.BF16, 0, None, ws.data_ptr(), nb_ws, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    small = out[:nb_out].view(4, (S - 1) * D * 2)
    assert torch.equal(torch.cat([far[:2], far[-2:]]), small), "the first / last two of 60 000 crops differ in bits from the four-crop pass"
    assert len({bytes(r[:64]) for r in small.cpu().numpy()}) == 4, "distinct crops"


def test_llama_attention_with_workspace_past_4_gib(dev):
    """slime_llama_attn_forward on the smallest head-shard slice (hidden 512, one query and one kv head), 43 750 sequences of 128
    tokens: the packed q/k/v rows end past 2^32 bytes, the context rows start there, x and out are 5.7 GB each.  The first and the last
    sequence must equal a two-sequence call bit for bit."""
    from slime_amd import _lib, ops
    lib, c = _lib.load(), XC.llama_extent_case()
    hidden, hq, hkv, batch, S, rows = c["hidden"], c["hq"], c["hkv"], c["batch"], c["S"], c["rows"]
    g = torch.Generator().manual_seed(7)
    w = [torch.randn(a, b, generator=g) * b ** -0.5 for a, b in ((hq * 128, hidden), (hkv * 128, hidden), (hkv * 128, hidden), (hidden, hq * 128))]
    pa = ops.pack_llama_attention(w[0], w[1], w[2], w[3], hq, hkv, torch.bfloat16, dev)
    need = lib.slime_llama_attn_workspace_bytes(C.byref(pa.desc), batch, S)
    assert c["ctx_off"] + c["ctx_bytes"] <= need <= c["ctx_off"] + c["ctx_bytes"] + 512
    assert c["qkv_bytes"] > 1 << 32 and c["ctx_off"] > 1 << 32 and c["x_bytes"] > 1 << 32 and batch <= 65535
    pool = Pool(dev, [("x", c["x_bytes"]), ("out", c["out_bytes"]), ("ws", need)])
    x = pool.view("x", torch.bfloat16).view(batch, S * hidden)
    _fill_normal(x, 23)
    two = torch.stack([x[0], x[-1]]).contiguous()
    pos = torch.arange(S, dtype=torch.int32, device=dev).repeat(batch).contiguous()
    rc = lib.slime_llama_attn_forward(C.byref(pa.desc), pool.ptr("x"), pos.data_ptr(), None, None, batch, S, pool.ptr("out"), _lib.BF16,
                                      pool.ptr("ws"), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert pool.guards_intact(), "the layer wrote outside out and its workspace"
    far = pool.view("out").view(batch, S * hidden * 2)
    assert not _sentinel_row(far.view(rows, hidden * 2)), "an output row was not written"
    nb_out, nb_ws = 2 * S * hidden * 2, lib.slime_llama_attn_workspace_bytes(C.byref(pa.desc), 2, S)
    out, ws = _small(nb_out, dev), _small(nb_ws, dev)
    rc = lib.slime_llama_attn_forward(C.byref(pa.desc), two.data_ptr(), pos.data_ptr(), None, None, 2, S, out.data_ptr(), _lib.BF16,
                                      ws.data_ptr(), nb_ws, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    small = out[:nb_out].view(2, S * hidden * 2)
    assert torch.equal(torch.stack([far[0], far[-1]]), small), "the first / last of 43 750 sequences differ in bits from the two-sequence call"
    assert not torch.equal(small[0], small[1])


# ------------------------------------------------------------------------------------------------ slime_gemm_ex / slime_gemm_ksplit
def _gemm_call(lib, fields, splits, dev):
    from slime_amd import _lib
    g = _lib.GemmArgs(**fields)
    if splits == 1:
        rc = lib.slime_gemm_ex(C.byref(g), _stream())
    else:
        nbytes = lib.slime_gemm_ksplit_workspace_bytes(fields["M"], fields["N"], splits)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rc = lib.slime_gemm_ksplit(C.byref(g), splits, ws.data_ptr(), nbytes, _stream())
    torch.cuda.synchronize()
    return rc


def _run_gemm(arena, dev, case):
    p, lay = case.params, case.layout
    dtype, form, M, N, K = DT[p["dtype"]], p["form"], p["M"], p["N"], p["K"]
    c = GC.make_case("random", dtype, form, M, N, K, guard="attract", alias=p["alias"], seed=M + K, device=dev)
    b = c.buf
    in_place = form in ("resid_f32", "resid_f32_ln", "resid_split_ln") or (form == "resid_t" and p["alias"])
    with _forced(p["tile"]) as lib:
        frag = None
        if p["operand"] != "B":
            frag = torch.empty(N * K + GC.TAIL, dtype=dtype, device=dev)
            assert lib.slime_gemm_pack_b(b["B"].ptr(), N, K, frag.data_ptr(), _stream()) == 0, lib.slime_last_error().decode()
        base = c.arg_fields(p["operand"], frag.data_ptr() if frag is not None else None)
        # ---- far: the same values, rows 16 MiB apart
        arena.place(lay["A"], b["A"].win)
        far = dict(base, A=arena.ptr("A"), lda=p["lda"], ldc=p["ldc"])
        rm = None
        if p["row_map"] is not None:
            rm = torch.tensor(p["row_map"], dtype=torch.int32, device=dev)
            far.update(row_map=rm.data_ptr())
        arena.place(lay["C"], b["C"].win if in_place else None)
        far.update(C=arena.ptr("C"))
        if "A2" in lay:
            arena.place(lay["A2"], b["A2"].win)
            far.update(A2=arena.ptr("A2"))
        if "x16" in lay:
            arena.place(lay["x16"])
            far.update(x16=arena.ptr("x16"), ldx=p["ldx"])
        if "lo8" in lay:
            arena.place(lay["lo8"], b["lo8"].win)
            far.update(lo8=arena.ptr("lo8"), ldlo=p["ldlo"])
        if form == "resid_t":
            if p["alias"]:
                far.update(resid=arena.ptr("C"), ldr=p["ldc"])
            else:
                arena.place(lay["resid"], b["resid"].win)
                far.update(resid=arena.ptr("resid"), ldr=p["ldr"])
        rc = _gemm_call(lib, far, p["splits"], dev)
        assert rc == 0, f"{case.id}: far call returned {rc}: {lib.slime_last_error().decode()}"
        far_stats = b["stats_out"].win.clone() if "stats_out" in b else None
        outs = arena.check_untouched()
        # ---- compact: the call the element-wise conformance tests bound against float64
        c.restore()
        rc = _gemm_call(lib, base, p["splits"], dev)
        assert rc == 0, f"{case.id}: compact call returned {rc}: {lib.slime_last_error().decode()}"
    want = c.windows()
    for name in c.outputs:
        got = far_stats if name == "stats_out" else outs[name]
        _same_bits(got, want[name], f"{case.id}: {name}")


@pytest.mark.parametrize("case", BY_ENTRY["slime_gemm_ex"], ids=_ids("slime_gemm_ex"))
def test_gemm_ex(arena, dev, case):
    """Every kernel family (forced in the diagnostic library) x every epilogue form: lda = ldc = ldx = ldr = 2^23 elements, ldlo = 2^23
    bytes with 529 rows, the row map into rows past 2^32 bytes, A2, the in-place split residual; the three operand forms in turn."""
    _run_gemm(arena, dev, case)


@pytest.mark.parametrize("case", BY_ENTRY["slime_gemm_ksplit"], ids=_ids("slime_gemm_ksplit"))
def test_gemm_ksplit(arena, dev, case):
    _run_gemm(arena, dev, case)


@pytest.mark.parametrize("entry", ["slime_gemm_ex", "slime_gemm_ksplit"])
def test_gemm_lda_past_the_tile_offsets_is_refused(arena, dev, entry):
    """lda = 2^24, M = 256 on a 256-row tile: rows 128..255 of the tile used to be computed from rows 0..127 with SLIME_OK.  Now
    SLIME_EINVAL with the limit named, and nothing is launched (C keeps the sentinel)."""
    M, N, K, ld = 256, 256, 128, XC.GEMM_LD_REFUSED
    c = GC.make_case("random", torch.bfloat16, "bias_t", M, N, K, guard="attract", seed=5, device=dev)
    lay = XC.gemm_layout("bias_t", M, N, K, 2, lda=ld, ldc=XC.GEMM_LD)
    assert lay["A"].extent > 1 << 32 and XC.truncations(((128, ld, 2),))["u32"] == 0
    arena.place(lay["A"], c.buf["A"].win)
    arena.place(lay["C"])
    fields = dict(c.arg_fields("B"), A=arena.ptr("A"), lda=ld, C=arena.ptr("C"), ldc=XC.GEMM_LD)
    with _forced(11 if entry == "slime_gemm_ex" else 0) as lib:
        rc = _gemm_call(lib, fields, 1 if entry == "slime_gemm_ex" else 2, dev)
        msg = lib.slime_last_error().decode()
    assert rc == -1, f"SLIME_EINVAL expected, got {rc}"
    assert f"lda={ld}" in msg and "4294967296" in msg and "8388608" in msg, msg
    outs = arena.check_untouched()
    assert bool((outs["C"].view(torch.uint8) == XC.SENTINEL_BYTE).all()), "a refused call wrote C"


# ------------------------------------------------------------------------------------------------ row kernels
def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


@pytest.mark.parametrize("case", BY_ENTRY["slime_layernorm"], ids=_ids("slime_layernorm"))
def test_layernorm(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    rows, D = p["rows"], p["D"]
    g = _gen(dev, 1)
    x = torch.randn(rows, D, generator=g, device=dev) * 2 + 0.5
    w, b = torch.randn(D, generator=g, device=dev), torch.randn(D, generator=g, device=dev)
    add = torch.randn(7, D, generator=g, device=dev)

    def run(xptr, ldx):
        o32 = torch.empty(rows, D, dtype=torch.float32, device=dev)
        ot, ot2 = (torch.empty(rows, D, dtype=torch.bfloat16, device=dev) for _ in range(2))
        rc = lib.slime_layernorm(xptr, ldx, rows, D, w.data_ptr(), b.data_ptr(), 1e-5, 1, o32.data_ptr(), ot.data_ptr(), ot2.data_ptr(),
                                 add.data_ptr(), 7, _lib.BF16, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return o32, ot, ot2

    arena.place(case.layout["x"], x)
    far = run(arena.ptr("x"), p["ldx"])
    arena.check_untouched()
    for name, f, cpt in zip(("out_f32", "out_t", "out_t2"), far, run(x.data_ptr(), D)):
        _same_bits(f, cpt, f"{case.id}: {name}")


@pytest.mark.parametrize("case", BY_ENTRY["slime_rope"], ids=_ids("slime_rope"))
def test_rope(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    rows, heads, hd = p["rows"], p["heads"], p["head_dim"]
    g = _gen(dev, 2)
    x = torch.randn(rows, heads * hd, generator=g, device=dev).to(torch.bfloat16)
    pos = torch.randint(0, 4096, (rows,), generator=g, device=dev).to(torch.int32)
    inv = (10000.0 ** (-torch.arange(0, hd, 2, device=dev).float() / hd)).contiguous()

    def run(ptr, stride):
        rc = lib.slime_rope(ptr, stride, pos.data_ptr(), rows, heads, 1, hd, inv.data_ptr(), 0.125, _lib.BF16, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["x"], x)
    run(arena.ptr("x"), p["row_stride"])
    far = arena.check_untouched()["x"]
    cpt = x.clone()
    run(cpt.data_ptr(), heads * hd)
    assert not torch.equal(_bits(cpt), _bits(x)), "the compact call rotated nothing"
    _same_bits(far, cpt, f"{case.id}: qkv in place")


def _compact_groups(rows2d, groups, rows_out, pad_front=2, pad_back=3):
    """[groups * rows_out, C] -> the same rows inside a small [groups, pad_front + rows_out + pad_back, C] buffer of other values."""
    C_ = rows2d.shape[1]
    buf = torch.full((groups, pad_front + rows_out + pad_back, C_), 3.0, dtype=rows2d.dtype, device=rows2d.device)
    buf[:, pad_front:pad_front + rows_out] = rows2d.view(groups, rows_out, C_)
    return buf, pad_front + rows_out + pad_back, pad_front


@pytest.mark.parametrize("case", BY_ENTRY["slime_gather_rows"], ids=_ids("slime_gather_rows"))
def test_gather_rows(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    C_, groups, rows_out = p["C"], p["groups"], p["rows_out"]
    src = torch.randn(groups * rows_out, C_, generator=_gen(dev, 3), device=dev)
    cbuf, c_rows_in, c_off = _compact_groups(src, groups, rows_out)
    for odt in (torch.bfloat16, torch.float32):
        def run(ptr, rows_in, off):
            out = torch.empty(groups * rows_out, C_, dtype=odt, device=dev)
            rc = lib.slime_gather_rows(ptr, rows_in, off, out.data_ptr(), _code(odt), groups, rows_out, C_, _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.slime_last_error().decode()
            return out

        arena.place(case.layout["in"], src)
        far = run(arena.ptr("in"), p["rows_in"], p["row_off"])
        arena.check_untouched()
        _same_bits(far, run(cbuf.data_ptr(), c_rows_in, c_off), f"{case.id}: out {odt}")
        assert torch.equal(far.float(), src.to(odt).float())


@pytest.mark.parametrize("case", BY_ENTRY["slime_gather_rows_split"], ids=_ids("slime_gather_rows_split"))
def test_gather_rows_split(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    C_, groups, rows_out = p["C"], p["groups"], p["rows_out"]
    g = _gen(dev, 4)
    hi = torch.randn(groups * rows_out, C_, generator=g, device=dev).to(torch.bfloat16)
    lo = torch.randint(-128, 128, (groups * rows_out, C_), generator=g, device=dev).to(torch.int8)
    chi, c_rows_in, c_off = _compact_groups(hi, groups, rows_out)
    clo, _, _ = _compact_groups(lo, groups, rows_out)

    def run(hptr, lptr, rows_in, off):
        out = torch.empty(groups * rows_out, C_, dtype=torch.float32, device=dev)
        rc = lib.slime_gather_rows_split(hptr, lptr, _lib.BF16, rows_in, off, out.data_ptr(), _lib.F32, groups, rows_out, C_, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return out

    arena.place(case.layout["hi"], hi)
    arena.place(case.layout["lo"], lo)
    far = run(arena.ptr("hi"), arena.ptr("lo"), p["rows_in"], p["row_off"])
    arena.check_untouched()
    _same_bits(far, run(chi.data_ptr(), clo.data_ptr(), c_rows_in, c_off), f"{case.id}: out")
    assert torch.equal(far.double(), GC.join64(hi, lo, torch.bfloat16))


@pytest.mark.parametrize("case", BY_ENTRY["slime_select_crops"], ids=_ids("slime_select_crops"))
def test_select_crops(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    P, C_, per_image, images = p["P"], p["C"], p["per_image"], p["images"]
    n = per_image * images
    feats = torch.randn(n, P * C_, generator=_gen(dev, 5), device=dev).to(torch.bfloat16)
    cbuf, c_period, c_first = _compact_groups(feats, images, per_image)

    def run(ptr, period, first):
        o32 = torch.empty(n, P * C_, dtype=torch.float32, device=dev)
        ot = torch.empty(n, P * C_, dtype=torch.bfloat16, device=dev)
        rc = lib.slime_select_crops(ptr, _lib.BF16, P, C_, period, first, per_image, images, o32.data_ptr(), ot.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return o32, ot

    arena.place(case.layout["feats"], feats)
    far = run(arena.ptr("feats"), p["period"], p["first"])
    arena.check_untouched()
    for name, f, cpt in zip(("out_f32", "out_t"), far, run(cbuf.data_ptr(), c_period, c_first)):
        _same_bits(f, cpt, f"{case.id}: {name}")
    assert torch.equal(_bits(far[1]), _bits(feats))


@pytest.mark.parametrize("case", BY_ENTRY["slime_ln_gather"], ids=_ids("slime_ln_gather"))
def test_ln_gather(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    D, idx = p["D"], p["idx"]
    uniq = sorted(set(idx))
    g = _gen(dev, 6)
    src = torch.randn(len(uniq), D, generator=g, device=dev) * 3 + 1
    w, b = torch.randn(D, generator=g, device=dev), torch.randn(D, generator=g, device=dev)

    def run(ptr, src_rows, index):
        it = torch.tensor(index, dtype=torch.int64, device=dev)
        out = torch.empty(len(index), D, dtype=torch.bfloat16, device=dev)
        rc = lib.slime_ln_gather(ptr, src_rows, it.data_ptr(), len(index), D, w.data_ptr(), b.data_ptr(), 1e-5, out.data_ptr(), _lib.BF16, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return out

    arena.place(case.layout["src"], src)
    far = run(arena.ptr("src"), p["src_rows"], idx)
    arena.check_untouched()
    cpt = run(src.data_ptr(), len(uniq), [uniq.index(i) for i in idx])
    _same_bits(far, cpt, f"{case.id}: out_t")
    assert len({bytes(r) for r in _bits(cpt).cpu().numpy()}) == len(uniq), "the gathered rows are distinct"


# ------------------------------------------------------------------------------------------------ attention
def _run_attention(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    dtype, B, H, HKV, dh, n_q, n_kv = DT[p["dtype"]], p["B"], p["H"], p["HKV"], p["dh"], p["n_q"], p["n_kv"]
    Eq, Ekv = H * dh, HKV * dh
    shared = p["q_bs"] == 0
    g = _gen(dev, n_q + n_kv)
    q = (torch.randn(1 if shared else B, n_q, Eq, generator=g, device=dev) * 0.4).to(dtype)
    k = torch.randn(B, n_kv, Ekv, generator=g, device=dev).to(dtype)
    v = torch.randn(B, n_kv, Ekv, generator=g, device=dev).to(dtype)
    prefill = case.entry == "slime_prefill_attention"
    start = length = None
    if p["ranges"] is not None:
        start = torch.tensor(p["ranges"][0], dtype=torch.int32, device=dev)
        length = torch.tensor(p["ranges"][1], dtype=torch.int32, device=dev)

    def run(qp, q_bs, q_rs, kp, vp, k_bs, k_rs, op, o_bs, o_rs):
        if prefill:
            rc = lib.slime_prefill_attention(qp, q_bs, q_rs, kp, k_bs, k_rs, vp, k_bs, k_rs, op, o_bs, o_rs, B, H, HKV, dh, n_q,
                                             start.data_ptr(), length.data_ptr(), _code(dtype), _stream())
        else:
            rc = lib.slime_attention(qp, q_bs, q_rs, kp, k_bs, k_rs, vp, k_bs, k_rs, op, o_bs, o_rs, B, H, dh, n_q, n_kv, _code(dtype), _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{case.id}: {lib.slime_last_error().decode()}"

    lay = case.layout
    arena.place(lay["q"], q.view(-1, Eq))
    arena.place(lay["k"], k.view(-1, Ekv))
    arena.place(lay["v"], v.view(-1, Ekv))
    arena.place(lay["o"])
    run(arena.ptr("q"), p["q_bs"], p["q_rs"], arena.ptr("k"), arena.ptr("v"), p["k_bs"], p["k_rs"], arena.ptr("o"), p["o_bs"], p["o_rs"])
    far = arena.check_untouched()["o"]
    o = torch.empty(B, n_q, Eq, dtype=dtype, device=dev)
    o.view(torch.uint8).fill_(XC.SENTINEL_BYTE)
    run(q.data_ptr(), 0 if shared else n_q * Eq, Eq, k.data_ptr(), v.data_ptr(), n_kv * Ekv, Ekv, o.data_ptr(), n_q * Eq, Eq)
    assert not bool((_bits(o).reshape(B * n_q, -1) == XC.SENTINEL_BYTE).all(1).any()), "the compact call left an output row unwritten"
    _same_bits(far, o.view(-1, Eq), f"{case.id}: o")


@pytest.mark.parametrize("case", BY_ENTRY["slime_attention"], ids=_ids("slime_attention"))
def test_attention(arena, dev, case):
    """generic head_dim 64, attn64r, generic head_dim 128 (shared q in its batch-stride case): row strides that put the last key row
    and the last query / output row past 2^32 bytes, and batch strides (two batch entries) that do the same."""
    _run_attention(arena, dev, case)


@pytest.mark.parametrize("case", BY_ENTRY["slime_prefill_attention"], ids=_ids("slime_prefill_attention"))
def test_prefill_attention(arena, dev, case):
    """The eight-wave kernel and prefill32, with kv_start / kv_len ranges (rows outside a range are zeroed: still written)."""
    _run_attention(arena, dev, case)


# ------------------------------------------------------------------------------------------------ adapter glue, router, splice
def _sentinel(shape, dtype, dev):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(XC.SENTINEL_BYTE)
    return t


@pytest.mark.parametrize("case", BY_ENTRY["slime_merge_rows_batched"], ids=_ids("slime_merge_rows_batched"))
def test_merge_rows_batched(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    C_, images, per = p["C"], p["images"], p["nw"] * p["nh"] * p["g"] * p["g"]
    src = torch.randn(images * per, C_, generator=_gen(dev, 7), device=dev)

    def run(iptr, iis, optr, ois, row0):
        rc = lib.slime_merge_rows_batched(iptr, iis, optr, _lib.F32, ois, row0, images, p["nw"], p["nh"], p["g"], C_, 1, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["in"], src)
    arena.place(case.layout["out"])
    run(arena.ptr("in"), p["in_image_stride"], arena.ptr("out"), p["out_image_stride"], p["dst_row0"])
    far = arena.check_untouched()["out"]
    cpt = _sentinel((images, per + 5, C_), torch.float32, dev)
    run(src.data_ptr(), per, cpt.data_ptr(), per + 5, 2)
    _same_bits(far, cpt[:, 2:2 + per].reshape(-1, C_), f"{case.id}: out")
    assert sorted(bytes(r) for r in _bits(far).cpu().numpy()) == sorted(bytes(r) for r in _bits(src).cpu().numpy()), "a permutation of the rows"


@pytest.mark.parametrize("case", BY_ENTRY["slime_gate_mix_ex"], ids=_ids("slime_gate_mix_ex"))
def test_gate_mix_ex(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, D, rows, rpg = p["H"], p["D"], p["rows"], p["rows_per_group"]
    g = _gen(dev, 8)
    x, wg = torch.randn(rows, D, generator=g, device=dev), torch.randn(D, 2, generator=g, device=dev) * 0.2
    e0, e1 = torch.randn(rows, H, generator=g, device=dev), torch.randn(rows, H, generator=g, device=dev)

    def run(optr, gs, row0):
        rc = lib.slime_gate_mix_ex(x.data_ptr(), D, wg.data_ptr(), e0.data_ptr(), e1.data_ptr(), optr, _lib.F32, rows, H, rpg, gs, row0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["out"])
    run(arena.ptr("out"), p["group_stride"], p["row0"])
    far = arena.check_untouched()["out"]
    cpt = _sentinel((rows // rpg, rpg + 5, H), torch.float32, dev)
    run(cpt.data_ptr(), rpg + 5, 2)
    _same_bits(far, cpt[:, 2:2 + rpg].reshape(-1, H), f"{case.id}: out")
    assert not bool((_bits(far) == XC.SENTINEL_BYTE).all(1).any())


@pytest.mark.parametrize("case", BY_ENTRY["slime_router_scores_batched"], ids=_ids("slime_router_scores_batched"))
def test_router_scores_batched(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, L, T_max, n_rows = p["H"], p["L"], p["T_max"], p["n_rows"]
    B = len(n_rows)
    g = _gen(dev, 9)
    img = torch.randn(sum(n_rows), H, generator=g, device=dev)
    text = torch.randn(B, L, H, generator=g, device=dev)
    nr = torch.tensor(n_rows, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.slime_router_batched_workspace_floats(B, L, H), dtype=torch.float32, device=dev)

    def run(iptr, row_off):
        ro = torch.tensor(row_off, dtype=torch.int64, device=dev)
        scores = _sentinel((B, T_max), torch.float32, dev)
        rc = lib.slime_router_scores_batched(iptr, ro.data_ptr(), nr.data_ptr(), B, T_max, text.data_ptr(), L, None, H, scores.data_ptr(),
                                             ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return scores

    arena.place(case.layout["img"], img)
    far = run(arena.ptr("img"), p["row_off"])
    arena.check_untouched()
    cpt = run(img.data_ptr(), [0, n_rows[0]])
    _same_bits(far, cpt, f"{case.id}: scores")
    assert len(set(cpt[1, :n_rows[1]].tolist())) == n_rows[1], "distinct scores"


@pytest.mark.parametrize("case", BY_ENTRY["slime_splice_merged"], ids=_ids("slime_splice_merged"))
def test_splice_merged(arena, dev, case):
    """tokens and extra rows past 2^32 bytes; token rows go through bf16 on the way (mid_dtype), extra rows are copied."""
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, src, k_rows, e_rows, n_tab = p["H"], p["src"], p["k_rows"], p["e_rows"], p["table_rows"]
    g = _gen(dev, 14)
    table = torch.randn(n_tab, H, generator=g, device=dev)
    tokens = torch.randn(len(k_rows), H, generator=g, device=dev)
    extra = torch.randn(len(e_rows), H, generator=g, device=dev)

    def run(kptr, n_k, eptr, n_e, index):
        it = torch.tensor(index, dtype=torch.int64, device=dev)
        out = _sentinel((len(index), H), torch.float32, dev)
        rc = lib.slime_splice_merged(table.data_ptr(), _lib.F32, n_tab, kptr, n_k, _lib.BF16, eptr, _lib.F32, n_e, it.data_ptr(), out.data_ptr(),
                                     _lib.F32, len(index), H, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return out

    nk, ne = p["token_rows"], p["extra_rows"]

    def source(s):
        """('table' | 'tokens' | 'extra' | None, index into the compact tensor) of a far src entry"""
        if s >= 0:
            return ("table", s) if s < n_tab else (None, 0)
        if s == -1:
            return None, 0
        k = -2 - s
        if k < nk:
            return "tokens", k_rows.index(k)
        return ("extra", e_rows.index(k - nk)) if k - nk < ne else (None, 0)

    def compact_index(s):
        kind, i = source(s)
        if kind == "table":
            return i
        if kind == "tokens":
            return -2 - i
        if kind == "extra":
            return -2 - (len(k_rows) + i)
        return s if s >= -1 else -2 - (len(k_rows) + len(e_rows) + 4)          # zeros there as here

    arena.place(case.layout["tokens"], tokens)
    arena.place(case.layout["extra"], extra)
    far = run(arena.ptr("tokens"), nk, arena.ptr("extra"), ne, src)
    arena.check_untouched()
    cpt = run(tokens.data_ptr(), len(k_rows), extra.data_ptr(), len(e_rows), [compact_index(s) for s in src])
    _same_bits(far, cpt, f"{case.id}: out")
    pick = {"table": table, "tokens": tokens.to(torch.bfloat16).float(), "extra": extra}
    want = torch.stack([pick[k][i] if k else torch.zeros(H, device=dev) for k, i in map(source, src)])
    assert torch.equal(_bits(far), _bits(want)), "token rows rounded through bf16, table and extra rows copied, the rest zero"
    assert {k for k, _ in map(source, src)} == {"table", "tokens", "extra", None}


@pytest.mark.parametrize("case", BY_ENTRY["slime_splice_routed"], ids=_ids("slime_splice_routed"))
def test_splice_routed(arena, dev, case):
    """The routed splice with image 1's global and kept local token rows past 2^32 bytes of `tokens` (local_row_off[1]): every feature
    position of both images, the separator, text ids, padding, and a position past keep_count (zeros)."""
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, P, T_max, n_tab = p["H"], p["P"], p["T_max"], p["table_rows"]
    g = _gen(dev, 17)
    table = torch.randn(n_tab, H, generator=g, device=dev)
    tokens = torch.randn(len(p["far_rows"]), H, generator=g, device=dev)
    n_rows = torch.tensor(p["n_rows"], dtype=torch.int32, device=dev)
    keep = torch.tensor(p["keep_idx"], dtype=torch.int32, device=dev)
    cnt = torch.tensor(p["keep_count"], dtype=torch.int32, device=dev)
    feat = lambda b, q: -2 - ((b << 32) | q)
    src_list = ([3, -1] + [feat(0, q) for q in range(P + 1 + p["keep_count"][0])] + [7] + [feat(1, q) for q in range(P + 1 + p["keep_count"][1])]
                + [feat(1, P + 1 + p["keep_count"][1]), feat(2, 0), -1])
    src = torch.tensor(src_list, dtype=torch.int64, device=dev)

    def run(tptr, token_rows, row_off):
        off = torch.tensor(row_off, dtype=torch.int64, device=dev)
        out = _sentinel((len(src_list), H), torch.float32, dev)
        rc = lib.slime_splice_routed(table.data_ptr(), _lib.F32, n_tab, p["sep_id"], tptr, token_rows, off.data_ptr(), n_rows.data_ptr(), 2, P, T_max,
                                     keep.data_ptr(), cnt.data_ptr(), _lib.BF16, src.data_ptr(), out.data_ptr(), _lib.F32, len(src_list), H,
                                     _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return out

    arena.place(case.layout["tokens"], tokens)
    far = run(arena.ptr("tokens"), p["token_rows"], p["local_row_off"])
    arena.check_untouched()
    cpt = run(tokens.data_ptr(), tokens.shape[0], p["compact_row_off"])
    _same_bits(far, cpt, f"{case.id}: out")
    # image 1, position 0 is its first global token (compact row local_row_off - P), through bf16; its last kept token is local row keep[1][2]
    i1 = src_list.index(feat(1, 0))
    c_off = p["compact_row_off"][1]
    assert torch.equal(far[i1], tokens[c_off - P].to(torch.bfloat16).float())
    last = src_list.index(feat(1, P + p["keep_count"][1]))
    assert torch.equal(far[last], tokens[c_off + p["keep_idx"][1][p["keep_count"][1] - 1]].to(torch.bfloat16).float())
    assert torch.equal(far[src_list.index(feat(0, P))], table[p["sep_id"]].to(torch.bfloat16).float()) and not bool(far[-2].any()) and not bool(far[-3].any())


@pytest.mark.parametrize("case", BY_ENTRY["slime_router_attn_scores"], ids=_ids("slime_router_attn_scores"))
def test_router_attn_scores(arena, dev, case):
    """The attention router over a token buffer of more than 2^32 bytes: ops.router_attention_scores builds tok_idx from row_off /
    n_rows and calls slime_router_attn_scores; `tokens` is a view of the arena from the pointer to the last row."""
    from slime_amd import ops, weights as W
    p = case.params
    H, L, row_off, n_rows, token_rows = p["H"], p["L"], p["row_off"], p["n_rows"], p["token_rows"]
    pra = ops.pack_router_attention(W.make_router_attention_state_dict(H, seed=3), H, torch.bfloat16, dev)
    g = _gen(dev, 18)
    toks = torch.randn(sum(n_rows), H, generator=g, device=dev)
    text = torch.randn(len(n_rows), L, H, generator=g, device=dev)
    lay = arena.place(case.layout["tokens"], toks)
    view = arena.buf[lay.ptr_off:lay.ptr_off + token_rows * H * 4].view(torch.float32).view(token_rows, H)
    assert view.data_ptr() == arena.ptr("tokens") and view.numel() * 4 == lay.extent
    far = ops.router_attention_scores(pra, view, row_off, n_rows, text, None, 0.7)
    torch.cuda.synchronize()
    del view
    arena.check_untouched()
    cpt = ops.router_attention_scores(pra, toks, [0, n_rows[0]], n_rows, text, None, 0.7)
    torch.cuda.synchronize()
    for b, nb in enumerate(n_rows):
        _same_bits(far[b:b + 1, :nb], cpt[b:b + 1, :nb], f"{case.id}: scores of image {b}")
        assert len(set(cpt[b, :nb].tolist())) == nb, "distinct scores"


@pytest.mark.parametrize("case", BY_ENTRY["slime_resize_bicubic_u8_batched"], ids=_ids("slime_resize_bicubic_u8_batched"))
def test_resize_bicubic_u8_batched(arena, dev, case):
    """Both passes (the horizontal one staged in tmp) and the horizontal pass alone (written to dst directly): row strides of 256 MiB,
    image 1 and its last rows past 2^32 bytes in src and in dst."""
    from slime_amd import _lib, ops
    lib, p = _lib.load(), case.params
    sh, sw, oh, ow, images = p["src_h"], p["src_w"], p["out_h"], p["out_w"], p["images"]
    src = torch.randint(0, 256, (images * sh, sw * 3), generator=_gen(dev, 13), device=dev).to(torch.uint8)
    bh, kh, ksh = ops._device_tables(sw, ow, dev)
    bv, kv, ksv = ops._device_tables(sh, oh, dev) if oh != sh else (None, None, 0)
    tmp = torch.empty(images * sh * ow * 3, dtype=torch.uint8, device=dev)

    def run(sptr, sis, ss, dptr, dis, ds):
        rc = lib.slime_resize_bicubic_u8_batched(sptr, images, sis, sh, sw, ss, dptr, dis, ds, oh, ow, bh.data_ptr(), kh.data_ptr(), ksh,
                                                 bv.data_ptr() if bv is not None else None, kv.data_ptr() if kv is not None else None, ksv,
                                                 tmp.data_ptr(), tmp.numel(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["src"], src)
    arena.place(case.layout["dst"])
    run(arena.ptr("src"), p["src_image_stride"], p["src_stride"], arena.ptr("dst"), p["dst_image_stride"], p["dst_stride"])
    far = arena.check_untouched()["dst"]
    cpt = _sentinel((images * oh, ow * 3), torch.uint8, dev)
    run(src.data_ptr(), sh * sw * 3, sw * 3, cpt.data_ptr(), oh * ow * 3, ow * 3)
    _same_bits(far, cpt, f"{case.id}: dst")
    assert len({bytes(r) for r in cpt.cpu().numpy()}) == images * oh, "distinct output rows"


@pytest.mark.parametrize("case", BY_ENTRY["slime_slice_jobs"], ids=_ids("slime_slice_jobs"))
def test_slice_jobs(arena, dev, case):
    """Two jobs that run both passes (the second one's tmp_offset > 0): src rows 256 / 512 MiB apart, and job 0's tile at a crop index
    whose byte offset in `out` passes 2^32; the table goes through the ctypes mirror of slime_slice_job (its `long` fields)."""
    from slime_amd import _lib, ops
    lib, p = _lib.load(), case.params
    crop, jobs = p["crop"], p["jobs"]
    g = _gen(dev, 15)
    srcs = [torch.randint(0, 256, (j["src_h"], j["src_w"] * 3), generator=g, device=dev).to(torch.uint8) for j in jobs]
    mean, std = (C.c_float * 3)(0.48, 0.46, 0.41), (C.c_float * 3)(0.27, 0.26, 0.28)
    tiles = [(j["canvas_h"] // crop) * (j["canvas_w"] // crop) for j in jobs]

    def run(src_ptrs, strides, firsts, optr, out_crops):
        table = (_lib.SliceJob * len(jobs))()
        for J, j, sp, ss, fc in zip(table, jobs, src_ptrs, strides, firsts):
            J.src, J.src_stride, J.src_h, J.src_w = sp, ss, j["src_h"], j["src_w"]
            J.out_h, J.out_w, J.canvas_h, J.canvas_w, J.x0, J.y0, J.first_crop = j["out_h"], j["out_w"], j["canvas_h"], j["canvas_w"], j["x0"], j["y0"], fc
            b, k, J.ksize_h = ops._device_tables(j["src_w"], j["out_w"], dev)
            J.bounds_h, J.kk_h = b.data_ptr(), k.data_ptr()
            b, k, J.ksize_v = ops._device_tables(j["src_h"], j["out_h"], dev)
            J.bounds_v, J.kk_v = b.data_ptr(), k.data_ptr()
        tmp_bytes = C.c_size_t(0)
        assert lib.slime_slice_jobs_plan(table, len(jobs), crop, C.byref(tmp_bytes)) == 0, lib.slime_last_error().decode()
        assert table[1].tmp_offset > 0
        nbytes = len(jobs) * C.sizeof(_lib.SliceJob)
        host = torch.empty(nbytes, dtype=torch.uint8)
        C.memmove(host.data_ptr(), table, nbytes)
        table_dev = host.to(dev)
        tmp = torch.empty(tmp_bytes.value, dtype=torch.uint8, device=dev)
        rc = lib.slime_slice_jobs(table, table_dev.data_ptr(), len(jobs), crop, mean, std, optr, out_crops, _lib.F32, tmp.data_ptr(),
                                  tmp_bytes.value, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["src0"], srcs[0])
    arena.place(case.layout["src1"], srcs[1])
    arena.place(case.layout["out"])
    assert p["out_order"] == [jobs[1]["first_crop"], jobs[1]["first_crop"] + 1, jobs[0]["first_crop"]] and tiles == [1, 2]
    run([arena.ptr("src0"), arena.ptr("src1")], [j["src_stride"] for j in jobs], [j["first_crop"] for j in jobs], arena.ptr("out"), p["out_crops"])
    far = arena.check_untouched()["out"]
    cpt = _sentinel((4, 3 * crop * crop), torch.float32, dev)
    run([s.data_ptr() for s in srcs], [j["src_w"] * 3 for j in jobs], [2, 0], cpt.data_ptr(), 4)      # job 1 -> crops 0, 1; job 0 -> crop 2
    _same_bits(far, cpt[:3], f"{case.id}: out")
    assert bool((_bits(cpt[3]) == XC.SENTINEL_BYTE).all()) and len({bytes(r) for r in _bits(far).cpu().numpy()}) == 3


@pytest.mark.parametrize("case", BY_ENTRY["slime_view_jobs"], ids=_ids("slime_view_jobs"))
def test_view_jobs(arena, dev, case):
    """A padded, resized (both passes) box with two overlapping windows: image rows 256 / 512 MiB apart, the windows' crops at a byte
    offset of `out` past 2^32; the table goes through the ctypes mirror of slime_view_job (its `long` fields)."""
    from slime_amd import _lib, ops
    lib, p = _lib.load(), case.params
    crop, j = p["crop"], p["job"]
    img = torch.randint(0, 256, (j["img_h"], j["img_w"] * 3), generator=_gen(dev, 16), device=dev).to(torch.uint8)
    mean, std = (C.c_float * 3)(0.48, 0.46, 0.41), (C.c_float * 3)(0.27, 0.26, 0.28)
    wins = j["windows"][3] * j["windows"][4]

    def run(iptr, stride, first, optr, out_crops):
        table = (_lib.ViewJob * 1)()
        J = table[0]
        J.img, J.img_stride, J.img_h, J.img_w = iptr, stride, j["img_h"], j["img_w"]
        J.box_x0, J.box_y0, J.box_w, J.box_h = j["box"]
        (J.field_w, J.field_h), (J.paste_x, J.paste_y) = j["field"], j["paste"]
        J.bg[0], J.bg[1], J.bg[2] = j["bg"]
        (J.out_w, J.out_h), J.filter = j["out"], _lib.FILTER_BICUBIC
        J.win_x0, J.win_y0, J.win_step, J.win_nx, J.win_ny = j["windows"]
        J.first_crop = first
        b, k, J.ksize_h = ops._device_tables(J.field_w, J.out_w, dev)
        J.bounds_h, J.kk_h = b.data_ptr(), k.data_ptr()
        b, k, J.ksize_v = ops._device_tables(J.field_h, J.out_h, dev)
        J.bounds_v, J.kk_v = b.data_ptr(), k.data_ptr()
        tmp_bytes = C.c_size_t(0)
        assert lib.slime_view_jobs_plan(table, 1, crop, C.byref(tmp_bytes)) == 0, lib.slime_last_error().decode()
        assert tmp_bytes.value > 0, "both passes run"
        nbytes = C.sizeof(_lib.ViewJob)
        host = torch.empty(nbytes, dtype=torch.uint8)
        C.memmove(host.data_ptr(), table, nbytes)
        table_dev = host.to(dev)
        tmp = torch.empty(tmp_bytes.value, dtype=torch.uint8, device=dev)
        rc = lib.slime_view_jobs(table, table_dev.data_ptr(), 1, crop, mean, std, optr, out_crops, _lib.F32, tmp.data_ptr(), tmp_bytes.value,
                                 _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["img"], img)
    arena.place(case.layout["out"])
    run(arena.ptr("img"), j["img_stride"], j["first_crop"], arena.ptr("out"), p["out_crops"])
    far = arena.check_untouched()["out"]
    cpt = _sentinel((wins + 2, 3 * crop * crop), torch.float32, dev)
    run(img.data_ptr(), j["img_w"] * 3, 1, cpt.data_ptr(), wins + 2)
    _same_bits(far, cpt[1:1 + wins], f"{case.id}: out")
    assert bool((_bits(cpt[0]) == XC.SENTINEL_BYTE).all()) and bool((_bits(cpt[-1]) == XC.SENTINEL_BYTE).all())
    assert not torch.equal(far[0], far[1]), "the two windows differ"


@pytest.mark.parametrize("case", BY_ENTRY["slime_tile_normalize_batched"], ids=_ids("slime_tile_normalize_batched"))
def test_tile_normalize_batched(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    crop, Hc, Wc, images = p["crop"], p["Hc"], p["Wc"], p["images"]
    tiles = (Hc // crop) * (Wc // crop)
    canvas = torch.randint(0, 256, (images, Hc * Wc * 3), generator=_gen(dev, 11), device=dev).to(torch.uint8)
    mean, std = (C.c_float * 3)(0.48, 0.46, 0.41), (C.c_float * 3)(0.27, 0.26, 0.28)

    def run(cptr, cis, optr, oic):
        rc = lib.slime_tile_normalize_batched(cptr, images, cis, Hc, Wc, crop, mean, std, optr, oic, _lib.F32, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["canvas"], canvas)
    arena.place(case.layout["out"])
    run(arena.ptr("canvas"), p["canvas_image_stride"], arena.ptr("out"), p["out_image_crops"])
    far = arena.check_untouched()["out"]
    cpt = _sentinel((images, tiles + 1, 3 * crop * crop), torch.float32, dev)
    run(canvas.data_ptr(), Hc * Wc * 3, cpt.data_ptr(), tiles + 1)
    _same_bits(far, cpt[:, :tiles].reshape(images * tiles, -1), f"{case.id}: out")
    assert bool((_bits(cpt[:, tiles]) == XC.SENTINEL_BYTE).all()) and len({bytes(r) for r in _bits(far).cpu().numpy()}) == images * tiles


SPLICE_SOURCES = [c for c in BY_ENTRY["slime_splice_rows"] if "src" in c.params]
SPLICE_OUT = [c for c in BY_ENTRY["slime_splice_rows"] if "named" in c.params]


@pytest.mark.parametrize("case", SPLICE_OUT, ids=[c.ident for c in SPLICE_OUT])
def test_splice_rows_out_past_4_gib(arena, dev, case):
    """262 160 fp32 rows of 16 KiB: `out` itself passes 2^32 bytes.  src is -1 (zeros) but for the first, a few middle and the last
    rows; the compact run is the same call into a tensor of its own."""
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, rows = p["H"], p["rows"]
    table = torch.randn(p["table_rows"], H, generator=_gen(dev, 12), device=dev)
    src = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    for r, t in p["named"].items():
        src[r] = t

    def run(optr):
        rc = lib.slime_splice_rows(table.data_ptr(), _lib.F32, p["table_rows"], None, _lib.F32, 0, src.data_ptr(), optr, _lib.F32, rows, H, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    arena.place(case.layout["out"])
    run(arena.ptr("out"))
    cpt = _sentinel((rows, H), torch.float32, dev)
    run(cpt.data_ptr())
    far = arena.view_bulk("out")                       # 4 GiB: compared in place, then wiped
    same = torch.equal(far.view(torch.int64), cpt.view(torch.int64))
    last = rows - 1
    ends = torch.equal(_bits(far[last]), _bits(table[p["named"][last]])) and not bool(far[rows // 3].any())
    del far
    arena.check_untouched(copy_outputs=False)
    assert same, f"{case.id}: out differs in bits from the compact run"
    assert ends, f"{case.id}: the last row is not its table row, or a padding row is not zero"


@pytest.mark.parametrize("case", SPLICE_SOURCES, ids=[c.ident for c in SPLICE_SOURCES])
def test_splice_rows(arena, dev, case):
    from slime_amd import _lib
    lib, p = _lib.load(), case.params
    H, src, t_rows, f_rows = p["H"], p["src"], p["t_rows"], p["f_rows"]
    g = _gen(dev, 10)
    table = torch.randn(len(t_rows), H, generator=g, device=dev)
    feats = torch.randn(len(f_rows), H, generator=g, device=dev)

    def run(tptr, n_t, fptr, n_f, index):
        it = torch.tensor(index, dtype=torch.int64, device=dev)
        out = _sentinel((len(index), H), torch.float32, dev)
        rc = lib.slime_splice_rows(tptr, _lib.F32, n_t, fptr, _lib.F32, n_f, it.data_ptr(), out.data_ptr(), _lib.F32, len(index), H, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()
        return out

    def compact_index(s):
        if s >= 0:
            return t_rows.index(s) if s in t_rows else len(t_rows) + 5          # outside the table there as here: zeros
        if s == -1:
            return -1
        return -2 - (f_rows.index(-2 - s) if (-2 - s) in f_rows else len(f_rows) + 9)

    arena.place(case.layout["table"], table)
    arena.place(case.layout["feats"], feats)
    far = run(arena.ptr("table"), p["table_rows"], arena.ptr("feats"), p["feat_rows"], src)
    arena.check_untouched()
    cpt = run(table.data_ptr(), len(t_rows), feats.data_ptr(), len(f_rows), [compact_index(s) for s in src])
    _same_bits(far, cpt, f"{case.id}: out")
    want = torch.stack([table[t_rows.index(s)] if s in t_rows else feats[f_rows.index(-2 - s)] if (-2 - s) in f_rows else torch.zeros(H, device=dev)
                        for s in src])
    assert torch.equal(_bits(far), _bits(want)), "equal dtypes are copied bit for bit, padding and out-of-range rows are zero"
