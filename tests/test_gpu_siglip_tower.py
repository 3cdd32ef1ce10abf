"""SigLIP vision towers on the GPU (helpers: tests/siglip_tower_conformance.py; the CPU side: tests/test_siglip_tower_cpu.py).

  1. GEMM conformance of the LayerNorm-fold consumer with SLIME_EPI_BIAS_GELU_TANH_T: element by element under the derived bound in
     every kernel family (forced in the diagnostic library), sentinels intact, the three operand forms bit-equal; the product
     dispatch and kernel name; ``slime_gemm_ksplit`` with this form; the un-folded use.
  2. The plain front end (``slime_patch_embed_plain``) element by element against float64: h inside its bound, x16 / lo8 the split of
     h in bits, stats the sums of the rounded rows, rows P and beyond untouched.
  3. The tower against HF ``SiglipVisionModel`` (fp32, CPU): every hidden state and ``encode`` at test_gpu_path's tolerances; the
     quick-GELU states lie outside the fp16 tolerance on these inputs.
  4. ``slime_siglip_forward`` bit-equal to a replay of its launches through the C ABI (guarded, exactly sized workspace; k-split on
     and off); batch and shard invariance in bits.
  5. The plugin surface: ``build_vision_tower`` on a 1024-wide g = 24 directory, ``encode_images`` with mlp2x_gelu, the gated adapter
     and the sampler on the TINY-sized tower.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import gemm_conformance as GC
import siglip_tower_conformance as S
from adapter_conformance import GuardedWorkspace, guarded_input, guarded_output, sentinel_rows

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}
TOL = {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}           # tests/test_gpu_path.py's own
GUARDS = ("nan", "attract")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _L():
    from slime_amd import _lib
    return _lib


def _lib():
    return _L().load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _biteq(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


# ------------------------------------------------------------------------------------------------ 1. GEMM conformance
class _forced:
    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        self.ctx = _L().diag()
        self.lib = self.ctx.__enter__()
        self.lib.slime_gemm_force_tile(self.tile)
        return self.lib

    def __exit__(self, *exc):
        self.lib.slime_gemm_force_tile(0)
        return self.ctx.__exit__(*exc)


def _pack(lib, c):
    f = GC.Padded(c.N, c.K, c.dtype, c.buf["B"].flat.device, pad_cols=0, guard_rows=0, tail=GC.TAIL)
    if c.guard == "nan":
        f.flat.fill_(float("nan"))
    _L().check(lib.slime_gemm_pack_b(c.buf["B"].ptr(), c.N, c.K, f.ptr(), _stream()), "slime_gemm_pack_b")
    return f


def _gemm(lib, c, operand="B", frag=None, splits=None, ws=None, **override):
    fields = c.arg_fields(operand, frag.ptr() if frag is not None else None)
    fields.update(override)
    g = _L().GemmArgs(**fields)
    if splits is None:
        rc = lib.slime_gemm_ex(C.byref(g), _stream())
    else:
        rc = lib.slime_gemm_ksplit(C.byref(g), splits, ws.ptr() if ws is not None else None, ws.nbytes if ws is not None else 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"returned {rc}: {lib.slime_last_error().decode()}"


def _what(c, extra=""):
    return f"{S.FORM} {c.kind} {DT_ID[c.dtype]} M={c.M} N={c.N} K={c.K} guard={c.guard} {extra}"


def _run(lib, c, what, bm, **kw):
    """reference -> one launch per operand form -> the first inside the bound element by element, the others bit-equal to it, every
    byte outside the C window untouched.  -> worst |err| / bound."""
    r = S.reference(c)
    if c.has_bias:
        assert S.tail_share(r) >= S.TAIL_SHARE, f"{what}: the case does not reach the tail"
    frag = _pack(lib, c)
    first = None
    for op in ("B+frag", "B", "frag"):
        c.restore()
        _gemm(lib, c, op, frag, **kw)
        assert c.intact() is None, f"{what} [{op}]: a byte outside the C window was written"
        outs = c.windows()
        if first is None:
            first = outs
            ratio, msg = S.check(c, r, outs, bm)
            assert msg is None, f"{what} [{op}]: {msg}"
        else:
            assert _biteq(outs["C"], first["C"]), f"{what}: operand form {op} differs in bits from B+frag"
    return ratio


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("tile", S.TILES)
def test_fold_gelu_tanh_in_every_kernel_family(dev, tile, dtype):
    """One kernel family x one dtype: the row edges of the family's tile (1, 15, 16, 17, BM - 1, BM, BM + 1, 2 BM + 17), K = 64 / 192 /
    2112, two widths, the kinds and guard passes in turn (the shapes of test_gpu_gelu_tower's section 5)."""
    bm, worst, n = GC.TILE_BM[tile], 0.0, 0
    with _forced(tile) as lib:
        for N in S.fold_n(tile):
            for M in GC.m_table(bm):
                for K in S.FOLD_K:
                    n += 1
                    c = S.make_case(("random", "tails")[n % 2], dtype, M, N, K, guard=GUARDS[(n // 2) % 2], seed=n, device=dev)
                    worst = max(worst, _run(lib, c, _what(c, f"tile {tile}"), bm))
    print(f"\n{GC.TILE_FAMILY[tile]} {S.FORM} {DT_ID[dtype]}: worst |err| / bound {worst:.3f} over {n} cases")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_fold_gelu_tanh_product_dispatch_kernel_name_and_unfolded_use(dev, dtype):
    """The product library where auto_tile picks the direct-B kernel (fc1 of a tower pass) and the 64 x 64 ring, each proven by
    slime_gemm_kernel_name with epilogue code 9; a bias of NULL; and the same epilogue WITHOUT the fold (ln_stats = NULL): the
    activation of the plain pre-activation, inside the un-folded bound."""
    from slime_amd import ops
    lib = _lib()
    t = {torch.bfloat16: "BF16", torch.float16: "F16"}[dtype]
    assert ops.gemm_kernel_name(2049, 4096, 128, dtype, S.EPI_BIAS_GELU_TANH_T, True) == f"gemm_db_kernel<{t}, 9, 0, 8>"
    assert ops.gemm_kernel_name(100, 256, 64, dtype, S.EPI_BIAS_GELU_TANH_T, False) == f"gemm_kernel<{t}, 64, 64, 4, 1, 9, 2>"
    for n, (M, N, K) in enumerate(((2049, 4096, 128), (100, 256, 64))):
        c = S.make_case(("random", "tails")[n], dtype, M, N, K, guard=GUARDS[n], seed=n, device=dev)
        _run(lib, c, _what(c, "product"), 128)
    c = S.make_case("tails", dtype, 145, 256, 128, guard="nan", bias=False, seed=3, device=dev)
    _run(lib, c, _what(c, "bias = NULL"), 128)
    # un-folded: a gemm_conformance case of the plain quick-GELU form, run under epilogue 9
    for M, N, K in ((145, 256, 128), (300, 512, 192)):
        p = GC.make_case("tails", dtype, "quickgelu_t", M, N, K, guard="nan", seed=5, device=dev)
        r = GC.reference(p)
        want = S.gelu_tanh64(r.x)
        bd = GC._round_T(want, S.d_gelu_tanh(r.x, r.dx), dtype)
        g = _L().GemmArgs(**dict(p.arg_fields("B"), epilogue=S.EPI_BIAS_GELU_TANH_T))
        assert lib.slime_gemm_ex(C.byref(g), _stream()) == 0, lib.slime_last_error()
        torch.cuda.synchronize()
        assert p.intact() is None
        ratio, ex, *_ = GC.worst(p.windows()["C"], want, bd)
        assert ex <= 0, GC.describe_failure("gelu_tanh_t (un-folded)", p.windows()["C"], want, bd)


def _row_ptr(p, r):
    return p.ptr() + r * p.ld * p.flat.element_size()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_fold_gelu_tanh_ksplit(dev, dtype):
    """slime_gemm_ksplit with this form: inside the bound and operand-form invariant at splits 2, 3 and 4 (exactly sized guarded
    workspace), deterministic on a workspace full of NaN patterns; splits = 1 is slime_gemm_ex; the rows do not depend on M nor on
    how they are cut into calls."""
    lib = _lib()
    for n, (M, N, K, sp) in enumerate(((273, 384, 576, 4), (65, 128, 192, 2), (129, 256, 2112, 3))):
        c = S.make_case(("random", "tails")[n % 2], dtype, M, N, K, guard=GUARDS[n % 2], seed=n, device=dev)
        ws = GuardedWorkspace(lib.slime_gemm_ksplit_workspace_bytes(M, N, sp), dev)
        _run(lib, c, _what(c, f"splits {sp}"), 64, splits=sp, ws=ws)
        assert ws.intact(), "slime_gemm_ksplit wrote outside its workspace"
        first = c.windows()["C"]
        c.restore()
        ws.window.fill_(0xFF)
        _gemm(lib, c, "B", None, splits=sp, ws=ws)
        assert _biteq(c.windows()["C"], first), "not deterministic"
    c = S.make_case("random", dtype, 65, 128, 320, seed=9, device=dev)
    _gemm(lib, c, "B", None, splits=1)
    one = c.windows()["C"]
    c.restore()
    _gemm(lib, c, "B", None)
    assert _biteq(c.windows()["C"], one), "splits = 1 is not slime_gemm_ex"
    M, N, K, sp = 4100, 128, 384, 2
    c = S.make_case("random", dtype, M, N, K, seed=sp, device=dev)
    ws = GuardedWorkspace(lib.slime_gemm_ksplit_workspace_bytes(M, N, sp), dev)
    _gemm(lib, c, "B", None, splits=sp, ws=ws)
    assert c.intact() is None and ws.intact()
    whole = c.windows()["C"]
    c.restore()
    for lo, hi in ((0, 65), (65, 4000), (4000, 4100)):
        b = c.buf
        _gemm(lib, c, "B", None, splits=sp, ws=ws, A=_row_ptr(b["A"], lo), C=_row_ptr(b["C"], lo), M=hi - lo, ln_stats=_row_ptr(b["ln_stats"], lo))
        assert _biteq(c.windows()["C"][lo:hi], whole[lo:hi]), f"rows {lo}..{hi} depend on M or on the cut"
    assert _biteq(c.windows()["C"], whole) and c.intact() is None


# ------------------------------------------------------------------------------------------------ 2. the plain front end
# image, D, crops: the smallest grid, an odd one (a one-row last pair), a released geometry, the largest LDS layout; the wide forms
FRONT = [(64, 128, 3), (80, 128, 2), (224, 128, 2), (384, 128, 2), (64, 768, 2), (64, 1024, 2)]


@pytest.mark.parametrize("pix", ["f32", "t"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("image,D,n", FRONT, ids=[f"{i}-D{d}" for i, d, _ in FRONT])
def test_plain_front_end_element_by_element(dev, image, D, n, dtype, pix):
    from slime_amd import ops, weights as W
    lib, L_ = _lib(), _L()
    cfg = S.siglip_config(image, 16, D, 256, 1)
    P, g = cfg.num_patches, cfg.grid
    sd = W.make_siglip_state_dict(cfg, seed=31 + g, head=False)
    host = ops.siglip_host_tensors(sd, cfg, dtype, 0)
    pos = host["pos"].to(dev)
    frag = ops.pack_b_frag(host["patch_w"].to(dev))
    px = W.synthetic_pixels(n, seed=g, image_size=image)
    px_in = px.to(dev) if pix == "f32" else px.to(dtype).to(dev)
    pad = guarded_input(px_in, n * 3 * image)
    h = guarded_output(n * P, D, torch.float32, dev)
    x16 = guarded_output(n * P, D, dtype, dev)
    lo = guarded_output(n * P, D, torch.int8, dev)
    st = guarded_output(n * P, 2 * (D // 64), torch.float32, dev)
    bufs = (h, x16, lo, st)
    snaps = [b.snapshot() for b in bufs]
    rc = lib.slime_patch_embed_plain(pad.ptr(), ops.dtype_code(px_in.dtype), frag.data_ptr(), pos.data_ptr(), h.ptr(), x16.ptr(), lo.ptr(),
                                     st.ptr(), ops.dtype_code(dtype), n, image, 16, 768, D, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    for b, s in zip(bufs, snaps):                           # row n P and beyond (and everything in front) untouched; every row written
        assert b.intact(s) and not bool(sentinel_rows(b.win).any())
    want, dh = S.embed64(px, {"patch_w": host["patch_w"], "pos": host["pos"]}, cfg, dtype)
    got = h.win.cpu()
    ratio, ex, *_ = GC.worst(got, want, dh * (1 + 2.0 ** -10))
    assert ex <= 0, GC.describe_failure(f"plain front end {image}/16 D={D}", got, want, dh, 48, "h")
    hi, l8 = ops.resid_split(h.win, dtype)
    assert _biteq(x16.win, hi) and _biteq(lo.win, l8), "x16 / lo8 are not the split of h"
    r = x16.win.double().view(n * P, D // 64, 64)
    sums = torch.stack([r.sum(-1), (r * r).sum(-1)], -1)
    bd = 70 * GC.E32 * torch.stack([r.abs().sum(-1), (r * r).sum(-1)], -1) + 1e-30         # 63 additions + the fmas of the squares
    assert bool(((st.win.double().view(n * P, D // 64, 2) - sums).abs() <= bd).all()), "stats are not the sums of the rounded rows"
    print(f"\nplain front end {image}/16 g={g} D={D} {DT_ID[dtype]} pixels {pix}: worst |err| / bound {ratio:.3f}")
    # outputs are optional one by one: x16 alone gives the same bits
    only = guarded_output(n * P, D, dtype, dev)
    assert lib.slime_patch_embed_plain(pad.ptr(), ops.dtype_code(px_in.dtype), frag.data_ptr(), pos.data_ptr(), None, only.ptr(), None, None,
                                       ops.dtype_code(dtype), n, image, 16, 768, D, _stream()) == 0
    torch.cuda.synchronize()
    assert _biteq(only.win, x16.win)


# ------------------------------------------------------------------------------------------------ towers and the HF yardstick
# name -> (image, D, inter, layers, crops)
GEOMS = {"d128g4": (64, 128, 256, 2, 3), "d128g5": (80, 128, 256, 2, 3), "d768g4": (64, 768, 3072, 1, 2), "d1024g24": (384, 1024, 4096, 1, 1)}
_cases, _packed = {}, {}


def _case(name):
    """(cfg, prefixed state dict, pixels, HF fp32 hidden states) -- weights seed 7, pixels seed 3, built once and left unchanged."""
    if name not in _cases:
        from slime_amd import weights as W
        image, D, inter, layers, n = GEOMS[name]
        cfg = S.siglip_config(image, 16, D, inter, layers)
        sd = W.make_siglip_state_dict(cfg, seed=7)
        px = W.synthetic_pixels(n, seed=3, image_size=image)
        _cases[name] = (cfg, sd, px, S.hf_states(cfg, sd, px))
    return _cases[name]


def _pack_tower(name, dtype, dev):
    cfg, sd, _, _ = _case(name)
    if (name, dtype) not in _packed:
        from slime_amd import ops
        _packed[(name, dtype)] = ops.pack_siglip_tower(sd, cfg, dtype, dev, select_layer=cfg.num_hidden_layers)
    return _packed[(name, dtype)]


def _within(got, want, dtype, what):
    r, w = S.rel_l2(got, want), S.worst_token(got, want)
    print(f"{what}: rel-L2 {r:.3e} (tolerance {TOL[dtype]:.1e}), worst token {w:.3e}")
    assert r < TOL[dtype], (what, r)
    assert w <= 4 * TOL[dtype], (what, w)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_tower_against_hf(dev, name, dtype):
    """Every hidden state (ops.siglip_tower_hidden_states) and HipSiglipVisionModel.encode at select_layer = -2 and L against HF
    SiglipVisionModel: rel-L2 below test_gpu_path's tolerance, worst token at most four times it.  A float64 replay of the same
    weights with the quick-GELU in place of the tanh form lies outside the fp16 tolerance on these inputs: the comparison can tell."""
    from slime_amd import ops
    from slime_amd.model.multimodal_encoder.siglip_encoder import HipSiglipVisionModel
    cfg, sd, px, hf = _case(name)
    L = cfg.num_hidden_layers
    host = ops.siglip_host_tensors(sd, cfg, None, L)
    quick = S.replay_siglip(S.TorchBackend(None, "quick"), host, cfg, px, L, want_states=True)["states"]
    apart = [S.rel_l2(quick[i].view_as(hf[i]), hf[i]) for i in range(1, L + 1)]
    print(f"\n{name}: quick-GELU replay vs HF states 1..{L}: " + " ".join(f"{v:.2e}" for v in apart))
    assert min(apart) > TOL[torch.float16], apart
    pt = _pack_tower(name, dtype, dev)
    st = ops.siglip_tower_hidden_states(pt, px.to(dev))
    assert st.shape == (L + 1, px.shape[0], cfg.num_patches, cfg.hidden_size) and st.dtype == torch.float32
    for i in range(L + 1):
        _within(st[i], hf[i], dtype, f"{name} {DT_ID[dtype]} state {i}")
    m = HipSiglipVisionModel(cfg, dtype)
    m.load_state_dict(sd)
    m.to(dev)
    out = m.encode(px.to(dev), -2, out_dtype=torch.float32)
    assert out.shape == hf[-2].shape
    _within(out, hf[-2], dtype, f"{name} {DT_ID[dtype]} encode select_layer=-2")
    assert _biteq(m.encode(px.to(dev), L, out_dtype=torch.float32), st[L])
    hs = m(px.to(dev), output_hidden_states=True).hidden_states
    assert len(hs) == L + 1 and _biteq(hs[L], st[L]) and _biteq(m(px.to(dev)).last_hidden_state, st[L])


# ------------------------------------------------------------------------------------------------ 4. the entry and its replay
def _siglip_call(desc, pad, pix_dtype, n, out, hidden, states, ks, ws, nbytes=None):
    from slime_amd import ops
    p = lambda x: None if x is None else x.ptr()
    odt = ops.dtype_code(out.win.dtype) if out is not None else _L().F32
    return _lib().slime_siglip_forward(C.byref(desc), pad.ptr(), ops.dtype_code(pix_dtype), n, p(out), odt, p(hidden), p(states),
                                       None if ks is None else C.byref(_L().VitKsplit(*ks)), ws.ptr(), ws.nbytes if nbytes is None else nbytes,
                                       _stream())


def _derived_ws_bytes(cfg, n, ks=None):
    """The workspace size from the header's description of the plan, derived here: lo (1 B), xn (2 B), the shared q/k/v + ctx | ff
    region, the statistics -- each at a 256-B boundary -- and, with a k-split, the largest partial-product region."""
    up = lambda b: (b + 255) // 256 * 256
    M, D, F = n * cfg.num_patches, cfg.hidden_size, cfg.intermediate_size
    total = up(M * D) + up(M * D * 2) + up(max(M * F * 2, up(M * 3 * D * 2) + M * D * 2)) + up(M * (D // 64) * 8)
    if ks is not None:
        total += max(_lib().slime_gemm_ksplit_workspace_bytes(M, N, s) for N, s in zip((3 * D, D, F, D), ks))
    return total


def _run_entry(pt, cfg, pad, pix_dtype, n, out_dtype, dev, ks=None):
    D, P, L = cfg.hidden_size, cfg.num_patches, pt.layers_run
    out = guarded_output(n * P, D, out_dtype, dev)
    hid = guarded_output(n * P, D, torch.float32, dev)
    sts = guarded_output((L + 1) * n * P, D, torch.float32, dev)
    bufs = (out, hid, sts)
    snaps = [b.snapshot() for b in bufs]
    need = _derived_ws_bytes(cfg, n, ks)
    lib = _lib()
    q = lib.slime_siglip_workspace_bytes(C.byref(pt.desc), n) if ks is None else \
        lib.slime_siglip_ksplit_workspace_bytes(C.byref(pt.desc), n, C.byref(_L().VitKsplit(*ks)))
    assert q == need, (q, need)
    ws = GuardedWorkspace(need, dev)
    assert _siglip_call(pt.desc, pad, pix_dtype, n, out, hid, sts, ks, ws, need - 256) == -2       # one block short: refused, nothing launched
    rc = _siglip_call(pt.desc, pad, pix_dtype, n, out, hid, sts, ks, ws)
    assert rc == 0, lib.slime_last_error().decode()
    torch.cuda.synchronize()
    assert ws.intact(), "the tower wrote outside the workspace the size query told the caller to allocate"
    for b, s in zip(bufs, snaps):
        assert b.intact(s) and not bool(sentinel_rows(b.win).any())
    return out.win, hid.win, sts.win.view(L + 1, n * P, D)


def _guarded_pixels(px, pix_dtype, dev):
    n, I = px.shape[0], px.shape[-1]
    pad = guarded_input(px.to(pix_dtype).to(dev), n * 3 * I)
    return pad, pad.win.view(n, 3, I, I)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", ["d128g5", "d768g4"])
def test_siglip_forward_equals_the_replay_bit_for_bit(dev, name, dtype):
    """The fused entry against ``replay_siglip`` on a backend that makes the same launches through slime_patch_embed_plain,
    slime_gemm_ex (or slime_gemm_ksplit), slime_attention and slime_gather_rows_split, fc1 under epilogue 9: out (fp32 and T),
    hidden_f32 and every state, unsplit and with the k-split (2, 1, 2, 4); the two settings differ in bits."""
    cfg, sd, px, _ = _case(name)
    L, n = cfg.num_hidden_layers, px.shape[0]
    pt = _pack_tower(name, dtype, dev)
    outs = {}
    for pix, odt, ks in ((torch.float32, torch.float32, None), (dtype, dtype, None), (torch.float32, torch.float32, (2, 1, 2, 4))):
        pad, view = _guarded_pixels(px, pix, dev)
        out, hid, sts = _run_entry(pt, cfg, pad, pix, n, odt, dev, ks=ks)
        be = S.HipBackend(dtype, dev)
        ref = S.replay_siglip(be, pt.tensors, cfg, view, L, out_dtype=odt, want_hidden=True, want_states=True, k_split=ks or (1, 1, 1, 1))
        what = (name, DT_ID[dtype], DT_ID.get(pix, "f32"), ks)
        assert [k[4] for k in be.kernels if k[0] == "w_fc1"] == [S.EPI_BIAS_GELU_TANH_T] * L, be.kernels
        assert _biteq(out, ref["out"]) and _biteq(hid, ref["hidden"]), what
        for i in range(L + 1):
            assert _biteq(sts[i], ref["states"][i]), (what, i)
        assert _biteq(sts[L], hid)
        outs[(pix, ks)] = hid
    assert not _biteq(outs[(torch.float32, None)], outs[(torch.float32, (2, 1, 2, 4))]), "the k-split setting changed nothing"
    # any one output alone: the same bits
    pad, _ = _guarded_pixels(px, torch.float32, dev)
    only = guarded_output(n * cfg.num_patches, cfg.hidden_size, torch.float32, dev)
    ws = GuardedWorkspace(_derived_ws_bytes(cfg, n), dev)
    assert _siglip_call(pt.desc, pad, torch.float32, n, None, only, None, None, ws) == 0
    torch.cuda.synchronize()
    assert ws.intact() and _biteq(only.win, outs[(torch.float32, None)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_batch_and_shard_invariance_in_bits(dev, dtype):
    """1 + 2 crops = 3 crops: with one k-split setting the features do not depend on how the crops are cut into calls (the
    unsplit call may change its tile with M; the split pair is M-invariant by construction); ops.siglip_tower_forward's ``out=``
    slices land in one tensor; the two-stream encode equals the one-stream encode."""
    from slime_amd import ops
    from slime_amd.model.multimodal_encoder.siglip_encoder import HipSiglipVisionModel
    cfg, sd, px, _ = _case("d128g5")
    pt = _pack_tower("d128g5", dtype, dev)
    x = px.to(dev)
    for ks in ((2, 2, 2, 4), None):
        whole = ops.siglip_tower_forward(pt, x, torch.float32, k_split=ks)
        parts = torch.empty_like(whole)
        ops.siglip_tower_forward(pt, x[:1], torch.float32, out=parts[:1], k_split=ks)
        ops.siglip_tower_forward(pt, x[1:], torch.float32, out=parts[1:], k_split=ks)
        torch.cuda.synchronize()
        assert _biteq(parts, whole), f"k_split={ks}: 1 + 2 crops differ from 3 crops"
    m = HipSiglipVisionModel(cfg, dtype)
    m.load_state_dict(sd)
    m.to(dev)
    big = torch.cat([x, x, x], 0)                            # 9 crops: the two-stream split (5 + 4)
    m.k_split = (2, 2, 2, 4)
    two = m.encode(big, -2, out_dtype=torch.float32)
    m.two_streams = False
    one = m.encode(big, -2, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert _biteq(two, one) and _biteq(two[:3], two[3:6]) and two.shape == (9, cfg.num_patches, cfg.hidden_size)


# ------------------------------------------------------------------------------------------------ 5. plugin surface
HIDDEN = 256


def _projector_state(D):
    g = torch.Generator().manual_seed(12)
    r = lambda *s, std: torch.randn(*s, generator=g) * std
    return {"0.weight": r(HIDDEN, D, std=D ** -0.5), "0.bias": r(HIDDEN, std=0.02),
            "2.weight": r(HIDDEN, HIDDEN, std=HIDDEN ** -0.5), "2.bias": r(HIDDEN, std=0.02)}


def test_plugin_surface_over_a_1024_wide_g24_tower(dev, tmp_path):
    """SigLipVisionTower from a directory written here (1024 wide, 384 / 16, one layer): its features against HF's (all 576
    tokens), the list branch, then encode_images on the plain branch with mlp2x_gelu against oracle.mlp_projector on HF's features."""
    from oracle import slime_oracle as O
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    from slime_amd.model.multimodal_encoder.siglip_encoder import SigLipVisionTower
    dtype = torch.float16
    cfg, sd, px32, _ = _case("d1024g24")
    S.write_hf_dir(tmp_path, sd, cfg)
    px = px32.to(dtype)
    hf = S.hf_states(cfg, sd, px.float())[-1]
    t = build_vision_tower(SimpleNamespace(mm_vision_tower=str(tmp_path), mm_vision_select_layer=-1, mm_vision_select_feature="patch",
                                           mm_vision_compute_dtype=dtype))
    assert type(t) is SigLipVisionTower and t.config == cfg and t.hidden_size == 1024 and t.num_patches == 576 and t.num_patches_per_side == 24
    t.to(dev)
    feats = t(px.float().to(dev))
    assert feats.dtype == torch.float32 and feats.shape == hf.shape == (1, 576, 1024)
    _within(feats, hf, dtype, "SigLipVisionTower fp16")
    one = t([p for p in px.to(dev)])
    assert len(one) == 1 and one[0].dtype == dtype and one[0].shape == (1, 576, 1024)
    assert t.dummy_feature.shape == (1, 1024)
    ecfg = default_slime_config(str(tmp_path), hidden_size=HIDDEN, mm_hidden_size=1024, mm_resampler_type=None, mm_projector_type="mlp2x_gelu",
                                mm_vision_select_layer=-1)
    enc = SlimeVisualEncoder(ecfg)
    enc.get_vision_tower().load_model()
    psd = _projector_state(1024)
    enc.get_model().mm_projector.load_state_dict(psd)
    enc.to(dev)
    enc.get_vision_tower().vision_tower.to(dtype)
    got, _ = enc.encode_images(px.to(dev))
    want = O.mlp_projector({"projection." + k: v for k, v in psd.items()}, hf)
    assert got.dtype == dtype and got.shape == want.shape == (1, 576, HIDDEN)
    r = S.rel_l2(got, want)
    print(f"encode_images plain, mlp2x_gelu fp16: rel-L2 {r:.3e}")
    assert r < TOL[dtype], r


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_gated_adapter_and_sampler_on_the_tiny_siglip_tower(dev, tmp_path, dtype):
    """The TINY-sized SigLIP tower (128 wide, 384 / 16: the adapter's 24 x 24 token grid) from a directory, its features through the
    GatedBlock and post_qformer of the tiny adapter, against the oracle on HF's features."""
    import dataclasses
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    cfg = dataclasses.replace(W.SIGLIP_TINY, num_hidden_layers=2)
    sd = W.make_siglip_state_dict(cfg, seed=11)
    S.write_hf_dir(tmp_path, sd, cfg)
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    enc = SlimeVisualEncoder(default_slime_config(str(tmp_path), hidden_size=256, mm_hidden_size=128, mm_vision_select_layer=-1))
    vt = enc.get_vision_tower()
    vt.load_model()
    enc.load_visual_state(None, asd)
    enc.to(dev)
    vt.vision_tower.to(dtype)
    px = W.synthetic_pixels(3, seed=22, image_size=384)
    hf = S.hf_states(cfg, sd, px.to(dtype).float())[-1]
    x = vt(px.to(dev).to(dtype))
    assert x.dtype == dtype and x.shape == (3, 576, 128)
    _within(x, hf, dtype, f"tiny SigLIP tower {DT_ID[dtype]}")
    proj_sd, post_sd = W.sub_state(asd, "mm_projector."), W.sub_state(asd, "sampler.post_qformer.")
    m = enc.get_model()
    g = m.mm_projector(x[:1])
    # two links, each held to TOL by its own tests (the tower above; the adapter modules on exact features in test_gpu_modules):
    # their sum bounds the chain
    rg, rc = S.rel_l2(g, O.gated_block_forward(proj_sd, hf[:1], 1)), None
    comp = m.sampler.post_qformer(x[1:])
    rc = S.rel_l2(comp, O.resampler_forward(post_sd, hf[1:], 1))
    print(f"gated {rg:.3e}, post_qformer {rc:.3e} (tolerance {2 * TOL[dtype]:.1e})")
    assert g.shape == (1, 576, 256) and comp.shape == (2, 144, 128) and rg < 2 * TOL[dtype] and rc < 2 * TOL[dtype]
