"""Towers with the erf GELU (HF ``hidden_act='gelu'``) and width 768 on the GPU (helpers: tests/gelu_tower_conformance.py; the CPU
side: tests/test_gelu_tower_cpu.py).

  5. GEMM conformance of the LayerNorm-fold consumer with SLIME_EPI_BIAS_GELU_T: element by element under the derived bound, in
     every kernel family (forced in the diagnostic library), sentinels intact, the three operand forms bit-equal;
     ``slime_gemm_ksplit`` with this form.
  6. The tower against HF ``CLIPVisionModel`` (fp32, CPU): every hidden state and ``encode``, at the tolerances of
     tests/test_gpu_path.py.  The fp16 exact-GELU cases are the ones that tell the two activations apart (measured at these seeds:
     the quick-GELU states lie 5.9e-3 .. 8.7e-3 from the exact-GELU states, inside the bf16 tolerance of 8e-3 and about five times
     the fp16 tolerance of 1.2e-3), and carry an assertion that the input keeps that power.
  7. ``slime_vit_forward_opts`` bit-equal to a replay of its launches through the C ABI, fc1's epilogue taken from the activation.
  8. ``slime_vit_forward_opts`` with opts = NULL and act = 0 bit-equal to the existing entries.
  9. The plugin surface over a 768-wide exact-GELU tower loaded from a directory.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import gelu_tower_conformance as G
import gemm_conformance as GC
import tower_conformance as TC
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


# ------------------------------------------------------------------------------------------------ 5. GEMM conformance
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
    return f"{G.FORM} {c.kind} {DT_ID[c.dtype]} M={c.M} N={c.N} K={c.K} guard={c.guard} {extra}"


def _run(lib, c, what, bm, **kw):
    """reference -> one launch per operand form -> the first inside the bound element by element, the others bit-equal to it, every
    byte outside the C window untouched.  -> worst |err| / bound."""
    r = G.reference(c)
    frag = _pack(lib, c)
    first = None
    for op in ("B+frag", "B", "frag"):
        c.restore()
        _gemm(lib, c, op, frag, **kw)
        assert c.intact() is None, f"{what} [{op}]: a byte outside the C window was written"
        outs = c.windows()
        if first is None:
            first = outs
            ratio, msg = G.check(c, r, outs, bm)
            assert msg is None, f"{what} [{op}]: {msg}"
        else:
            assert _biteq(outs["C"], first["C"]), f"{what}: operand form {op} differs in bits from B+frag"
    return ratio


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("tile", G.TILES)
def test_fold_gelu_in_every_kernel_family(dev, tile, dtype):
    """One kernel family x one dtype: the row edges of the family's tile (1, 15, 16, 17, BM - 1, BM, BM + 1, 2 BM + 17), K = 64 / 192 /
    2112 (one k-tile, fewer than the ring's stages, the long-K instantiation), two widths, the kinds and guard passes in turn."""
    bm, worst, n = GC.TILE_BM[tile], 0.0, 0
    with _forced(tile) as lib:
        for N in G.fold_n(tile):
            for M in GC.m_table(bm):
                for K in G.FOLD_K:
                    n += 1
                    c = G.make_case(("random", "tails")[n % 2], dtype, M, N, K, guard=GUARDS[(n // 2) % 2], seed=n, device=dev)
                    worst = max(worst, _run(lib, c, _what(c, f"tile {tile}"), bm))
    print(f"\n{GC.TILE_FAMILY[tile]} {G.FORM} {DT_ID[dtype]}: worst |err| / bound {worst:.3f} over {n} cases")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_fold_gelu_product_dispatch_and_kernel_name(dev, dtype):
    """The product library at the shapes where auto_tile picks the direct-B kernel (fc1 of a tower pass) and the 64 x 64 ring, each
    proven by slime_gemm_kernel_name with the epilogue code of this form; a bias of NULL."""
    from slime_amd import ops
    lib = _lib()
    t = {torch.bfloat16: "BF16", torch.float16: "F16"}[dtype]
    assert ops.gemm_kernel_name(2049, 4096, 128, dtype, GC.EPI_BIAS_GELU_T, True) == f"gemm_db_kernel<{t}, 2, 0, 8>"
    assert ops.gemm_kernel_name(100, 256, 64, dtype, GC.EPI_BIAS_GELU_T, False) == f"gemm_kernel<{t}, 64, 64, 4, 1, 2, 2>"
    for n, (M, N, K) in enumerate(((2049, 4096, 128), (100, 256, 64))):
        c = G.make_case(("random", "tails")[n], dtype, M, N, K, guard=GUARDS[n], seed=n, device=dev)
        _run(lib, c, _what(c, "product"), 128)
    c = G.make_case("tails", dtype, 145, 256, 128, guard="nan", bias=False, seed=3, device=dev)
    _run(lib, c, _what(c, "bias = NULL"), 128)


def _row_ptr(p, r):
    return p.ptr() + r * p.ld * p.flat.element_size()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_fold_gelu_ksplit(dev, dtype):
    """slime_gemm_ksplit with this form: inside the bound and operand-form invariant at splits 2 and 4 (exactly sized guarded
    workspace); splits = 1 is slime_gemm_ex; per setting the rows do not depend on M (65 rows alone and inside 4100: both tiles of the
    pair) nor on how they are cut into calls; a second run on a workspace full of NaN patterns gives the same bits."""
    lib = _lib()
    for n, (M, N, K, S) in enumerate(((273, 384, 576, 4), (65, 128, 192, 2), (129, 256, 2112, 3))):
        c = G.make_case(("random", "tails")[n % 2], dtype, M, N, K, guard=GUARDS[n % 2], seed=n, device=dev)
        ws = GuardedWorkspace(lib.slime_gemm_ksplit_workspace_bytes(M, N, S), dev)
        _run(lib, c, _what(c, f"splits {S}"), 64, splits=S, ws=ws)
        assert ws.intact(), "slime_gemm_ksplit wrote outside its workspace"
        first = c.windows()["C"]
        c.restore()
        ws.window.fill_(0xFF)
        _gemm(lib, c, "B", None, splits=S, ws=ws)
        assert _biteq(c.windows()["C"], first), "not deterministic"
    c = G.make_case("random", dtype, 65, 128, 320, seed=9, device=dev)
    _gemm(lib, c, "B", None, splits=1)                       # ws = NULL is accepted: the unsplit call itself
    one = c.windows()["C"]
    c.restore()
    _gemm(lib, c, "B", None)
    assert _biteq(c.windows()["C"], one), "splits = 1 is not slime_gemm_ex"
    for S in (2, 4):
        M, N, K = 4100, 128, 384                            # 6 k-tiles; a statistics row is 48 bytes: every row offset stays 16-byte aligned
        c = G.make_case("random", dtype, M, N, K, seed=S, device=dev)
        ws = GuardedWorkspace(lib.slime_gemm_ksplit_workspace_bytes(M, N, S), dev)
        _gemm(lib, c, "B", None, splits=S, ws=ws)
        assert c.intact() is None and ws.intact()
        whole = c.windows()["C"]
        c.restore()
        for lo, hi in ((0, 65), (4000, 4065), (65, 4000), (4065, 4100)):       # M-invariance at 65 rows, and a partition of all rows
            b = c.buf
            _gemm(lib, c, "B", None, splits=S, ws=ws, A=_row_ptr(b["A"], lo), C=_row_ptr(b["C"], lo), M=hi - lo,
                  ln_stats=_row_ptr(b["ln_stats"], lo))
            assert _biteq(c.windows()["C"][lo:hi], whole[lo:hi]), f"splits={S}: rows {lo}..{hi} depend on M or on the cut"
        assert _biteq(c.windows()["C"], whole) and c.intact() is None


# ------------------------------------------------------------------------------------------------ towers and the HF yardstick
# name -> (image, patch, D, inter, layers, crops)
GEOMS = {"d128": (224, 14, 128, 512, 3, 2), "d768": (224, 16, 768, 3072, 2, 2), "d1024": (336, 14, 1024, 4096, 2, 1)}
_cases = {}


def _case(name, act):
    """(cfg, prefixed state dict, pixels, HF fp32 hidden states) -- weights seed 7, pixels seed 3, built once and left unchanged."""
    key = (name, act)
    if key not in _cases:
        from slime_amd import weights as W
        image, patch, D, inter, layers, n = GEOMS[name]
        cfg = G.vision_config(image, patch, D, inter, layers, act)
        other = _cases.get((name, "gelu" if act == "quick_gelu" else "quick_gelu"))
        sd = other[1] if other else W.make_tower_state_dict(cfg, seed=7)
        px = other[2] if other else W.synthetic_pixels(n, seed=3, image_size=image)
        _cases[key] = (cfg, sd, px, G.hf_states(cfg, sd, px))
    return _cases[key]


_packed = {}


def _pack_tower(name, act, dtype, dev, select_layer=None):
    cfg, sd, _, _ = _case(name, act)
    L = cfg.num_hidden_layers if select_layer is None else select_layer
    key = (name, act, dtype, L)
    if key not in _packed:
        from slime_amd import ops
        _packed[key] = ops.pack_tower(sd, cfg, dtype, dev, select_layer=L)
    return _packed[key]


def _within(got, want, dtype, what):
    r, w = G.rel_l2(got, want), G.worst_token(got, want)
    print(f"{what}: rel-L2 {r:.3e} (tolerance {TOL[dtype]:.1e}), worst token {w:.3e}")
    assert r < TOL[dtype], (what, r)
    assert w <= 4 * TOL[dtype], (what, w)


# both activations at 768, the exact GELU at 128, fp16 and bf16; one exact-GELU case at the production width, fp16
TOWER_CASES = [(n, a, dt) for n, a in (("d768", "gelu"), ("d768", "quick_gelu"), ("d128", "gelu")) for dt in DTYPES] + \
              [("d1024", "gelu", torch.float16)]


@pytest.mark.parametrize("name,act,dtype", TOWER_CASES, ids=[f"{n}-{a}-{DT_ID[dt]}" for n, a, dt in TOWER_CASES])
def test_tower_against_hf(dev, name, act, dtype):
    """Every hidden state (ops.tower_hidden_states) and HipCLIPVisionModel.encode at select_layer = -2, 'patch' and 'cls_patch',
    against HF: rel-L2 below test_gpu_path's tolerance, worst token at most four times it.  With fp16 and the exact GELU the HF
    quick-GELU states must lie at least three tolerances from the HF exact-GELU states (a condition on the input: the comparison
    can tell the activations apart)."""
    from slime_amd import _lib, ops
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    cfg, sd, px, hf = _case(name, act)
    L = cfg.num_hidden_layers
    if dtype == torch.float16 and act == "gelu":
        _, _, _, hfq = _case(name, "quick_gelu")
        apart = [G.rel_l2(hfq[i], hf[i]) for i in range(1, L + 1)]
        print(f"\n{name}: HF quick-GELU vs HF exact-GELU states 1..{L}: " + " ".join(f"{v:.2e}" for v in apart))
        assert min(apart) >= 3 * TOL[dtype], apart
    pt = _pack_tower(name, act, dtype, dev)
    assert pt.act == _lib.ACT_BY_NAME[act] and pt.layers_run == L
    st = ops.tower_hidden_states(pt, px.to(dev))
    assert st.shape == (L + 1, px.shape[0], cfg.seq_len, cfg.hidden_size) and st.dtype == torch.float32
    for i in range(L + 1):
        _within(st[i], hf[i], dtype, f"{name} {act} {DT_ID[dtype]} state {i}")
    m = HipCLIPVisionModel(cfg, dtype)
    m.load_state_dict(sd)
    m.to(dev)
    for keep in (False, True):
        out = m.encode(px.to(dev), -2, keep_cls=keep, out_dtype=torch.float32)
        want = hf[-2] if keep else hf[-2][:, 1:]
        assert out.shape == want.shape
        _within(out, want, dtype, f"{name} {act} {DT_ID[dtype]} encode select_layer=-2 {'cls_patch' if keep else 'patch'}")
    assert _biteq(m.encode(px.to(dev), L, keep_cls=True, out_dtype=torch.float32), st[L])


# ------------------------------------------------------------------------------------------------ 7. bit-equal replay
def _opts_call(desc, opts, pad, pix_dtype, n, out, out_dtype, keep_cls, hidden, states, ks, ws, nbytes=None):
    from slime_amd import ops
    p = lambda x: None if x is None else x.ptr()
    return _lib().slime_vit_forward_opts(C.byref(desc), opts, pad.ptr(), ops.dtype_code(pix_dtype), n, p(out), ops.dtype_code(out_dtype),
                                         keep_cls, p(hidden), p(states), None if ks is None else C.byref(_L().VitKsplit(*ks)),
                                         ws.ptr(), ws.nbytes if nbytes is None else nbytes, _stream())


def _ws_bytes(desc, n, ks=None):
    if ks is None:
        return _lib().slime_vit_workspace_bytes(C.byref(desc), n)
    return _lib().slime_vit_ksplit_workspace_bytes(C.byref(desc), n, C.byref(_L().VitKsplit(*ks)))


def _run_opts(pt, opts, cfg, pad, pix_dtype, n, out_dtype, keep_cls, dev, ks=None, want_states=False):
    """slime_vit_forward_opts into guarded buffers (out, hidden_f32 and optionally the states) with an exactly sized workspace."""
    D, S, L = cfg.hidden_size, cfg.seq_len, pt.layers_run
    out = guarded_output(n * (S if keep_cls else S - 1), D, out_dtype, dev)
    hid = guarded_output(n * S, D, torch.float32, dev)
    sts = guarded_output((L + 1) * n * S, D, torch.float32, dev) if want_states else None
    bufs = [b for b in (out, hid, sts) if b is not None]
    snaps = [b.snapshot() for b in bufs]
    ws = GuardedWorkspace(_ws_bytes(pt.desc, n, ks), dev)
    rc = _opts_call(pt.desc, opts, pad, pix_dtype, n, out, out_dtype, keep_cls, hid, sts, ks, ws)
    assert rc == 0, _lib().slime_last_error().decode()
    torch.cuda.synchronize()
    assert ws.intact(), "the tower wrote outside the workspace the size query told the caller to allocate"
    for b, s in zip(bufs, snaps):
        assert b.intact(s) and not bool(sentinel_rows(b.win).any())
    return out.win, hid.win, (sts.win.view(L + 1, n * S, D) if want_states else None)


def _guarded_pixels(px, pix_dtype, dev):
    n, I = px.shape[0], px.shape[-1]
    pad = guarded_input(px.to(pix_dtype).to(dev), n * 3 * I)
    return pad, pad.win.view(n, 3, I, I)


REPLAY_CASES = [("d768", "gelu"), ("d768", "quick_gelu"), ("d128", "gelu")]        # S = 197, 197, 257


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name,act", REPLAY_CASES, ids=[f"{n}-{a}" for n, a in REPLAY_CASES])
def test_forward_opts_equals_the_replay_bit_for_bit(dev, name, act, dtype):
    """The fused entry against tower_conformance.replay_vit on a backend that makes the same launches through slime_patch_embed_prenorm,
    slime_gemm_ex (or slime_gemm_ksplit), slime_attention and slime_gather_rows_split, fc1 with the activation's epilogue: out (fp32
    without, T with the class token), hidden_f32 and every state, unsplit and with the k-split (2, 1, 2, 4)."""
    cfg, sd, px, _ = _case(name, act)
    assert cfg.seq_len == {"d768": 197, "d128": 257}[name]
    L, n = cfg.num_hidden_layers, px.shape[0]
    pt = _pack_tower(name, act, dtype, dev)
    opts = C.byref(_L().VitOpts(pt.act))
    for pix, odt, keep, ks in ((torch.float32, torch.float32, 0, None), (dtype, dtype, 1, None), (torch.float32, torch.float32, 0, (2, 1, 2, 4))):
        pad, view = _guarded_pixels(px, pix, dev)
        out, hid, sts = _run_opts(pt, opts, cfg, pad, pix, n, odt, keep, dev, ks=ks, want_states=True)
        be = G.HipBackend(dtype, dev, act)
        ref = TC.replay_vit(be, pt.tensors, cfg, view, L, keep_cls=keep, out_dtype=odt, want_hidden=True, want_states=True,
                            k_split=ks or (1, 1, 1, 1))
        what = (name, act, DT_ID[dtype], DT_ID.get(pix, "f32"), keep, ks)
        assert [k[4] for k in be.kernels if k[0] == "w_fc1"] == [G.fc1_epilogue(act)] * L, be.kernels
        assert _biteq(out, ref["out"]) and _biteq(hid, ref["hidden"]), what
        for i in range(L + 1):
            assert _biteq(sts[i], ref["states"][i]), (what, i)
        assert _biteq(sts[L], hid)
    if act == "quick_gelu":            # the 768-wide quick-GELU tower through the entries that existed: the same bits
        pad, _ = _guarded_pixels(px, torch.float32, dev)
        out, hid, _ = _run_opts(pt, None, cfg, pad, torch.float32, n, torch.float32, 0, dev)
        o2 = guarded_output(n * (cfg.seq_len - 1), cfg.hidden_size, torch.float32, dev)
        ws = GuardedWorkspace(_ws_bytes(pt.desc, n), dev)
        assert _lib().slime_vit_forward(C.byref(pt.desc), pad.ptr(), _L().F32, n, o2.ptr(), _L().F32, 0, None, ws.ptr(), ws.nbytes, _stream()) == 0
        torch.cuda.synchronize()
        assert ws.intact() and _biteq(o2.win, out)
    else:                              # and the activation is not a no-op: the quick-GELU pass over the same weights differs
        pad, _ = _guarded_pixels(px, torch.float32, dev)
        a, _, _ = _run_opts(pt, opts, cfg, pad, torch.float32, n, torch.float32, 0, dev)
        b, _, _ = _run_opts(pt, None, cfg, pad, torch.float32, n, torch.float32, 0, dev)
        assert not _biteq(a, b) and G.rel_l2(a, b) > 1e-3


# ------------------------------------------------------------------------------------------------ 8. nothing moved
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_opts_null_and_act_0_are_the_existing_entries(dev, dtype):
    """The TINY tower at 336 / 14: slime_vit_forward_opts with opts = NULL and with act = SLIME_ACT_QUICKGELU stores the bits of
    slime_vit_forward, of slime_vit_forward_ksplit at (2, 2, 2, 4) and of slime_vit_forward_states."""
    from slime_amd import ops, weights as W
    lib, L_ = _lib(), _L()
    cfg, n = W.TINY, 3
    pt = ops.pack_tower(W.strip_tower_prefix(W.make_tower_state_dict(cfg, seed=11)), cfg, dtype, dev, select_layer=cfg.num_hidden_layers)
    L, S, D = pt.layers_run, cfg.seq_len, cfg.hidden_size
    pad, _ = _guarded_pixels(W.synthetic_pixels(n, seed=22), torch.float32, dev)
    d, px = C.byref(pt.desc), pad.ptr()
    mk_out = lambda: guarded_output(n * (S - 1), D, dtype, dev)
    mk_hid = lambda: guarded_output(n * S, D, torch.float32, dev)
    mk_ws = lambda ks=None: GuardedWorkspace(_ws_bytes(pt.desc, n, ks), dev)
    code = ops.dtype_code(dtype)
    ks = (2, 2, 2, 4)
    o0, h0, w0 = mk_out(), mk_hid(), mk_ws()
    assert lib.slime_vit_forward(d, px, L_.F32, n, o0.ptr(), code, 0, h0.ptr(), w0.ptr(), w0.nbytes, _stream()) == 0
    o1, h1, w1 = mk_out(), mk_hid(), mk_ws(ks)
    assert lib.slime_vit_forward_ksplit(d, px, L_.F32, n, o1.ptr(), code, 0, h1.ptr(), C.byref(L_.VitKsplit(*ks)), w1.ptr(), w1.nbytes,
                                        _stream()) == 0
    s2, w2 = guarded_output((L + 1) * n * S, D, torch.float32, dev), mk_ws()
    assert lib.slime_vit_forward_states(d, px, L_.F32, n, s2.ptr(), w2.ptr(), w2.nbytes, _stream()) == 0
    torch.cuda.synchronize()
    assert w0.intact() and w1.intact() and w2.intact()
    for opts in (None, C.byref(L_.VitOpts(L_.ACT_QUICKGELU))):
        out, hid, _ = _run_opts(pt, opts, cfg, pad, torch.float32, n, dtype, 0, dev)
        assert _biteq(out, o0.win) and _biteq(hid, h0.win), "slime_vit_forward"
        out, hid, _ = _run_opts(pt, opts, cfg, pad, torch.float32, n, dtype, 0, dev, ks=ks)
        assert _biteq(out, o1.win) and _biteq(hid, h1.win), "slime_vit_forward_ksplit"
        assert not _biteq(o1.win, o0.win), "the k-split setting changed nothing: the comparison above shows nothing"
        _, hid, sts = _run_opts(pt, opts, cfg, pad, torch.float32, n, torch.float32, 1, dev, want_states=True)
        assert _biteq(sts, s2.win.view(L + 1, n * S, D)) and _biteq(hid, h0.win), "slime_vit_forward_states"


# ------------------------------------------------------------------------------------------------ 9. plugin surface
PINPOINTS = "[(224, 448), (448, 224), (448, 448)]"
HIDDEN = 256


def _projector_state(kind, D):
    g = torch.Generator().manual_seed(12)
    r = lambda *s, std: torch.randn(*s, generator=g) * std
    if kind == "linear":
        return {"weight": r(HIDDEN, D, std=D ** -0.5), "bias": r(HIDDEN, std=0.02)}
    return {"0.weight": r(HIDDEN, D, std=D ** -0.5), "0.bias": r(HIDDEN, std=0.02),
            "2.weight": r(HIDDEN, HIDDEN, std=HIDDEN ** -0.5), "2.bias": r(HIDDEN, std=0.02)}


def _encoder(path, dev, dtype, projector, embed=None, **over):
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    cfg = default_slime_config(str(path), hidden_size=HIDDEN, mm_hidden_size=768, mm_resampler_type=None, mm_projector_type=projector,
                               image_grid_pinpoints=PINPOINTS, **over)
    enc = SlimeVisualEncoder(cfg, embed_tokens=embed)
    enc.get_vision_tower().load_model()
    psd = _projector_state(projector, 768)
    enc.get_model().mm_projector.load_state_dict(psd)
    enc.to(dev)
    enc.get_vision_tower().vision_tower.to(dtype)
    return enc, psd


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_plugin_surface_over_a_768_wide_gelu_tower(dev, tmp_path, dtype):
    """CLIPVisionTower from a directory written here (hidden_act 'gelu', 768 wide, 224 / 16): its features against HF's; encode_images on
    the plain branch with mlp2x_gelu and with linear against oracle.mlp_projector / F.linear on HF's features; a list of images;
    split_sizes without a sampler; one un-sampled 'spatial' merge over two images against the per-image features, row for row."""
    import torch.nn as nn
    from oracle import slime_oracle as O
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    cfg, sd, px32, _ = _case("d768", "gelu")
    G.write_hf_dir(tmp_path, sd, cfg)
    px = px32.to(dtype)                                       # what `images.to(dtype=self.dtype)` hands the reference's tower
    hf = G.hf_states(cfg, sd, px.float())[-2][:, 1:]
    t = build_vision_tower(SimpleNamespace(mm_vision_tower=str(tmp_path), mm_vision_select_layer=-2, mm_vision_select_feature="patch",
                                           mm_vision_compute_dtype=dtype))
    assert t.is_loaded and t.config == cfg and t.hidden_size == 768 and t.num_patches == 196 and t.num_patches_per_side == 14
    t.to(dev)
    feats = t(px.float().to(dev))
    assert feats.dtype == torch.float32 and feats.shape == hf.shape
    _within(feats, hf, dtype, f"CLIPVisionTower {DT_ID[dtype]}")
    one = t([p for p in px.to(dev)])
    assert len(one) == px.shape[0] and one[0].dtype == dtype and one[0].shape == (1, 196, 768)
    for kind in ("mlp2x_gelu", "linear"):
        enc, psd = _encoder(tmp_path, dev, dtype, kind)
        got, _ = enc.encode_images(px.to(dev))
        if kind == "linear":
            want = torch.nn.functional.linear(hf, psd["weight"], psd["bias"])
        else:
            want = O.mlp_projector({"projection." + k: v for k, v in psd.items()}, hf)
        assert got.dtype == dtype and got.shape == want.shape == (px.shape[0], 196, HIDDEN)
        r = G.rel_l2(got, want)
        print(f"encode_images plain, {kind} {DT_ID[dtype]}: rel-L2 {r:.3e}")
        assert r < TOL[dtype], (kind, r)
        per, splits = enc.encode_images(px.to(dev), split_sizes=[1, 1])
        assert splits == [1, 1] and len(per) == 2 and all(_biteq(per[i], got[i:i + 1]) for i in range(2))
    # the un-sampled 'spatial' merge over two images with different grids.  The grid is the reference's rule as it stands (the uhd
    # canvas of a 336 crop, divided by the tower's image size: mm_utils.get_anyres_image_grid_shape), taken from the library
    from slime_amd import weights as W
    from slime_amd.mm_utils import get_anyres_image_grid_shape
    embed = nn.Embedding(64, HIDDEN)
    embed.weight.data.copy_(torch.randn(64, HIDDEN, generator=torch.Generator().manual_seed(3)) * 0.5)
    enc, _ = _encoder(tmp_path, dev, dtype, "mlp2x_gelu", embed=embed.to(dtype), mm_patch_merge_type="spatial")
    sizes = [(448, 224), (448, 448)]
    grids = [tuple(int(v) for v in get_anyres_image_grid_shape(sz, PINPOINTS, 224)) for sz in sizes]
    assert grids[0] != grids[1] and all(nw * nh > 1 for nw, nh in grids), grids
    splits = [1 + nw * nh for nw, nh in grids]
    pxs = [W.synthetic_pixels(c, seed=60 + i, image_size=224).to(dev).to(dtype) for i, c in enumerate(splits)]
    ids = torch.randint(3, 64, (2, 8), generator=torch.Generator().manual_seed(5))
    ids[0, 2] = ids[1, 5] = IMAGE_TOKEN_INDEX
    ids, am = ids.to(dev), torch.ones(2, 8, dtype=torch.long, device=dev)
    lab = torch.where(ids == IMAGE_TOKEN_INDEX, torch.full_like(ids, -100), ids)
    pos = torch.arange(8, device=dev).expand(2, 8).contiguous()
    per, _ = enc.encode_images(torch.cat(pxs, 0), ids, splits, am, None, sizes, labels=lab)
    assert [tuple(f.shape) for f in per] == [(s, 196, HIDDEN) for s in splits]
    got = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, pxs, image_sizes=sizes)
    emb = got[4]
    for b, (f, (nw, nh), at) in enumerate(zip(per, grids, (2, 5))):
        x = f[1:].view(nh, nw, 14, 14, HIDDEN).permute(0, 2, 1, 3, 4).reshape(nh * 14 * nw * 14, HIDDEN)
        want = torch.cat([f[0], x], 0).to(emb.dtype)
        rows = 196 + nw * nh * 196
        assert want.shape[0] == rows and int(got[2][b].sum()) == 8 - 1 + rows          # row count: text + base + the raster
        assert _biteq(emb[b, at:at + rows], want), f"image {b}: the merged rows are not the per-image features in raster order"
        assert _biteq(emb[b, :at], enc.get_model().embed_tokens.weight.detach()[ids[b, :at]])
