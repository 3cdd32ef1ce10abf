"""DINOv2 vision towers on the GPU (helpers: tests/dinov2_tower_conformance.py; the CPU side: tests/test_dinov2_tower_cpu.py).

  1. The prefix front end (``slime_patch_embed_prefix``) element by element against float64: the patch rows of h inside the plain
     form's bound, x16 / lo8 the split of h in bits, stats the sums of the rounded rows, the prefix rows bit-equal to a host
     restatement (stats included: the kernel's order of additions), every byte around the outputs untouched, h-only and x16-only calls.
  2. The tower against HF ``Dinov2Model`` / ``Dinov2WithRegistersModel`` (fp32, CPU): every hidden state and ``encode`` at
     test_gpu_path's tolerances, with HF's own 16-bit drift measured beside them.
  3. ``slime_dinov2_forward`` bit-equal to a replay of its launches through the C ABI (guarded, exactly sized workspace; k-split on
     and off; keep_prefix 0 and 1; every output mode); batch and shard invariance in bits.
  4. The plugin surface: ``build_vision_tower`` on a 1024-wide, 16-per-side, 4-register directory, ``encode_images`` with
     mlp2x_gelu, the gated adapter and the sampler on a tiny tower, 'spatial_unpad' end to end, 'cls_patch' without registers.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import dinov2_tower_conformance as DV
import gemm_conformance as GC
from adapter_conformance import GuardedWorkspace, guarded_input, guarded_output, sentinel_rows

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "f32"}
TOL = {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}           # tests/test_gpu_path.py's own
DRIFT_FACTOR = 1.5                                            # test_gpu_router_attention.py's allowance on the reference's own drift


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


# ------------------------------------------------------------------------------------------------ 1. the prefix front end
# image, patch, D, n_prefix, crops: the smallest grids with and without registers, an odd grid (a one-row last pair: the last workgroup
# half empty), an even patch-16 grid, a released geometry, the largest LDS layout
FRONT = [(56, 14, 128, 1, 3), (56, 14, 128, 5, 3), (48, 16, 256, 1, 3), (64, 16, 256, 5, 3), (224, 14, 768, 1, 3), (336, 14, 1024, 5, 1)]


def _prefix_stats(rows16, D):
    """(sum, sum of squares) per 64-column group of rounded rows [R, D] (float32 values of T) in pe_prefix_row's order: a lane holds
    VEC consecutive columns and adds them in column order (the squares by fma), then a butterfly over the 64 / VEC lanes of a group."""
    VEC = 4 if D // 64 >= 4 else 2
    r = rows16.float().view(rows16.shape[0], D // 64, 64 // VEC, VEC)
    sx = torch.zeros(r.shape[:3], dtype=torch.float32)
    sq = torch.zeros(r.shape[:3], dtype=torch.float32)
    for j in range(VEC):
        sx = sx + r[..., j]
        sq = (sq.double() + r[..., j].double() * r[..., j].double()).float()          # fmaf: one rounding (the product is exact in float64)
    lanes = 64 // VEC
    idx = torch.arange(lanes)
    off = lanes // 2
    while off > 0:
        sx, sq = sx + sx[..., idx ^ off], sq + sq[..., idx ^ off]
        off //= 2
    return torch.stack([sx[..., 0], sq[..., 0]], -1)            # [R, D / 64, 2]


@pytest.mark.parametrize("pix", ["f32", "t"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("image,patch,D,npre,n", FRONT, ids=[f"{i}-p{p}-D{d}-pre{r}" for i, p, d, r, _ in FRONT])
def test_prefix_front_end_element_by_element(dev, image, patch, D, npre, n, dtype, pix):
    from slime_amd import ops, weights as W
    lib = _lib()
    cfg = DV.dinov2_config(image, D, 1, npre - 1, image // patch + 1, patch=patch)          # a table for one more patch per side
    P, g, S_ = cfg.num_patches, cfg.grid, cfg.seq_len
    kpad = (3 * patch * patch + 63) // 64 * 64
    sd = W.make_dinov2_state_dict(cfg, seed=31 + g)
    host = ops.dinov2_host_tensors(sd, cfg, dtype, 0)
    pos, prefix = host["pos"].to(dev), host["cls"].to(dev)
    assert pos.shape == (P, D) and prefix.shape == (npre, D)
    frag = ops.pack_b_frag(host["patch_w"].to(dev))
    px = W.synthetic_pixels(n, seed=g, image_size=image)
    px_in = px.to(dev) if pix == "f32" else px.to(dtype).to(dev)
    pad = guarded_input(px_in, n * 3 * image)
    h = guarded_output(n * S_, D, torch.float32, dev)
    x16 = guarded_output(n * S_, D, dtype, dev)
    lo = guarded_output(n * S_, D, torch.int8, dev)
    st = guarded_output(n * S_, 2 * (D // 64), torch.float32, dev)
    bufs = (h, x16, lo, st)
    snaps = [b.snapshot() for b in bufs]

    def call(h_, x_, lo_, st_):
        rc = lib.slime_patch_embed_prefix(pad.ptr(), ops.dtype_code(px_in.dtype), frag.data_ptr(), prefix.data_ptr(), npre, pos.data_ptr(),
                                          h_, x_, lo_, st_, ops.dtype_code(dtype), n, image, patch, kpad, D, _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.slime_last_error().decode()

    call(h.ptr(), x16.ptr(), lo.ptr(), st.ptr())
    for b, s in zip(bufs, snaps):                           # every byte around the outputs untouched; every row written
        assert b.intact(s) and not bool(sentinel_rows(b.win).any())
    is_patch = (torch.arange(n * S_) % S_ >= npre).to(dev)
    # the patch rows: the plain form's reference and bound, at row n_prefix + p of every crop
    want, dh = DV.embed64(px, {"patch_w": host["patch_w"], "pos": host["pos"]}, cfg, dtype)
    got = h.win[is_patch].cpu()
    ratio, ex, *_ = GC.worst(got, want, dh * (1 + 2.0 ** -10))
    assert ex <= 0, GC.describe_failure(f"prefix front end {image}/{patch} D={D}", got, want, dh, 48, "h")
    hi, l8 = ops.resid_split(h.win, dtype)
    assert _biteq(x16.win, hi) and _biteq(lo.win, l8), "x16 / lo8 are not the split of h"
    r = x16.win.double().view(n * S_, D // 64, 64)
    sums = torch.stack([r.sum(-1), (r * r).sum(-1)], -1)
    bd = 70 * GC.E32 * torch.stack([r.abs().sum(-1), (r * r).sum(-1)], -1) + 1e-30         # 63 additions + the fmas of the squares
    assert bool(((st.win.double().view(n * S_, D // 64, 2) - sums).abs() <= bd).all()), "stats are not the sums of the rounded rows"
    # the prefix rows: the table's own bits, its rounding, the split's lower part and the kernel's sums -- no arithmetic beyond them
    pre_h = h.win.view(n, S_, D)[:, :npre]
    assert _biteq(pre_h, prefix[None].expand(n, -1, -1)), "h's prefix rows are not the table"
    t16, tl8 = ops.resid_split(prefix, dtype)
    assert _biteq(x16.win.view(n, S_, D)[:, :npre], t16[None].expand(n, -1, -1)) and _biteq(t16, prefix.to(dtype))
    assert _biteq(lo.win.view(n, S_, D)[:, :npre], tl8[None].expand(n, -1, -1))
    want_st = _prefix_stats(prefix.to(dtype).cpu(), D)
    assert _biteq(st.win.view(n, S_, D // 64, 2)[:, :npre].cpu(), want_st[None].expand(n, -1, -1, -1)), "prefix stats"
    print(f"\nprefix front end {image}/{patch} g={g} D={D} n_prefix={npre} {DT_ID[dtype]} pixels {pix}: worst |err| / bound {ratio:.3f}")
    # outputs are optional one by one: h alone and x16 alone give the same bits
    only_h = guarded_output(n * S_, D, torch.float32, dev)
    call(only_h.ptr(), None, None, None)
    assert _biteq(only_h.win, h.win)
    only_x = guarded_output(n * S_, D, dtype, dev)
    call(None, only_x.ptr(), None, None)
    assert _biteq(only_x.win, x16.win)


# ------------------------------------------------------------------------------------------------ towers and the HF yardstick
# name -> (run size, D, layers, registers, table grid, crops): D 128 / 2 layers at 56 px; D 256 at 112 px under a table for 5 x 5
# (interpolated); D 128 / 1 layer at 224 px, S = 257 and 261: the generic attention kernel off every block boundary
GEOMS = {"d128g4": (56, 128, 2, 0, 4, 3), "d128g4r4": (56, 128, 2, 4, 4, 3),
         "d256g8": (112, 256, 2, 0, 5, 2), "d256g8r4": (112, 256, 2, 4, 5, 2),
         "d128g16": (224, 128, 1, 0, 16, 2), "d128g16r4": (224, 128, 1, 4, 16, 2)}
_cases, _packed = {}, {}


def _case(name):
    """(cfg, state dict, pixels, HF fp32 hidden states) -- weights seed 7, pixels seed 3, built once and left unchanged."""
    if name not in _cases:
        from slime_amd import weights as W
        image, D, layers, R, tg, n = GEOMS[name]
        cfg = DV.dinov2_config(image, D, layers, R, tg)
        sd = W.make_dinov2_state_dict(cfg, seed=7)
        px = W.synthetic_pixels(n, seed=3, image_size=image)
        _cases[name] = (cfg, sd, px, DV.hf_states(cfg, sd, px))
    return _cases[name]


def _pack_tower(name, dtype, dev):
    cfg, sd, _, _ = _case(name)
    if (name, dtype) not in _packed:
        from slime_amd import ops
        _packed[(name, dtype)] = ops.pack_dinov2_tower(sd, cfg, dtype, dev, select_layer=cfg.num_hidden_layers)
    return _packed[(name, dtype)]


def _within(got, want, dtype, what, drift=None):
    """rel-L2 below test_gpu_path's tolerance and the worst token within four times it; where ``drift`` (HF's own rel-L2 drift in the
    same 16-bit type on the same inputs) is given and the tolerance is missed, DRIFT_FACTOR x the drift decides, and says so."""
    r, w = DV.rel_l2(got, want), DV.worst_token(got, want)
    print(f"{what}: rel-L2 {r:.3e} (tolerance {TOL[dtype]:.1e}" + (f", HF's own drift {drift:.3e}" if drift is not None else "") +
          f"), worst token {w:.3e}")
    if r < TOL[dtype] and w <= 4 * TOL[dtype]:
        return
    assert drift is not None and r <= DRIFT_FACTOR * drift, (what, r, w, drift)
    print(f"{what}: outside the tolerance, inside {DRIFT_FACTOR} x HF's own {DT_ID[dtype]} drift")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_tower_against_hf(dev, name, dtype):
    """Every hidden state (ops.dinov2_tower_hidden_states, all S rows) and HipDinov2VisionModel.encode at select_layer = -2 and L
    against HF in fp32 on the CPU: rel-L2 below test_gpu_path's tolerance (fp16 1.2e-3, bf16 8e-3), worst token at most four times it.

    HF's own 16-bit drift on the same inputs (the HF model cast to T on the CPU against its fp32 self on the T-rounded pixels, rel-L2
    per state; printed by every run), over the six geometries: fp16 3.5e-4 .. 3.6e-4 at the embeddings, 5.5e-4 .. 5.8e-4 after one
    layer, 6.7e-4 .. 7.2e-4 after two; bf16 2.8e-3 .. 2.9e-3, 4.3e-3 .. 4.5e-3, 5.2e-3 .. 5.8e-3.  HF itself, with a 16-bit residual
    stream, uses 0.6 (fp16) and 0.7 (bf16) of the tolerances after two layers, so the tolerances stand for towers this deep; a
    state that misses one is still accepted within 1.5 x that drift (test_gpu_router_attention.py's rule), and the test says so
    where it happens."""
    from slime_amd import ops
    from slime_amd.model.multimodal_encoder.dinov2_encoder import HipDinov2VisionModel
    cfg, sd, px, hf = _case(name)
    L = cfg.num_hidden_layers
    own = DV.hf_states(cfg, sd, px.to(dtype).float(), dtype)
    ref_t = DV.hf_states(cfg, sd, px.to(dtype).float())
    drift = [DV.rel_l2(own[i].float(), ref_t[i]) for i in range(L + 1)]
    print(f"\n{name} {DT_ID[dtype]}: HF's own drift per state: " + " ".join(f"{v:.2e}" for v in drift))
    pt = _pack_tower(name, dtype, dev)
    st = ops.dinov2_tower_hidden_states(pt, px.to(dev))
    assert st.shape == (L + 1, px.shape[0], cfg.seq_len, cfg.hidden_size) and st.dtype == torch.float32
    for i in range(L + 1):
        _within(st[i], hf[i], dtype, f"{name} {DT_ID[dtype]} state {i}", drift[i])
    m = HipDinov2VisionModel(cfg, dtype)
    m.load_state_dict(sd)
    m.to(dev)
    out = m.encode(px.to(dev), -2, out_dtype=torch.float32)
    assert out.shape == (px.shape[0], cfg.num_patches, cfg.hidden_size)
    _within(out, hf[-2][:, cfg.n_prefix:], dtype, f"{name} {DT_ID[dtype]} encode select_layer=-2", drift[L - 1])
    assert _biteq(m.encode(px.to(dev), L, keep_cls=True, out_dtype=torch.float32), st[L])
    assert _biteq(m.encode(px.to(dev), L, out_dtype=torch.float32), st[L][:, cfg.n_prefix:])
    hs = m(px.to(dev), output_hidden_states=True).hidden_states
    assert len(hs) == L + 1 and _biteq(hs[L], st[L]) and _biteq(m(px.to(dev)).last_hidden_state, st[L])


# ------------------------------------------------------------------------------------------------ 3. the entry and its replay
def _dinov2_call(desc, npre, pad, pix_dtype, n, out, keep, hidden, states, ks, ws, nbytes=None):
    from slime_amd import ops
    p = lambda x: None if x is None else x.ptr()
    odt = ops.dtype_code(out.win.dtype) if out is not None else _L().F32
    return _lib().slime_dinov2_forward(C.byref(desc), npre, pad.ptr(), ops.dtype_code(pix_dtype), n, p(out), odt, keep, p(hidden), p(states),
                                       None if ks is None else C.byref(_L().VitKsplit(*ks)), ws.ptr(), ws.nbytes if nbytes is None else nbytes,
                                       _stream())


def _derived_ws_bytes(cfg, n, ks=None):
    """The workspace size from the header's description of the plan, derived here for S = n_prefix + P rows per crop: lo (1 B), xn
    (2 B), the shared q/k/v + ctx | ff region, the statistics -- each at a 256-B boundary -- and, with a k-split, the largest
    partial-product region."""
    up = lambda b: (b + 255) // 256 * 256
    M, D, F = n * cfg.seq_len, cfg.hidden_size, cfg.intermediate_size
    total = up(M * D) + up(M * D * 2) + up(max(M * F * 2, up(M * 3 * D * 2) + M * D * 2)) + up(M * (D // 64) * 8)
    if ks is not None:
        total += max(_lib().slime_gemm_ksplit_workspace_bytes(M, N, s) for N, s in zip((3 * D, D, F, D), ks))
    return total


def _run_entry(pt, cfg, pad, pix_dtype, n, out_dtype, keep, dev, ks=None):
    D, P, S_, L, npre = cfg.hidden_size, cfg.num_patches, cfg.seq_len, pt.layers_run, cfg.n_prefix
    out = guarded_output(n * (S_ if keep else P), D, out_dtype, dev)
    hid = guarded_output(n * S_, D, torch.float32, dev)
    sts = guarded_output((L + 1) * n * S_, D, torch.float32, dev)
    bufs = (out, hid, sts)
    snaps = [b.snapshot() for b in bufs]
    need = _derived_ws_bytes(cfg, n, ks)
    lib = _lib()
    q = lib.slime_dinov2_workspace_bytes(C.byref(pt.desc), npre, n) if ks is None else \
        lib.slime_dinov2_ksplit_workspace_bytes(C.byref(pt.desc), npre, n, C.byref(_L().VitKsplit(*ks)))
    assert q == need, (q, need)
    ws = GuardedWorkspace(need, dev)
    assert _dinov2_call(pt.desc, npre, pad, pix_dtype, n, out, keep, hid, sts, ks, ws, need - 256) == -2   # one block short: refused, nothing launched
    rc = _dinov2_call(pt.desc, npre, pad, pix_dtype, n, out, keep, hid, sts, ks, ws)
    assert rc == 0, lib.slime_last_error().decode()
    torch.cuda.synchronize()
    assert ws.intact(), "the tower wrote outside the workspace the size query told the caller to allocate"
    for b, s in zip(bufs, snaps):
        assert b.intact(s) and not bool(sentinel_rows(b.win).any())
    return out.win, hid.win, sts.win.view(L + 1, n * S_, D)


def _guarded_pixels(px, pix_dtype, dev):
    n, I = px.shape[0], px.shape[-1]
    pad = guarded_input(px.to(pix_dtype).to(dev), n * 3 * I)
    return pad, pad.win.view(n, 3, I, I)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", ["d128g4", "d128g4r4", "d256g8r4"])
def test_dinov2_forward_equals_the_replay_bit_for_bit(dev, name, dtype):
    """The fused entry against ``replay_dinov2`` on a backend that makes the same launches through slime_patch_embed_prefix,
    slime_gemm_ex (or slime_gemm_ksplit), slime_attention and slime_gather_rows_split, fc1 under SLIME_EPI_BIAS_GELU_T: out (fp32
    and T; the patch rows and all rows), hidden_f32 and every state, unsplit and with the k-split (2, 1, 2, 4); the two settings
    differ in bits; each output alone gives the same bits."""
    cfg, sd, px, _ = _case(name)
    L, n = cfg.num_hidden_layers, px.shape[0]
    pt = _pack_tower(name, dtype, dev)
    outs = {}
    for pix, odt, keep, ks in ((torch.float32, torch.float32, 0, None), (dtype, dtype, 1, None), (torch.float32, torch.float32, 1, (2, 1, 2, 4)),
                               (dtype, dtype, 0, (2, 1, 2, 4))):
        pad, view = _guarded_pixels(px, pix, dev)
        out, hid, sts = _run_entry(pt, cfg, pad, pix, n, odt, keep, dev, ks=ks)
        be = DV.HipBackend(dtype, dev)
        ref = DV.replay_dinov2(be, pt.tensors, cfg, view, L, keep_prefix=keep, out_dtype=odt, want_hidden=True, want_states=True,
                               k_split=ks or (1, 1, 1, 1))
        what = (name, DT_ID[dtype], DT_ID[pix], keep, ks)
        assert [k[4] for k in be.kernels if k[0] == "w_fc1"] == [GC.EPI_BIAS_GELU_T] * L, be.kernels
        assert _biteq(out, ref["out"]) and _biteq(hid, ref["hidden"]), what
        for i in range(L + 1):
            assert _biteq(sts[i], ref["states"][i]), (what, i)
        assert _biteq(sts[L], hid)
        # keep_prefix: the patch rows are rows n_prefix.. of every crop, all rows are the state itself (cast to the out dtype)
        rows = hid.view(n, cfg.seq_len, -1) if keep else hid.view(n, cfg.seq_len, -1)[:, cfg.n_prefix:]
        assert _biteq(out.view(n, -1, cfg.hidden_size), rows.to(odt)), what
        outs[(pix, ks)] = hid
    assert not _biteq(outs[(torch.float32, None)], outs[(torch.float32, (2, 1, 2, 4))]), "the k-split setting changed nothing"
    # any one output alone: the same bits
    D, S_, P, npre = cfg.hidden_size, cfg.seq_len, cfg.num_patches, cfg.n_prefix
    pad, _ = _guarded_pixels(px, torch.float32, dev)
    ws = GuardedWorkspace(_derived_ws_bytes(cfg, n), dev)
    only_h = guarded_output(n * S_, D, torch.float32, dev)
    assert _dinov2_call(pt.desc, npre, pad, torch.float32, n, None, 0, only_h, None, None, ws) == 0
    only_o = guarded_output(n * P, D, torch.float32, dev)
    assert _dinov2_call(pt.desc, npre, pad, torch.float32, n, only_o, 0, None, None, None, ws) == 0
    only_s = guarded_output((L + 1) * n * S_, D, torch.float32, dev)
    assert _dinov2_call(pt.desc, npre, pad, torch.float32, n, None, 1, None, only_s, None, ws) == 0
    torch.cuda.synchronize()
    want = outs[(torch.float32, None)]
    assert ws.intact() and _biteq(only_h.win, want) and _biteq(only_s.win.view(L + 1, n * S_, D)[L], want)
    assert _biteq(only_o.win.view(n, P, D), want.view(n, S_, D)[:, npre:])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_batch_and_shard_invariance_in_bits(dev, dtype):
    """1 + 2 crops = 3 crops: with one k-split setting the features do not depend on how the crops are cut into calls (the unsplit
    call may change its tile with M; the split pair is M-invariant by construction); ops.dinov2_tower_forward's ``out=`` slices
    land in one tensor; the two-stream encode equals the one-stream encode."""
    from slime_amd import ops
    from slime_amd.model.multimodal_encoder.dinov2_encoder import HipDinov2VisionModel
    cfg, sd, px, _ = _case("d128g4r4")
    pt = _pack_tower("d128g4r4", dtype, dev)
    x = px.to(dev)
    for ks in ((2, 2, 2, 4), None):
        for keep in (False, True):
            whole = ops.dinov2_tower_forward(pt, x, torch.float32, keep_prefix=keep, k_split=ks)
            parts = torch.empty_like(whole)
            ops.dinov2_tower_forward(pt, x[:1], torch.float32, keep_prefix=keep, out=parts[:1], k_split=ks)
            ops.dinov2_tower_forward(pt, x[1:], torch.float32, keep_prefix=keep, out=parts[1:], k_split=ks)
            torch.cuda.synchronize()
            assert _biteq(parts, whole), f"k_split={ks} keep_prefix={keep}: 1 + 2 crops differ from 3 crops"
    m = HipDinov2VisionModel(cfg, dtype)
    m.load_state_dict(sd)
    m.to(dev)
    big = torch.cat([x, x, x], 0)                            # 9 crops: the two-stream split (5 + 4)
    m.k_split = (2, 2, 2, 4)
    two = m.encode(big, -2, out_dtype=torch.float32)
    m.two_streams = False
    one = m.encode(big, -2, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert _biteq(two, one) and _biteq(two[:3], two[3:6]) and two.shape == (9, cfg.num_patches, cfg.hidden_size)


# ------------------------------------------------------------------------------------------------ 4. plugin surface
HIDDEN = 256


def _projector_state(D):
    g = torch.Generator().manual_seed(12)
    r = lambda *s, std: torch.randn(*s, generator=g) * std
    return {"0.weight": r(HIDDEN, D, std=D ** -0.5), "0.bias": r(HIDDEN, std=0.02),
            "2.weight": r(HIDDEN, HIDDEN, std=HIDDEN ** -0.5), "2.bias": r(HIDDEN, std=0.02)}


def test_plugin_surface_over_a_1024_wide_g16_tower_with_registers(dev, tmp_path):
    """Dinov2VisionTower from a directory written here (1024 wide, 224 / 14 under a table for 37 x 37, 4 registers, two layers): its
    features against HF's patch rows, the list branch, then encode_images on the plain branch with mlp2x_gelu against
    oracle.mlp_projector on HF's features."""
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    from slime_amd.model.multimodal_encoder.dinov2_encoder import Dinov2VisionTower
    dtype = torch.float16
    cfg = DV.dinov2_config(224, 1024, 2, 4, 37)
    sd = W.make_dinov2_state_dict(cfg, seed=7)
    DV.write_hf_dir(tmp_path, sd, cfg)
    px = W.synthetic_pixels(1, seed=3, image_size=224).to(dtype)
    hf = DV.hf_states(cfg, sd, px.float())[-1][:, cfg.n_prefix:]
    t = build_vision_tower(SimpleNamespace(mm_vision_tower=str(tmp_path), mm_vision_select_layer=-1, mm_vision_select_feature="patch",
                                           mm_vision_compute_dtype=dtype))
    assert type(t) is Dinov2VisionTower and t.config == cfg and t.hidden_size == 1024 and t.num_patches == 256 and t.num_patches_per_side == 16
    t.to(dev)
    feats = t(px.float().to(dev))
    assert feats.dtype == torch.float32 and feats.shape == hf.shape == (1, 256, 1024)
    _within(feats, hf, dtype, "Dinov2VisionTower fp16")
    one = t([p for p in px.to(dev)])
    assert len(one) == 1 and one[0].dtype == dtype and one[0].shape == (1, 256, 1024)
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
    assert got.dtype == dtype and got.shape == want.shape == (1, 256, HIDDEN)
    r = DV.rel_l2(got, want)
    print(f"encode_images plain, mlp2x_gelu fp16: rel-L2 {r:.3e}")
    assert r < TOL[dtype], r


def _tiny_dir(tmp_path, registers, layers=2):
    """A tiny tower (128 wide) at 336 / 14: the adapter's 24 x 24 token grid, S = 577 / 581 (the attn64r kernel)."""
    from slime_amd import weights as W
    cfg = DV.dinov2_config(336, 128, layers, registers, 37)
    sd = W.make_dinov2_state_dict(cfg, seed=11)
    DV.write_hf_dir(tmp_path, sd, cfg)
    return cfg, sd


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_gated_adapter_and_sampler_on_the_tiny_dinov2_tower(dev, tmp_path, dtype):
    """The tiny DINOv2 tower with 4 registers from a directory, its patch features through the GatedBlock and post_qformer of the
    tiny adapter, against the oracle on HF's features."""
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    cfg, sd = _tiny_dir(tmp_path, 4)
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    enc = SlimeVisualEncoder(default_slime_config(str(tmp_path), hidden_size=256, mm_hidden_size=128, mm_vision_select_layer=-1))
    vt = enc.get_vision_tower()
    vt.load_model()
    enc.load_visual_state(None, asd)
    enc.to(dev)
    vt.vision_tower.to(dtype)
    px = W.synthetic_pixels(3, seed=22, image_size=336)
    hf = DV.hf_states(cfg, sd, px.to(dtype).float())[-1][:, cfg.n_prefix:]
    x = vt(px.to(dev).to(dtype))
    assert x.dtype == dtype and x.shape == (3, 576, 128)
    _within(x, hf, dtype, f"tiny DINOv2 tower {DT_ID[dtype]}")
    proj_sd, post_sd = W.sub_state(asd, "mm_projector."), W.sub_state(asd, "sampler.post_qformer.")
    m = enc.get_model()
    g = m.mm_projector(x[:1])
    # two links, each held to TOL by its own tests (the tower above; the adapter modules on exact features in test_gpu_modules):
    # their sum bounds the chain
    rg = DV.rel_l2(g, O.gated_block_forward(proj_sd, hf[:1], 1))
    comp = m.sampler.post_qformer(x[1:])
    rc = DV.rel_l2(comp, O.resampler_forward(post_sd, hf[1:], 1))
    print(f"gated {rg:.3e}, post_qformer {rc:.3e} (tolerance {2 * TOL[dtype]:.1e})")
    assert g.shape == (1, 576, 256) and comp.shape == (2, 144, 128) and rg < 2 * TOL[dtype] and rc < 2 * TOL[dtype]


def test_cls_patch_without_registers(dev, tmp_path):
    """'cls_patch' on a tower without registers: class token + patches, all S = 1 + P rows of the selected state."""
    from slime_amd import weights as W
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    dtype = torch.bfloat16
    cfg = DV.dinov2_config(56, 128, 2, 0, 5)
    sd = W.make_dinov2_state_dict(cfg, seed=7)
    DV.write_hf_dir(tmp_path, sd, cfg)
    px = W.synthetic_pixels(2, seed=3, image_size=56)
    hf = DV.hf_states(cfg, sd, px)
    args = lambda f: SimpleNamespace(mm_vision_tower=str(tmp_path), mm_vision_select_layer=-2, mm_vision_select_feature=f,
                                     mm_vision_compute_dtype=dtype)
    both, patch = build_vision_tower(args("cls_patch")), build_vision_tower(args("patch"))
    both.to(dev), patch.to(dev)
    a, b = both(px.to(dev)), patch(px.to(dev))
    assert a.shape == (2, 17, 128) and b.shape == (2, 16, 128) and _biteq(a[:, 1:], b)
    _within(a, hf[-2], dtype, "cls_patch bf16")
    out = both.vision_tower(px.to(dev), output_hidden_states=True)
    assert _biteq(both.feature_select(out), out.hidden_states[-2]) and _biteq(patch.feature_select(out), out.hidden_states[-2][:, 1:])


@pytest.mark.parametrize("merge_type", ["spatial", "spatial_unpad"])
def test_spatial_merge_end_to_end_over_the_tiny_dinov2_tower(dev, tmp_path, merge_type):
    """prepare_inputs_labels_for_multimodal over a DINOv2 tower (24 per side, 4 registers, no sampler) against the materialising
    yardstick of test_gpu_merge_unsampled, built from encode_images' per-image features: bit for bit."""
    import test_gpu_merge_unsampled as MU
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    dtype = torch.bfloat16
    cfg, sd = _tiny_dir(tmp_path, 4, layers=1)
    ecfg = default_slime_config(str(tmp_path), hidden_size=256, mm_hidden_size=128, mm_resampler_type=None, mm_projector_type="mlp2x_gelu",
                                mm_patch_merge_type=merge_type, mm_vision_select_layer=-1)
    enc = SlimeVisualEncoder(ecfg, embed_tokens=MU._embedding(torch.bfloat16))
    enc.get_vision_tower().load_model()
    enc.get_model().mm_projector.load_state_dict(_projector_state(128))
    if hasattr(enc.get_model(), "image_newline"):
        with torch.no_grad():
            enc.get_model().image_newline.copy_(torch.randn(256, generator=torch.Generator().manual_seed(21)) + 2.0 ** -10)
    enc.to(dev)
    enc.get_vision_tower().vision_tower.to(dtype)
    assert enc.get_vision_tower().num_patches_per_side == 24 and enc.get_vision_tower().config.image_size == 336
    splits, sizes, grids = MU.SPLITS[:2], MU.SIZES[:2], MU.GRIDS[:2]
    px = [W.synthetic_pixels(c, seed=60 + i, image_size=336).to(dev).to(dtype) for i, c in enumerate(splits)]
    ids, am, lab, pos = MU._text(dev, n_seq=2, where=((3,), (5,)))
    merged, got = MU._check(enc, dev, px, ids, am, lab, pos, sizes, grids, None, merge_type)
    assert [m.shape[0] for m in merged] == ([2340, 577] if merge_type == "spatial_unpad" else [2880, 576])
