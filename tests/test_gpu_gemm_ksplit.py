"""The opt-in deterministic split-K GEMM on the GPU (slime_gemm_ksplit, slime_vit_forward_ksplit): element-wise conformance against
the float64 reference and the DERIVED bound of tests/gemm_conformance.py (order-free in the accumulation: test_gemm_ksplit_host.py),
and the properties the knob is shipped for -- a result depends on (row of A, B, K, splits) alone: operand forms, row partitions, tiles
and repeated runs give the same bits.

Shapes are the smallest at which the pair of kernels can go wrong: M on both sides of the 64- and 128-row tiles and over more than one
tile (1, 63, 65, 127, 129, 273), N of one and three 128-column tiles, and chunks of one k-tile (K = 128, S = 2), 3 + 2 (320, 2),
2 + 2 + 2 + 3 (576, 4) and 1 + 1 + 1 (192, 3): shorter than, equal to and longer than the ring's depth.  Every case lives in padded,
poisoned buffers (gemm_conformance.Padded), the workspace carries a sentinel tail, and nothing here provokes a fault.

The tile rule of the pair (csrc/gemm_ksplit.inc) takes 64 x 64 tiles while 128 x 128 workgroups x splits x 2 fit the CU count: on a
256-CU device M = 65, N = 128 runs 64-row tiles at any split, M = 4100, N = 128 runs them at splits = 2 (132 <= 256) and 128-row
tiles at splits = 4 (264 > 256).
"""
import ctypes as C
import itertools

import pytest
import torch

import gemm_conformance as GC
from conftest import GOLDEN, rel_l2
from oracle import golden_parts

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}
MS = (1, 63, 65, 127, 129, 273)
NS = (128, 384)
KS = ((128, 2), (320, 2), (576, 4), (192, 3))
TOL = {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}          # test_gpu_path.TOL's values
WS_TAIL = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from slime_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Ws:
    """slime_gemm_ksplit_workspace_bytes bytes at a 256-byte aligned address, WS_TAIL sentinel bytes behind them."""

    def __init__(self, lib, M, N, splits, dev, fill=0x7B):
        self.need = lib.slime_gemm_ksplit_workspace_bytes(M, N, splits)
        self.buf = torch.empty(self.need + 256 + WS_TAIL, dtype=torch.uint8, device=dev)
        self.base = (self.buf.data_ptr() + 255) // 256 * 256
        self.off = self.base - self.buf.data_ptr()
        self.buf.fill_(fill)
        self.buf[self.off + self.need:].fill_(0xA5)

    def garbage(self, byte):
        self.buf[self.off:self.off + self.need].fill_(byte)

    def tail_intact(self):
        return bool((self.buf[self.off + self.need:] == 0xA5).all())


def _pack(lib, c):
    from slime_amd import _lib
    f = GC.Padded(c.N, c.K, c.dtype, c.buf["B"].flat.device, pad_cols=0, guard_rows=0, tail=GC.TAIL)
    if c.guard == "nan":
        f.flat.fill_(float("nan"))
    _lib.check(lib.slime_gemm_pack_b(c.buf["B"].ptr(), c.N, c.K, f.ptr(), _stream()), "slime_gemm_pack_b")
    return f


def _call(lib, c, splits, ws, operand="B", frag=None, **override):
    from slime_amd import _lib
    fields = c.arg_fields(operand, frag.ptr() if frag is not None else None)
    fields.update(override)
    g = _lib.GemmArgs(**fields)
    rc = lib.slime_gemm_ksplit(C.byref(g), splits, ws.base if ws is not None else None, ws.need if ws is not None else 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"slime_gemm_ksplit returned {rc}: {lib.slime_last_error().decode()}"


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _what(c, S):
    return f"{c.form} {c.kind} {DT_ID[c.dtype]} M={c.M} N={c.N} K={c.K} splits={S} guard={c.guard}"


def conformance_cases():
    """Three cases per form (one per kind), the shapes dealt round-robin: every form, kind, M, N and (K, S) appears for each dtype."""
    cases = []
    for i, (form, kind) in enumerate(itertools.product(GC.WAVE_FORMS, GC.KINDS)):
        cases.append((form, kind, MS[i % len(MS)], NS[(i // 2) % len(NS)], KS[(i + i // len(KS)) % len(KS)], ("nan", "attract")[i % 2]))
    return cases


def test_the_pruned_product_covers_every_axis():
    cases = conformance_cases()
    assert {c[0] for c in cases} == set(GC.WAVE_FORMS) and {c[1] for c in cases} == set(GC.KINDS)
    assert {c[2] for c in cases} == set(MS) and {c[3] for c in cases} == set(NS) and {c[4] for c in cases} == set(KS)
    for form in GC.WAVE_FORMS:
        assert {c[1] for c in cases if c[0] == form} == set(GC.KINDS)
    for form in GC.EXACT_FORMS:
        assert any(c[0] == form and c[1] == "integer" for c in cases)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form,kind,M,N,KS_,guard", conformance_cases(),
                         ids=[f"{f}-{k}-M{m}-N{n}-K{ks[0]}-S{ks[1]}" for f, k, m, n, ks, _ in conformance_cases()])
def test_conformance(lib, dev, form, kind, M, N, KS_, guard, dtype):
    """Inside the bound element by element (kind "integer" on EXACT_FORMS: bit-equal, GC.check); the three operand forms bit-equal;
    every byte outside the output windows and behind the workspace untouched."""
    K, S = KS_
    c = GC.make_case(kind, dtype, form, M, N, K, guard=guard, device=dev)
    r = GC.reference(c)
    frag = _pack(lib, c)
    ws = Ws(lib, M, N, S, dev)
    first = None
    for op in ("B+frag", "B", "frag"):
        c.restore()
        _call(lib, c, S, ws, op, frag)
        touched = c.intact()
        assert touched is None, f"{_what(c, S)} [{op}]: a byte of {touched} outside its window was written"
        assert ws.tail_intact(), f"{_what(c, S)} [{op}]: the bytes behind the workspace were written"
        outs = c.windows()
        if first is None:
            first = outs
            ratio, msg = GC.check(c, r, outs, 64)
            print(f"{_what(c, S)}: worst |err| / bound {ratio:.3f}")
            assert msg is None, f"{_what(c, S)} [{op}]: {msg}"
        else:
            for name, t in outs.items():
                assert _bits_equal(t, first[name]), f"{_what(c, S)}: {name} with operand form {op} differs in bits from B+frag"


def _row_ptr(p, r):
    return p.ptr() + r * p.ld * p.flat.element_size()


def _sub_call_fields(c, lo, hi):
    """slime_gemm_args overrides that make the call work on rows [lo, hi) of the case's buffers."""
    b = c.buf
    f = dict(A=_row_ptr(b["A"], lo), C=_row_ptr(b["C"], lo), M=hi - lo)
    if c.form == "resid_split_ln":
        f.update(lo8=_row_ptr(b["lo8"], lo), stats_out=_row_ptr(b["stats_out"], lo))
    if c.fold:
        f.update(ln_stats=_row_ptr(b["ln_stats"], lo))
    return f


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", ["resid_split_ln", "fold_quickgelu_t"])
def test_row_partition_invariance(lib, dev, form, dtype):
    """One call over 273 rows against two calls over rows [0, 100) and [100, 273): C, lo8, stats_out / the fold's output bit-equal."""
    M, N, K, S = 273, 128, 320, 2
    c = GC.make_case("random", dtype, form, M, N, K, device=dev)
    ws = Ws(lib, M, N, S, dev)
    _call(lib, c, S, ws)
    whole = c.windows()
    c.restore()
    for lo, hi in ((0, 100), (100, 273)):
        _call(lib, c, S, ws, **_sub_call_fields(c, lo, hi))
    assert c.intact() is None
    for name, t in c.windows().items():
        assert _bits_equal(t, whole[name]), f"{form} {DT_ID[dtype]}: {name} depends on how the rows are cut into calls"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("form", ["bias_f32", "resid_split_ln"])
def test_tile_invariance_m65_inside_m4100(lib, dev, form, S, dtype):
    """The rows of an M = 65 call against the same rows inside an M = 4100 call (N = 128, K = 320): the two sides of the tile rule
    (module docstring: at splits = 4 the large call runs 128-row tiles on 256 CUs, the small one 64-row tiles)."""
    M, N, K = 4100, 128, 320
    c = GC.make_case("random", dtype, form, M, N, K, device=dev)
    ws = Ws(lib, M, N, S, dev)
    _call(lib, c, S, ws)
    assert c.intact() is None and ws.tail_intact()
    whole = c.windows()
    c.restore()
    for lo in (0, 4000):
        _call(lib, c, S, ws, **_sub_call_fields(c, lo, lo + 65))
        for name, t in c.windows().items():
            assert _bits_equal(t[lo:lo + 65], whole[name][lo:lo + 65]), f"{form} {DT_ID[dtype]} splits={S}: {name} rows {lo}.. depend on M"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_deterministic_whatever_the_workspace_held(lib, dev, dtype):
    M, N, K, S = 273, 384, 576, 4
    for form in ("bias_f32", "resid_split_ln"):
        c = GC.make_case("random", dtype, form, M, N, K, device=dev)
        ws = Ws(lib, M, N, S, dev, fill=0x00)
        _call(lib, c, S, ws)
        first = c.windows()
        c.restore()
        ws.garbage(0xFF)                                  # NaN patterns in every plane
        _call(lib, c, S, ws)
        for name, t in c.windows().items():
            assert _bits_equal(t, first[name]), f"{form}: {name} differs between two runs"
        assert ws.tail_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_one_split_is_the_unsplit_call(lib, dev, dtype):
    from slime_amd import _lib
    for form, M in (("bias_t", 273), ("resid_split_ln", 129), ("fold_quickgelu_t", 65)):
        c = GC.make_case("random", dtype, form, M, 128, 320, device=dev)
        _call(lib, c, 1, None)                            # ws = NULL is accepted
        got = c.windows()
        c.restore()
        g = _lib.GemmArgs(**c.arg_fields("B"))
        assert lib.slime_gemm_ex(C.byref(g), _stream()) == 0
        torch.cuda.synchronize()
        for name, t in c.windows().items():
            assert _bits_equal(t, got[name]), f"{form}: {name}"


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("form", ["bias_t", "bias_f32"])
def test_row_map_scatter(lib, dev, form, dtype):
    M, N, K, S = 129, 128, 320, 2
    c = GC.make_case("random", dtype, form, M, N, K, row_map=True, device=dev)
    r = GC.reference(c)
    ws = Ws(lib, M, N, S, dev)
    _call(lib, c, S, ws)
    assert c.intact() is None and ws.tail_intact()
    ratio, msg = GC.check(c, r, c.windows(), 64)
    assert msg is None, msg


def test_ops_wrappers(dev):
    """ops.gemm_ksplit (row-major and fragment-image operand, splits = 1) and the split form of gemm_resid_split."""
    from slime_amd import _lib, ops
    torch.manual_seed(5)
    M, N, K = 200, 256, 512
    a = torch.randn(M, K, device=dev).bfloat16()
    w = (torch.randn(N, K, device=dev) * K ** -0.5).bfloat16()
    bias = torch.randn(N, device=dev)
    ref = ops.gemm(a, w, bias, _lib.EPI_BIAS_F32)
    got = ops.gemm_ksplit(a, w, bias, _lib.EPI_BIAS_F32, 4)
    exact = a.double() @ w.double().T + bias.double()
    S_ = a.double().abs() @ w.double().abs().T + bias.double().abs()
    assert bool(((got.double() - exact).abs() <= GC.E32 * (K + 4) * S_).all())
    assert torch.equal(ops.gemm_ksplit(a, w, bias, _lib.EPI_BIAS_F32, 1), ref)
    assert torch.equal(ops.gemm_ksplit(a, None, bias, _lib.EPI_BIAS_F32, 4, w_frag=ops.pack_b_frag(w)), got)
    h = torch.randn(M, N, device=dev)
    hi, lo = ops.resid_split(h, torch.bfloat16)
    hi2, lo2 = hi.clone(), lo.clone()
    st = ops.gemm_resid_split(a, w, bias, hi, lo, splits=4)
    st2 = ops.gemm_resid_split(a, w, bias, hi2, lo2)
    assert rel_l2(ops.resid_join(hi, lo), ops.resid_join(hi2, lo2)) < 1e-5 and rel_l2(st, st2) < 1e-5


# ------------------------------------------------------------------------------------------------ the tower
KSPLIT = (2, 2, 2, 4)


@pytest.fixture(scope="module")
def tiny(dev):
    """TINY weights, 3 crops of pixels and the fp32 oracle's features, computed once and left unchanged."""
    from slime_amd import weights as W
    from oracle import slime_oracle as O
    tsd = W.strip_tower_prefix(W.make_tower_state_dict(W.TINY, seed=11))
    px = W.synthetic_pixels(3, seed=22)
    return tsd, px, O.tower_forward(tsd, W.TINY, px)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_tiny_tower_ksplit(dev, tiny, dtype):
    from slime_amd import ops, weights as W
    tsd, px, ref = tiny
    pt = ops.pack_tower(tsd, W.TINY, dtype, dev)
    pxd = px.to(dev)
    out, hidden = ops.tower_forward(pt, pxd, out_dtype=torch.float32, want_hidden=True, k_split=KSPLIT)
    g = golden_parts.load(GOLDEN, "tiny_stages")
    e_ref, e_gold = rel_l2(out.cpu(), ref), rel_l2(out.cpu(), g["n2_tower"])
    print(f"tiny tower k_split={KSPLIT} {DT_ID[dtype]}: rel-L2 {e_ref:.3e} (oracle), {e_gold:.3e} (golden)")
    assert out.shape == (3, 576, 128)
    assert e_ref < TOL[dtype] and e_gold < TOL[dtype]
    assert torch.equal(hidden[:, 1:], out)                                # want_hidden: the same rows, class token included
    with_cls = ops.tower_forward(pt, pxd, out_dtype=torch.float32, keep_cls=True, k_split=KSPLIT)
    assert with_cls.shape == (3, 577, 128) and torch.equal(with_cls, hidden)
    # all-ones is the unsplit pass
    plain = ops.tower_forward(pt, pxd, out_dtype=torch.float32)
    assert torch.equal(ops.tower_forward(pt, pxd, out_dtype=torch.float32, k_split=(1, 1, 1, 1)), plain)
    # partition invariance: 3 crops in one call = 1 + 2 crops in two
    parts = torch.cat([ops.tower_forward(pt, pxd[:1].contiguous(), out_dtype=torch.float32, k_split=KSPLIT),
                       ops.tower_forward(pt, pxd[1:].contiguous(), out_dtype=torch.float32, k_split=KSPLIT)])
    assert torch.equal(parts, out)
    assert torch.equal(ops.tower_forward(pt, pxd, out_dtype=torch.float32, k_split=KSPLIT), out)      # and from run to run


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_encode_forwards_k_split_on_one_and_two_streams(dev, tiny, dtype):
    from slime_amd import ops, weights as W
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    _, px, ref = tiny
    vm = HipCLIPVisionModel(W.TINY)
    vm.load_state_dict(W.make_tower_state_dict(W.TINY, seed=11))
    vm.to(dev).to(dtype)
    pxd = px.to(dev).to(dtype)
    vm.force_streams = 1
    vm.k_split = KSPLIT
    one = vm.encode(pxd, select_layer=-2)
    vm.force_streams = 2
    two = vm.encode(pxd, select_layer=-2)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    want = ops.tower_forward(vm.packed(-2), pxd, k_split=KSPLIT)
    assert torch.equal(one, want)                                         # the knob reached the tower on both branches
    assert rel_l2(one.float().cpu(), ref) < TOL[dtype] * 1.5              # 16-bit output: test_gpu_path's factor for it


@pytest.fixture(scope="module")
def vit_l_two_layers(dev):
    """ViT-L widths (1024 / 4096, 16 heads), two layers run, 2 crops; the fp32 oracle on both crops, computed once."""
    from slime_amd import weights as W
    from oracle import slime_oracle as O
    cfg = W.VisionConfig(num_hidden_layers=3)                             # select_layer -2 of 3 layers: two are run
    tsd = W.strip_tower_prefix(W.make_tower_state_dict(cfg, seed=77))
    px = W.synthetic_pixels(2, seed=5)
    return cfg, tsd, px, O.tower_forward(tsd, cfg, px)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_vit_l_width_tower_ksplit(dev, vit_l_two_layers, dtype):
    from slime_amd import ops
    cfg, tsd, px, ref = vit_l_two_layers
    pt = ops.pack_tower(tsd, cfg, dtype, dev)
    assert pt.layers_run == 2
    pxd = px.to(dev)
    one = ops.tower_forward(pt, pxd[:1].contiguous(), out_dtype=torch.float32, k_split=KSPLIT)
    err = rel_l2(one.cpu(), ref[:1])
    print(f"ViT-L widths, 1 crop, 2 layers, k_split={KSPLIT} {DT_ID[dtype]}: rel-L2 {err:.3e}")
    assert err < TOL[dtype]
    both = ops.tower_forward(pt, pxd, out_dtype=torch.float32, k_split=KSPLIT)
    assert torch.equal(both[:1], one)
    assert rel_l2(both.cpu(), ref) < TOL[dtype]
