"""Element-wise conformance of the front end (slime_patch_embed_prenorm), slime_layernorm, the gate kernels, the row copies, slime_rope
and the router's selection on the GPU, through the C ABI, against the float64 references and the DERIVED bounds of
tests/rowwise_conformance.py (its docstring holds the derivations; the test of the bounds themselves is tests/test_rowwise_bound_cpu.py).

Every case lives in padded buffers (gemm_conformance.Padded): the window 16 bytes into an allocation of its own, guard rows behind it,
NaN around every input, the sentinel byte 0x7B in every output.  After the call every element is inside its bound -- bit-equal where
the operation is a copy, a cast or a stated identity -- and every byte outside every output window is what it was.  All guards are
inside the test's own allocations; nothing here provokes a fault.

What is walked.  Front end: the eight geometries of rowwise_conformance.GEOMETRIES (the shipped 336 / 14; CLIP-L/14-224 with its third
row tile masked; D = 256 with a tile cut at row 24; two tiles masked; 8 valid rows; odd g with kpad == 3 patch^2, KS = 6; the largest
accepted LDS) x both dtypes x random / offset / constant inputs x fp32 and T pixels, all four outputs, batch invariance, the refusals.
The whole tower at 112 / 14, 112 / 16 and 224 / 14 against the oracle at the project's tower tolerance.  slime_layernorm over D x rows x
ldx x output subsets x add_period x input kinds, normalize = 0, refusals.  The three gate kernels over D x H x rows x logit kinds, the
grouped scatter, in place and out of place, and the bit-equality of the gates between the three kernels.  The copies with sentinels.
slime_rope over head counts, strides, rows and positions up to 131071.  The router's selection at T on both sides of 1024 / 2048 / 3072
with tied probabilities.

Worst |err| / bound observed on an MI355X (the module prints this table at the end of a run and writes it to the file
SLIME_ROWWISE_CONFORMANCE_REPORT names).  These are measurements against the float64 reference, not targets.
    operation, output                    bf16     fp16
    front end h, patch rows              0.005    0.006
    front end h, class-token rows        0.130    0.130
    front end stats                      0.151    0.232
    layernorm out_f32                    0.318    0.318
    layernorm out_t                      0.995    0.996
    layernorm out_t2                     0.996    0.996
    gate_premix                          0.996    0.996
    rope                                 0.995    0.994
    gate_weights (fp32) 0.205; gate_mix into f32 / bf16 / f16 0.262 / 0.996 / 0.996.
Where the output is T the figure is the sharpness of the final RNE term (nothing comes on top of it); the fp32 outputs show the
accumulation terms alone -- the front end's is a worst case linear in 3 patch^2, as the GEMM's is in K.  x16, lo8, the casts of
normalize = 0, the copies, RoPE at pos = 0, the gates between the three gate kernels and the router's kept sets are exact.  All 60
tests passed on the kernels as they were: the geometries, the D = 256 instantiation, the odd-g and masked-tile paths and
slime_select_crops, none of which had run before, needed no kernel change.
"""
import json
import math
import os

import pytest
import torch

import gemm_conformance as GC
import rowwise_conformance as RC
from rowwise_conformance import Padded

pytestmark = pytest.mark.gpu

DTYPES = list(RC.DTYPES)
DT_ID = RC.DT_ID
NAN = math.nan


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    """worst |err| / bound per (operation, output, dtype), printed when the module is done (and written to the file
    SLIME_ROWWISE_CONFORMANCE_REPORT names, if set)."""
    table = {}
    yield table
    lines = [f"    {k:56s} {v:.3f}" for k, v in sorted(table.items())]
    print("\nrow-kernel conformance, worst |err| / bound per operation, output and dtype:\n" + "\n".join(lines))
    path = os.environ.get("SLIME_ROWWISE_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _note(ratios, key, value):
    ratios[key] = max(ratios.get(key, 0.0), float(value))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _code(dt):
    from slime_amd import ops
    return ops.dtype_code(dt)


def _guarded(t, rows=1):
    """A copy of an input tensor in a buffer of its own, NaN in front of it and behind it."""
    t = t.contiguous()
    return Padded(rows, t.numel() // rows, t.dtype, t.device, pad_cols=0, guard_rows=0, tail=GC.TAIL).fill(t.view(rows, -1), NAN)


def _unchanged(p, snap, what):
    assert torch.equal(p.flat.view(torch.uint8), snap.view(torch.uint8)), f"{what} was written"


# ================================================================================================ front end
class _FrontEnd:
    """One packed embeddings-only tower with every operand of the call copied into a guarded buffer."""

    def __init__(self, sd, geom, dtype, dev):
        from slime_amd import ops
        self.geom, self.dtype, self.dev = geom, dtype, dev
        self.cfg = geom.config()
        self.pt = ops.pack_tower(sd, self.cfg, dtype, dev, select_layer=0)
        assert self.pt.desc.kpad == geom.kpad and self.cfg.head_dim == 64
        T = self.pt.tensors
        self.ops = {k: _guarded(T[k]) for k in ("patch_w_frag", "cls", "pos", "pre_ln_w", "pre_ln_b")}

    def outputs(self, n):
        g, rows = self.geom, n * self.geom.S
        return {"h": Padded(rows, g.D, torch.float32, self.dev, pad_cols=0), "x16": Padded(rows, g.D, self.dtype, self.dev, pad_cols=0),
                "lo8": Padded(rows, g.D, torch.int8, self.dev, pad_cols=0), "stats": Padded(rows, 2 * (g.D // 64), torch.float32, self.dev, pad_cols=0)}

    def call(self, px, out, **override):
        """px [n, 3, image, image] fp32 or T, copied into a guarded buffer; out: name -> Padded (or None).  -> return code"""
        from slime_amd import _lib
        lib, g, o = _lib.load(), self.geom, self.ops
        n = px.shape[0]
        pb = Padded(n * 3 * g.image, g.image, px.dtype, self.dev, pad_cols=0).fill(px.reshape(-1, g.image), NAN)
        a = dict(image=g.image, patch=g.patch, kpad=g.kpad, D=g.D)
        a.update(override)
        ptr = lambda k: out[k].ptr() if out.get(k) is not None else None
        rc = lib.slime_patch_embed_prenorm(pb.ptr(), _code(px.dtype), o["patch_w_frag"].ptr(), o["cls"].ptr(), o["pos"].ptr(), o["pre_ln_w"].ptr(),
                                           o["pre_ln_b"].ptr(), self.cfg.layer_norm_eps, ptr("h"), ptr("x16"), ptr("lo8"), ptr("stats"),
                                           _code(self.dtype), n, a["image"], a["patch"], a["kpad"], a["D"], _stream())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("geom", list(RC.GEOMETRIES), ids=[g.name.replace("/", "_") for g in RC.GEOMETRIES])
def test_front_end(dev, ratios, geom, dtype):
    """One geometry x one dtype: random / offset / constant inputs, fp32 pixels against the bound (h, class rows apart, stats) with
    x16 = T(h) and lo8 = ops.resid_split(h)[1] bit for bit; T pixels and the last crop alone reproduce the bits."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    assert RC.fe_lds_bytes(geom.image, geom.patch, geom.kpad, geom.D) == RC.GEOMETRIES[geom] <= RC.LDS_LIMIT
    n = 1 if geom.image == 384 else 3
    S = geom.S
    for i, kind in enumerate(RC.FE_KINDS):
        sd, px = RC.fe_inputs(geom, kind, n, seed=100 + i)
        fe = _FrontEnd(sd, geom, dtype, dev)
        px = px.to(dev)
        ref = RC.fe_reference(sd, geom, px, dtype, fe.cfg.layer_norm_eps)
        if kind == "offset":
            assert RC.fe_mu_over_sigma(ref) >= 10.0
        what = f"front end {geom.name} {DT_ID[dtype]} {kind}"
        out = fe.outputs(n)
        snaps = {k: p.snapshot() for k, p in out.items()}
        rc = fe.call(px, out)
        assert rc == 0, f"{what}: {lib.slime_last_error().decode()}"
        for k, p in out.items():
            assert p.intact(snaps[k]), f"{what}: a byte of {k} outside its window was written"
        got = {k: p.win.clone() for k, p in out.items()}
        got["stats"] = got["stats"].view(n * S, geom.D // 64, 2)
        r, msg = RC.fe_check(ref, got, dtype)
        assert msg is None, f"{what}: {msg}"
        assert torch.equal(got["lo8"], ops.resid_split(got["h"], dtype)[1]), f"{what}: lo8 is not ops.resid_split(h)[1]"
        for k, v in r.items():
            _note(ratios, f"front end {k} {DT_ID[dtype]}", v)
        # T pixels: the same bits
        out2 = fe.outputs(n)
        assert fe.call(px.to(dtype), out2) == 0, f"{what}: {lib.slime_last_error().decode()}"
        for k in out:
            assert RC.bits_equal(out2[k].win, out[k].win), f"{what}: {k} from T pixels differs from fp32 pixels at {RC.first_diff(out2[k].win, out[k].win)}"
            assert out2[k].intact(snaps[k]), f"{what} (T pixels): a byte of {k} outside its window was written"
        # the last crop alone: its rows bit for bit, whatever the batch
        out3 = fe.outputs(1)
        snap3 = {k: p.snapshot() for k, p in out3.items()}
        assert fe.call(px[n - 1:], out3) == 0, f"{what}: {lib.slime_last_error().decode()}"
        for k in out:
            assert RC.bits_equal(out3[k].win, out[k].win[(n - 1) * S:]), f"{what}: {k} of the last crop alone differs at {RC.first_diff(out3[k].win, out[k].win[(n - 1) * S:])}"
            assert out3[k].intact(snap3[k])


def test_front_end_output_subsets(dev):
    """h alone and x16 + stats alone (what the tower driver asks for) are the bits of the full call."""
    geom, dtype = RC.Geom(112, 16, 256), torch.bfloat16
    sd, px = RC.fe_inputs(geom, "random", 2, seed=7)
    fe = _FrontEnd(sd, geom, dtype, dev)
    full = fe.outputs(2)
    assert fe.call(px.to(dev), full) == 0
    for names in (("h",), ("x16", "stats"), ("x16", "lo8", "stats")):
        out = fe.outputs(2)
        snaps = {k: p.snapshot() for k, p in out.items()}
        assert fe.call(px.to(dev), {k: out[k] for k in names}) == 0
        for k, p in out.items():
            if k in names:
                assert RC.bits_equal(p.win, full[k].win) and p.intact(snaps[k]), (names, k)
            else:
                _unchanged(p, snaps[k], f"{k} (not requested)")


def test_front_end_refusals(dev):
    """A geometry the front end cannot run is refused when the tower is PACKED, with the limit named; the entry point refuses a bad
    kpad and an unsupported width, and nothing is launched."""
    from slime_amd import _lib, ops, weights as W
    lib = _lib.load()
    for image, patch, needle in ((392, 14, "patches per side"), (84, 14, "multiple of the patch")):
        cfg = W.VisionConfig(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=image, patch_size=patch)
        with pytest.raises(_lib.SlimeHipError, match=needle):
            ops.pack_tower(W.make_tower_state_dict(cfg, seed=3), cfg, torch.bfloat16, dev, select_layer=0)
    geom = RC.Geom(56, 14, 128)
    sd, px = RC.fe_inputs(geom, "random", 1, seed=3)
    fe = _FrontEnd(sd, geom, torch.bfloat16, dev)
    for override, needle in ((dict(kpad=600), "kpad"), (dict(kpad=576), "kpad"), (dict(D=512), "D=512 unsupported"), (dict(image=392), "patches per side"),
                             (dict(image=60, patch=15), "multiple of the patch")):
        out = fe.outputs(1)
        snaps = {k: p.snapshot() for k, p in out.items()}
        rc = fe.call(px.to(dev), out, **override)
        assert rc == -1, (override, rc)
        assert needle in lib.slime_last_error().decode(), (override, lib.slime_last_error().decode())
        for k, p in out.items():
            _unchanged(p, snaps[k], f"{override}: {k}")


# ================================================================================================ the whole tower at other geometries
TOWER_CASES = [RC.Geom(112, 14, 128), RC.Geom(112, 16, 128), RC.Geom(224, 14, 128), RC.Geom(112, 16, 256)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("geom", TOWER_CASES, ids=[g.name.replace("/", "_") for g in TOWER_CASES])
def test_tower_at_other_geometries(dev, geom, dtype):
    """ops.tower_forward against the oracle at S = 65, 50 and 257 (TINY's depth), held to the project's tower tolerance."""
    from slime_amd import ops, weights as W
    from oracle import slime_oracle as O
    from test_gpu_path import TOL
    cfg = geom.config(layers=W.TINY.num_hidden_layers)
    assert cfg.seq_len == geom.S and cfg.head_dim == 64
    tsd = W.strip_tower_prefix(W.make_tower_state_dict(cfg, seed=11))
    px = W.synthetic_pixels(3, seed=22, image_size=geom.image)
    pt = ops.pack_tower(tsd, cfg, dtype, dev)
    out = ops.tower_forward(pt, px.to(dev), out_dtype=torch.float32)
    ref = O.tower_forward(tsd, cfg, px)
    assert out.shape == (3, geom.P, geom.D)
    err = GC.rel_l2(out.cpu(), ref)
    print(f"\ntower {geom.name} {DT_ID[dtype]}: rel-L2 {err:.3e} (tolerance {TOL[dtype]:.1e})")
    assert err < TOL[dtype], (geom.name, err)
    alone = ops.tower_forward(pt, px[2:].to(dev), out_dtype=torch.float32)
    assert torch.equal(alone[0], out[2]), "a crop's features depend on the batch"


# ================================================================================================ slime_layernorm
def _ln_call(lib, c, **override):
    b = c.buf
    ptr = lambda k: b[k].ptr() if k in b else None
    a = dict(ldx=c.ldx, D=c.D, add=ptr("add"), add_period=c.add_period if c.has_add else 0)
    a.update(override)
    rc = lib.slime_layernorm(b["x"].ptr(), a["ldx"], c.rows, a["D"], b["w"].ptr(), b["b"].ptr(), c.eps, int(c.normalize), ptr("out_f32"), ptr("out_t"),
                             ptr("out_t2"), a["add"], a["add_period"], _code(c.dtype), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("D", [128, 256, 1024])
def test_layernorm(dev, ratios, D, dtype):
    """rows on both sides of the four-row workgroup x ldx x input kinds x output subsets x add periods (1, 2 -- which divides neither 5
    nor 9 -- and rows; one period where out_t2 is not asked for), then normalize = 0 with and without add."""
    from slime_amd import _lib
    lib = _lib.load()
    n = 0
    for rows in (1, 3, 4, 5, 9):
        for ldx in (D, D + 4, D + 64):
            for kind in RC.LN_KINDS:
                for subset in RC.LN_SUBSETS:
                    for period in sorted({1, 2, rows}) if "out_t2" in subset else (1,):
                        n += 1
                        c = RC.make_ln_case(D, dtype, rows, ldx, kind, subset, add_period=period, seed=n, device=dev)
                        ref = RC.ln_reference(c)
                        assert _ln_call(lib, c) == 0, f"{c.what()}: {lib.slime_last_error().decode()}"
                        assert c.intact() is None, f"{c.what()}: a byte of {c.intact()} outside its window was written"
                        r, msg = RC.ln_check(c, ref, c.windows())
                        assert msg is None, f"{c.what()}: {msg}"
                        for k, v in r.items():
                            _note(ratios, f"layernorm {k} {DT_ID[dtype]}", v)
    for rows in (1, 5):
        for with_add in (False, True):
            outs = ("out_f32", "out_t") + (("out_t2",) if with_add else ())
            c = RC.make_ln_case(D, dtype, rows, D + 4, "random", outs, add_period=2, normalize=False, seed=rows, device=dev)
            assert _ln_call(lib, c) == 0, f"{c.what()}: {lib.slime_last_error().decode()}"
            assert c.intact() is None
            r, msg = RC.ln_check(c, RC.ln_reference(c), c.windows())
            assert msg is None, f"{c.what()}: {msg}"


def test_layernorm_refusals(dev):
    from slime_amd import _lib
    lib = _lib.load()
    c = RC.make_ln_case(128, torch.bfloat16, 5, 132, device=dev)
    for override, needle in ((dict(ldx=124), "bad input"), (dict(ldx=130), "multiple of 4"), (dict(D=512, ldx=512), "D=512 unsupported"),
                             (dict(add=None), "out_t2 needs add")):
        assert _ln_call(lib, c, **override) == -1, override
        assert needle in lib.slime_last_error().decode(), (override, lib.slime_last_error().decode())
        for k in c.outputs:
            _unchanged(c.buf[k], c.snaps[k], f"{override}: {k}")


# ================================================================================================ gates
def _gate_bufs(x, wg):
    return Padded(x.shape[0], x.shape[1], torch.float32, x.device, pad_cols=0).fill(x, NAN), Padded(wg.shape[0], 2, torch.float32, x.device, pad_cols=0).fill(wg, NAN)


def _gate_weights(lib, xb, wb, rows, D):
    out = Padded(rows, 2, torch.float32, xb.flat.device, pad_cols=0)
    snap = out.snapshot()
    rc = lib.slime_gate_weights(xb.ptr(), D, wb.ptr(), out.ptr(), rows, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert out.intact(snap), "gate_weights: a byte outside the window was written"
    return out.win.clone()


def _gate_mix(lib, xb, wb, e0, e1, rows, D, H, odt, scatter):
    """-> (rows of the output the call addresses [rows, H], the Padded output); asserts that every other byte kept the sentinel."""
    dev = xb.flat.device
    if scatter:
        rmap, total = RC.scatter_rows(rows)
        rpg, stride, row0 = RC.SCATTER
    else:
        rmap, total, rpg, stride, row0 = torch.arange(rows), rows, rows, 0, 0
    out = Padded(total, H, odt, dev, pad_cols=0)
    snap = out.snapshot()
    rc = lib.slime_gate_mix_ex(xb.ptr(), D, wb.ptr(), e0.ptr(), e1.ptr(), out.ptr(), _code(odt), rows, H, rpg, stride, row0, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    got = out.win[rmap.to(dev)].clone()
    out.win[rmap.to(dev)] = out.window_of(snap)[rmap.to(dev)]                   # put the addressed rows back: everything must be the snapshot again
    _unchanged(out, snap, "gate_mix: a row or byte the call does not address")
    return got


def _gate_premix(lib, xb, wb, a0, a1, rows, D, H, dtype, in_place):
    dev = xb.flat.device
    out = a1 if in_place else Padded(rows, H, dtype, dev, pad_cols=0)
    snap, before = out.snapshot(), a1.win.clone()
    rc = lib.slime_gate_premix(xb.ptr(), D, wb.ptr(), a0.ptr(), a1.ptr(), out.ptr(), _code(dtype), rows, H, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert out.intact(snap), "gate_premix: a byte outside the window was written"
    got = out.win.clone()
    if in_place:
        a1.win.copy_(before)
    return got


@pytest.mark.parametrize("kind", RC.GATE_KINDS)
def test_gates(dev, ratios, kind):
    """slime_gate_weights, slime_gate_mix_ex (into f32 / bf16 / f16, plain and scattered into a token buffer) and slime_gate_premix
    (both dtypes, in place over a1 and apart) against the bound; the gates of the three kernels are the same bits."""
    from slime_amd import _lib
    lib = _lib.load()
    n = 0
    for D in (64, 72, 128, 1024):
        for rows in (1, 5, 9):
            n += 1
            x, wg = RC.gate_inputs(D, rows, kind, n, dev)
            gts, dg, delta = RC.gate_reference(x, wg)
            if kind == "saturated":
                assert float(delta.min()) > 200.0
            xb, wb = _gate_bufs(x, wg)
            what = f"gates {kind} D={D} rows={rows}"
            gw = _gate_weights(lib, xb, wb, rows, D)
            r, msg = RC.check("gate_weights", gw, gts, dg)
            assert msg is None, f"{what}: {msg}"
            _note(ratios, "gate_weights f32", r)
            g = torch.Generator(device=dev).manual_seed(n)
            # instruction for instruction: the gates the mix applies (e0 = 1, e1 = 0, H = 4, and the other way round) are gate_weights' bits
            one, zero = Padded(rows, 4, torch.float32, dev, pad_cols=0).fill(torch.ones(rows, 4, device=dev), NAN), Padded(rows, 4, torch.float32, dev, pad_cols=0).fill(torch.zeros(rows, 4, device=dev), NAN)
            assert RC.bits_equal(_gate_mix(lib, xb, wb, one, zero, rows, D, 4, torch.float32, False), gw[:, :1].expand(rows, 4).contiguous()), f"{what}: g0 of the mix"
            assert RC.bits_equal(_gate_mix(lib, xb, wb, zero, one, rows, D, 4, torch.float32, True), gw[:, 1:].expand(rows, 4).contiguous()), f"{what}: g1 of the mix"
            for dt in DTYPES:                                           # ... and the premix's, read back through T(1) and T(0)
                o8, z8 = Padded(rows, 8, dt, dev, pad_cols=0).fill(torch.ones(rows, 8, device=dev), NAN), Padded(rows, 8, dt, dev, pad_cols=0).fill(torch.zeros(rows, 8, device=dev), NAN)
                assert RC.bits_equal(_gate_premix(lib, xb, wb, o8, z8, rows, D, 8, dt, False), gw[:, :1].to(dt).expand(rows, 8).contiguous()), f"{what}: g0 of the premix"
                assert RC.bits_equal(_gate_premix(lib, xb, wb, z8, o8, rows, D, 8, dt, True), gw[:, 1:].to(dt).expand(rows, 8).contiguous()), f"{what}: g1 of the premix"
            for j, H in enumerate((4, 260, 4096)):
                e0, e1 = torch.randn(rows, H, generator=g, device=dev), torch.randn(rows, H, generator=g, device=dev)
                b0, b1 = Padded(rows, H, torch.float32, dev, pad_cols=0).fill(e0, NAN), Padded(rows, H, torch.float32, dev, pad_cols=0).fill(e1, NAN)
                for odt in (torch.float32, torch.bfloat16, torch.float16):
                    for scatter in (False, True):
                        got = _gate_mix(lib, xb, wb, b0, b1, rows, D, H, odt, scatter)
                        y, dy = RC.mix_reference(gts, dg, e0, e1, odt)
                        r, msg = RC.check("gate_mix", got, y, dy)
                        assert msg is None, f"{what} H={H} out={DT_ID[odt]} scatter={scatter}: {msg}"
                        _note(ratios, f"gate_mix {DT_ID[odt]}", r)
            for H in (8, 264, 520, 4096):
                for dt in DTYPES:
                    a0, a1 = torch.randn(rows, H, generator=g, device=dev).to(dt), torch.randn(rows, H, generator=g, device=dev).to(dt)
                    p0, p1 = Padded(rows, H, dt, dev, pad_cols=0).fill(a0, NAN), Padded(rows, H, dt, dev, pad_cols=0).fill(a1, NAN)
                    y, dy = RC.mix_reference(gts, dg, a0, a1, dt)
                    first = None
                    for in_place in (False, True):
                        got = _gate_premix(lib, xb, wb, p0, p1, rows, D, H, dt, in_place)
                        r, msg = RC.check("gate_premix", got, y, dy)
                        assert msg is None, f"{what} H={H} {DT_ID[dt]} in_place={in_place}: {msg}"
                        _note(ratios, f"gate_premix {DT_ID[dt]}", r)
                        assert first is None or RC.bits_equal(first, got), f"{what}: in place differs from out of place"
                        first = got


# ================================================================================================ copies (bit-equal, with sentinels)
OUT_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _filled(rows, C, dtype, dev, seed, guard=NAN):
    g = torch.Generator(device=dev).manual_seed(seed)
    return Padded(rows, C, dtype, dev, pad_cols=0).fill(3.0 * torch.randn(rows, C, generator=g, device=dev), guard)


@pytest.mark.parametrize("C", [4, 132, 1024])
def test_gather_rows(dev, C):
    from slime_amd import _lib
    lib = _lib.load()
    rows_in, rows_out = 7, 4
    for groups in (1, 3):
        src = _filled(groups * rows_in, C, torch.float32, dev, C + groups)
        for odt in OUT_DTYPES:
            for off in (0, rows_in - rows_out):
                out = Padded(groups * rows_out, C, odt, dev, pad_cols=0)
                snap = out.snapshot()
                rc = lib.slime_gather_rows(src.ptr(), rows_in, off, out.ptr(), _code(odt), groups, rows_out, C, _stream())
                torch.cuda.synchronize()
                assert rc == 0, lib.slime_last_error().decode()
                want = src.win.view(groups, rows_in, C)[:, off:off + rows_out].reshape(-1, C).to(odt)
                assert RC.bits_equal(out.win, want) and out.intact(snap), (C, groups, odt, off)


@pytest.mark.parametrize("C", [8, 520])
def test_gather_rows_split(dev, C):
    from slime_amd import _lib, ops
    lib = _lib.load()
    rows_in, rows_out, groups = 6, 4, 2
    for dt in DTYPES:
        h = 3.0 * torch.randn(groups * rows_in, C, generator=torch.Generator(device=dev).manual_seed(C), device=dev)
        hi, lo = ops.resid_split(h, dt)
        hb, lb = Padded(groups * rows_in, C, dt, dev, pad_cols=0).fill(hi, NAN), Padded(groups * rows_in, C, torch.int8, dev, pad_cols=0).fill(lo, 0x55)
        want = ops.resid_join(hi, lo).view(groups, rows_in, C)
        for odt in OUT_DTYPES:
            for off in (0, rows_in - rows_out):
                out = Padded(groups * rows_out, C, odt, dev, pad_cols=0)
                snap = out.snapshot()
                rc = lib.slime_gather_rows_split(hb.ptr(), lb.ptr(), _code(dt), rows_in, off, out.ptr(), _code(odt), groups, rows_out, C, _stream())
                torch.cuda.synchronize()
                assert rc == 0, lib.slime_last_error().decode()
                assert RC.bits_equal(out.win, want[:, off:off + rows_out].reshape(-1, C).to(odt)) and out.intact(snap), (C, dt, odt, off)


@pytest.mark.parametrize("grid", [(1, 1), (1, 3), (3, 1), (2, 3)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_merge_rows_batched(dev, grid):
    """images = 3 with image strides larger than the payload on both sides: the rows between the images keep the sentinel."""
    from slime_amd import _lib
    lib = _lib.load()
    nw, nh = grid
    g, C, images, row0 = 3, 8, 3, 2
    payload = nw * nh * g * g
    in_stride, out_stride = payload + 3, payload + row0 + 4
    src = _filled(images * in_stride, C, torch.float32, dev, nw * 10 + nh)
    for merge in (0, 1):
        dst = RC.merge_dst(nw, nh, g, bool(merge)).to(dev)
        for odt in OUT_DTYPES:
            out = Padded(images * out_stride, C, odt, dev, pad_cols=0)
            snap = out.snapshot()
            rc = lib.slime_merge_rows_batched(src.ptr(), in_stride, out.ptr(), _code(odt), out_stride, row0, images, nw, nh, g, C, merge, _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.slime_last_error().decode()
            want = out.window_of(snap).clone()
            for b in range(images):
                want[b * out_stride + row0 + dst] = src.win[b * in_stride:b * in_stride + payload].to(odt)
            assert RC.bits_equal(out.win, want), (grid, merge, odt, RC.first_diff(out.win, want))
            assert out.intact(snap)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("C", [8, 520])
def test_select_crops(dev, C, dtype):
    """slime_select_crops (no caller in the package: this is its only test): period 5, the window at both ends, one and four crops per
    image, either output alone and both."""
    from slime_amd import _lib
    lib = _lib.load()
    period, images, P = 5, 2, 5
    feats = _filled(images * period * P, C, dtype, dev, C)
    for first, per_image in ((0, 1), (1, 4), (0, 4), (1, 1)):
        idx = RC.select_crops_index(period, first, per_image, images).to(dev)
        want = feats.win.view(images * period, P, C)[idx].reshape(-1, C)
        rows = images * per_image * P
        for want_f32, want_t in ((True, False), (False, True), (True, True)):
            o32, ot = Padded(rows, C, torch.float32, dev, pad_cols=0), Padded(rows, C, dtype, dev, pad_cols=0)
            s32, st = o32.snapshot(), ot.snapshot()
            rc = lib.slime_select_crops(feats.ptr(), _code(dtype), P, C, period, first, per_image, images, o32.ptr() if want_f32 else None,
                                        ot.ptr() if want_t else None, _stream())
            torch.cuda.synchronize()
            assert rc == 0, lib.slime_last_error().decode()
            for on, p, snap, exp in ((want_f32, o32, s32, want.float()), (want_t, ot, st, want)):
                if on:
                    assert RC.bits_equal(p.win, exp) and p.intact(snap), (C, first, per_image, want_f32, want_t)
                else:
                    _unchanged(p, snap, "an output that was not requested")
    o32 = Padded(P, C, torch.float32, dev, pad_cols=0)
    snap = o32.snapshot()
    for args, needle in (((_code(dtype), P, C, period, 2, 4, images), "window outside"), ((_code(dtype), P, 12, period, 0, 1, images), "bad input"),
                         ((_code(torch.float32), P, C, period, 0, 1, images), "BF16 or F16")):
        assert lib.slime_select_crops(feats.ptr(), *args, o32.ptr(), None, _stream()) == -1, args
        assert needle in lib.slime_last_error().decode(), (args, lib.slime_last_error().decode())
    torch.cuda.synchronize()
    _unchanged(o32, snap, "a refused call's output")


# ================================================================================================ RoPE
def _rope_run(lib, c):
    b = c.buf
    psnap = b["pos"].snapshot()
    rc = lib.slime_rope(b["qkv"].ptr(), c.row_stride, b["pos"].ptr(), c.rows, c.n_rot, c.n_q, 128, b["inv_freq"].ptr(), c.q_scale, _code(c.dtype), _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{c.what()}: {lib.slime_last_error().decode()}"
    assert b["qkv"].intact(c.snap), f"{c.what()}: a byte outside the qkv window was written"
    _unchanged(b["pos"], psnap, "pos")
    win = b["qkv"].win
    assert RC.bits_equal(win[:, c.n_rot * 128:], c.before[:, c.n_rot * 128:]), f"{c.what()}: v / the padding of a row was written"
    return RC.rope_check(c, win[:, :c.n_rot * 128].reshape(c.rows, c.n_rot, 128).clone())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rope(dev, ratios, dtype):
    """n_rot x n_q x row_stride (the heads alone, and 136 elements of v / padding behind them) x rows 1 / 5 x positions up to 131071,
    theta = 5e5: every element inside the bound of the DEFINED fp32 angle; pos = 0 exact; v and the padding untouched."""
    from slime_amd import _lib
    lib = _lib.load()
    n = 0
    for n_rot in (1, 3, 10):
        for n_q in sorted({0, 1, n_rot}):
            for extra in (0, 136):
                n += 1
                cases = [RC.make_rope_case(dtype, n_rot, n_q, 5, extra, [0, 1, 4095, 4096, 131071], seed=n, device=dev),
                         RC.make_rope_case(dtype, n_rot, n_q, 5, extra, [8191, 4096, 1, 0, 131071], seed=n + 100, device=dev)]
                cases += [RC.make_rope_case(dtype, n_rot, n_q, 1, extra, [p], seed=n + p, device=dev) for p in RC.ROPE_POS]
                for c in cases:
                    ratio, msg = _rope_run(lib, c)
                    assert msg is None, f"{c.what()}: {msg}"
                    _note(ratios, f"rope {DT_ID[dtype]}", ratio)


# ================================================================================================ router selection (exact)
@pytest.mark.parametrize("T", RC.ROUTER_T)
def test_router_selection(dev, T):
    """The kept set and count equal torch's STABLE descending sort of the device's own probabilities -- all probabilities tied (the
    lowest indices are kept), ties in blocks of 7, separated scores -- on both sides of every change of the compaction's positions per
    thread; the batched entry on the same scores equals the single calls bit for bit."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    scores = torch.stack([RC.router_scores(T, kind) for kind in RC.ROUTER_KINDS]).to(dev)
    B = scores.shape[0]
    cnt_in = torch.full((B,), T, dtype=torch.int32, device=dev)
    for topp in RC.ROUTER_TOPP:
        singles = []
        for b, kind in enumerate(RC.ROUTER_KINDS):
            keep, cnt, probs = ops.router_select(scores[b].contiguous(), topp, 1.0, want_probs=True)
            n = int(cnt.item())
            exp = RC.router_expected(probs.cpu(), topp)
            assert n == exp.numel(), (T, kind, topp, n, exp.numel())
            assert torch.equal(keep[:n].cpu().long(), exp), (T, kind, topp)
            if kind == "tied":
                assert torch.equal(exp, torch.arange(n)), "tied probabilities: the lowest indices are kept"
            singles.append((keep, n))
        keep_b = torch.full((B, T), -1, dtype=torch.int32, device=dev)
        cnt_b = torch.full((B,), -1, dtype=torch.int32, device=dev)
        _lib.check(lib.slime_router_select_batched(scores.data_ptr(), cnt_in.data_ptr(), B, T, 1.0, float(topp), keep_b.data_ptr(), cnt_b.data_ptr(),
                                                   _stream()), "slime_router_select_batched")
        torch.cuda.synchronize()
        for b, (keep, n) in enumerate(singles):
            assert int(cnt_b[b]) == n and torch.equal(keep_b[b, :n], keep[:n]), (T, RC.ROUTER_KINDS[b], topp)
