"""Adapter conformance on the GPU: every fused adapter entry equals, BIT FOR BIT, a replay of its launch sequence through the public
element-wise bounded kernel entries (tests/adapter_conformance.py).

The replay makes the same calls -- M, N, K, epilogue, operand form and weight pointers of every GEMM -- with intermediates in
tensors of the test's own and every index (which crop, which segment, which token-buffer row, which rows stay untouched) computed
in integer Python.  Shapes are the smallest at which each branch exists (adapter_conformance.LAYOUTS).  Inputs sit in buffers with
NaN around them, outputs and the exactly sized workspace in buffers with a sentinel byte around them.  The only rel-L2 of the module
is test_small_grid_vs_oracle, at the project's existing tolerance: bit-equality to a replay says nothing if both misread the
reference at small grids.

Measured on an MI355X (printed at the end of a run and written to the file SLIME_ADAPTER_CONFORMANCE_REPORT names): see DESIGN.md
section 2 for the count of bit-equal (entry, layout, branch) combinations and the small-grid rel-L2 figures.
"""
import ctypes as C
import json
import os

import pytest
import torch

import adapter_conformance as AC
from adapter_conformance import GuardedWorkspace, HipBackend, LAYOUTS, guarded_input, guarded_output, sentinel_rows

pytestmark = pytest.mark.gpu

DT_ID = AC.DT_ID
OTHER = {torch.bfloat16: torch.float16, torch.float16: torch.bfloat16}
EINVAL, EWORKSPACE = -1, -2
CASES = [(n, dt) for n in sorted(LAYOUTS) for dt in LAYOUTS[n].dtypes]
CASE_IDS = [f"{n}-{DT_ID[dt]}" for n, dt in CASES]


def _cases(names):
    sel = [(n, dt) for n, dt in CASES if n in names]
    return pytest.mark.parametrize("name,dtype", sel, ids=[f"{n}-{DT_ID[dt]}" for n, dt in sel])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tally():
    """(entry, layout, dtype, branch) -> number of bit-equal comparisons; printed when the module is done (and written to the file
    SLIME_ADAPTER_CONFORMANCE_REPORT names, if set) together with the small-grid rel-L2 measurements."""
    table = {"bit_equal": {}, "small_grid_rel_l2": {}}
    yield table
    n = sum(table["bit_equal"].values())
    print(f"\nadapter conformance: {n} fused calls bit-equal to the replay in {len(table['bit_equal'])} (entry, layout, dtype, branch) combinations")
    for k, v in sorted(table["small_grid_rel_l2"].items()):
        print(f"    small grid vs oracle {k:24s} {v:.3e}")
    path = os.environ.get("SLIME_ADAPTER_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


_tinies = {}


def _tiny(name, dtype, dev):
    if (name, dtype) not in _tinies:
        _tinies[(name, dtype)] = AC.make_tiny(LAYOUTS[name], dtype, dev)
    return _tinies[(name, dtype)]


def _lib():
    from slime_amd import _lib as L
    return L.load()


def _code(dt):
    from slime_amd import ops
    return ops.dtype_code(dt)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err():
    return _lib().slime_last_error().decode()


def _biteq(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


def _note(tally, entry, name, dtype, branch):
    k = f"{entry} {name} {DT_ID[dtype]} {branch}"
    tally["bit_equal"][k] = tally["bit_equal"].get(k, 0) + 1


def _ptr(p):
    return None if p is None else p.ptr()


def _feats(L, dtype, dev, n_crops=None, seed=5):
    """(Padded with NaN around the features, the [n_crops, P, D] view the replay indexes)."""
    n_crops = L.n_crops if n_crops is None else n_crops
    f = AC.make_feats(n_crops, L.P, L.D, dtype, seed).to(dev)
    pad = guarded_input(f, n_crops * L.P)
    return pad, pad.win.view(n_crops, L.P, L.D)


# ------------------------------------------------------------------------------------------------ the fused entries, raw
def _call_resampler(pr, x, n, o32, ot, ws, ws_bytes=None):
    return _lib().slime_resampler_forward(C.byref(pr.desc), x.ptr(), x.ld, n, _ptr(o32), _ptr(ot), ws.ptr(),
                                          ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _call_mlp(pm, x32, xt, rows, out, ws, ws_bytes=None):
    return _lib().slime_mlp_forward(C.byref(pm.desc), _ptr(x32), _ptr(xt), rows, out.ptr(), ws.ptr(),
                                    ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _call_gated(t, x, n, gated, out, ws, ws_bytes=None, attn=None, w_gate=True):
    pg = t.pg
    return _lib().slime_gated_forward(C.byref(pg.mlp.desc), C.byref(attn if attn is not None else pg.attn.desc),
                                      pg.w_gate.data_ptr() if w_gate else None, gated, x.ptr(), n, out.ptr(), ws.ptr(),
                                      ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _call_adapter(t, feats, n_images, n_local, nw, nh, merge, gated, out, stride, ws, ws_bytes=None, attn=None, post="own",
                  w_gate=True):
    pg = t.pg
    pdesc = (C.byref(t.post.desc) if n_local else None) if isinstance(post, str) else (None if post is None else C.byref(post))
    return _lib().slime_adapter_forward(C.byref(pg.mlp.desc), C.byref(attn if attn is not None else pg.attn.desc),
                                        pg.w_gate.data_ptr() if w_gate else None, gated, pdesc, feats.ptr(), n_images, n_local, nw, nh,
                                        int(merge), out.ptr(), _code(out.dtype), stride, ws.ptr(),
                                        ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _ints(v, ctype=C.c_int):
    return None if v is None else (ctype * max(len(v), 1))(*v)


def _call_ragged(t, feats, grids, merge, gated, out, out_rows, row0, ws, ws_bytes=None, post="own", out_code=None, n_images=None,
                 attn=None, w_gate=True):
    pg = t.pg
    pdesc = C.byref(t.post.desc) if isinstance(post, str) else (None if post is None else C.byref(post))
    nw, nh = _ints([g[0] for g in grids]), _ints([g[1] for g in grids])
    return _lib().slime_adapter_forward_ragged(C.byref(pg.mlp.desc), C.byref(attn if attn is not None else pg.attn.desc),
                                               pg.w_gate.data_ptr() if w_gate else None, gated, pdesc, feats.ptr(),
                                               len(grids) if n_images is None else n_images, nw, nh, int(merge), out.ptr(),
                                               _code(out.dtype) if out_code is None else out_code, _ints(row0, C.c_longlong), out_rows,
                                               ws.ptr(), ws.nbytes if ws_bytes is None else ws_bytes, _stream())


def _adapter_ws_bytes(t, n_images, n_local):
    pg = t.pg
    return _lib().slime_adapter_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), C.byref(t.post.desc) if n_local else None,
                                                n_images, n_local)


def _ragged_ws_bytes(t, grids, post=True):
    pg = t.pg
    return _lib().slime_adapter_ragged_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), C.byref(t.post.desc) if post else None,
                                                       len(grids), _ints([g[0] for g in grids]), _ints([g[1] for g in grids]))


def _flat_grids(grids, merge):
    return list(grids) if merge else [(nw * nh, 1 if nw * nh else 0) for nw, nh in grids]


# ------------------------------------------------------------------------------------------------ tests
@_cases("abceg")
def test_resampler(dev, tally, name, dtype):
    """slime_resampler_forward == replay_resampler bit for bit: post_qformer (q queries) of every layout and the GatedBlock's own
    resampler (P queries) of layout a; n in {1, 3}, ldx in {D, D + 8}, either output alone and both."""
    t, L = _tiny(name, dtype, dev), LAYOUTS[name]
    lib = _lib()
    for which, pr in (("post", t.post),) + ((("attn", t.pg.attn),) if name == "a" else ()):
        for n in (1, 3):
            x32 = AC.make_feats(n, L.P, L.D, dtype, seed=3 + n).float().to(dev).reshape(n * L.P, L.D)
            for pad in (0, 8):
                x = guarded_input(x32, n * L.P, pad_cols=pad)
                for want32, want_t in ((True, False), (False, True), (True, True)):
                    o32, ot = guarded_output(n * pr.n_query, L.D, torch.float32, dev), guarded_output(n * pr.n_query, L.D, dtype, dev)
                    s32, st = o32.snapshot(), ot.snapshot()
                    ws = GuardedWorkspace(lib.slime_resampler_workspace_bytes(C.byref(pr.desc), n), dev)
                    rc = _call_resampler(pr, x, n, o32 if want32 else None, ot if want_t else None, ws)
                    assert rc == 0, _err()
                    r32, rt = AC.replay_resampler(HipBackend(dtype, dev), pr, x.win, n, want32, want_t)
                    what = (name, which, n, pad, want32, want_t)
                    assert ws.intact() and o32.intact(s32) and ot.intact(st), what
                    assert _biteq(o32.win, r32) if want32 else o32.flat.equal(s32), what
                    assert _biteq(ot.win, rt) if want_t else ot.flat.equal(st), what
                    _note(tally, "resampler", name, dtype, f"{which} ldx=D+{pad}")


@_cases("abc")
def test_mlp(dev, tally, name, dtype):
    """slime_mlp_forward == replay_mlp bit for bit for the fp32 and the T input, rows in {1, 5, 2 P}."""
    t, L = _tiny(name, dtype, dev), LAYOUTS[name]
    pm, lib = t.pg.mlp, _lib()
    for rows in (1, 5, 2 * L.P):
        xt = AC.make_feats(1, rows, L.D, dtype, seed=rows).to(dev)[0]
        for is_t in (False, True):
            x = guarded_input(xt if is_t else xt.float(), rows)
            out = guarded_output(rows, L.H, torch.float32, dev)
            snap = out.snapshot()
            ws = GuardedWorkspace(lib.slime_mlp_workspace_bytes(C.byref(pm.desc), rows), dev)
            assert _call_mlp(pm, None if is_t else x, x if is_t else None, rows, out, ws) == 0, _err()
            ref = AC.replay_mlp(HipBackend(dtype, dev), pm, x.win, is_t)
            assert ws.intact() and out.intact(snap) and _biteq(out.win, ref), (name, rows, is_t)
            _note(tally, "mlp", name, dtype, "T input" if is_t else "fp32 input")


@_cases("abf")
@pytest.mark.parametrize("gated", [-1, 0, 1])
def test_gated(dev, tally, name, dtype, gated):
    """slime_gated_forward == replay_gated bit for bit; with both experts, layout a mixes in the GEMM's epilogue and layouts b, f
    through slime_gate_premix (the replay's kernel list says which)."""
    t, L = _tiny(name, dtype, dev), LAYOUTS[name]
    lib, pg = _lib(), t.pg
    for n in (1, 2):
        x = guarded_input(AC.make_feats(n, L.P, L.D, dtype, seed=20 + n).float().to(dev).reshape(n * L.P, L.D), n * L.P)
        out = guarded_output(n * L.P, L.H, torch.float32, dev)
        snap = out.snapshot()
        ws = GuardedWorkspace(lib.slime_gated_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), n), dev)
        assert _call_gated(t, x, n, gated, out, ws) == 0, _err()
        be = HipBackend(dtype, dev)
        ref = AC.replay_gated(be, pg, x.win, n, gated)
        assert ws.intact() and out.intact(snap) and _biteq(out.win, ref), (name, n, gated)
        mixes = [k for k in be.kernels if k[4] == AC.EPI_BIAS_GELU_MIX_T]
        assert len(mixes) == (1 if gated < 0 and name == "a" else 0), be.kernels
        _note(tally, "gated", name, dtype, f"gated={gated} " + ("gemm_mix" if mixes else "premix" if gated < 0 else "one expert"))


@pytest.mark.parametrize("name,dtype", CASES, ids=CASE_IDS)
def test_adapter_uniform(dev, tally, name, dtype):
    """slime_adapter_forward == replay_adapter bit for bit: learnable_gated x merge x out_dtype (fp32, T: the direct store through the
    row map; the other 16-bit type: fp32 rows + slime_merge_rows_batched) x out_image_stride (exact, exact + 5).  Rows beyond an
    image's tokens keep the sentinel, every byte outside the output window and the exactly sized workspace is intact."""
    t, L = _tiny(name, dtype, dev), LAYOUTS[name]
    fpad, feats = _feats(L, dtype, dev)
    need = _adapter_ws_bytes(t, L.n_images, L.n_local)
    assert need > 0
    for gated in (-1, 0, 1):
        for merge in (0, 1):
            nw, nh = ((L.nw, L.nh) if merge else (L.n_local, 1)) if L.n_local else (1, 1)
            for odt in (torch.float32, dtype, OTHER[dtype]):
                for extra in (0, 5):
                    stride = L.rows_per_image + extra
                    out, ref = (guarded_output(L.n_images * stride, L.H, odt, dev) for _ in range(2))
                    snap = out.snapshot()
                    ws = GuardedWorkspace(need, dev)
                    what = (name, gated, merge, odt, extra)
                    assert _call_adapter(t, fpad, L.n_images, L.n_local, nw, nh, merge, gated, out, stride, ws) == 0, (what, _err())
                    be = HipBackend(dtype, dev)
                    AC.replay_adapter(be, t, feats, L.n_images, L.n_local, nw, nh, merge, gated, ref.win, stride)
                    assert ws.intact() and out.intact(snap), what
                    assert _biteq(out.flat, ref.flat), what
                    untouched = sentinel_rows(out.win).view(L.n_images, stride)
                    assert not bool(untouched[:, :L.rows_per_image].any()) and bool(untouched[:, L.rows_per_image:].all()), what
                    mix = any(k[4] == AC.EPI_BIAS_GELU_MIX_T for k in be.kernels)
                    assert mix == (gated < 0 and name in "acdeg"), (what, be.kernels)
                    path = "direct" if odt != OTHER[dtype] else "fp32 rows + merge"
                    _note(tally, "adapter", name, dtype, f"gated={gated} merge={merge} out={DT_ID[odt]} {path}" +
                          (" gemm_mix" if mix else " premix" if gated < 0 else ""))


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_ID.get)
def test_adapter_ragged(dev, tally, dtype):
    """slime_adapter_forward_ragged == replay_adapter_ragged bit for bit (P, q, D, H of layout a): an image without local crops that
    is neither first nor last, a batch without any (post cleared), one image; packed rows and explicit out_row0 with gaps between the
    images and slack behind the last (rows no image owns keep the sentinel); and == slime_adapter_forward on a batch of equal grids."""
    t, L = _tiny("a", dtype, dev), LAYOUTS["a"]
    for grids in AC.RAGGED_GRIDS:
        n_crops = sum(1 + nw * nh for nw, nh in grids)
        fpad, feats = _feats(L, dtype, dev, n_crops, seed=8)
        rows = [L.P + nw * nh * L.q for nw, nh in grids]
        gaps, r = [], 2
        for x in rows:
            gaps.append(r)
            r += x + 3
        need = _ragged_ws_bytes(t, grids)
        assert need > 0
        for row0, total in ((None, sum(rows)), (gaps, r + 4)):
            for merge in (0, 1):
                g_ = _flat_grids(grids, merge)
                for gated in (-1, 1):
                    for odt in (torch.float32, dtype):
                        out, ref = (guarded_output(total, L.H, odt, dev) for _ in range(2))
                        snap = out.snapshot()
                        ws = GuardedWorkspace(need, dev)
                        what = (grids, row0, merge, gated, odt)
                        assert _call_ragged(t, fpad, g_, merge, gated, out, total, row0, ws) == 0, (what, _err())
                        AC.replay_adapter_ragged(HipBackend(dtype, dev), t, feats, g_, merge, gated, ref.win, row0)
                        assert ws.intact() and out.intact(snap) and _biteq(out.flat, ref.flat), what
                        owned = torch.zeros(total, dtype=torch.bool, device=dev)
                        o = 0
                        for i, x in enumerate(rows):
                            start = o if row0 is None else row0[i]
                            owned[start:start + x] = True
                            o += x
                        assert bool((sentinel_rows(out.win) == ~owned).all()), what
                        _note(tally, "adapter_ragged", "a", dtype, f"{grids} {'out_row0' if row0 else 'packed'} gated={gated} merge={merge} "
                              f"out={DT_ID[odt]}")
    # equal grids: the ragged entry and the uniform entry store the same bits
    fpad, _ = _feats(L, dtype, dev)
    grids = [(L.nw, L.nh)] * L.n_images
    for merge in (0, 1):
        g_ = _flat_grids(grids, merge)
        for gated in (-1, 1):
            for odt in (torch.float32, dtype):
                total = L.n_images * L.rows_per_image
                a, b = (guarded_output(total, L.H, odt, dev) for _ in range(2))
                assert _call_ragged(t, fpad, g_, merge, gated, a, total, None, GuardedWorkspace(_ragged_ws_bytes(t, g_), dev)) == 0, _err()
                assert _call_adapter(t, fpad, L.n_images, L.n_local, g_[0][0], g_[0][1], merge, gated, b, L.rows_per_image,
                                     GuardedWorkspace(_adapter_ws_bytes(t, L.n_images, L.n_local), dev)) == 0, _err()
                assert _biteq(a.flat, b.flat), (merge, gated, odt)
                _note(tally, "adapter_ragged", "a", dtype, f"== uniform gated={gated} merge={merge} out={DT_ID[odt]}")


def _entries(t, dtype, dev):
    """The five entries at layout a: name -> (workspace bytes, output factory, call(out, ws, ws_bytes))."""
    L, lib, pg = t.layout, _lib(), t.pg
    n = 2
    x = guarded_input(AC.make_feats(n, L.P, L.D, dtype, seed=41).float().to(dev).reshape(n * L.P, L.D), n * L.P)
    fpad, _ = _feats(L, dtype, dev)
    grids = AC.RAGGED_GRIDS[0]
    rpad, _ = _feats(L, dtype, dev, sum(1 + nw * nh for nw, nh in grids), seed=8)
    r_rows = sum(L.P + nw * nh * L.q for nw, nh in grids)
    return {
        "resampler": (lib.slime_resampler_workspace_bytes(C.byref(t.post.desc), n),
                      lambda: guarded_output(n * L.q, L.D, dtype, dev),
                      lambda out, ws, b: _call_resampler(t.post, x, n, None, out, ws, b)),
        "mlp": (lib.slime_mlp_workspace_bytes(C.byref(pg.mlp.desc), n * L.P),
                lambda: guarded_output(n * L.P, L.H, torch.float32, dev),
                lambda out, ws, b: _call_mlp(pg.mlp, x, None, n * L.P, out, ws, b)),
        "gated": (lib.slime_gated_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), n),
                  lambda: guarded_output(n * L.P, L.H, torch.float32, dev),
                  lambda out, ws, b: _call_gated(t, x, n, -1, out, ws, b)),
        "adapter": (_adapter_ws_bytes(t, L.n_images, L.n_local),
                    lambda: guarded_output(L.n_images * L.rows_per_image, L.H, dtype, dev),
                    lambda out, ws, b: _call_adapter(t, fpad, L.n_images, L.n_local, L.nw, L.nh, 1, -1, out, L.rows_per_image, ws, b)),
        "adapter_ragged": (_ragged_ws_bytes(t, grids),
                           lambda: guarded_output(r_rows, L.H, dtype, dev),
                           lambda out, ws, b: _call_ragged(t, rpad, grids, 1, -1, out, r_rows, None, ws, b)),
    }


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_ID.get)
def test_workspace(dev, dtype):
    """Each entry stays inside the workspace its *_workspace_bytes told the caller to allocate, reads nothing of it before it wrote
    it (0xFF = NaN patterns against 0x00), does not depend on a larger one, and refuses a short or misaligned one before it writes a
    byte; the size functions return 0 for the argument combinations the code names."""
    t = _tiny("a", dtype, dev)
    for entry, (need, mk, call) in _entries(t, dtype, dev).items():
        assert need > 0 and need % 256 == 0, entry
        results = []
        for fill, extra in ((0xFF, 0), (0x00, 0), (0xFF, 4096)):
            out, ws = mk(), GuardedWorkspace(need + extra, dev, fill)
            snap = out.snapshot()
            assert call(out, ws, None) == 0, (entry, _err())
            assert ws.intact() and out.intact(snap), (entry, fill, extra)
            assert not bool(sentinel_rows(out.win).any()), entry
            results.append(out.flat.clone())
        assert _biteq(results[0], results[1]), f"{entry}: the result depends on what the workspace held"
        assert _biteq(results[0], results[2]), f"{entry}: the result depends on the workspace's size"
        for ws, nbytes, why in ((GuardedWorkspace(need, dev), need - 1, "short"), (GuardedWorkspace(need + 128, dev, misalign=128), need, "misaligned")):
            out = mk()
            so, sw = out.snapshot(), ws.snapshot()
            assert call(out, ws, nbytes) == EWORKSPACE, (entry, why)
            assert "need" in _err(), (entry, why, _err())
            assert out.flat.equal(so) and ws.unchanged(sw), (entry, why)
    lib, pg, L = _lib(), t.pg, t.layout
    m, a, p = C.byref(pg.mlp.desc), C.byref(pg.attn.desc), C.byref(t.post.desc)
    assert lib.slime_resampler_workspace_bytes(None, 1) == 0 and lib.slime_resampler_workspace_bytes(p, 0) == 0
    assert lib.slime_mlp_workspace_bytes(None, 1) == 0 and lib.slime_mlp_workspace_bytes(m, 0) == 0
    assert lib.slime_gated_workspace_bytes(None, a, 1) == 0 and lib.slime_gated_workspace_bytes(m, None, 1) == 0
    assert lib.slime_gated_workspace_bytes(m, a, 0) == 0
    for args in ((None, a, p, 1, 1), (m, None, p, 1, 1), (m, a, p, 0, 1), (m, a, p, 1, -1), (m, a, None, 1, 1)):
        assert lib.slime_adapter_workspace_bytes(*args) == 0, args
    assert lib.slime_adapter_workspace_bytes(m, a, None, 1, 0) > 0
    one, zero = _ints([1]), _ints([0])
    many = _ints([0] * 65)
    for args in ((None, a, p, 1, one, one), (m, None, p, 1, one, one), (m, a, p, 1, None, one), (m, a, p, 1, one, None), (m, a, p, 0, one, one),
                 (m, a, p, 65, many, many), (m, a, p, 1, _ints([-1]), one), (m, a, p, 1, zero, one), (m, a, p, 1, one, zero),
                 (m, a, p, 1, _ints([257]), _ints([256])), (m, a, None, 1, one, one)):
        assert lib.slime_adapter_ragged_workspace_bytes(*args) == 0, args
    assert lib.slime_adapter_ragged_workspace_bytes(m, a, None, 1, zero, zero) > 0


def _copy(desc, **fields):
    d = type(desc).from_buffer_copy(desc)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_ID.get)
def test_refusals(dev, dtype):
    """One case for every SLIME_REQUIRE of slime_gated_forward, slime_adapter_forward and the ragged entry's layout check: the call
    returns SLIME_EINVAL, slime_last_error names the limit, and neither the output nor the workspace changes (nothing was launched)."""
    t = _tiny("a", dtype, dev)
    L, pg, post = t.layout, t.pg, t.post.desc
    n = 2
    x = guarded_input(AC.make_feats(n, L.P, L.D, dtype, seed=41).float().to(dev).reshape(n * L.P, L.D), n * L.P)
    fpad, _ = _feats(L, dtype, dev)
    other = _code(OTHER[dtype])
    S, B, nl = L.rows_per_image, L.n_images, L.n_local
    gws = _lib().slime_gated_workspace_bytes(C.byref(pg.mlp.desc), C.byref(pg.attn.desc), n)
    aws = _adapter_ws_bytes(t, B, nl)
    grids = AC.RAGGED_GRIDS[0]
    rpad, _ = _feats(L, dtype, dev, sum(1 + nw * nh for nw, nh in grids), seed=8)
    rrows = sum(L.P + nw * nh * L.q for nw, nh in grids)
    rws = _ragged_ws_bytes(t, grids)
    row0_ok, o = [], 0
    for nw, nh in grids:
        row0_ok.append(o)
        o += L.P + nw * nh * L.q
    null = type("Null", (), {"ptr": staticmethod(lambda: None)})()

    def gated(**kw):
        a = dict(n=n, gated=-1, xin=x)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        return gws, (n * L.P, torch.float32), lambda out, ws: _call_gated(t, a["xin"], a["n"], a["gated"], out, ws, **kw)

    def adapter(**kw):
        a = dict(n_images=B, n_local=nl, nw=L.nw, nh=L.nh, gated=-1, stride=S, feats=fpad, odt=dtype)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        return aws, (B * S, a["odt"]), lambda out, ws: _call_adapter(t, a["feats"], a["n_images"], a["n_local"], a["nw"], a["nh"], 1, a["gated"],
                                                                      out, a["stride"], ws, **kw)

    def ragged(**kw):
        a = dict(grids=grids, gated=-1, rows=rrows, row0=None, feats=rpad)
        a.update({k: kw.pop(k) for k in list(kw) if k in a})
        return rws, (rrows, dtype), lambda out, ws: _call_ragged(t, a["feats"], a["grids"], 1, a["gated"], out, a["rows"], a["row0"], ws, **kw)

    cases = [
        ("bad input", gated(n=0)),
        ("bad input", gated(xin=null)),
        ("gated: attn must map the token grid onto itself", gated(attn=_copy(pg.attn.desc, n_query=L.q))),
        ("gated: missing w_gate", gated(w_gate=False)),
        ("gated: expert index 2", gated(gated=2)),
        ("adapter: bad input", adapter(n_images=0)),
        ("adapter: bad input", adapter(n_local=-1)),
        ("adapter: bad input", adapter(feats=null)),
        ("adapter: attn must map the token grid onto itself", adapter(attn=_copy(pg.attn.desc, n_query=L.q))),
        ("adapter: missing w_gate", adapter(w_gate=False)),
        ("adapter: expert index 2", adapter(gated=2)),
        ("adapter: mixed operand dtypes", adapter(attn=_copy(pg.attn.desc, dtype=other))),
        ("post_qformer does not match the tower grid", adapter(post=_copy(post, dim=256, heads=2))),
        ("post_qformer does not match the tower grid", adapter(post=_copy(post, n_kv=L.P + 1))),
        ("post_qformer does not match the tower grid", adapter(post=_copy(post, dtype=other))),
        ("query count 8 is not a square grid", adapter(post=_copy(post, n_query=8))),
        ("grid 3x3 does not hold 6 local crops", adapter(nw=3, nh=3)),
        ("grid 0x6 does not hold", adapter(nw=0, nh=6)),
        (f"out_image_stride {S - 1} too small", adapter(stride=S - 1)),
        ("resampler: null descriptor", adapter(post=None)),
        ("token buffer too large for the 32-bit row map", adapter(stride=(1 << 31) // B + 1)),
        ("adapter_ragged: bad input", ragged(n_images=0)),
        ("adapter_ragged: bad input", ragged(feats=null)),
        ("more than SLIME_ADAPTER_RAGGED_MAX_IMAGES", ragged(grids=[(0, 0)] * 65)),
        ("a grid is 0x0", ragged(grids=[(2, 3), (0, 3), (1, 1), (3, 1)])),
        ("a grid is 0x0", ragged(grids=[(2, 3), (-1, 1), (1, 1), (3, 1)])),
        ("holds more than 65536 crops", ragged(grids=[(257, 256)])),
        ("local crops without post_qformer", ragged(post=None)),
        ("query count 8 is not a square grid", ragged(post=_copy(post, n_query=8))),
        ("post_qformer does not match the tower grid", ragged(post=_copy(post, n_kv=L.P + 1))),
        ("beyond the 32-bit row map", ragged(rows=0)),
        ("beyond the 32-bit row map", ragged(rows=1 << 31)),
        ("too small for the packed images", ragged(rows=rrows - 1)),
        ("are outside the token buffer", ragged(row0=[-1] + row0_ok[1:])),
        ("are outside the token buffer", ragged(row0=row0_ok[:-1] + [row0_ok[-1] + 1])),
        ("overlap", ragged(row0=[row0_ok[0], row0_ok[1] - 1] + row0_ok[2:])),
        ("neither fp32 nor the operand type", ragged(out_code=other)),
        ("adapter: attn must map the token grid onto itself", ragged(attn=_copy(pg.attn.desc, n_query=L.q))),
        ("adapter: missing w_gate", ragged(w_gate=False)),
        ("adapter: expert index 2", ragged(gated=2)),
        ("adapter: mixed operand dtypes", ragged(attn=_copy(pg.attn.desc, dtype=other))),
    ]
    for needle, (need, (rows, odt), call) in cases:
        out, ws = guarded_output(rows, L.H, odt, dev), GuardedWorkspace(need, dev)
        so, sw = out.snapshot(), ws.snapshot()
        rc = call(out, ws)
        assert rc == EINVAL, (needle, rc, _err())
        assert needle in _err(), (needle, _err())
        assert out.flat.equal(so) and ws.unchanged(sw), needle


@_cases("abc")
def test_small_grid_vs_oracle(dev, tally, name, dtype):
    """The fused adapter (both experts, merged) at the small grids against the fp32 oracle on the same rounded features: the global
    and the local rows of every image within the project's per-stage tolerance x 1.5 (test_gpu_path.TOL, as
    test_cfg3_layout_17_crops_vs_oracle).  Bit-equality to the replay says nothing if both misread the reference at small grids.
    Measured on an MI355X: see DESIGN.md section 2."""
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    from test_gpu_path import TOL
    t, L = _tiny(name, dtype, dev), LAYOUTS[name]
    fpad, feats = _feats(L, dtype, dev)
    out = guarded_output(L.n_images * L.rows_per_image, L.H, torch.float32, dev)
    ws = GuardedWorkspace(_adapter_ws_bytes(t, L.n_images, L.n_local), dev)
    assert _call_adapter(t, fpad, L.n_images, L.n_local, L.nw, L.nh, 1, -1, out, L.rows_per_image, ws) == 0, _err()
    got = out.win.view(L.n_images, L.rows_per_image, L.H).cpu().double()
    f32 = feats.float().cpu()
    proj, post = W.sub_state(t.sd, "mm_projector."), W.sub_state(t.sd, "sampler.post_qformer.")
    worst_g = worst_l = 0.0
    for i in range(L.n_images):
        f = f32[i * (1 + L.n_local):(i + 1) * (1 + L.n_local)]
        glob = O.gated_block_forward(proj, f[:1], L.heads, -1, target_len=L.P)[0].double()
        merged = O.spatial_merge(O.mlp_projector(proj, O.resampler_forward(post, f[1:], L.heads, t.cfg.ln_eps)), L.nw, L.nh, L.g).double()
        eg = float((got[i, :L.P] - glob).norm() / glob.norm())
        el = float((got[i, L.P:] - merged).norm() / merged.norm())
        print(f"small grid {name} {DT_ID[dtype]} image {i}: global {eg:.3e} local {el:.3e} (bound {TOL[dtype] * 1.5:.1e})")
        worst_g, worst_l = max(worst_g, eg), max(worst_l, el)
    tally["small_grid_rel_l2"][f"{name} {DT_ID[dtype]} global"] = worst_g
    tally["small_grid_rel_l2"][f"{name} {DT_ID[dtype]} local"] = worst_l
    assert worst_g < TOL[dtype] * 1.5 and worst_l < TOL[dtype] * 1.5, (worst_g, worst_l)
