"""Tower and Llama attention conformance on the GPU: slime_vit_forward / _ex / _ksplit / _states and slime_llama_attn_forward / _resid
equal, BIT FOR BIT, a replay of their launch sequence through the public element-wise bounded kernel entries
(tests/tower_conformance.py).

The replay makes the same calls -- M, N, K, epilogue, operand form and weight pointers of every GEMM, the strides and column offsets
of every attention launch -- with every intermediate in a tensor of the test's own and every offset computed in Python; it never
sees the library's workspace.  Shapes are the smallest at which each branch exists.  Inputs sit in buffers with NaN around them,
outputs and the exactly sized workspace in buffers with a sentinel byte around them.  The only tolerances of the module are the two
rel-L2 checks against the oracle at the project's existing bounds (test_gpu_path.TOL, test_gpu_prefill.TOL): bit-equality to a
replay says nothing if both misread the reference.

Measured on an MI355X (printed at the end of a run and written to the file SLIME_TOWER_CONFORMANCE_REPORT names): see DESIGN.md
section 2 for the count of bit-equal (entry, case, dtype, branch) combinations.
"""
import ctypes as C
import itertools
import json
import os

import pytest
import torch

import tower_conformance as TC
from adapter_conformance import GuardedWorkspace, guarded_input, guarded_output, sentinel_rows
from tower_conformance import DT_ID, DTYPES, HipBackend

pytestmark = pytest.mark.gpu

OTHER = {torch.bfloat16: torch.float16, torch.float16: torch.bfloat16}
EINVAL, EWORKSPACE = -1, -2
GEOMS = {"s17": (56, 14, 128), "s50": (112, 16, 256), "s226": (120, 8, 128), "s577": (336, 14, 1024)}       # image, patch, D
# (geometry, inter, layers_run, n, dtypes)
TOWER_CASES = (
    [("s17", 512, 3, n, DTYPES) for n in (1, 3, 8)]                          # M = 17, 51, 136: below a 64-row tile, below 128, across 128
    + [("s17", inter, 3, 3, DTYPES) for inter in (256, 768)]                 # ff_bytes below and above qkv + ctx (512: equal)
    + [("s17", 512, L, 3, DTYPES) for L in (0, 1)]
    + [("s50", 1024, 3, 2, DTYPES), ("s226", 512, 2, 2, DTYPES)]
    + [("s577", 4096, 2, 1, (torch.bfloat16,))]                              # 577 keys: attn64r
)
TOWER_PARAMS = [(g, i, L, n, dt) for g, i, L, n, dts in TOWER_CASES for dt in dts]
TOWER_IDS = [f"{g}-inter{i}-L{L}-n{n}-{DT_ID[dt]}" for g, i, L, n, dt in TOWER_PARAMS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tally():
    """(entry, case, dtype, branch) -> number of bit-equal comparisons; printed when the module is done (and written to the file
    SLIME_TOWER_CONFORMANCE_REPORT names, if set) together with the two rel-L2 measurements."""
    table = {"bit_equal": {}, "rel_l2": {}}
    yield table
    n = sum(table["bit_equal"].values())
    print(f"\ntower / llama conformance: {n} fused calls bit-equal to the replay in {len(table['bit_equal'])} (entry, case, dtype, branch) "
          f"combinations")
    per = {}
    for k, v in table["bit_equal"].items():
        per[k.split(" ")[0]] = per.get(k.split(" ")[0], 0) + v
    print("    " + ", ".join(f"{k}: {v}" for k, v in sorted(per.items())))
    for k, v in sorted(table["rel_l2"].items()):
        print(f"    vs oracle {k:28s} {v:.3e}")
    path = os.environ.get("SLIME_TOWER_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _lib():
    from slime_amd import _lib as L
    return L.load()


def _L():
    from slime_amd import _lib as L
    return L


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


def _note(tally, entry, case, dtype, branch):
    k = f"{entry} {case} {DT_ID[dtype]} {branch}"
    tally["bit_equal"][k] = tally["bit_equal"].get(k, 0) + 1


def _ptr(p):
    return None if p is None else p.ptr()


def _copy(desc, **fields):
    d = type(desc).from_buffer_copy(desc)
    for k, v in fields.items():
        setattr(d, k, v)
    return d


NULL = type("Null", (), {"ptr": staticmethod(lambda: None)})()

# ------------------------------------------------------------------------------------------------ towers
_towers = {}


def _tower(geom, inter, layers_run, dtype, dev):
    """(cfg, state dict, host tensors, packed tower) -- packed once per (geometry, inter, layers_run, dtype)."""
    key = (geom, inter, layers_run, dtype)
    if key not in _towers:
        from slime_amd import ops
        image, patch, D = GEOMS[geom]
        cfg = TC.tower_config(image, patch, D, inter, max(layers_run, 1))
        sd = TC.tower_state(cfg)
        _towers[key] = (cfg, sd, ops.tower_host_tensors(sd, cfg, dtype, select_layer=layers_run),
                        ops.pack_tower(sd, cfg, dtype, dev, select_layer=layers_run))
    return _towers[key]


def _pixels(cfg, n, pix_dtype, dev, seed=22):
    """(Padded with NaN around the pixels, the [n, 3, image, image] view the replay reads)."""
    from slime_amd import weights as W
    I = cfg.image_size
    px = W.synthetic_pixels(n, seed=seed, image_size=I).to(pix_dtype).to(dev)
    pad = guarded_input(px, n * 3 * I)
    return pad, pad.win.view(n, 3, I, I)


def _vit_ws_bytes(desc, n, ks=None):
    if ks is None:
        return _lib().slime_vit_workspace_bytes(C.byref(desc), n)
    return _lib().slime_vit_ksplit_workspace_bytes(C.byref(desc), n, C.byref(_L().VitKsplit(*ks)))


def _call_vit(desc, px, pix_dtype, n, out, out_dtype, keep_cls, hidden, ws, ws_bytes=None, entry="forward", probe=None, ks=None, states=None):
    lib, d = _lib(), (None if desc is None else C.byref(desc))
    nbytes = ws.nbytes if ws_bytes is None else ws_bytes
    odt = _code(out_dtype) if isinstance(out_dtype, torch.dtype) else out_dtype
    pdt = _code(pix_dtype) if isinstance(pix_dtype, torch.dtype) else pix_dtype
    if entry == "forward":
        return lib.slime_vit_forward(d, px.ptr(), pdt, n, _ptr(out), odt, keep_cls, _ptr(hidden), ws.ptr(), nbytes, _stream())
    if entry == "ex":
        return lib.slime_vit_forward_ex(d, px.ptr(), pdt, n, _ptr(out), odt, keep_cls, _ptr(hidden), ws.ptr(), nbytes, _stream(),
                                        None if probe is None else C.byref(probe))
    if entry == "ksplit":
        return lib.slime_vit_forward_ksplit(d, px.ptr(), pdt, n, _ptr(out), odt, keep_cls, _ptr(hidden),
                                            None if ks is None else C.byref(_L().VitKsplit(*ks)), ws.ptr(), nbytes, _stream())
    assert entry == "states"
    return lib.slime_vit_forward_states(d, px.ptr(), pdt, n, _ptr(states), ws.ptr(), nbytes, _stream())


def _run_vit(desc, cfg, px, pix_dtype, n, out_dtype, keep_cls, want_out, want_hidden, dev, **kw):
    """One fused call into guarded buffers with an exactly sized workspace; every guard checked.  -> (out window | None, hidden | None)."""
    D, S = cfg.hidden_size, cfg.seq_len
    out = guarded_output(n * (S if keep_cls else S - 1), D, out_dtype, dev) if want_out else None
    hid = guarded_output(n * S, D, torch.float32, dev) if want_hidden else None
    so, sh = (out.snapshot() if out else None), (hid.snapshot() if hid else None)
    ws = GuardedWorkspace(_vit_ws_bytes(desc, n, kw.get("ks")), dev)
    rc = _call_vit(desc, px, pix_dtype, n, out, out_dtype, keep_cls, hid, ws, **kw)
    assert rc == 0, _err()
    assert ws.intact(), "the tower wrote outside the workspace slime_vit*_workspace_bytes told the caller to allocate"
    assert (out is None or out.intact(so)) and (hid is None or hid.intact(sh))
    for o in (out, hid):
        assert o is None or not bool(sentinel_rows(o.win).any())
    return (out.win if out else None), (hid.win if hid else None)


@pytest.mark.parametrize("geom,inter,layers_run,n,dtype", TOWER_PARAMS, ids=TOWER_IDS)
def test_tower(dev, tally, geom, inter, layers_run, n, dtype):
    """slime_vit_forward == replay_vit bit for bit: the three forms of the layer matrices in the descriptor x pixels in fp32 and in T x
    (out in F32 / BF16 / F16 with and without the class token; hidden_f32 alone; hidden_f32 with out), hidden_f32 equal to the replay's
    join of the split stream."""
    cfg, sd, host, pt = _tower(geom, inter, layers_run, dtype, dev)
    case = f"{geom}/inter{inter}/L{layers_run}/n{n}"
    branch = "attn64r" if 321 <= cfg.seq_len <= 608 else "attn"
    outs = [(odt, keep, True, False) for odt in (torch.float32, torch.bfloat16, torch.float16) for keep in (0, 1)]
    outs += [(torch.float32, 0, False, True), (torch.float32, 0, True, True)]
    # the larger geometries: every form and pixel type with out in fp32, out with the class token in the 16-bit type that is not the
    # operand type, and hidden_f32 with out
    full = geom == "s17"
    for form in TC.FORMS:
        T, desc = TC.with_form(pt, host, form)
        for pix in (torch.float32, dtype):
            pad, px = _pixels(cfg, n, pix, dev)
            for odt, keep, want_out, want_hidden in (outs if full else (outs[0], outs[5 if dtype == torch.bfloat16 else 3], outs[7])):
                got_o, got_h = _run_vit(desc, cfg, pad, pix, n, odt, keep, want_out, want_hidden, dev)
                be = HipBackend(dtype, dev)
                ref = TC.replay_vit(be, T, cfg, px, layers_run, keep_cls=keep, out_dtype=odt, want_out=want_out, want_hidden=want_hidden)
                what = (case, form, pix, odt, keep, want_out, want_hidden)
                assert len(be.kernels) == 4 * layers_run, be.kernels
                if want_out:
                    assert _biteq(got_o, ref["out"]), what
                if want_hidden:
                    assert _biteq(got_h, ref["hidden"]), what
                if want_out and want_hidden:
                    assert _biteq(got_o, got_h.view(n, cfg.seq_len, -1)[:, 1:].reshape(got_o.shape)), what
                _note(tally, "vit_forward", case, dtype, f"{branch} {form} pix={DT_ID[pix]} " +
                      (f"out={DT_ID[odt]} keep_cls={keep}" if want_out else "") + (" hidden" if want_hidden else ""))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("geom,inter,n", [("s17", 512, 3), ("s50", 1024, 2)])
def test_tower_states_and_probe(dev, tally, geom, inter, n, dtype):
    """slime_vit_forward_states: every state equals the replay's snapshot and state layers_run equals hidden_f32 of the plain call;
    slime_vit_forward_ex with a probe on (layer 1, kernel 3) stores the same bits as without."""
    L = 3
    cfg, sd, host, pt = _tower(geom, inter, L, dtype, dev)
    case = f"{geom}/inter{inter}/L{L}/n{n}"
    M, D = n * cfg.seq_len, cfg.hidden_size
    pad, px = _pixels(cfg, n, torch.float32, dev)
    states = guarded_output((L + 1) * M, D, torch.float32, dev)
    snap = states.snapshot()
    ws = GuardedWorkspace(_vit_ws_bytes(pt.desc, n), dev)
    assert _call_vit(pt.desc, pad, torch.float32, n, None, torch.float32, 1, None, ws, entry="states", states=states) == 0, _err()
    assert ws.intact() and states.intact(snap) and not bool(sentinel_rows(states.win).any())
    ref = TC.replay_vit(HipBackend(dtype, dev), pt.tensors, cfg, px, L, want_out=False, want_states=True)["states"]
    got = states.win.view(L + 1, M, D)
    for i in range(L + 1):
        assert _biteq(got[i], ref[i]), (case, i)
    out, hidden = _run_vit(pt.desc, cfg, pad, torch.float32, n, torch.float32, 0, True, True, dev)
    assert _biteq(got[L], hidden), case
    _note(tally, "vit_forward_states", case, dtype, f"{L + 1} states")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record(); torch.cuda.synchronize()          # force creation of the HIP events
    probe = _L().Probe(1, 3, e0.cuda_event, e1.cuda_event)
    out_p, hidden_p = _run_vit(pt.desc, cfg, pad, torch.float32, n, torch.float32, 0, True, True, dev, entry="ex", probe=probe)
    torch.cuda.synchronize()
    assert _biteq(out_p, out) and _biteq(hidden_p, hidden), case
    _note(tally, "vit_forward_ex", case, dtype, "probe (1, 3)")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("ks", [(1, 1, 1, 1), (2, 1, 2, 4)], ids=str)
def test_tower_ksplit(dev, tally, dtype, ks):
    """slime_vit_forward_ksplit == the replay that makes the same launches through slime_gemm_ksplit with the same splits; the setting
    (1, 1, 1, 1) also equals slime_vit_forward."""
    geom, inter, L, n = "s17", 512, 3, 3
    cfg, sd, host, pt = _tower(geom, inter, L, dtype, dev)
    case = f"{geom}/inter{inter}/L{L}/n{n}"
    pad, px = _pixels(cfg, n, torch.float32, dev)
    for form in TC.FORMS:
        T, desc = TC.with_form(pt, host, form)
        for odt in (torch.float32, dtype):
            out, hidden = _run_vit(desc, cfg, pad, torch.float32, n, odt, 0, True, True, dev, entry="ksplit", ks=ks)
            ref = TC.replay_vit(HipBackend(dtype, dev), T, cfg, px, L, out_dtype=odt, want_hidden=True, k_split=ks)
            assert _biteq(out, ref["out"]) and _biteq(hidden, ref["hidden"]), (case, form, odt, ks)
            if ks == (1, 1, 1, 1):
                plain, plain_h = _run_vit(desc, cfg, pad, torch.float32, n, odt, 0, True, True, dev)
                assert _biteq(out, plain) and _biteq(hidden, plain_h), (case, form, odt)
            _note(tally, "vit_forward_ksplit", case, dtype, f"{form} k_split={ks} out={DT_ID[odt]}")


def _live_bytes(cfg, n):
    """The bytes of the tower's workspace that are live at once, from the geometry: lo + xn + max(ff, qkv + ctx) + stats."""
    M, D, F = n * cfg.seq_len, cfg.hidden_size, cfg.intermediate_size
    return M * D + M * D * 2 + max(M * F * 2, M * 3 * D * 2 + M * D * 2) + M * (D // 64) * 2 * 4


def _ksplit_partial_bytes(cfg, n, ks):
    """include/slime_hip.h: splits x ceil(M / 128) 128 x N fp32, rounded up to 256 (0 for splits == 1); the largest of the four."""
    M, D, F = n * cfg.seq_len, cfg.hidden_size, cfg.intermediate_size
    one = lambda N, s: 0 if s == 1 else (s * ((M + 127) // 128) * 128 * N * 4 + 255) // 256 * 256
    return max(one(3 * D, ks[0]), one(D, ks[1]), one(F, ks[2]), one(D, ks[3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_tower_workspace(dev, dtype):
    """slime_vit_workspace_bytes holds what is live at once (computed here from the geometry) and no more than 256 bytes per region
    above it, on both sides of and at ff_bytes = qkv + ctx; the k-split size adds the largest region of partial products.  A run
    does not depend on what the workspace held or on a larger one; need - 1 bytes and a pointer misaligned by 128 bytes return
    SLIME_EWORKSPACE with outputs and workspace untouched."""
    lib = _lib()
    for geom, inter, L, n in (("s17", 256, 3, 3), ("s17", 512, 3, 3), ("s17", 768, 3, 8), ("s50", 1024, 3, 2), ("s17", 512, 0, 1)):
        cfg, sd, host, pt = _tower(geom, inter, L, dtype, dev)
        need, live = _vit_ws_bytes(pt.desc, n), _live_bytes(cfg, n)
        assert need % 256 == 0 and live <= need <= live + 6 * 256, (geom, inter, n, need, live)
        for ks in ((1, 1, 1, 1), (2, 2, 2, 4)):
            kneed = _vit_ws_bytes(pt.desc, n, ks)
            part = _ksplit_partial_bytes(cfg, n, ks)
            assert kneed == need + part, (geom, inter, n, ks, kneed, need, part)
            for N, s in zip((3 * cfg.hidden_size, cfg.hidden_size, inter, cfg.hidden_size), ks):
                assert lib.slime_gemm_ksplit_workspace_bytes(n * cfg.seq_len, N, s) <= part
    cfg, sd, host, pt = _tower("s17", 512, 3, dtype, dev)
    n = 3
    pad, _ = _pixels(cfg, n, torch.float32, dev)
    mk = lambda: guarded_output(n * (cfg.seq_len - 1), cfg.hidden_size, dtype, dev)
    for entry, ks in (("forward", None), ("ksplit", (2, 1, 2, 4))):
        need = _vit_ws_bytes(pt.desc, n, ks)
        results = []
        for fill, extra in ((0xFF, 0), (0x00, 0), (0xFF, 4096)):
            out, ws = mk(), GuardedWorkspace(need + extra, dev, fill)
            snap = out.snapshot()
            assert _call_vit(pt.desc, pad, torch.float32, n, out, dtype, 0, None, ws, entry=entry, ks=ks) == 0, (entry, _err())
            assert ws.intact() and out.intact(snap) and not bool(sentinel_rows(out.win).any()), (entry, fill, extra)
            results.append(out.flat.clone())
        assert _biteq(results[0], results[1]), f"{entry}: the result depends on what the workspace held"
        assert _biteq(results[0], results[2]), f"{entry}: the result depends on the workspace's size"
        for ws, nbytes, why in ((GuardedWorkspace(need, dev), need - 1, "short"), (GuardedWorkspace(need + 128, dev, misalign=128), need, "misaligned")):
            out = mk()
            so, sw = out.snapshot(), ws.snapshot()
            assert _call_vit(pt.desc, pad, torch.float32, n, out, dtype, 0, None, ws, ws_bytes=nbytes, entry=entry, ks=ks) == EWORKSPACE, (entry, why)
            assert "need" in _err(), (entry, why, _err())
            assert out.flat.equal(so) and ws.unchanged(sw), (entry, why)
    d = C.byref(pt.desc)
    assert lib.slime_vit_workspace_bytes(None, 1) == 0 and lib.slime_vit_workspace_bytes(d, 0) == 0
    assert lib.slime_vit_workspace_bytes(C.byref(_copy(pt.desc, patch=0)), 1) == 0
    k1 = C.byref(_L().VitKsplit(1, 1, 1, 1))
    assert lib.slime_vit_ksplit_workspace_bytes(None, 1, k1) == 0 and lib.slime_vit_ksplit_workspace_bytes(d, 1, None) == 0
    assert lib.slime_vit_ksplit_workspace_bytes(d, 0, k1) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_tower_refusals(dev, dtype):
    """One case for every SLIME_REQUIRE of vit_validate, vit_run, vit_ksplit_validate and the entries' own: the call returns
    SLIME_EINVAL, slime_last_error names the limit, and neither an output nor the workspace changes (nothing was launched).
    vit_validate's `hidden % 64` cannot fail behind `hidden in {128, 256, 1024}`: it has no case."""
    cfg, sd, host, pt = _tower("s17", 512, 3, dtype, dev)
    n, D, S = 3, cfg.hidden_size, cfg.seq_len
    pad, _ = _pixels(cfg, n, torch.float32, dev)
    d0 = pt.desc
    need = _vit_ws_bytes(d0, n)
    kneed = _vit_ws_bytes(d0, n, (2, 2, 2, 8))
    U8 = _code(torch.uint8)
    cases = [
        ("vit: null descriptor", dict(desc=None)),
        ("vit: dtype must be BF16 or F16", dict(desc=_copy(d0, dtype=_code(torch.float32)))),
        ("vit: hidden=192 unsupported", dict(desc=_copy(d0, hidden=192, heads=3))),
        ("vit: head_dim must be 64", dict(desc=_copy(d0, heads=1))),
        ("vit: head_dim must be 64", dict(desc=_copy(d0, heads=0))),
        ("vit: head_dim must be 64", dict(desc=_copy(d0, heads=3))),
        ("vit: intermediate size 320 must be a multiple of 128", dict(desc=_copy(d0, inter=320))),
        ("vit: image 57 not a multiple of patch 14", dict(desc=_copy(d0, image=57))),
        ("vit: image 56 not a multiple of patch 0", dict(desc=_copy(d0, patch=0))),
        ("patch_embed: image 60 must be a multiple of the patch 12 and of 8", dict(desc=_copy(d0, image=60, patch=12))),
        ("patch_embed: kpad=576", dict(desc=_copy(d0, kpad=576))),
        ("patch_embed: 25 patches per side", dict(desc=_copy(d0, image=200, patch=8))),
        ("vit: layers_run < 0", dict(desc=_copy(d0, layers_run=-1))),
        ("vit: missing embedding weights", dict(desc=_copy(d0, cls=None))),
        ("vit: missing embedding weights", dict(desc=_copy(d0, patch_w_frag=None))),
        ("vit: missing layer weights", dict(desc=_copy(d0, b_qkv=None))),
        ("vit: missing layer weights", dict(desc=_copy(d0, colsum_fc1=None))),
        ("vit: missing layer weights", dict(desc=_copy(d0, w_o=None, w_o_frag=None))),
        ("vit: bad input", dict(px=NULL)),
        ("vit: bad input", dict(n=0)),
        ("vit: no output requested", dict(out=False)),
        ("vit: bad out dtype", dict(out_dtype=U8)),
        ("vit_forward_ksplit: null k-split setting", dict(entry="ksplit", ks=None)),
        ("vit: k-split qkv=0 outside 1..2", dict(entry="ksplit", ks=(0, 1, 1, 1))),
        ("vit: k-split qkv=3 outside 1..2", dict(entry="ksplit", ks=(3, 1, 1, 1))),
        ("vit: k-split out_proj=3 outside 1..2", dict(entry="ksplit", ks=(1, 3, 1, 1))),
        ("vit: k-split fc1=3 outside 1..2", dict(entry="ksplit", ks=(1, 1, 3, 1))),
        ("vit: k-split fc2=9 outside 1..8", dict(entry="ksplit", ks=(1, 1, 1, 9))),
        ("vit_forward_states: states_f32 is required", dict(entry="states", states=False)),
    ]
    for needle, kw in cases:
        entry = kw.get("entry", "forward")
        out = guarded_output(n * (S - 1), D, dtype, dev)
        hid = guarded_output(n * S, D, torch.float32, dev)
        states = guarded_output(4 * n * S, D, torch.float32, dev)
        ws = GuardedWorkspace(kneed if entry == "ksplit" else need, dev)
        snaps = [b.snapshot() for b in (out, hid, states, ws)]
        use_out = kw.get("out", True)
        rc = _call_vit(kw.get("desc", d0), kw.get("px", pad), torch.float32, kw.get("n", n), out if use_out else None,
                       kw.get("out_dtype", dtype), 0, hid if use_out and entry != "states" else None, ws, entry=entry, ks=kw.get("ks"),
                       states=states if kw.get("states", True) else None)
        assert rc == EINVAL, (needle, rc, _err())
        assert needle in _err(), (needle, _err())
        assert out.flat.equal(snaps[0]) and hid.flat.equal(snaps[1]) and states.flat.equal(snaps[2]) and ws.unchanged(snaps[3]), needle


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_pack_tower_is_the_host_tensors(dev, dtype):
    """pack_tower's device tensors are ops.tower_host_tensors moved to the device, byte for byte: every fp32 tensor, and every matrix
    as the fragment-order image of the host matrix (the row-major matrix is dropped by default)."""
    from slime_amd import ops
    cfg, sd, host, pt = _tower("s17", 512, 3, dtype, dev)
    for k, v in host.items():
        if k in TC.LAYER_WEIGHTS or k == "patch_w":
            assert v.dtype == dtype
            assert _biteq(pt.tensors[k + "_frag"], ops.pack_b_frag(v.to(dev))), k
            if pt.tensors.get(k) is not None:
                assert _biteq(pt.tensors[k], v.to(dev)), k
        else:
            assert v.dtype == torch.float32 and _biteq(pt.tensors[k], v.to(dev)), k


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_tower_vs_oracle(dev, tally, dtype):
    """The one rel-L2 of the tower here: the smallest geometry against the oracle at the project's tower tolerance."""
    from oracle import slime_oracle as O
    from conftest import rel_l2
    from test_gpu_path import TOL
    cfg, sd, host, pt = _tower("s17", 512, 3, dtype, dev)
    n = 3
    pad, px = _pixels(cfg, n, torch.float32, dev)
    out, _ = _run_vit(pt.desc, cfg, pad, torch.float32, n, torch.float32, 0, True, False, dev)
    ref = O.tower_forward(sd, cfg, px.cpu(), select_layer=3)
    err = rel_l2(out.view(ref.shape).cpu(), ref)
    print(f"\ntower s17 {DT_ID[dtype]}: rel-L2 {err:.3e} (tolerance {TOL[dtype]:.1e})")
    tally["rel_l2"][f"tower s17 {DT_ID[dtype]}"] = err
    assert err < TOL[dtype], err


# ------------------------------------------------------------------------------------------------ the Llama attention layer
LLAMA_GEOMS = [(256, 2, 1), (512, 4, 4), (512, 4, 1)]                 # hidden, heads, kv heads: GQA groups 2, 1, 4
LLAMA_SHAPES = [(1, 1), (3, 5), (2, 65), (1, 193)]                   # batch, S
_llamas = {}


def _llama(hidden, hq, hkv, dtype, dev):
    """(fp32 weights, packed layer, {form: (tensors, descriptor)})."""
    key = (hidden, hq, hkv, dtype)
    if key not in _llamas:
        from slime_amd import ops
        g = torch.Generator().manual_seed(7)
        w = [torch.randn(n, k, generator=g) * k ** -0.5 for n, k in ((hq * 128, hidden), (hkv * 128, hidden), (hkv * 128, hidden), (hidden, hq * 128))]
        pa = ops.pack_llama_attention(w[0], w[1], w[2], w[3], hq, hkv, dtype, dev)
        rm = {"w_qkv": torch.cat(w[:3]).to(dtype).to(dev).contiguous(), "w_o": w[3].to(dtype).to(dev).contiguous()}
        forms = {}
        for form in TC.FORMS:
            T, d = dict(pa.tensors), _copy(pa.desc)
            for name in ("w_qkv", "w_o"):
                assert pa.tensors[name + "_frag"] is not None
                T[name] = rm[name] if form != "frag" else None
                T[name + "_frag"] = pa.tensors[name + "_frag"] if form != "row_major" else None
                for k in (name, name + "_frag"):
                    setattr(d, k, None if T[k] is None else T[k].data_ptr())
            forms[form] = (T, d)
        _llamas[key] = (w, pa, forms)
    return _llamas[key]


def _ranges(pad, batch, S, dev):
    """kv_start / kv_len int32 [batch] (None: absent): sequence b holds max(1, S - 2 b - 1) tokens at the front or at the back."""
    if pad == "none":
        return None, None
    ln = [max(1, S - 2 * b - 1) for b in range(batch)]
    st = [0 if pad == "right" else S - x for x in ln]
    return torch.tensor(st, dtype=torch.int32, device=dev), torch.tensor(ln, dtype=torch.int32, device=dev)


def _call_llama(desc, x, pos, start, length, batch, S, out, out_dtype, ws, ws_bytes=None, resid=None, entry="forward"):
    lib, d = _lib(), (None if desc is None else C.byref(desc))
    p = lambda t: None if t is None else t.data_ptr()
    nbytes = ws.nbytes if ws_bytes is None else ws_bytes
    if entry == "forward":
        odt = _code(out_dtype) if isinstance(out_dtype, torch.dtype) else out_dtype
        return lib.slime_llama_attn_forward(d, _ptr(x), p(pos), p(start), p(length), batch, S, _ptr(out), odt, ws.ptr(), nbytes, _stream())
    return lib.slime_llama_attn_forward_resid(d, _ptr(x), p(pos), p(start), p(length), batch, S, _ptr(resid), _ptr(out), ws.ptr(), nbytes,
                                              _stream())


def _llama_inputs(hidden, batch, S, dtype, dev, seed=3):
    g = torch.Generator().manual_seed(seed + 17 * S + batch)
    x = torch.randn(batch * S, hidden, generator=g).to(dtype).to(dev)
    r = torch.randn(batch * S, hidden, generator=g).to(dtype).to(dev)
    pos = (torch.arange(S)[None] + 7 * torch.arange(batch)[:, None]).reshape(-1).to(torch.int32).to(dev)
    return x, r, pos


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("hidden,hq,hkv", LLAMA_GEOMS, ids=[f"h{h}-q{q}-kv{k}" for h, q, k in LLAMA_GEOMS])
def test_llama_attention(dev, tally, hidden, hq, hkv, dtype):
    """slime_llama_attn_forward (out in T and in fp32) and _resid (out apart from resid, out = resid) == replay_llama_attn bit for bit:
    (batch, S) x kv ranges absent / right padded / left padded, position ids with a per-row offset; the three weight forms at (3, 5)
    and (2, 65)."""
    w, pa, forms = _llama(hidden, hq, hkv, dtype, dev)
    lib = _lib()
    case = f"h{hidden}/q{hq}/kv{hkv}"
    for (batch, S), pad in itertools.product(LLAMA_SHAPES, ("none", "right", "left")):
        M = batch * S
        x, r, pos = _llama_inputs(hidden, batch, S, dtype, dev)
        xin, rin = guarded_input(x, M), guarded_input(r, M)
        start, length = _ranges(pad, batch, S, dev)
        for form in (TC.FORMS if (batch, S) in ((3, 5), (2, 65)) else ("frag",)):
            T, desc = forms[form]
            need = lib.slime_llama_attn_workspace_bytes(C.byref(desc), batch, S)
            for mode in ("T", "fp32", "resid", "resid_alias"):
                odt = torch.float32 if mode == "fp32" else dtype
                out = guarded_output(M, hidden, odt, dev)
                if mode == "resid_alias":
                    out.win.copy_(r)
                snap = out.snapshot()
                ws = GuardedWorkspace(need, dev)
                what = (case, batch, S, pad, form, mode)
                be = HipBackend(dtype, dev)
                args = (be, T, hidden, hq, hkv, xin.win, pos, start, length, batch, S)
                if mode in ("T", "fp32"):
                    rc = _call_llama(desc, xin, pos, start, length, batch, S, out, odt, ws)
                    ref = TC.replay_llama_attn(*args, epilogue=TC.EPI_BIAS_F32 if mode == "fp32" else TC.EPI_BIAS_T)
                else:
                    rc = _call_llama(desc, xin, pos, start, length, batch, S, out, None, ws, resid=out if mode == "resid_alias" else rin,
                                     entry="resid")
                    own = r.clone()
                    ref = TC.replay_llama_attn(*args, epilogue=TC.EPI_BIAS_RESID_T, resid=own, out=own if mode == "resid_alias" else None)
                assert rc == 0, (what, _err())
                assert ws.intact() and out.intact(snap) and not bool(sentinel_rows(out.win).any()), what
                assert _biteq(out.win, ref), what
                assert [k[4] for k in be.kernels] == [TC.EPI_BIAS_T, {"T": TC.EPI_BIAS_T, "fp32": TC.EPI_BIAS_F32}.get(mode, TC.EPI_BIAS_RESID_T)]
                _note(tally, "llama_attn_resid" if mode.startswith("resid") else "llama_attn", case, dtype, f"B{batch} S{S} pad={pad} {form} {mode}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_llama_workspace_and_refusals(dev, dtype):
    """slime_llama_attn_workspace_bytes holds the packed q/k/v rows and the context rows and at most 256 bytes per region more; a run
    does not depend on what the workspace held; need - 1 bytes and a misaligned pointer return SLIME_EWORKSPACE, and every
    SLIME_REQUIRE of llama_validate, llama_attn_run and the two entries SLIME_EINVAL with the limit named, all with the output and the
    workspace untouched.  llama_validate's null-descriptor check cannot fail behind the entries' own: it has no case."""
    hidden, hq, hkv, batch, S = 256, 2, 1, 3, 5
    w, pa, forms = _llama(hidden, hq, hkv, dtype, dev)
    lib, M = _lib(), batch * S
    T, d0 = forms["frag"]
    for b, s in LLAMA_SHAPES:
        need, live = lib.slime_llama_attn_workspace_bytes(C.byref(d0), b, s), b * s * (hq + 2 * hkv) * 128 * 2 + b * s * hq * 128 * 2
        assert need % 256 == 0 and live <= need <= live + 2 * 256, (b, s, need, live)
    need = lib.slime_llama_attn_workspace_bytes(C.byref(d0), batch, S)
    assert lib.slime_llama_attn_workspace_bytes(None, 1, 1) == 0 and lib.slime_llama_attn_workspace_bytes(C.byref(d0), 0, 1) == 0
    assert lib.slime_llama_attn_workspace_bytes(C.byref(d0), 1, 0) == 0
    x, r, pos = _llama_inputs(hidden, batch, S, dtype, dev)
    xin, rin = guarded_input(x, M), guarded_input(r, M)
    mk = lambda odt=dtype: guarded_output(M, hidden, odt, dev)
    for entry in ("forward", "resid"):
        results = []
        for fill in (0xFF, 0x00):
            out, ws = mk(), GuardedWorkspace(need, dev, fill)
            assert _call_llama(d0, xin, pos, None, None, batch, S, out, dtype, ws, resid=rin, entry=entry) == 0, _err()
            assert ws.intact()
            results.append(out.flat.clone())
        assert _biteq(results[0], results[1]), f"{entry}: the result depends on what the workspace held"
        for ws, nbytes, why in ((GuardedWorkspace(need, dev), need - 1, "short"), (GuardedWorkspace(need + 128, dev, misalign=128), need, "misaligned")):
            out = mk()
            so, sw = out.snapshot(), ws.snapshot()
            assert _call_llama(d0, xin, pos, None, None, batch, S, out, dtype, ws, ws_bytes=nbytes, resid=rin, entry=entry) == EWORKSPACE, (entry, why)
            assert "need" in _err(), (entry, why, _err())
            assert out.flat.equal(so) and ws.unchanged(sw), (entry, why)
    F32 = _code(torch.float32)
    cases = [
        ("llama_attn: bad input", dict(desc=None)),
        ("llama_attn: bad input", dict(out=False)),
        ("llama_attn: out dtype must be the operand type or F32", dict(out_dtype=OTHER[dtype])),
        ("llama_attn: dtype must be BF16 or F16", dict(desc=_copy(d0, dtype=F32), out_dtype=torch.float32)),
        ("llama_attn: heads", dict(desc=_copy(d0, head_dim=64))),
        ("llama_attn: heads", dict(desc=_copy(d0, n_heads=0))),
        ("llama_attn: heads", dict(desc=_copy(d0, n_kv_heads=0))),
        ("llama_attn: heads", dict(desc=_copy(d0, n_heads=3, n_kv_heads=2))),
        ("llama_attn: hidden=192 must be a multiple of 128", dict(desc=_copy(d0, hidden=192))),
        ("llama_attn: missing weights", dict(desc=_copy(d0, inv_freq=None))),
        ("llama_attn: missing weights", dict(desc=_copy(d0, w_qkv=None, w_qkv_frag=None))),
        ("llama_attn: missing weights", dict(desc=_copy(d0, w_o=None, w_o_frag=None))),
        ("llama_attn: bad input", dict(x=NULL)),
        ("llama_attn: bad input", dict(pos=None)),
        ("llama_attn: bad input", dict(batch=0)),
        ("llama_attn: bad input", dict(S=0)),
        ("llama_attn_resid: resid and out are required", dict(entry="resid", desc=None)),
        ("llama_attn_resid: resid and out are required", dict(entry="resid", resid=NULL)),
        ("llama_attn_resid: resid and out are required", dict(entry="resid", out=False)),
        ("llama_attn_resid: out may alias resid, not the layer's input rows", dict(entry="resid", x="out")),
        ("llama_attn: bad input", dict(entry="resid", batch=0)),
        ("llama_attn: heads", dict(entry="resid", desc=_copy(d0, head_dim=64))),
    ]
    for needle, kw in cases:
        out, ws = mk(), GuardedWorkspace(need, dev)
        so, sw = out.snapshot(), ws.snapshot()
        xarg = out if kw.get("x") == "out" else kw.get("x", xin)
        rc = _call_llama(kw.get("desc", d0), xarg, kw.get("pos", pos), None, None, kw.get("batch", batch), kw.get("S", S),
                         out if kw.get("out", True) else None, kw.get("out_dtype", dtype), ws, resid=kw.get("resid", rin),
                         entry=kw.get("entry", "forward"))
        assert rc == EINVAL, (needle, rc, _err())
        assert needle in _err(), (needle, _err())
        assert out.flat.equal(so) and ws.unchanged(sw), needle


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_llama_vs_oracle(dev, tally, dtype):
    """The one rel-L2 of the Llama layer here: the smallest geometry, right padded, against the oracle on the rounded input at the
    project's tolerance for this layer (test_gpu_prefill.TOL)."""
    from oracle import prefill_oracle as P
    from conftest import rel_l2
    from test_gpu_prefill import TOL
    hidden, hq, hkv, batch, S = 256, 2, 1, 3, 5
    w, pa, forms = _llama(hidden, hq, hkv, dtype, dev)
    T, d0 = forms["frag"]
    x, r, pos = _llama_inputs(hidden, batch, S, dtype, dev)
    start, length = _ranges("right", batch, S, dev)
    out = guarded_output(batch * S, hidden, torch.float32, dev)
    ws = GuardedWorkspace(_lib().slime_llama_attn_workspace_bytes(C.byref(d0), batch, S), dev)
    assert _call_llama(d0, guarded_input(x, batch * S), pos, start, length, batch, S, out, torch.float32, ws) == 0, _err()
    mask = (torch.arange(S)[None] < length.cpu()[:, None]).long()
    ref = P.llama_attention_forward(x.float().cpu().view(batch, S, hidden), w[0], w[1], w[2], w[3], hq, hkv, pos.cpu().view(batch, S).long(), mask,
                                    head_dim=128)
    err = rel_l2(out.win.view(batch, S, hidden).cpu(), ref)
    print(f"\nllama h256 {DT_ID[dtype]}: rel-L2 {err:.3e} (tolerance {TOL[dtype]:.1e})")
    tally["rel_l2"][f"llama h256/q2/kv1 {DT_ID[dtype]}"] = err
    assert err < TOL[dtype], err
