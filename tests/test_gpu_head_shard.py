"""Head-sharded Llama attention on the GPU: what ``bench.py --gpus N --prefill-shard heads`` executes on every rank, pinned on one GPU
(tests/head_shard_conformance.py; DESIGN.md sections 2 and 7).

A rank's call is ``slime_llama_attn_forward`` / ``_resid`` on a descriptor with n_heads * 128 < hidden: a q/k/v GEMM with
N = (hq_r + 2 hkv_r) 128 and an o_proj with K = hq_r 128.  The slices are ``slime_amd.dist.shard_llama_attention_weights`` of one seeded
full layer, packed per rank.  Inputs sit in buffers with NaN around them, outputs and the exactly sized workspace in buffers with a
sentinel byte around them.

 1. the fused entry on every (geometry, rank) equals ``replay_llama_attn`` with the slice's (hidden, hq_r, hkv_r) BIT FOR BIT (T, fp32,
    _resid apart from and into resid), and the workspace is the slice's packed rows and context rows;
 2. a rank's packed q/k/v rows after RoPE and its context rows are the full layer's column blocks, bit for bit;
 3. the fp32 partials summed in float64 lie within e (K_r + 4) S + e (K + 4) S of the full layer's fp32 o_proj;
 4. the 16-bit terms are the roundings of the fp32 partials, and summed in T in every order they lie within
    (world - 1) u A (1 + 2^-6) + (world - 1) g of their float64 sum;
 5. one rel-L2 per geometry and dtype against the oracle on the FULL layer (the module's only tolerance that is not derived element
    by element: 1 - 4 would all pass if slice and replay misread the layer alike);
 6. ``dist.head_sharded_attention`` with the ops entries as the local call, 2 and 4 ranks on cuda:0 over gloo, two stacked layers
    (tests/head_shard_gpu_worker.py);
 7. ``ops.adapter_forward_precompressed`` -- the adapter of the compressed-local exchange -- equals ``ops.adapter_forward`` on the same
    features bit for bit, global and local rows.

Measured on an MI355X (printed at the end of a run and written to the file SLIME_HEAD_SHARD_CONFORMANCE_REPORT names; measurements,
not targets) -- worst |err| / bound of checks 3 and 4, rel-L2 of check 5 (sharded / unsharded, tolerance bf16 8e-3, fp16 1.2e-3):

    geometry dtype           3: partials   4: reduce   5: sharded   unsharded
    (512, 4, 4, 2)  bf16       0.002        0.981      2.80e-3     2.23e-3
    (512, 4, 4, 2)  fp16       0.002        0.984      3.52e-4     2.81e-4
    (512, 4, 4, 4)  bf16       0.003        0.881      3.62e-3     2.23e-3
    (512, 4, 4, 4)  fp16       0.003        0.900      4.55e-4     2.81e-4
    (512, 4, 2, 2)  bf16       0.002        0.981      2.80e-3     2.24e-3
    (512, 4, 2, 2)  fp16       0.002        0.984      3.53e-4     2.81e-4
    (1024, 8, 2, 2) bf16       0.002        0.981      2.77e-3     2.21e-3
    (1024, 8, 2, 2) fp16       0.001        0.984      3.47e-4     2.75e-4
    (4096, 32, 8, 8) bf16     < 0.001       0.576      4.85e-3     2.22e-3
3096 bit-equal comparisons (checks 1, 2, 7): no bit-equality had to be replaced by a tolerance.  Check 6: reduce 0.981 / 0.984 (world
2, bf16 / fp16) and 0.812 / 0.785 (world 4); two layers against the oracle 4.3e-3 / 5.4e-4 and 5.1e-3 / 6.5e-4 (tolerance 1.6e-2 /
2.4e-3).  The whole module runs in under 20 s, 12 s of it the two rank tests.
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch

import head_shard_conformance as HS
import test_gpu_tower_conformance as TT
import tower_conformance as TC
from adapter_conformance import GuardedWorkspace, guarded_input, guarded_output, sentinel_rows
from tower_conformance import DT_ID, DTYPES, HipBackend

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

GEOM_PARAMS, GEOM_IDS = HS.geom_params()
SLICE_PARAMS = [(g, r, dt) for g, dt in GEOM_PARAMS for r in range(g[3])]
SLICE_IDS = [f"{HS.geom_id(g)}-rank{r}-{DT_ID[dt]}" for g, r, dt in SLICE_PARAMS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def report():
    """check -> "geometry dtype" -> worst |err| / bound (checks 3, 4), rel-L2 (check 5), bit-equal comparisons (checks 1, 2, 7);
    printed when the module is done and written to the file SLIME_HEAD_SHARD_CONFORMANCE_REPORT names, if set."""
    table = {"bit_equal": {}, "partials": {}, "reduce": {}, "rel_l2_sharded": {}, "rel_l2_unsharded": {}}
    yield table
    print(f"\nhead-shard conformance: {sum(table['bit_equal'].values())} bit-equal comparisons in {len(table['bit_equal'])} (check, case) combinations")
    for k in sorted(set(table["partials"]) | set(table["reduce"]) | set(table["rel_l2_sharded"])):
        f = lambda name, fmt: format(table[name][k], fmt) if k in table[name] else "-"
        print(f"    {k:24s} worst |err| / bound: partials {f('partials', '.3f')}  reduce {f('reduce', '.3f')};  rel-L2 vs oracle: sharded "
              f"{f('rel_l2_sharded', '.2e')}  unsharded {f('rel_l2_unsharded', '.2e')}")
    path = os.environ.get("SLIME_HEAD_SHARD_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _count(report, key, n=1):
    report["bit_equal"][key] = report["bit_equal"].get(key, 0) + n


def _worst(report, name, key, value):
    report[name][key] = max(report[name].get(key, 0.0), value)


# ------------------------------------------------------------------------------------------------ packed layers and slices
_layers = {}


def _pack(w4, hq, hkv, dtype, dev, forms):
    """(packed layer, {form: (tensors, descriptor)}) as test_gpu_tower_conformance._llama builds them, from given fp32 weights."""
    from slime_amd import ops
    pa = ops.pack_llama_attention(w4[0], w4[1], w4[2], w4[3], hq, hkv, dtype, dev)
    out = {}
    for form in forms:
        T, d = dict(pa.tensors), TT._copy(pa.desc)
        for name, rm in (("w_qkv", torch.cat(w4[:3])), ("w_o", w4[3])):
            assert pa.tensors[name + "_frag"] is not None
            T[name] = rm.to(dtype).to(dev).contiguous() if form != "frag" else None
            T[name + "_frag"] = pa.tensors[name + "_frag"] if form != "row_major" else None
            for k in (name, name + "_frag"):
                setattr(d, k, None if T[k] is None else T[k].data_ptr())
        out[form] = (T, d)
    return pa, out


def _layer(geom, dtype, dev):
    """{"w": fp32 weights of the full layer, "full": forms of the full layer, "ranks": [forms of rank r's slice]} -- the slices are
    shard_llama_attention_weights of the full layer's fp32 weights, packed (rounded to T) once per (geometry, dtype)."""
    key = (geom, dtype)
    if key not in _layers:
        hidden, hq, hkv, world = geom
        w = HS.layer_weights(hidden, hq, hkv)
        forms = ("frag",) if geom == HS.REAL_GEOM else TC.FORMS
        ranks = []
        for wq, wk, wv, wo, hq_r, hkv_r in HS.rank_slices(w, hq, hkv, world):
            assert (hq_r, hkv_r) == HS.slice_heads(geom)
            ranks.append(_pack((wq, wk, wv, wo), hq_r, hkv_r, dtype, dev, forms)[1])
        _layers[key] = {"w": w, "full": _pack(w, hq, hkv, dtype, dev, ("frag",))[1], "ranks": ranks,
                        "wo_t": w[3].to(dtype).to(dev)}
    return _layers[key]


def _fused(desc, hidden, xin, rin, r, pos, start, length, batch, S, dtype, mode, dev, what):
    """One fused call into a guarded output with an exactly sized guarded workspace; every guard checked.  mode: "T" / "fp32"
    (slime_llama_attn_forward) or "resid" / "resid_alias" (slime_llama_attn_forward_resid, out apart from / equal to resid)."""
    M = batch * S
    odt = torch.float32 if mode == "fp32" else dtype
    out = guarded_output(M, hidden, odt, dev)
    if mode == "resid_alias":
        out.win.copy_(r)
    snap = out.snapshot()
    ws = GuardedWorkspace(TT._lib().slime_llama_attn_workspace_bytes(C.byref(desc), batch, S), dev)
    if mode in ("T", "fp32"):
        rc = TT._call_llama(desc, xin, pos, start, length, batch, S, out, odt, ws)
    else:
        rc = TT._call_llama(desc, xin, pos, start, length, batch, S, out, None, ws, resid=out if mode == "resid_alias" else rin, entry="resid")
    assert rc == 0, (what, TT._err())
    assert ws.intact(), (what, "the call wrote outside the workspace slime_llama_attn_workspace_bytes told the caller to allocate")
    assert out.intact(snap) and not bool(sentinel_rows(out.win).any()), what
    return out.win


def _inputs(hidden, batch, S, pad, dtype, dev):
    x, r, pos = TT._llama_inputs(hidden, batch, S, dtype, dev)
    start, length = TT._ranges(pad, batch, S, dev)
    return x, r, pos, start, length, guarded_input(x, batch * S), guarded_input(r, batch * S)


# ------------------------------------------------------------------------------------------------ check 1
@pytest.mark.parametrize("geom,rank,dtype", SLICE_PARAMS, ids=SLICE_IDS)
def test_fused_entry_equals_replay_on_a_slice(dev, report, geom, rank, dtype):
    """slime_llama_attn_forward (out in T and in fp32) and _resid (out apart from resid, out = resid) on rank ``rank``'s slice ==
    replay_llama_attn with (hidden, hq_r, hkv_r) bit for bit: (batch, S) x kv ranges absent / right padded / left padded; the three
    weight forms at (3, 5) and (2, 65).  The workspace holds the slice's packed q/k/v rows and context rows and at most 256 bytes per
    region more."""
    hidden, hq, hkv, world = geom
    hq_r, hkv_r = HS.slice_heads(geom)
    forms = _layer(geom, dtype, dev)["ranks"][rank]
    lib = TT._lib()
    case = f"{HS.geom_id(geom)} rank{rank} {DT_ID[dtype]}"
    for (batch, S), pad in itertools.product(HS.geom_shapes(geom), HS.PADS):
        x, r, pos, start, length, xin, rin = _inputs(hidden, batch, S, pad, dtype, dev)
        for form in (forms if (batch, S) in HS.FORM_SHAPES else ("frag",)):
            T, desc = forms[form]
            assert (desc.hidden, desc.n_heads, desc.n_kv_heads) == (hidden, hq_r, hkv_r)
            need, live = lib.slime_llama_attn_workspace_bytes(C.byref(desc), batch, S), HS.slice_workspace_bytes(batch * S, hq_r, hkv_r)
            assert need % 256 == 0 and live <= need <= live + 2 * 256, (case, batch, S, need, live)
            for mode in ("T", "fp32", "resid", "resid_alias"):
                what = (case, batch, S, pad, form, mode)
                got = _fused(desc, hidden, xin, rin, r, pos, start, length, batch, S, dtype, mode, dev, what)
                be = HipBackend(dtype, dev)
                args = (be, T, hidden, hq_r, hkv_r, xin.win, pos, start, length, batch, S)
                if mode in ("T", "fp32"):
                    ref = TC.replay_llama_attn(*args, epilogue=TC.EPI_BIAS_F32 if mode == "fp32" else TC.EPI_BIAS_T)
                else:
                    own = r.clone()
                    ref = TC.replay_llama_attn(*args, epilogue=TC.EPI_BIAS_RESID_T, resid=own, out=own if mode == "resid_alias" else None)
                assert TT._biteq(got, ref), what
                assert [(k[2], k[3]) for k in be.kernels] == [((hq_r + 2 * hkv_r) * 128, hidden), (hidden, hq_r * 128)], be.kernels
                _count(report, f"fused==replay {case}")


# ------------------------------------------------------------------------------------------------ the walk checks 2 - 5 share
_walks = {}


def _walk(geom, dtype, shape, pad, dev):
    """Everything checks 2 - 5 look at, computed once per (geometry, dtype, shape, padding) and left unchanged: the replay of the full
    layer and of every slice with the packed rows after RoPE and the context rows kept (fragment form), the fused fp32 outputs P and
    p_r -- each bit-equal to its replay, so that S is computed from the context rows P and p_r were multiplied from -- and the 16-bit
    terms t_0 (rank 0, _resid) and t_r (T)."""
    key = (geom, dtype, shape, pad)
    if key in _walks:
        return _walks[key]
    hidden, hq, hkv, world = geom
    hq_r, hkv_r = HS.slice_heads(geom)
    L = _layer(geom, dtype, dev)
    batch, S = shape
    x, r, pos, start, length, xin, rin = _inputs(hidden, batch, S, pad, dtype, dev)
    common = (xin.win, pos, start, length, batch, S)
    call = lambda desc, mode, what: _fused(desc, hidden, xin, rin, r, pos, start, length, batch, S, dtype, mode, dev, what)
    Tf, df = L["full"]["frag"]
    rec = HS.Recorder(HipBackend(dtype, dev))
    ref = TC.replay_llama_attn(rec, Tf, hidden, hq, hkv, *common, epilogue=TC.EPI_BIAS_F32)
    P = call(df, "fp32", (geom, "full", shape, pad))
    assert TT._biteq(P, ref), (HS.geom_id(geom), "full layer", shape, pad)
    out = {"x": x, "resid": r, "pos": pos, "start": start, "length": length, "qkv": rec.qkv, "ctx": rec.ctx, "P": P,
           "unsharded": call(df, "resid", (geom, "full resid", shape, pad)), "rank_qkv": [], "rank_ctx": [], "p": [], "t": []}
    for rank in range(world):
        Tr, dr = L["ranks"][rank]["frag"]
        rec = HS.Recorder(HipBackend(dtype, dev))
        ref = TC.replay_llama_attn(rec, Tr, hidden, hq_r, hkv_r, *common, epilogue=TC.EPI_BIAS_F32)
        p = call(dr, "fp32", (geom, rank, shape, pad))
        assert TT._biteq(p, ref), (HS.geom_id(geom), rank, shape, pad)
        out["rank_qkv"].append(rec.qkv), out["rank_ctx"].append(rec.ctx), out["p"].append(p)
        out["t"].append(call(dr, "resid" if rank == 0 else "T", (geom, rank, "term", shape, pad)))
    _walks[key] = out
    return out


def _cases(geom):
    return itertools.product(HS.geom_shapes(geom), HS.PADS)


# ------------------------------------------------------------------------------------------------ check 2
@pytest.mark.parametrize("geom,dtype", GEOM_PARAMS, ids=GEOM_IDS)
def test_a_ranks_heads_do_not_depend_on_the_other_heads_in_the_call(dev, report, geom, dtype):
    """Rank r's packed q/k/v rows after RoPE == the q, k and v column blocks of the full layer's rows, and its context rows == columns
    [r hq_r 128, (r + 1) hq_r 128) of the full layer's context, bit for bit: what makes "sharded equals replicated up to the o_proj
    sum" true.  A failure names the stage that differs."""
    hidden, hq, hkv, world = geom
    key = f"{HS.geom_id(geom)} {DT_ID[dtype]}"
    for shape, pad in _cases(geom):
        wk = _walk(geom, dtype, shape, pad, dev)
        for rank in range(world):
            blk = HS.column_blocks(hq, hkv, world, rank)
            mine, at = wk["rank_qkv"][rank], 0
            for name in "qkv":
                lo, hi = blk[name]
                assert TT._biteq(mine[:, at:at + hi - lo], wk["qkv"][:, lo:hi]), \
                    (key, shape, pad, rank, f"the {name} block differs: the q/k/v GEMM at N = {mine.shape[1]}" + (" or RoPE" if name != "v" else ""))
                at += hi - lo
            lo, hi = blk["ctx"]
            assert TT._biteq(wk["rank_ctx"][rank], wk["ctx"][:, lo:hi]), (key, shape, pad, rank, "the context rows differ: the attention kernel")
            _count(report, f"slice==full-layer columns {key}", 4)


# ------------------------------------------------------------------------------------------------ checks 3 and 4
@pytest.mark.parametrize("geom,dtype", GEOM_PARAMS, ids=GEOM_IDS)
def test_fp32_partials_sum_to_the_full_layers_o_proj(dev, report, geom, dtype):
    """|sum_r p_r (float64) - P| <= e (K_r + 4) S + e (K + 4) S element by element, S = sum_k |ctx_k w_k| in float64 from the device's
    own context rows and the T-rounded W_o."""
    hidden, hq, hkv, world = geom
    hq_r, _ = HS.slice_heads(geom)
    key = f"{HS.geom_id(geom)} {DT_ID[dtype]}"
    wo_t = _layer(geom, dtype, dev)["wo_t"]
    worst = 0.0
    for shape, pad in _cases(geom):
        wk = _walk(geom, dtype, shape, pad, dev)
        S = HS.abs_products(wk["ctx"], wo_t)
        ratio = HS.worst_ratio(HS.float64_sum(wk["p"]) - wk["P"].double(), HS.partial_sum_bound(S, hq_r * HS.DH, hq * HS.DH))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (key, shape, pad, ratio)
    print(f"\npartials {key}: worst |err| / bound {worst:.3f}")
    _worst(report, "partials", key, worst)


@pytest.mark.parametrize("geom,dtype", GEOM_PARAMS, ids=GEOM_IDS)
def test_the_reduce_in_process(dev, report, geom, dtype):
    """t_0 = the rank-0 _resid output, t_r = the T output of rank r >= 1: t_0 == T(fp32(p_0 + resid)) and t_r == T(p_r) bit for bit,
    and their sum in T on the device in every order (world 8: 0..7, 7..0, one seeded shuffle) lies within
    (world - 1) u A (1 + 2^-6) + (world - 1) g of the float64 sum."""
    key = f"{HS.geom_id(geom)} {DT_ID[dtype]}"
    worst = 0.0
    for shape, pad in _cases(geom):
        wk = _walk(geom, dtype, shape, pad, dev)
        bad = HS.check_terms_are_roundings(wk["t"], wk["p"], wk["resid"], dtype)
        assert not bad, (key, shape, pad, bad)
        ratio = HS.check_reduce(wk["t"], dtype)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (key, shape, pad, ratio)
    print(f"\nreduce {key}: worst |err| / bound {worst:.3f}")
    _worst(report, "reduce", key, worst)


# ------------------------------------------------------------------------------------------------ check 5
@pytest.mark.parametrize("geom,dtype", GEOM_PARAMS, ids=GEOM_IDS)
def test_reduced_layer_vs_oracle(dev, report, geom, dtype):
    """The module's one rel-L2: the terms reduced in rank order, and the unsharded slime_llama_attn_forward_resid, against resid + the
    oracle's FULL layer in float64, right padded, at the project's per-stage tolerance."""
    hidden, hq, hkv, world = geom
    key = f"{HS.geom_id(geom)} {DT_ID[dtype]}"
    shape = HS.REAL_SHAPE if geom == HS.REAL_GEOM else HS.ORACLE_SHAPE
    wk = _walk(geom, dtype, shape, "right", dev)
    ref = HS.oracle_layer(_layer(geom, dtype, dev)["w"], hq, hkv, wk["x"], wk["resid"], wk["pos"], wk["start"], wk["length"], *shape)
    rel = lambda t: float((t.double().cpu() - ref).norm() / ref.norm())
    sharded, unsharded = rel(HS.reduce_in_T(wk["t"], tuple(range(world)))), rel(wk["unsharded"])
    print(f"\n{key}: rel-L2 vs oracle sharded {sharded:.3e} unsharded {unsharded:.3e} (tolerance {HS.TOL[dtype]:.1e})")
    report["rel_l2_sharded"][key], report["rel_l2_unsharded"][key] = sharded, unsharded
    assert sharded < HS.TOL[dtype] and unsharded < HS.TOL[dtype], (key, sharded, unsharded)


# ------------------------------------------------------------------------------------------------ check 6
@pytest.mark.parametrize("world", [2, 4])
def test_head_sharded_attention_ranks_on_one_gpu(world):
    """dist.head_sharded_attention with ops.llama_attention_forward_resid / ops.llama_attention_forward as the local call, every rank
    on cuda:0, gloo between the processes (RCCL refuses two ranks on one device), two stacked layers, both dtypes in one worker run:
    world 2 on (1024, 8, 2), world 4 on (512, 4, 4).  The worker asserts; a failing rank exits non-zero."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29640 + world), os.path.join(HERE, "head_shard_gpu_worker.py")]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout[-1500:])
    assert res.returncode == 0, res.stdout[-3000:]


# ------------------------------------------------------------------------------------------------ check 7
_adapters = {}


def _adapter(dtype, dev):
    """(packed TINY tower, packed GatedBlock, packed post_qformer) of smoke()'s seeds."""
    if dtype not in _adapters:
        from slime_amd import ops, weights as W
        tsd = W.strip_tower_prefix(W.make_tower_state_dict(W.TINY, seed=11))
        asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
        cfg = W.ADAPTER_TINY
        post = ops.pack_resampler(W.sub_state(asd, "sampler.post_qformer."), cfg.mm_hidden_size, cfg.num_heads, W.TINY.num_patches, dtype, dev,
                                  cfg.ln_eps)
        _adapters[dtype] = (ops.pack_tower(tsd, W.TINY, dtype, dev), ops.pack_gated(W.sub_state(asd, "mm_projector."), cfg, dtype, dev), post)
    return _adapters[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("n_images,nw,nh,merge", [(2, 2, 2, True), (2, 2, 2, False), (1, 1, 1, True)],
                         ids=["2x(1+4)-merge", "2x(1+4)-flat", "1x(1+1)-merge"])
def test_adapter_forward_precompressed_equals_adapter_forward(dev, report, n_images, nw, nh, merge, dtype):
    """The adapter of the compressed-local exchange on what sharded_tower_compressed delivers (glob = the global crops' tower features,
    comp = the local crops already through post_qformer, T) == ops.adapter_forward on the same features, bit for bit: the local rows
    (the stacked GEMM's rows are independent, and BIAS_T rounds the fp32 value that the fp32 store followed by the merge's cast
    rounds), and the global rows (both calls take the same GatedBlock form for one PackedGated).  out is exact-sized: shape and dtype
    are checked, for T and for an fp32 out_dtype."""
    from slime_amd import ops, weights as W
    pt, pg, post = _adapter(dtype, dev)
    n_local = nw * nh
    per_image, P, q = 1 + n_local, W.TINY.num_patches, W.ADAPTER_TINY.local_queries
    n = n_images * per_image
    feats = ops.tower_forward(pt, W.synthetic_pixels(n, seed=22).to(dev), out_dtype=dtype)
    assert tuple(feats.shape) == (n, P, W.TINY.hidden_size) and feats.dtype == dtype
    is_g = torch.arange(n, device=dev) % per_image == 0
    glob, local = feats[0::per_image], feats[~is_g]
    comp = ops.resampler_forward(post, local.float(), want_t=True)[1]
    assert tuple(comp.shape) == (n_images * n_local, q, W.TINY.hidden_size) and comp.dtype == dtype
    for out_dtype in (None, torch.float32):
        want = ops.adapter_forward(pg, post, feats, n_images, n_local, nw, nh, merge, -1, out_dtype)
        got = ops.adapter_forward_precompressed(pg, glob, comp, n_images, n_local, nw, nh, merge, -1, out_dtype)
        torch.cuda.synchronize()
        what = (n_images, nw, nh, merge, DT_ID[dtype], out_dtype)
        assert got.dtype == (out_dtype or dtype) and tuple(got.shape) == (n_images, P + n_local * q, W.ADAPTER_TINY.hidden_size), what
        assert got.shape == want.shape and got.dtype == want.dtype, what
        assert bool(torch.isfinite(got.float()).all()), what
        assert TT._biteq(got[:, P:], want[:, P:]), (what, "local rows")
        assert TT._biteq(got[:, :P], want[:, :P]), (what, "global rows")
        _count(report, f"precompressed==adapter_forward {DT_ID[dtype]}", 2)
