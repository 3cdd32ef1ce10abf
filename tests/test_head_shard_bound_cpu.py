"""The test of the head-shard conformance test (tests/head_shard_conformance.py), without a GPU.

``HS.emulate`` restates one head-sharded Llama attention layer in torch: float64 q/k/v, RoPE and attention rounded to T where the
kernels round, an fp32 o_proj per rank, fp32 then T terms, T additions in every order.  At the first four geometries of ``HS.GEOMS``,
both dtypes, (batch, S) = (3, 5) left padded and (2, 65) right padded:

(1) the honest emulation slices as ``shard_llama_attention_weights`` does, its ranks' context rows are the full layer's column blocks,
    and it stays inside every bound of the module: the fp32 partials against the full layer's o_proj (bound 1), the reduction in T in
    every order (bound 2), the terms as roundings of the partials, the whole layer element by element (bound 3) and the rel-L2
    against the oracle (bound 4).
    Measured here, worst |err| / bound over the geometries (bf16 / fp16): bound 1 0.002 / 0.004 (torch's blocked fp32 sums sit far
    inside a bound that holds for any order), bound 2 0.981 / 0.984, bound 3 0.932 / 0.889; rel-L2 against the oracle 2.8e-3 ... 3.6e-3 /
    3.5e-4 ... 4.6e-4.  Bounds 2 and 3 are not slack.
(2) every mutant of ``HS.MUTANTS`` leaves a bound by more than ``HS.MARGIN`` wherever ``HS.mutant_applies`` says it can show (and
    changes nothing where it says it cannot): the two residual mutants bound 3 (bound 2 compares a sum with its own terms and cannot
    see them, which is asserted), the four slice mutants bound 1.
    Measured: the residual on every rank 3.7e2 - 4.4e3 and the residual dropped 3e4 - 1.3e5 times bound 3, the slice mutants
    2.7e3 - 1.3e4 times bound 1.
(3) bound 2 holds, and is nearly met (above 0.9), on terms built so that every addition rounds the same way.
"""
import pytest
import torch

import head_shard_conformance as HS

CASES = (((3, 5), "left"), ((2, 65), "right"))
PARAMS, IDS = HS.geom_params(HS.SMALL_GEOMS)


def _case(geom, dtype, shape, pad):
    hidden = geom[0]
    batch, S = shape
    x, resid, pos = HS.layer_inputs(hidden, batch, S, dtype)
    start, length = HS.kv_ranges(pad, batch, S)
    return x, resid, pos, start, length, batch, S


@pytest.mark.parametrize("geom,dtype", PARAMS, ids=IDS)
def test_honest_emulation_inside_every_bound(geom, dtype):
    hidden, hq, hkv, world = geom
    hq_r, hkv_r = HS.slice_heads(geom)
    w = HS.layer_weights(hidden, hq, hkv)
    wo_t = w[3].to(dtype)
    worst = {"partials": 0.0, "reduce": 0.0, "layer": 0.0, "rel_l2": 0.0}
    for shape, pad in CASES:
        args = _case(geom, dtype, shape, pad)
        x, resid = args[0], args[1]
        em = HS.emulate(geom, dtype, *args)
        # the emulation's slices are the product's
        for r, (wq_r, wk_r, wv_r, wo_r, a, b) in enumerate(HS.rank_slices(w, hq, hkv, world)):
            assert (a, b) == (hq_r, hkv_r)
            blk = HS.column_blocks(hq, hkv, world, r)
            packed = torch.cat(w[:3])
            assert torch.equal(torch.cat([wq_r, wk_r, wv_r]), HS.rows_of_rank(packed.t(), hq, hkv, world, r).t())
            assert torch.equal(wo_r, w[3][:, blk["ctx"][0]:blk["ctx"][1]])
            assert torch.equal(em.ctx[r], em.ctx_full[:, blk["ctx"][0]:blk["ctx"][1]])
        exact = em.ctx_full.double() @ wo_t.double().t()
        # bound (1): both sides against each other, and each against the exact product by its own term
        worst["partials"] = max(worst["partials"], HS.worst_ratio(HS.float64_sum(em.partials) - em.full.double(),
                                                                  HS.partial_sum_bound(em.S, hq_r * HS.DH, hq * HS.DH)))
        assert HS.worst_ratio(em.full.double() - exact, HS.gemm_term1(em.S, hq * HS.DH)) <= 1.0
        assert HS.worst_ratio(HS.float64_sum(em.partials) - exact, HS.gemm_term1(em.S, hq_r * HS.DH)) <= 1.0
        # (c) and bound (2)
        assert not HS.check_terms_are_roundings(em.terms, em.partials, resid, dtype)
        worst["reduce"] = max(worst["reduce"], HS.check_reduce(em.terms, dtype))
        # bound (3), every order
        bd = HS.layer_bound(em.terms, em.S, hq_r * HS.DH, resid, dtype)
        for order in HS.reduce_orders(world):
            got = HS.reduce_in_T(em.terms, order).double()
            worst["layer"] = max(worst["layer"], HS.worst_ratio(got - (resid.double() + exact), bd))
        # bound (4)
        if (shape, pad) == (HS.ORACLE_SHAPE, "right"):
            ref = HS.oracle_layer(w, hq, hkv, *args)
            got = HS.reduce_in_T(em.terms, tuple(range(world))).double()
            worst["rel_l2"] = float((got - ref).norm() / ref.norm())
    print(f"\nhonest emulation {HS.geom_id(geom)} {HS.DT_ID[dtype]}: worst |err| / bound  partials {worst['partials']:.3f}  reduce "
          f"{worst['reduce']:.3f}  layer {worst['layer']:.3f};  rel-L2 vs oracle {worst['rel_l2']:.2e} (tolerance {HS.TOL[dtype]:.1e})")
    assert worst["partials"] <= 1.0 and worst["reduce"] <= 1.0 and worst["layer"] <= 1.0, worst
    assert 0 < worst["rel_l2"] < HS.TOL[dtype], worst


@pytest.mark.parametrize("geom,dtype", PARAMS, ids=IDS)
def test_every_mutant_leaves_a_bound(geom, dtype):
    hidden, hq, hkv, world = geom
    hq_r, _ = HS.slice_heads(geom)
    wo_t = HS.layer_weights(hidden, hq, hkv)[3].to(dtype)
    shape, pad = CASES[1]
    args = _case(geom, dtype, shape, pad)
    resid = args[1]
    print()
    for mutant in HS.MUTANTS:
        if not HS.mutant_applies(mutant, hq, hkv, world):
            honest, wrong = HS.emulate(geom, dtype, *args), HS.emulate(geom, dtype, *args, mutant=mutant)
            assert all(torch.equal(a, b) for a, b in zip(honest.terms, wrong.terms)), f"{mutant} was said not to apply"
            continue
        em = HS.emulate(geom, dtype, *args, mutant=mutant)
        exact = em.ctx_full.double() @ wo_t.double().t()
        if mutant in HS.SLICE_MUTANTS:
            ratio = HS.worst_ratio(HS.float64_sum(em.partials) - em.full.double(), HS.partial_sum_bound(em.S, hq_r * HS.DH, hq * HS.DH))
            which = "bound 1"
        else:
            got = HS.reduce_in_T(em.terms, tuple(range(world))).double()
            ratio = HS.worst_ratio(got - (resid.double() + exact), HS.layer_bound(em.terms, em.S, hq_r * HS.DH, resid, dtype))
            which = "bound 3"
            # what the header says of bound 2: a sum against its own terms does not see a residual too many or too few
            assert HS.check_reduce(em.terms, dtype) <= 1.0
        print(f"{HS.geom_id(geom)} {HS.DT_ID[dtype]} {mutant:26s} leaves {which}: worst |err| / bound = {ratio:.3g}")
        assert ratio > HS.MARGIN, (mutant, which, ratio)


def test_mutant_table_covers_every_mutant():
    """Every mutant applies at one geometry at least, and the one that cannot show at a one-head slice is the only exception."""
    for m in HS.MUTANTS:
        hits = [g for g in HS.SMALL_GEOMS if HS.mutant_applies(m, *g[1:])]
        assert hits, m
        assert len(hits) == len(HS.SMALL_GEOMS) or m == "query_heads_round_robin"


def test_reduce_bound_on_terms_that_round_one_way():
    """Bound (2) where every addition loses in the same direction: 1 and world - 1 terms just below half a spacing of 1 (in the order
    1 first each of them is rounded away whole: the sum in T stays 1 while the float64 sum moves on by nearly (world - 1) u).  The
    bound holds in every order, and the worst order comes within a tenth of it: it is not slack."""
    for dtype in HS.DTYPES:
        u = HS.UNIT[dtype]
        for world in (2, 4, 8):
            small = torch.full((1, 4), u * (1 - 2.0 ** -5)).to(dtype)
            assert float(small[0, 0]) == u * (1 - 2.0 ** -5)
            terms = [torch.ones(1, 4).to(dtype)] + [small] * (world - 1)
            assert bool((HS.reduce_in_T(terms, tuple(range(world))) == 1).all())
            ratio = HS.check_reduce(terms, dtype)
            assert 0.9 < ratio <= 1.0, (dtype, world, ratio)
