"""The test of the cosine router's conformance test (tests/router_conformance.py), without a GPU.

(1) ``emulate_scores`` / ``emulate_scores_batched`` / ``emulate_probs`` -- the torch fp32 restatements of router_text_weight_kernel,
    router_text_dir_kernel, router_scores_kernel and the softmax of router_select_kernel in the kernels' summation order, the stand-ins
    for correct kernels -- stay inside the derived bounds on every element, for every case kind over 20 seeds (the product shape
    H = 4096 over 2), and meet the exact properties (zero image row, no valid text row, masked-out rows of 1e17, exact zeros of the
    softmax).  The worst |err| / bound of each is printed.
(2) Every named defect leaves the bound on the cases NAMED for it: a defect nobody catches, or one caught only somewhere else by
    accident, is a failing test.
(3) Every (T, top-p, temp) of the end-to-end test decides its kept set with at least 16 times the propagated bound to spare, and the
    fp32 emulation reproduces the float64 kept set of the oracle.
(4) The workspace formulas (single: L + H + 4 floats as the header says; batched: 2 B max(ceil4(L), H)) at L > H, L < H, ceil4(L) == H.
"""
import os
import re

import pytest
import torch

import rowwise_conformance as RC
import router_conformance as R

SEEDS = 20


def _cases(seed):
    return list(R.score_cases(seed))


def test_score_emulation_stays_inside_the_bound():
    worst = {}
    for seed in range(SEEDS):
        for c in _cases(seed):
            ratio, msg = R.check_scores(c, R.emulate_scores(c.img, c.text, c.mask))
            assert msg is None, msg
            worst[c.kind] = max(worst.get(c.kind, 0.0), ratio)
    T, L, H = R.PRODUCT_SHAPE
    for seed in range(2):
        for kind in R.SCORE_KINDS:
            for masked in (True, False):
                if masked or kind != "all_masked":
                    c = R.make_score_case(T, L, H, kind, masked, seed=seed)
                    ratio, msg = R.check_scores(c, R.emulate_scores(c.img, c.text, c.mask))
                    assert msg is None, msg
                    worst[kind] = max(worst.get(kind, 0.0), ratio)
    print("\nemulate_scores: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert set(worst) == set(R.SCORE_KINDS) and max(worst.values()) < 1.0


def test_case_builders_build_what_they_name():
    for c in _cases(0):
        valid = torch.arange(c.L) if c.mask is None else c.mask.nonzero().view(-1)
        if c.mask is not None and c.kind != "all_masked":
            assert valid.numel() >= 1 and (c.L == 1 or valid.numel() < c.L or c.kind == "cancelling"), c.what()
        x, y = c.img.double(), c.text.double()
        u = (y[valid] / y[valid].norm(dim=1, keepdim=True).clamp_min(R.EPS)).sum(0)
        if c.kind == "aligned":
            assert abs(float(u.norm()) - valid.numel()) < 1e-5 * valid.numel(), c.what()
        if c.kind == "cancelling" and c.L % 2 == 0:
            assert float(u.norm()) < 1e-6 and valid.numel() >= 2, c.what()
            assert not torch.equal(c.text[0], -c.text[1]) or c.L == 2, "partners are not neighbours"
        if c.kind == "zero_row":
            assert not bool(c.img[c.T // 2].any()), c.what()
        if c.kind == "tiny":
            n = x.norm(dim=1)
            assert float(n[0]) < R.EPS and (c.T < 2 or R.EPS < float(n[1]) < 1e-5), c.what()
            assert float(y[valid[0]].norm()) < R.EPS and (valid.numel() < 2 or R.EPS < float(y[valid[-1]].norm()) < 1e-5), c.what()
        if c.kind == "zero_text_row":
            assert not bool(c.text[valid[-1]].any()), c.what()
        if c.kind == "all_masked":
            assert c.mask is not None and not bool(c.mask.any())
            assert bool((R.emulate_scores(c.img, c.text, c.mask) == 0).all())
            kept = R.router_expected(R.emulate_probs(torch.zeros(c.T), 1.0), 0.5)        # all scores tied: the lowest indices
            assert torch.equal(kept, torch.arange(kept.numel())), c.what()
    shapes = set(R.SCORE_SHAPES)
    assert {t for t, _, _ in shapes} == {1, 4, 5, 7, 37} and {h for _, _, h in shapes} == {4, 128, 256, 260, 1024}
    assert {1, 3, 4, 5, 12} <= {l for _, l, _ in shapes} and (37, 260, 256) in shapes and (5, 125, 128) in shapes and R.ceil4(125) == 128


def test_masked_rows_and_row_order_do_not_matter_to_the_emulation():
    """The exactness properties the GPU test asserts of the kernel, on its stand-in."""
    for c in _cases(1):
        if c.mask is None or c.kind != "random" or c.L < 2:
            continue
        out = c.mask.eq(0).nonzero().view(-1)
        big, zero = c.text.clone(), c.text.clone()
        big[out] = R.BIG
        zero[out] = 0.0
        assert RC.bits_equal(R.emulate_scores(c.img, big, c.mask), R.emulate_scores(c.img, zero, c.mask)), c.what()
        perm = torch.randperm(c.T, generator=torch.Generator().manual_seed(c.T))
        assert RC.bits_equal(R.emulate_scores(c.img[perm], c.text, c.mask), R.emulate_scores(c.img, c.text, c.mask)[perm]), c.what()
        want, bd = R.score_reference(c.img, big, c.mask)
        want0, bd0 = R.score_reference(c.img, zero, c.mask)
        assert torch.equal(want, want0) and torch.equal(bd, bd0), "the reference ignores what a masked-out row holds"


def test_every_score_defect_leaves_the_bound_on_its_named_cases():
    cases = [(c, R.score_reference(c.img, c.text, c.mask)) for c in _cases(0)]
    plain = lambda c: c.kind == "random"
    valid = lambda c: c.L if c.mask is None else int(c.mask.sum())
    must = {"eps_on_the_product_of_the_norms": lambda c: c.kind == "tiny",
            "eps_on_the_squared_norm_root_outside": lambda c: c.kind == "tiny",
            "eps_added_to_the_norm": lambda c: c.kind == "tiny",
            "mean_over_the_valid_count": lambda c: plain(c) and c.mask is not None and valid(c) >= 2,
            "sum_instead_of_mean_without_mask": lambda c: plain(c) and c.mask is None and c.L >= 2,
            "mask_ignored": lambda c: plain(c) and c.mask is not None and c.L >= 2,
            "last_T_mod_4_rows_dropped": lambda c: plain(c) and c.T % 4 != 0,
            "column_tail_H_mod_256_dropped": lambda c: plain(c) and c.H % 256 != 0 and c.H != 128,
            "u_at_ws_plus_L": lambda c: plain(c) and c.L % 4 != 0}
    assert set(must) == set(R.SCORE_MUTANTS)
    for mname, defect in R.SCORE_MUTANTS.items():
        caught = [c.what() for c, ref in cases if R.check_scores(c, R.emulate_scores(c.img, c.text, c.mask, defect), ref)[1]]
        want = [c.what() for c, _ in cases if must[mname](c)]
        print(f"scores {mname:40s} caught by {len(caught)} cases, e.g. {caught[:1]}")
        assert want and all(w in caught for w in want), f"defect {mname}: not caught by {[w for w in want if w not in caught]}"
    # H = 128 has a tail of 128 columns as well: the whole row
    c, ref = next((c, r) for c, r in cases if c.H == 128 and c.kind == "random")
    assert R.check_scores(c, R.emulate_scores(c.img, c.text, c.mask, R.SCORE_MUTANTS["column_tail_H_mod_256_dropped"]), ref)[1]


def _batch_cases():
    for layout in R.BATCH_LAYOUTS:
        for masked in (True, False):
            yield R.make_batch_case(layout, 12, 128, masked)
    yield R.make_batch_case("fused", 260, 128, True)
    yield R.make_batch_case("ragged", 12, 128, True, B=1)


def test_batch_layout_and_the_defect_of_the_batched_entry():
    for bc in _batch_cases():
        if bc.B == 4:
            o, n = bc.row_off, bc.n_rows
            assert 0 in n and o[0] == 0 and o[3] + n[3] == bc.tokens.shape[0] and o[2] < o[3] < o[2] + n[2], bc.name
            if bc.mask is not None:
                assert len({int(v) for v in bc.mask.sum(1)}) == 4, bc.name
        got = R.emulate_scores_batched(bc.tokens, bc.row_off, bc.n_rows, bc.text, bc.mask)
        bad = R.emulate_scores_batched(bc.tokens, bc.row_off, bc.n_rows, bc.text, bc.mask, R.BATCH_MUTANTS["image_b_reads_u_of_image_0"])
        caught = []
        for b in range(bc.B):
            if bc.n_rows[b] == 0:
                continue
            rows = bc.tokens[bc.row_off[b]:bc.row_off[b] + bc.n_rows[b]]
            mb = None if bc.mask is None else bc.mask[b]
            ref = R.score_reference(rows, bc.text[b], mb)
            c = R.ScoreCase(bc.n_rows[b], bc.text.shape[1], bc.text.shape[2], "random", rows, bc.text[b], mb)
            assert R.check_scores(c, got[b], ref)[1] is None, (bc.name, b)
            assert RC.bits_equal(got[b], R.emulate_scores(rows, bc.text[b], mb))
            if R.check_scores(c, bad[b], ref)[1]:
                caught.append(b)
        assert caught == ([2, 3] if bc.B == 4 else []), (bc.name, caught)


def test_probs_emulation_inside_and_defects_outside():
    worst = {}
    for seed in range(SEEDS):
        for T in R.PROB_T:
            for temp in R.PROB_TEMP:
                for kind in R.PROB_KINDS:
                    s = R.prob_scores(T, kind, seed)
                    name = f"probs T={T} temp={temp} {kind}"
                    got = R.emulate_probs(s, temp)
                    ratio, msg = R.check_probs(name, got, s, temp)
                    assert msg is None, msg
                    worst[kind] = max(worst.get(kind, 0.0), ratio)
                    if kind == "spread" and T >= 2:
                        a = R.probs_reference(s, temp)[2]
                        assert float(a.min()) < -104.0 and bool((got[a < -104.0] == 0).all()) and bool((got == 0).any()), name
                        kept = R.router_expected(got, R.TOPP_ALMOST_ONE)
                        assert R.kept_zeros_are_the_lowest(got, kept), name
    print("\nemulate_probs: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) < 1.0
    named = {"softmax_without_the_max_subtraction": [(T, temp, "spread") for T in (2, 1023, 1025, 4096) for temp in R.PROB_TEMP],
             "temperature_after_the_exponent": [(T, temp, "cosine") for T in (2, 1023, 1025, 4096) for temp in (0.3, 2.0)]}
    assert set(named) == set(R.PROB_MUTANTS)
    for mname, defect in R.PROB_MUTANTS.items():
        for T, temp, kind in named[mname]:
            s = R.prob_scores(T, kind, 0)
            assert R.check_probs(mname, R.emulate_probs(s, temp, defect), s, temp)[1], f"defect {mname} stays inside at T={T} temp={temp} {kind}"


@pytest.mark.parametrize("T", R.SEP_T)
def test_separated_scores_decide_the_kept_set_with_margin(T):
    from oracle import slime_oracle as O
    assert set(R.SEP_CASES) == {(t, p, q) for t in R.SEP_T for p, q in R.SEP_PT}
    for topp, temp in R.SEP_PT:
        img, text, mask, want, margin = R.separated_case(T, topp, temp)
        print(f"\nseparated T={T} top-p={topp} temp={temp}: {want.numel()} kept, margin {margin:.1f} x the propagated bound")
        assert margin >= R.MARGIN, (T, topp, temp, margin)
        assert 1 <= want.numel() < T
        s32 = R.emulate_scores(img, text, mask)
        got = R.router_expected(R.emulate_probs(s32, temp), R.f32(topp))
        assert torch.equal(got, want), (T, topp, temp)
        assert torch.equal(O.router_select(O.router_cosine_scores(img, text, mask).double(), topp, temp), want), "the oracle's own fp32 scores decide otherwise"


def test_workspace_formulas():
    assert R.batched_workspace_floats(4, 260, 128) == 2 * 260 * 4            # L > H: the stride comes from L
    assert R.batched_workspace_floats(4, 261, 128) == 2 * 264 * 4
    assert R.batched_workspace_floats(4, 12, 128) == 2 * 128 * 4             # L < H
    assert R.batched_workspace_floats(3, 125, 128) == R.batched_workspace_floats(3, 128, 128) == 2 * 128 * 3    # ceil4(L) == H
    assert R.batched_workspace_floats(0, 12, 128) == R.batched_workspace_floats(1, 0, 128) == 0
    for L, H in ((1, 4), (3, 128), (125, 128), (260, 256), (300, 4096)):
        assert R.ceil4(L) + H <= R.single_workspace_floats(L, H) == L + H + 4
        per = max(R.ceil4(L), H)
        assert per % 4 == 0 and per >= L and per >= H                      # both tables of every image 16-byte aligned and apart
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "slime_hip.h")).read()
    doc = header[header.index("Text-guided router, scores"):header.index("int slime_router_select(")]
    assert re.search(r"L\s*\+\s*H\s*\+\s*4 floats", doc) and "16-byte aligned" in doc and "finite" in doc
    doc_b = header[header.index("Batched router for the B images"):header.index("int slime_router_select_batched(")]
    assert "slime_router_batched_workspace_floats(B, L, H) floats" in doc_b and "16-byte aligned" in doc_b and "finite" in doc_b
