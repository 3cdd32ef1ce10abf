"""The test of the row-kernel conformance test (tests/rowwise_conformance.py), without a GPU.

For the front end, slime_layernorm, the gate kernels and slime_rope, in both dtypes and at the small shapes of the GPU module:
(1) ``emulate_*`` -- the torch fp32 restatement of the kernel's arithmetic, the stand-in for a correct kernel -- stays inside the
    derived bound on every element of every output (and meets the bit-equalities: x16, lo8, normalize = 0, RoPE at pos = 0);
(2) every mutant leaves the bound (or a bit-equality) on at least one element of at least one case, and the case that is EXPECTED
    to catch it does: a mutant nobody catches, or one caught only by accident somewhere else, is a failing test;
(3) the LDS table of the geometries equals slime_patch_embed_geometry's formula, and the index arithmetic of the copy references
    (spatial merge, crop selection, grouped scatter) equals a plain-torch restatement.
The worst |err| / bound of each emulation is printed.
"""
import pytest
import torch

import rowwise_conformance as RC

DTYPES = list(RC.DTYPES)
DT_ID = RC.DT_ID


# ------------------------------------------------------------------------------------------------ front end
def _fe_cases(dtype):
    """name -> (sd, geom, px): the small geometries (g = 4, odd g = 7 with kpad == kreal, odd g = 15 with KS = 6, g = 8) x the kinds."""
    out = {}
    for i, geom in enumerate(RC.SMALL_GEOMETRIES):
        for kind in RC.FE_KINDS:
            if kind != "random" and geom.g not in (4, 7):
                continue
            sd, px = RC.fe_inputs(geom, kind, 2, seed=10 * i + len(kind))
            out[f"{geom.name} {kind}"] = (sd, geom, px)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_front_end_emulation_inside_and_mutants_outside(dtype):
    cases = {k: v + (RC.fe_reference(v[0], v[1], v[2], dtype),) for k, v in _fe_cases(dtype).items()}
    worst = {}
    for name, (sd, geom, px, ref) in cases.items():
        if name.endswith("offset"):
            assert RC.fe_mu_over_sigma(ref) >= 10.0, name
        for pix in (px, px.to(dtype)):                                   # T pixels: the same bits
            outs = RC.emulate_fe(sd, geom, pix, dtype)
            ratios, msg = RC.fe_check(ref, outs, dtype)
            assert msg is None, f"{name}: {msg}"
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"\nemulate_fe {DT_ID[dtype]}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) < 1.0
    expected = {"k_ordered_c_kx_ky": "56/14/128 random", "patch_row_r_over_16": "112/16/256 random", "position_row_t_minus_1": "56/14/128 random",
                "class_row_without_position_0": "56/14/128 random", "one_pass_variance": "56/14/128 offset",
                "stats_of_the_unrounded_row": "56/14/128 random", "pixels_not_rounded_to_T": "120/8/128 random"}
    assert set(expected) == set(RC.FE_MUTANTS)
    for mname, defect in RC.FE_MUTANTS.items():
        caught = [name for name, (sd, geom, px, ref) in cases.items() if RC.fe_check(ref, RC.emulate_fe(sd, geom, px, dtype, defect=defect), dtype)[1]]
        print(f"{DT_ID[dtype]} front end {mname:34s} caught by {caught}")
        assert expected[mname] in caught, f"mutant {mname} stays inside the bound on [{expected[mname]}] ({dtype}); caught by {caught}"


def test_geometry_table_matches_the_lds_formula():
    for geom, lds in RC.GEOMETRIES.items():
        assert RC.fe_lds_bytes(geom.image, geom.patch, geom.kpad, geom.D) == lds <= RC.LDS_LIMIT, geom.name
        assert 2 * geom.g <= RC.PE_ROWS and geom.image % 8 == 0 and 6 * geom.patch * geom.image < 65535
    g = {x.name: x for x in RC.GEOMETRIES}
    assert g["112/16/256"].kpad == g["112/16/256"].kreal == 768 and g["120/8/128"].kpad == g["120/8/128"].kreal == 192
    assert g["336/14/1024"].kpad == 640 > g["336/14/1024"].kreal and g["112/16/256"].g == 7 and g["120/8/128"].g == 15
    assert RC.fe_lds_bytes(392, 14, 640, 1024) <= RC.LDS_LIMIT           # 392 / 14 is refused for g = 28, not for its LDS


# ------------------------------------------------------------------------------------------------ slime_layernorm
def _ln_cases(dtype):
    n = 0
    for D in (128, 256, 1024):
        for rows in (1, 3, 4, 5, 9):
            for kind in RC.LN_KINDS:
                n += 1
                ldx = D + (0, 4, 64)[(n // 4) % 3]
                period = (1, 2, rows)[(n + n // 12) % 3]
                yield RC.make_ln_case(D, dtype, rows, ldx, kind, RC.LN_SUBSETS[(n + n // 4) % 4], add_period=period, seed=n)
    for with_add in (False, True):
        yield RC.make_ln_case(256, dtype, 5, 260, "random", ("out_f32", "out_t") + (("out_t2",) if with_add else ()), add_period=2, normalize=False, seed=99)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_layernorm_emulation_inside_and_mutants_outside(dtype):
    cases = [(c, RC.ln_reference(c)) for c in _ln_cases(dtype)]
    worst = {}
    for c, ref in cases:
        ratios, msg = RC.ln_check(c, ref, RC.emulate_ln(c))
        assert msg is None, f"{c.what()}: {msg}"
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\nemulate_ln {DT_ID[dtype]}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert max(worst.values()) < 1.0
    # what must catch: the offset kind through the fp32 output; a period that does not divide the rows; the fp32 output of plain rows
    # (eps / 2 var = 5e-7 of a row of variance 9, against e-sized terms; a constant row has d = 0 and hides any rstd)
    must = {"one_pass_variance": lambda c: c.kind == "offset" and "out_f32" in c.outputs and c.normalize,
            "add_row_modulo_rows": lambda c: "out_t2" in c.outputs and c.add_period == 2 and c.rows in (5, 9) and c.kind == "random",
            "eps_outside_the_square_root": lambda c: c.kind == "random" and "out_f32" in c.outputs and c.normalize}
    assert set(must) == set(RC.LN_MUTANTS)
    for mname, defect in RC.LN_MUTANTS.items():
        caught = [c.what() for c, ref in cases if RC.ln_check(c, ref, RC.emulate_ln(c, defect))[1]]
        want = [c.what() for c, _ in cases if must[mname](c)]
        print(f"{DT_ID[dtype]} layernorm {mname:30s} caught by {len(caught)} cases, e.g. {caught[:1]}")
        assert want and all(w in caught for w in want), f"mutant {mname}: not caught by {[w for w in want if w not in caught]}"


# ------------------------------------------------------------------------------------------------ gates
def _gate_cases():
    n = 0
    for D in (64, 72, 128, 1024):
        for rows in (1, 5, 9):
            for kind in RC.GATE_KINDS:
                n += 1
                x, wg = RC.gate_inputs(D, rows, kind, n, "cpu")
                yield f"D={D} rows={rows} {kind}", kind, x, wg


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_gates_emulation_inside_and_mutants_outside(dtype):
    gen = torch.Generator().manual_seed(5)
    cases = []
    for name, kind, x, wg in _gate_cases():
        rows, H = x.shape[0], 8
        a, b = torch.randn(rows, H, generator=gen), torch.randn(rows, H, generator=gen)
        gts, dg, delta = RC.gate_reference(x, wg)
        if kind == "saturated":
            assert float(delta.min()) > 200.0
        if kind == "equal":
            assert float(delta.max()) == 0.0
        cases.append((name, kind, x, wg, a, b, gts, dg))

    def run(defect):
        """-> {case name: message} over the three consumers: the stored gates, the fp32 / T mix of fp32 rows, the premix of T rows."""
        bad, worst = {}, {}
        for name, kind, x, wg, a, b, gts, dg in cases:
            g32 = RC.emulate_gates(x, wg, defect)
            checks = [("gate_weights", g32, gts, dg)]
            for odt in (torch.float32, dtype):
                y, dy = RC.mix_reference(gts, dg, a, b, odt)
                checks.append((f"gate_mix {DT_ID[odt]}", RC.emulate_mix(g32, a, b, odt), y, dy))
            y, dy = RC.mix_reference(gts, dg, a.to(dtype), b.to(dtype), dtype)
            checks.append(("gate_premix", RC.emulate_mix(g32, a.to(dtype), b.to(dtype), dtype), y, dy))
            for what, got, want, bd in checks:
                ratio, msg = RC.check(what, got, want, bd)
                worst[what] = max(worst.get(what, 0.0), ratio)
                if msg:
                    bad.setdefault(name, msg)
        return bad, worst

    bad, worst = run(RC.GateDefect())
    assert not bad, bad
    print(f"\nemulate_gates {DT_ID[dtype]}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    # the saturated rows see the missing renormalisation (s = 1 exactly, g = 1 / (1 + 1e-6)); random rows the swap; the zero row of the
    # "equal" kind (both logits exactly 0: g = 0.5 / (1 + 1e-6) against 1 / (2 + 1e-6)) the misplaced 1e-6
    expected = {"renormalisation_dropped": "D=64 rows=1 saturated", "gates_swapped": "D=64 rows=5 random",
                "1e-6_inside_the_softmax_denominator": "D=64 rows=1 equal"}
    assert set(expected) == set(RC.GATE_MUTANTS)
    for mname, defect in RC.GATE_MUTANTS.items():
        caught, _ = run(defect)
        print(f"{DT_ID[dtype]} gates {mname:38s} caught by {len(caught)} cases: {list(caught)[:3]}")
        assert expected[mname] in caught, f"mutant {mname} stays inside the bound on [{expected[mname]}]"


# ------------------------------------------------------------------------------------------------ RoPE
def _rope_cases(dtype):
    n = 0
    for n_rot in (1, 3, 10):
        for n_q in sorted({0, 1, n_rot}):
            for extra in (0, 136):
                n += 1
                yield RC.make_rope_case(dtype, n_rot, n_q, 5, extra, [0, 1, 4095, 4096, 131071], seed=n)
                yield RC.make_rope_case(dtype, n_rot, n_q, 1, extra, [RC.ROPE_POS[n % 6]], seed=n + 50)
    yield RC.make_rope_case(dtype, 3, 1, 5, 0, [8191, 4096, 1, 0, 131071], seed=77)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_rope_emulation_inside_and_mutants_outside(dtype):
    cases = list(_rope_cases(dtype))
    worst = 0.0
    for c in cases:
        ratio, msg = RC.rope_check(c, RC.emulate_rope(c))
        assert msg is None, f"{c.what()}: {msg}"
        worst = max(worst, ratio)
    print(f"\nemulate_rope {DT_ID[dtype]}: worst |err| / bound {worst:.3f}")
    assert worst < 1.0
    five = lambda c: c.rows == 5 and c.buf["pos"].win.view(-1).tolist() == [0, 1, 4095, 4096, 131071]
    must = {"cs_of_i_for_element_i_plus_1": five, "q_scale_on_the_k_heads": lambda c: five(c) and c.n_q < c.n_rot,
            "rotate_half_sign_flipped": five, "frequency_index_i_over_2": five, "angle_reduced_as_fp32_revolutions": five}
    assert set(must) == set(RC.ROPE_MUTANTS)
    for mname, defect in RC.ROPE_MUTANTS.items():
        caught = [c.what() for c in cases if RC.rope_check(c, RC.emulate_rope(c, defect))[1]]
        want = [c.what() for c in cases if must[mname](c)]
        print(f"{DT_ID[dtype]} rope {mname:36s} caught by {len(caught)} of {len(cases)} cases")
        assert want and all(w in caught for w in want), f"mutant {mname}: not caught by {[w for w in want if w not in caught]}"


def test_rope_fast_math_angle_leaves_the_fp16_bound_from_4096():
    """The fast-math reduction (fp32 revolutions) is inside the bound at pos <= 1 and outside it, in fp16, at each pos >= 4096."""
    d = RC.ROPE_MUTANTS["angle_reduced_as_fp32_revolutions"]
    for pos in RC.ROPE_POS:
        c = RC.make_rope_case(torch.float16, 10, 3, 1, 0, [pos], seed=pos)
        msg = RC.rope_check(c, RC.emulate_rope(c, d))[1]
        if pos >= 4096:
            assert msg is not None, pos
        if pos <= 1:
            assert msg is None, (pos, msg)


# ------------------------------------------------------------------------------------------------ copies, router expectations
def test_copy_index_arithmetic():
    nw, nh, g, C = 2, 3, 4, 1
    loc = torch.arange(nw * nh * g * g).float().view(-1, C)
    ref = loc.view(nh, nw, g, g, C).permute(0, 2, 1, 3, 4).reshape(-1, C)           # llava_arch's spatial merge
    out = torch.empty_like(loc)
    out[RC.merge_dst(nw, nh, g, True)] = loc
    assert torch.equal(out, ref) and torch.equal(RC.merge_dst(nw, nh, g, False), torch.arange(nw * nh * g * g))
    assert RC.select_crops_index(5, 1, 4, 2).tolist() == [1, 2, 3, 4, 6, 7, 8, 9] and RC.select_crops_index(5, 0, 1, 2).tolist() == [0, 5]
    m, total = RC.scatter_rows(5)
    assert m.tolist() == [2, 3, 4, 9, 10] and total > int(m.max()) + 1


def test_router_expectation_prefers_the_lowest_indices_among_ties():
    p = torch.full((8,), 0.125)
    assert RC.router_expected(p, 0.5).tolist() == [0, 1, 2, 3, 4] and RC.router_expected(p, 1e-4).tolist() == [0]
    for T in RC.ROUTER_T:
        for kind in RC.ROUTER_KINDS:
            assert RC.router_scores(T, kind).shape == (T,)
