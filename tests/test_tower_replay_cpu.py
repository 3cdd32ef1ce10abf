"""CPU companion of tests/test_gpu_tower_conformance.py: the replays are the reference's arithmetic, the pack-time LayerNorm fold
included (a replay from the packed tensors cannot see a wrong pack), and the chosen cases discriminate.

  * ``replay_vit`` on the float64 backend and the unrounded host tensors (ops.tower_host_tensors(dtype=None)) equals the oracle
    under the forward-error bounds tower_conformance.tower_error_bound derives (no measured constant): every hidden state link by
    link against the oracle's layer functions in float64 (the local bound of one link: this is the check that discriminates), and
    the whole chain against the oracle's chain in float64 and against oracle.tower_forward as it stands, in fp32 (the running bound,
    which grows by three to four orders of magnitude per layer because every step passes an error with its worst case);
  * every deliberately broken variant of the glue and of the fold (tower_conformance.BROKEN) breaks a link by more than FACTOR
    times its bound wherever ``applies`` says it can show, changes nothing where it says it cannot, and shows somewhere;
  * the ROUNDED fold (bf16 / fp16 host tensors) on a constant row, where the consumer's formula must return b' up to the fp32
    roundings of colsum and b': the shipped fold does, the colsum of the unrounded W' misses by the factor c rstd ~ 2^15 and more;
  * ``replay_llama_attn`` on the float64 backend equals oracle/prefill_oracle.py's attention at a GQA shape, without padding, right
    padded and left padded.
"""
import pytest
import torch

import tower_conformance as TC

FACTOR = 1e6                       # a broken variant's distance from the shipped replay, in units of the float64 bound
# the two variants that exist only where something is rounded move a row by a fraction of ulp_T(h) ~ 2^-9 |h| (bf16): thirteen orders
# of magnitude above 2^-53 |h|, of which a link's bound -- gamma_K times sums of |x| |W|, through three Linear steps and the
# attention's worst case -- takes up to ten
FACTOR_ROUNDED = 1e3
GEOMS = {"56_14_128": (56, 14, 128, 256), "112_16_256": (112, 16, 256, 1024)}          # image, patch, D, inter
LAYERS, N_CROPS = 3, 2
SELECT = (0, 1, -2, -1)
_cache = {}


def case(name):
    """(cfg, fp32 state dict, pixels, {layers_run: unrounded host tensors}) of a geometry, built once."""
    if name not in _cache:
        from slime_amd import weights as W
        image, patch, D, inter = GEOMS[name]
        cfg = TC.tower_config(image, patch, D, inter, LAYERS)
        sd = TC.tower_state(cfg)
        px = W.synthetic_pixels(N_CROPS, seed=22, image_size=image)
        _cache[name] = (cfg, sd, px, {})
    return _cache[name]


def host(name, layers_run, dtype=None, variant=None):
    cfg, sd, _, memo = case(name)
    key = (layers_run, dtype, variant)
    if key not in memo:
        memo[key] = TC.host_tensors(sd, cfg, dtype, layers_run, variant)
    return memo[key]


def bounds(name, layers_run, u_ref=TC.U64):
    """The running bound of the whole chain (tower_conformance.tower_error_bound without ``states``)."""
    cfg, sd, px, memo = case(name)
    key = ("bound", layers_run, u_ref)
    if key not in memo:
        memo[key] = TC.tower_error_bound(sd, host(name, layers_run), cfg, px, layers_run, u_ref)
    return memo[key]


def replay(name, layers_run, dtype=None, variant=None, **kw):
    cfg, _, px, _ = case(name)
    fold = variant if variant in TC.FOLD_BROKEN else None
    glue = variant if variant in TC.GLUE_BROKEN else None
    return TC.replay_vit(TC.TorchBackend(dtype), host(name, layers_run, dtype, fold), cfg, px, layers_run, want_hidden=True, want_states=True,
                         broken=glue, **kw)


def excess(got, want, bound):
    """max |got - want| / bound; inf where got is missing or not finite."""
    if got is None or not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound).max())


def oracle64(name):
    """The oracle's own functions on float64 tensors (clip_hidden_states itself casts the pixels to fp32): (embed(), layer(i, h))."""
    from oracle import slime_oracle as O
    cfg, sd, px, memo = case(name)
    if "sd64" not in memo:
        memo["sd64"] = {k: v.double() for k, v in sd.items()}
    sd64, D, S = memo["sd64"], cfg.hidden_size, cfg.seq_len
    embed = lambda: O._ln(O.clip_embeddings(sd64, px.double(), cfg.patch_size), sd64["pre_layrnorm.weight"], sd64["pre_layrnorm.bias"],
                          cfg.layer_norm_eps).reshape(-1, D)
    layer = lambda i, h: O.clip_encoder_layer(sd64, i, h.view(-1, S, D), cfg.num_attention_heads, cfg.layer_norm_eps).reshape(-1, D)
    return embed, layer


def link_excess(name, layers_run, res):
    """The replay held link by link: max over the states of |state[0] - oracle's embeddings| and |state[i + 1] - oracle's layer i
    applied to state[i]|, each in units of its LOCAL bound (the replay's and the reference's rounding of that one link, no input
    error), and inf where ``hidden`` is not the last state or ``out`` not ``hidden`` without the class token."""
    cfg, sd, px, _ = case(name)
    D, S = cfg.hidden_size, cfg.seq_len
    st = res["states"]
    if any(x is None or not bool(torch.isfinite(x).all()) for x in st):
        return float("inf")
    if not torch.equal(res["hidden"], st[layers_run]) or not torch.equal(res["out"], res["hidden"].view(-1, S, D)[:, 1:].reshape(-1, D)):
        return float("inf")
    embed, layer = oracle64(name)
    local = TC.tower_error_bound(sd, host(name, layers_run), cfg, px, layers_run, TC.U64, states=st)
    worst = excess(st[0], embed(), local[0])
    for i in range(layers_run):
        worst = max(worst, excess(st[i + 1], layer(i, st[i]), local[i + 1]))
    return worst


@pytest.mark.parametrize("select_layer", SELECT)
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_float64_replay_vs_oracle(name, select_layer):
    """The float64 replay on the unrounded host tensors against the oracle:
      * every hidden state link by link (``link_excess``: the oracle's layer functions in float64, the local bound);
      * every hidden state of the whole chain against the oracle's chain in float64, and ``out`` with and without the class token
        against oracle.tower_forward as it stands (fp32), under the running bound at 2^-53 + 2^-53 and 2^-53 + 2^-24."""
    from oracle import slime_oracle as O
    from slime_amd import ops
    cfg, sd, px, _ = case(name)
    L = ops.layers_for_select(cfg, select_layer)
    D, S = cfg.hidden_size, cfg.seq_len
    res = replay(name, L)
    assert len(res["states"]) == L + 1
    link = link_excess(name, L, res)
    assert link <= 1.0, (name, select_layer, link)
    embed, layer = oracle64(name)
    ref, bd = embed(), bounds(name, L)
    chain = excess(res["states"][0], ref, bd[0])
    for i in range(L):
        ref = layer(i, ref)
        chain = max(chain, excess(res["states"][i + 1], ref, bd[i + 1]))
    assert chain <= 1.0, (name, select_layer, chain)
    keep = replay(name, L, keep_cls=1)["out"]
    assert torch.equal(keep, res["hidden"])
    bd32 = bounds(name, L, TC.U32)[L].view(-1, S, D)
    for feature, got in (("patch", res["out"]), ("cls_patch", keep)):
        want = O.tower_forward(sd, cfg, px, select_layer, feature).double()
        b = bd32[:, 1:] if feature == "patch" else bd32
        x32 = excess(got.view(want.shape), want, b)
        assert x32 <= 1.0, (name, select_layer, feature, x32)
    print(f"\n{name} select_layer {select_layer}: |replay - oracle| / bound: link by link {link:.3g}, float64 chain {chain:.3g}, "
          f"fp32 tower_forward {x32:.3g}")


def test_fold_restatement_is_the_shipped_fold():
    """tower_conformance.fold_variant(None) is ops.fold_ln bit for bit, rounded and unrounded: the variants differ from what ships by
    their named defect alone."""
    for name in sorted(GEOMS):
        for dtype in (None,) + TC.DTYPES:
            a, b = host(name, LAYERS, dtype), TC.host_tensors(case(name)[1], case(name)[0], dtype, LAYERS, "none")
            assert a.keys() == b.keys()
            for k in a:
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (name, dtype, k)


def test_every_broken_variant_exceeds_the_bound():
    """Each wrong variant breaks a link of the float64 replay by more than FACTOR times that link's bound (``link_excess``) wherever
    ``applies`` says it can show, changes nothing where it says it cannot, and every variant shows at one case at least.  The two
    variants that need a rounding backend (a lower part that is not zero, a W' that differs from its rounded image) are measured on
    TorchBackend(bf16): their distance from the shipped replay on the same backend, in units of the last link's float64 bound, and
    FACTOR_ROUNDED."""
    rounded_only = ("ldlo_in_elements_of_T", "colsum_of_unrounded_w")
    seen = {b: 0 for b in TC.BROKEN}
    for name in sorted(GEOMS):
        cfg, sd, px, _ = case(name)
        for L in (0, 1, 3):
            good = replay(name, L)
            assert link_excess(name, L, good) <= 1.0
            for b in TC.BROKEN:
                if b in rounded_only:
                    continue
                bad = replay(name, L, None, b)
                if TC.applies(b, layers_run=L, n=N_CROPS, keep_cls=0, want_out=True, want_states=True, rounded=False):
                    x = link_excess(name, L, bad)
                    assert x > FACTOR, (name, L, b, x)
                    seen[b] += 1
                else:                                        # excluded by the case: it must indeed change nothing
                    assert torch.equal(bad["hidden"], good["hidden"]) and torch.equal(bad["out"], good["out"]), (name, L, b)
            if L == 0:
                continue
            local = TC.tower_error_bound(sd, host(name, L), cfg, px, L, TC.U64, states=good["states"])[L]
            good16 = replay(name, L, torch.bfloat16)
            for b in rounded_only:
                assert TC.applies(b, layers_run=L, n=N_CROPS, rounded=True) and not TC.applies(b, layers_run=L, n=N_CROPS, rounded=False)
                x = excess(replay(name, L, torch.bfloat16, b)["hidden"], good16["hidden"], local)
                assert x > FACTOR_ROUNDED, (name, L, b, x)
                seen[b] += 1
    assert all(seen.values()), seen


def test_unrounded_variants_that_cannot_show_are_identical():
    """``applies`` excludes the two rounding-only variants from the float64 backend for a reason: there they are the shipped replay."""
    for b in ("ldlo_in_elements_of_T", "colsum_of_unrounded_w"):
        good, bad = replay("56_14_128", 3), replay("56_14_128", 3, None, b)
        for i in range(4):
            assert torch.equal(good["states"][i], bad["states"][i]), b


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=TC.DT_ID.get)
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_rounded_fold_on_a_constant_row(name, dtype):
    """Row x = c 1 with c = 128: mu = c, var = 0, rstd = eps^-1/2, LayerNorm(x) = beta, so the consumer must return b' = (b + W beta)
    rowscale.  Its formula (include/slime_hip.h) in float64 on the ROUNDED host tensors gives
        y_n = rstd (c S_n - c colsum_n) + b'_n,   S_n = sum_k W'[n, k] exactly (float64 sums of K <= 256 16-bit numbers: error
                                                   gamma_K 2^-53 sum |W'|, carried below),
    and colsum_n = fl32(S_n), b'_n = fl32(b'exact_n), so
        |y_n - b'exact_n| <= rstd c 2^-24 |S_n| + 2^-24 |b'exact_n| + rstd c gamma_{K+2}(2^-53) sum_k |W'[n, k]|.
    The colsum of the UNROUNDED W' differs from S_n by the sum of W''s rounding errors, ~ sqrt(K) 2^-9 |w| instead of 2^-24 |S_n|: it
    misses the bound by about 2^15.  Checked for both folded GEMMs of every layer."""
    cfg, sd, _, _ = case(name)
    D, eps, c = cfg.hidden_size, cfg.layer_norm_eps, 128.0
    rstd = eps ** -0.5
    exact = host(name, LAYERS, None)

    def worst(T):
        w = 0.0
        for wn, bn, cn in (("w_qkv", "b_qkv", "colsum_qkv"), ("w_fc1", "b_fc1", "colsum_fc1")):
            for l in range(LAYERS):
                Wp, cs, bp = T[wn][l].double(), T[cn][l].double(), T[bn][l].double()
                assert T[wn][l].dtype == dtype and T[cn][l].dtype == T[bn][l].dtype == torch.float32
                S_n = Wp.sum(1)
                y = rstd * (c * S_n - c * cs) + bp
                b_exact = exact[bn][l]
                bound = rstd * c * TC.U32 * S_n.abs() + TC.U32 * b_exact.abs() + rstd * c * TC._gam(D + 2, TC.U64) * Wp.abs().sum(1)
                w = max(w, float(((y - b_exact).abs() / bound).max()))
        return w

    shipped, variant = worst(host(name, LAYERS, dtype)), worst(host(name, LAYERS, dtype, "colsum_of_unrounded_w"))
    print(f"\nrounded fold {name} {TC.DT_ID[dtype]}: |y - b'| / bound: shipped {shipped:.3g}, colsum of the unrounded W' {variant:.3g}")
    assert shipped <= 1.0, shipped
    assert variant > 2.0 ** 10, variant


PADS = {"none": None, "right": [[1, 1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1, 1]], "left": [[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1]]}


@pytest.mark.parametrize("pad", sorted(PADS))
def test_float64_llama_replay_vs_oracle(pad):
    """replay_llama_attn in float64 against oracle.prefill_oracle.llama_attention_forward on float64 operands: hidden 256, 4 query
    heads on 2 kv heads, batch 2, S = 7, position ids with a per-row offset; the k / v column swap exceeds the bound by FACTOR."""
    from oracle import prefill_oracle as P
    from slime_amd import ops
    D, HQ, HKV, B, S = 256, 4, 2, 2, 7
    g = torch.Generator().manual_seed(31)
    wq, wk, wv, wo = (torch.randn(n, k, generator=g, dtype=torch.float64) * k ** -0.5
                      for n, k in ((HQ * 128, D), (HKV * 128, D), (HKV * 128, D), (D, HQ * 128)))
    x = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    pos = torch.arange(S)[None] + torch.tensor([[3], [11]])
    mask = None if PADS[pad] is None else torch.tensor(PADS[pad])
    start, length = ops.token_ranges(mask) if mask is not None else (None, None)
    inv = ops.llama_inv_freq(128, 500000.0)
    T = {"w_qkv": torch.cat([wq, wk, wv]), "w_o": wo, "inv_freq": inv}
    args = (T, D, HQ, HKV, x.view(B * S, D), pos.reshape(-1).to(torch.int32), start, length, B, S)
    got = TC.replay_llama_attn(TC.TorchBackend(None), *args, epilogue=TC.EPI_BIAS_F32)
    want = P.llama_attention_forward(x, wq, wk, wv, wo, HQ, HKV, pos, mask, head_dim=128).view(B * S, D)
    bound = TC.llama_error_bound(wq, wk, wv, wo, x, pos, HQ, HKV, start, length, inv).view(B * S, D)
    if mask is not None:
        dead = ~mask.bool().view(-1)
        assert bool((got[dead] == 0).all()) and bool((want[dead] == 0).all())
        live = ~dead
    else:
        live = torch.ones(B * S, dtype=torch.bool)
    x_ = excess(got[live], want[live], bound[live])
    print(f"\nllama {pad}: |replay - oracle| / bound {x_:.3g}")
    assert x_ <= 1.0, x_
    bad = TC.replay_llama_attn(TC.TorchBackend(None), *args, epilogue=TC.EPI_BIAS_F32, broken="kv_columns_swapped")
    assert excess(bad[live], got[live], bound[live]) > FACTOR
    res = TC.replay_llama_attn(TC.TorchBackend(None), *args, epilogue=TC.EPI_BIAS_RESID_T, resid=x.view(B * S, D))
    assert torch.equal(res, got + x.view(B * S, D))
