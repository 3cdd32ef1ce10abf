"""GPU tests of the attention text-guided router (mm_resampler_type='qformer'): the two new row kernels element-wise against float64
within the bounds derived in router_attention_oracle.py, the scores against the reference's recorded fp32 scores within 1.5 x the
reference's OWN same-dtype drift (tests/golden/router_attention.npz), the selection against the oracle on the device's own scores
(exactly), batched against single calls (bit for bit), one case at the real width, and encode_images end to end on the tiny encoder."""
import pytest
import torch
import torch.nn as nn

import router_attention_oracle as RA
from gemm_conformance import Padded
from router_attention_oracle import CASES, golden, golden_case

pytestmark = pytest.mark.gpu
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
E32 = RA.E32
SENT = 7.0
FACTOR = 1.5                       # the allowance test_gpu_modules.py gives composed 16-bit paths, on the reference's own drift
# test_gpu_path.py's per-stage bounds against the fp32 oracle (fp16 1.2e-3, bf16 8e-3), 1.5 x at the end of the tower -> adapter chain
# (test_gpu_adapter_ragged.py); two paths that each lie within it of the oracle lie within twice it of each other
ADAPTER_TOL = {"fp16": 2 * 1.5 * 1.2e-3, "bf16": 2 * 1.5 * 8e-3}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same_bits(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(bits(got), bits(want)), what


# ------------------------------------------------------------------------------------------------ gathered LayerNorm
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("D", [128, 256, 512, 4096, 5120, 8192])
def test_ln_gather_elementwise_within_the_derived_bound(dev, D, dt):
    from slime_amd import ops
    dtype = DT[dt]
    src, idx, w, b = RA.ln_gather_inputs(D, device=dev)                      # 37 rows; idx repeats, reverses, skips; row 5: |mean| = 1000 sigma
    x5 = src[5].double()
    assert float(x5.mean().abs() / x5.std()) > 500
    out = Padded(idx.numel(), D, dtype, dev, pad_cols=0)
    snap = out.snapshot()
    ops.ln_gather(src, idx, w, b, RA.EPS, out.win)
    torch.cuda.synchronize()
    want, bd = RA.ln_gather_bound(src.double()[idx], w, b, dtype)
    ratio, msg = RA.RC.check(f"ln_gather D={D} {dt}", out.win, want, bd)
    print(f"ln_gather D={D} {dt}: worst |err| / bound {ratio:.3f}")
    assert msg is None, msg
    assert out.intact(snap), "bytes outside the output rows were written"
    # identity form (idx = NULL): the rows in order
    out2 = Padded(src.shape[0], D, dtype, dev, pad_cols=0)
    snap2 = out2.snapshot()
    ops.ln_gather(src, None, w, b, RA.EPS, out2.win)
    torch.cuda.synchronize()
    assert_same_bits(out2.win[idx], out.win, "identity and gathered rows differ")
    assert out2.intact(snap2)


# ------------------------------------------------------------------------------------------------ head and softmax
SEGMENTS = (1, 144, 0, 289)


@pytest.mark.parametrize("N1", [128, 1024])
def test_prob_head_and_segment_softmax(dev, N1):
    from slime_amd import ops
    rows, B, T_max, temp = sum(SEGMENTS), len(SEGMENTS), max(SEGMENTS), 0.7
    h, w2, b2 = RA.head_inputs(N1, rows, device=dev)
    logit = torch.full((rows + 8,), SENT, dtype=torch.float32, device=dev)
    scores = torch.full((B + 1, T_max), SENT, dtype=torch.float32, device=dev)
    ops.router_prob_head(h, w2, b2, SEGMENTS, temp, logit, scores[:B])
    torch.cuda.synchronize()
    want, bd = RA.head_bound(h, w2, b2)
    ratio, msg = RA.RC.check(f"logit N1={N1}", logit[:rows], want, bd)
    print(f"prob head N1={N1}: worst |err| / bound {ratio:.3f}")
    assert msg is None, msg
    assert bool((logit[rows:] == SENT).all()) and bool((scores[B] == SENT).all())
    lg = logit[:rows].cpu()
    ref = RA.segment_softmax(lg, SEGMENTS, temp)                             # float64 softmax of the DEVICE's logits
    for b, n in enumerate(SEGMENTS):
        row = scores[b].cpu()
        assert bool((row[n:] == SENT).all()), f"segment {b}: entries past n_rows = {n} were written"
        if n == 0:
            continue
        got = row[:n].double()
        assert abs(float(got.sum()) - 1.0) <= n * E32, (b, float(got.sum()) - 1.0)
        # l / temp and the subtraction: 3 e max|l / temp| absolute in the exponent, twice (numerator and sum); expf A_EXP e; the sum
        # (n / 256 values per thread, six butterfly levels, four partial sums) and the division
        o = sum(SEGMENTS[:b])
        amax = float(lg[o:o + n].double().abs().max()) / temp
        rel = (2 * RA.RC.A_EXP + 6 * amax + (n + 255) // 256 + 6 + 2 + 2) * E32 * RA.SLACK
        assert float(((got - ref[b]).abs() / ref[b]).max()) <= rel, (b, float(((got - ref[b]).abs() / ref[b]).max()), rel)
    assert float(scores[0, 0]) == 1.0                                         # one token: exactly 1


# ------------------------------------------------------------------------------------------------ scores against the golden
_runs = {}


def _golden_run(dev, name, dt):
    """One device run per (case, dtype), shared by the tests below: (case, device scores [T] on the host, kept indices, count)."""
    from slime_amd import ops
    key = (name, dt)
    if key not in _runs:
        g = golden()
        c = golden_case(g, name)
        topp, temp = float(g["topp"]), float(g["temp"])
        pra = ops.pack_router_attention(c["sd"], c["H"], DT[dt], dev)
        T = c["x"].shape[0]
        st, sc = ops.router_attention_select_batched_device(pra, c["x"].to(dev), [0], [T], c["text"].to(dev).unsqueeze(0), c["mask"].unsqueeze(0),
                                                            topp, temp, want_scores=True)
        torch.cuda.synchronize()
        _runs[key] = (c, sc[0, :T].cpu(), st.keep[0, :st.counts[0]].long().cpu(), topp, temp)
    return _runs[key]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", CASES)
def test_scores_within_the_reference_drift(dev, name, dt):
    c, sc, _, _, _ = _golden_run(dev, name, dt)
    rel, mx = RA.rel_l2(sc, c["scores"]), RA.max_abs(sc, c["scores"])
    d_rel, d_max = c["drift"][dt]
    print(f"{name} {dt}: rel-L2 {rel:.3e} (reference drift {d_rel:.3e}), max-abs {mx:.3e} (reference drift {d_max:.3e})")
    assert bool(torch.isfinite(sc).all())
    assert rel <= FACTOR * d_rel and mx <= FACTOR * d_max


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name", CASES)
def test_selection_is_the_oracle_on_the_device_scores(dev, name, dt):
    c, sc, kept, topp, temp = _golden_run(dev, name, dt)
    want = RA.select_device_order(sc, topp, temp)
    assert 0 < kept.numel() <= sc.numel()
    assert torch.equal(kept, want), (kept.numel(), want.numel())


# ------------------------------------------------------------------------------------------------ batched against single
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_batched_scores_equal_single_calls(dev, dt):
    from slime_amd import ops, weights as W
    H, L, P = 256, 24, 5
    n_rows, off = (288, 0, 144), (P, P + 288 + 3, P + 288 + 3 + P)
    g = torch.Generator().manual_seed(77)
    tokens = torch.randn(off[2] + 144 + 4, H, generator=g).to(dev)
    text = torch.randn(3, L, H, generator=g)
    mask = torch.zeros(3, L, dtype=torch.int64)
    mask[0, :17] = 1                                                         # right padded
    mask[2, L - 9:] = 1                                                      # left padded; image 1 has no token and no key
    text[mask == 0] = 0.0
    pra = ops.pack_router_attention(W.make_router_attention_state_dict(H, seed=3), H, DT[dt], dev)
    st, sc = ops.router_attention_select_batched_device(pra, tokens, off, n_rows, text.to(dev), mask, 0.5, 1.0, want_scores=True)
    torch.cuda.synchronize()
    assert st.counts[1] == 0 and 0 < st.counts[0] < 288 and 0 < st.counts[2] < 144
    for b in (0, 2):
        s1, sc1 = ops.router_attention_select_batched_device(pra, tokens, [off[b]], [n_rows[b]], text[b:b + 1].to(dev), mask[b:b + 1], 0.5, 1.0,
                                                             want_scores=True)
        torch.cuda.synchronize()
        assert_same_bits(sc[b, :n_rows[b]].cpu(), sc1[0, :n_rows[b]].cpu(), f"image {b}")
        assert s1.counts[0] == st.counts[b] and torch.equal(s1.keep[0, :s1.counts[0]].cpu(), st.keep[b, :st.counts[b]].cpu())
        assert torch.equal(st.keep[b, :st.counts[b]].long().cpu(), RA.select_device_order(sc[b, :n_rows[b]].cpu(), 0.5, 1.0))
    with pytest.raises(ValueError, match="no valid text key"):
        ops.router_attention_select_batched_device(pra, tokens, off, (288, 4, 144), text.to(dev), mask, 0.5, 1.0)


# ------------------------------------------------------------------------------------------------ the real width, once
def test_real_width_once(dev):
    """H = 4096 (32 heads, N1 = 1024), T = 144, L = 16, bf16, against the float64 oracle on the T-rounded weights.  Limit: 1.5 x the
    reference's recorded bf16 drift at H = 512, the widest width the golden file holds."""
    from slime_amd import ops, weights as W
    H, T, L = 4096, 144, 16
    sd = W.make_router_attention_state_dict(H, seed=41)
    g = torch.Generator().manual_seed(42)
    x, text = torch.randn(T, H, generator=g).to(dev), torch.randn(L, H, generator=g).to(dev)
    mask = torch.ones(L, dtype=torch.int64)
    mask[11:] = 0
    pra = ops.pack_router_attention(sd, H, torch.bfloat16, dev)
    assert pra.heads == 32 and pra.N1 == 1024
    sc = ops.router_attention_scores(pra, x, [0], [T], text.unsqueeze(0), mask.unsqueeze(0), 1.0)[0].cpu()
    torch.cuda.synchronize()
    use = {k: v.to(dev) for k, v in sd.items() if not k.startswith("self_attn") and k != "query"}
    want = RA.scores(use, x, text, mask.to(dev), 1.0, operand_dtype=torch.bfloat16).cpu()
    d_rel, d_max = golden_case(golden(), "h512_left_pad")["drift"]["bf16"]
    rel, mx = RA.rel_l2(sc, want), RA.max_abs(sc, want)
    print(f"H=4096 bf16: rel-L2 {rel:.3e} (limit {FACTOR * d_rel:.3e}), max-abs {mx:.3e} (limit {FACTOR * d_max:.3e})")
    assert rel <= FACTOR * d_rel and mx <= FACTOR * d_max


# ------------------------------------------------------------------------------------------------ end to end
def _encoder(dev, dtype, embed, kind, **cfg_over):
    """The tiny encoder of test_gpu_modules._tiny_encoder with the router chosen by ``kind``."""
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    from slime_amd.image_processor import ClipImageProcessor
    cfg = default_slime_config("synthetic:1", hidden_size=256, mm_hidden_size=128, mm_resampler_type=kind, **cfg_over)
    enc = SlimeVisualEncoder(cfg, embed_tokens=embed)
    vt = enc.get_vision_tower()
    vt.vision_tower = HipCLIPVisionModel(W.TINY)
    vt.image_processor = ClipImageProcessor()
    vt.is_loaded = True
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    if kind == "qformer":
        asd.update({"sampler.selector." + k: v for k, v in W.make_router_attention_state_dict(256, seed=13).items()})
    enc.load_visual_state(W.make_tower_state_dict(W.TINY, seed=11), asd)
    enc.to(dev)
    vt.vision_tower.to(dtype)
    return enc


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_encode_images_with_the_attention_router(dev, monkeypatch, dt, kind):
    from slime_amd import ops
    from test_gpu_splice_routed import _batch
    dtype = DT[dt]
    embed = nn.Embedding(2048, 256)
    embed.weight.data.copy_(torch.randn(2048, 256, generator=torch.Generator().manual_seed(3)) * 0.5)
    embed.to(dtype)
    counts, sizes, merge, px, ids, am, lab, pos = _batch(kind, dev, dtype)
    images = torch.cat(px, 0)
    enc = _encoder(dev, dtype, embed, "qformer", mm_patch_merge_type=merge)
    cfg, sampler = enc.config, enc.get_model().sampler
    assert sampler.router_type == "qformer"
    seen = []
    real = ops.router_attention_select_batched_device

    def spy(pra, tokens, off, n_rows, text, mask, topp, temp, **kw):
        st, sc = real(pra, tokens, off, n_rows, text, mask, topp, temp, want_scores=True)
        seen.append((pra.dtype, tokens, list(off), list(n_rows), st, sc))
        return st

    monkeypatch.setattr(ops, "router_attention_select_batched_device", spy)
    P = 576
    sep = embed.weight.detach()[int(cfg.seperator)].float().to(dtype)
    for topp, side in ((0.5, "right"), (0.95, "left")):
        sampler.topp, cfg.tokenizer_padding_side = topp, side
        cfg.fused_adapter, cfg.fused_splice = True, False
        del seen[:]
        f_on, _ = enc.encode_images(images, ids, counts, am, None, sizes, labels=lab)
        assert len(seen) == 1
        op_dtype, tokens, off, n_rows, st, sc = seen[0]
        assert op_dtype == dtype                                             # the operand type follows the images
        kept_n = []
        for b in range(len(counts)):
            want_keep = RA.select_device_order(sc[b, :n_rows[b]].cpu(), topp, float(sampler.temp)) if n_rows[b] else torch.zeros(0, dtype=torch.long)
            assert torch.equal(st.keep[b, :st.counts[b]].long().cpu(), want_keep), (topp, side, b)
            want = torch.cat([tokens[off[b] - P:off[b]], sep.float().unsqueeze(0), tokens[off[b]:off[b] + n_rows[b]][want_keep.to(dev)]]).to(dtype)
            assert_same_bits(f_on[b][0].cpu(), want.cpu(), f"{topp} {side} image {b}")
            kept_n.append(int(want_keep.numel()))
        if topp == 0.5:
            assert any(0 < k < n for k, n in zip(kept_n, n_rows)), (kept_n, n_rows)          # the gather is not the identity
        cfg.fused_splice = True
        f_spl, _ = enc.encode_images(images, ids, counts, am, None, sizes, labels=lab)
        for b in range(len(counts)):
            assert_same_bits(f_spl[b].cpu(), f_on[b].cpu(), f"fused_splice, {topp} {side} image {b}")
        # fused adapter off.  The two adapter forms hand over tokens that agree to the adapter's own tolerance, not bit for bit
        # (the module sequence takes the tower's fp32 features, the fused call its T features: the GLOBAL rows, which no router
        # touches, already differ in the last bits), so "on == off" is: the selection is exact on THIS path's own device scores, the
        # routed rows are this path's tokens bit for bit, and the tokens of the two paths agree within ADAPTER_TOL.
        cfg.fused_adapter, cfg.fused_splice = False, False
        f_off, _ = enc.encode_images(images, ids, counts, am, None, sizes, labels=lab)
        assert len(seen) == 3
        _, cat, offs, n_off, st2, sc2 = seen[2]
        assert n_off == n_rows
        for b in range(len(counts)):
            keep2 = RA.select_device_order(sc2[b, :n_off[b]].cpu(), topp, float(sampler.temp)) if n_off[b] else torch.zeros(0, dtype=torch.long)
            assert torch.equal(st2.keep[b, :st2.counts[b]].long().cpu(), keep2), (topp, side, b)
            out = f_off[b][0]
            assert out.shape[0] == P + 1 + keep2.numel()
            assert_same_bits(out[P].cpu(), sep.cpu(), "separator")
            assert_same_bits(out[P + 1:].cpu(), cat[offs[b]:offs[b] + n_off[b]][keep2.to(dev)].to(dtype).cpu(), f"routed rows, image {b}")
            assert RA.rel_l2(out[:P], f_on[b][0][:P]) <= ADAPTER_TOL[dt], "global rows of the two adapter forms"
            if n_off[b]:
                assert RA.rel_l2(cat[offs[b]:offs[b] + n_off[b]], tokens[off[b]:off[b] + n_rows[b]]) <= ADAPTER_TOL[dt], "local tokens"
    # the same batch through the cosine router: [global | sep | local[kept]] with kept from the oracle's selection on the device's
    # cosine scores, as before this router existed
    monkeypatch.setattr(ops, "router_attention_select_batched_device", real)
    cos = _encoder(dev, dtype, embed, "cosine", mm_patch_merge_type=merge)
    assert cos.get_model().sampler.router_type == "cosine" and not hasattr(cos.get_model().sampler, "selector")
    cos.get_model().sampler.topp = 0.5
    cos.config.tokenizer_padding_side = "right"
    f_cos, _ = cos.encode_images(images, ids, counts, am, None, sizes, labels=lab)
    tokens, off, n_rows, P2, st, cnts = cos._fused_route(images, ids, counts, am, None, sizes, lab, False)
    text, tmask = cos.get_pure_text_embedding(ids, am, lab)
    for b in range(len(counts)):
        local = tokens[off[b]:off[b] + n_rows[b]]
        keep = RA.select_device_order(ops.router_scores(local, text[b], tmask[b]).cpu(), 0.5, float(cos.get_model().sampler.temp)) if n_rows[b] \
            else torch.zeros(0, dtype=torch.long)
        want = torch.cat([tokens[off[b] - P:off[b]], sep.float().unsqueeze(0), local[keep.to(dev)]]).to(dtype)
        assert_same_bits(f_cos[b][0].cpu(), want.cpu(), f"cosine image {b}")
