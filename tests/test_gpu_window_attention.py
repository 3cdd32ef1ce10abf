"""Sliding-window prefill attention on the GPU: ``slime_prefill_attention_window`` element by element against the float64
reference and the derived bound (window_attention_conformance.py; the bound's own test, with the wrong windows that must leave
it, is test_window_attention_cpu.py), the bit-level promises of the two new entries, and ``HipMistralAttention`` / the patched HF
Mistral and Mixtral models against the stock HF forward.

Every element-wise case lives in attention_conformance's padded buffers (guard rows and columns NaN or finite attractors,
alternating from case to case; padding-token rows of a sequence always attractors; o pre-filled with a sentinel).

Which kernel runs: 0 < W < S takes the windowed instantiation of the kernel the unwindowed call takes -- ``prefill32_kernel<BF16, 6,
true>`` for the group-4 bf16 geometry (Mistral-7B, Mixtral), ``prefill_attn_kernel<T, true>`` (eight waves) for every other group and
for fp16; W = 0 and W >= S take the unwindowed kernels.  The library does not report the kernel it launched, so the name is stated
here and not asserted; the bit-level tests below hold the W = 0 / W >= S half of it.
"""
import copy

import pytest
import torch

import attention_conformance as AC
import window_attention_conformance as WC

pytestmark = pytest.mark.gpu

DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}
TOL = {torch.float16: 3e-3, torch.bfloat16: 1.5e-2}          # test_gpu_prefill.py's: rel-L2 of the sub-layer; worst token row < 6 x


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(c, window, entry="window"):
    """o (padded, sentinel-filled) after slime_prefill_attention_window(window) -- or, entry "plain", slime_prefill_attention."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    rq, rk = c.H * c.dh + AC.PAD_COLS, c.HKV * c.dh + AC.PAD_COLS
    S = c.n_q
    o = c.new_output()
    start, length = (None, None) if c.ranges is None else (c.ranges[0].data_ptr(), c.ranges[1].data_ptr())
    head = (c.qbuf.data_ptr(), (S + AC.PAD_ROWS) * rq, rq, c.kbuf.data_ptr(), (S + AC.PAD_ROWS) * rk, rk, c.vbuf.data_ptr(),
            (S + AC.PAD_ROWS) * rk, rk, o.data_ptr(), (S + AC.PAD_ROWS) * rq, rq, c.B, c.H, c.HKV, c.dh, S, start, length,
            ops.dtype_code(c.dtype))
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "plain":
        _lib.check(lib.slime_prefill_attention(*head, stream), "slime_prefill_attention")
    else:
        _lib.check(lib.slime_prefill_attention_window(*head, window, stream), "slime_prefill_attention_window")
    torch.cuda.synchronize()
    return o


def _verify(c, W, o, what):
    win, intact = c.check_output(o)
    r = WC.reference(c, W)
    assert torch.isfinite(win.float()).all(), AC.describe_failure(what + ": non-finite output", win, r, c.dtype)
    ratio, ex, idx, g, w = AC.worst(win, r, c.dtype)
    assert ex <= 0, AC.describe_failure(what, win, r, c.dtype)
    assert intact, what + ": an element of o outside the S x E window was written"
    return ratio


def _walk(dev, dtype, group, S, cases, HKV=2):
    worst = 0.0
    for n, (W, kind, B, seed) in enumerate(cases):
        guard = ("nan", "attract")[n % 2]
        c = WC.build(dtype, group, S, W, kind, B, seed, device=dev, guard=guard, HKV=HKV)
        what = f"slime_prefill_attention_window {DT_ID[dtype]} heads {c.H}/{c.HKV} S={S} W={W} ranges={kind} guard={guard}"
        worst = max(worst, _verify(c, W, _launch(c, W), what))
    print(f"{DT_ID[dtype]} group {group} S={S}: {n + 1} cases, worst |err| / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("dtype,group,S", [pytest.param(dt, g, S, id=f"{DT_ID[dt]}-group{g}-S{S}")
                                           for dt in (torch.bfloat16, torch.float16) for g in WC.EIGHT_WAVE_GROUPS[dt] for S in WC.EIGHT_WAVE_S])
def test_window_eight_wave_elementwise(dev, dtype, group, S):
    """Groups 1, 2, 4 (fp16), 8, 16 x both types; S in {1, 31, 33, 200, 257, 449}; every W of {1, 2, 31, 32, 33, 64, 191, 192, 193,
    256, S - 1} below S plus one at or above it; no token ranges, a left-padded, a right-padded sequence and a ragged batch of
    three.  With W small against QB = 256 / group most rows of a block have met no live key for most of their steps."""
    _walk(dev, dtype, group, S, WC.eight_wave_cases(dtype, group, S))


@pytest.mark.parametrize("S", WC.PREFILL32_S)
def test_window_group4_bf16_elementwise(dev, S):
    """The Mistral / Llama-3 geometry (bf16, group 4): S in {64, 65, 300, 600}, W in {1, 17, 32, 33, 64, 65, 96, 97, 255, 256, 257,
    300} -- for 64-row items: leading edges of one, two and three 32-key steps, odd and even step counts, windows longer than
    eight steps -- and the same token ranges.  Served by prefill32_kernel's windowed instantiation (module docstring)."""
    _walk(dev, torch.bfloat16, 4, S, WC.prefill32_cases(S))


def test_window_group4_bf16_more_items_than_workgroups(dev):
    """8 kv heads x batch 4 x S = 600: 320 64-row items, more than there are compute units, at W = 97 (three leading steps)
    and W = 256, one call without token ranges and one with four different ones."""
    for W, ranged in WC.MANY_ITEMS:
        c = WC.build_many_items(W, ranged, device=dev)
        ratio = _verify(c, W, _launch(c, W), f"320 items, W={W}, ranges={'yes' if ranged else 'no'}")
        print(f"bf16 32/8 heads B=4 S=600 W={W}: worst |err| / bound {ratio:.3f}")


def test_window_group4_bf16_rows_that_start_late_with_low_scores(dev):
    """Every logit shifted by -300 log2 units (column 0 of every query row set to 1, column 0 of every key row -300 lower): the
    softmax does not change, but a row whose window opens behind the item's first step -- it has seen no live key when the item's
    reference was taken -- must take its reference from the step it starts in; against a reference of 0 every P would underflow.
    W = 32, 64, 96 and 256 are the boundary: an item starts on a multiple of 64, so with W a multiple of 32 its last row's first
    visible key is the FIRST key of a step (W = 32, q_lo = 64: row 127 sees keys 96..127, step 3, two steps behind t_first)
    and the row starts in the last of the leading steps -- as with 4096, the Mistral default."""
    S = 300
    for W, kind in ((17, "none"), (97, "left"), (33, "ragged3"), (32, "none"), (64, "none"), (96, "none"), (256, "none"), (32, "left"),
                    (96, "ragged3")):
        c = WC.build(torch.bfloat16, 4, S, W, kind, 3 if kind == "ragged3" else 1, 300 + W, device=dev, guard="attract")
        c.view(c.qbuf, c.H)[:, :S, :, 0] = 1.0               # the edge-aligned rows too: an item's last row is always one of them
        c.view(c.kbuf, c.HKV)[:, :S, :, 0] -= 300.0
        ratio = _verify(c, W, _launch(c, W), f"logits - 300, S={S} W={W} ranges={kind}")
        print(f"bf16 group 4 S={S} W={W} {kind}, logits - 300: worst |err| / bound {ratio:.3f}")


# ------------------------------------------------------------------------------------------------ bit-level
BIT_GEOMETRIES = [pytest.param(torch.float16, 2, id="eight-wave-fp16-group2"), pytest.param(torch.bfloat16, 8, id="eight-wave-bf16-group8"),
                  pytest.param(torch.bfloat16, 4, id="prefill32-bf16-group4")]


@pytest.mark.parametrize("dtype,group", BIT_GEOMETRIES)
def test_window_zero_and_window_at_least_S_are_the_existing_entry_in_bits(dev, dtype, group):
    S = 300
    for kind in ("none", "ragged3"):
        c = WC.build(dtype, group, S, S - 1, kind, 3 if kind == "ragged3" else 2, 11, device=dev)      # key 0 heavy in the last row
        want = _launch(c, 0, entry="plain").view(torch.int16)
        for W in (0, S, S + 5):
            assert torch.equal(_launch(c, W).view(torch.int16), want), f"window={W}, ranges={kind}"
        if kind == "none":                 # (in the ragged batch no sequence is S tokens long: S - 1 hides nothing there)
            assert not torch.equal(_launch(c, S - 1).view(torch.int16), want), "the largest real window hides key 0 from the last row"


@pytest.mark.parametrize("dtype,group", BIT_GEOMETRIES)
def test_window_runs_and_batch_entries_are_bit_equal(dev, dtype, group):
    """Two runs of a windowed call agree in bits, and a ragged batch of three equals its three single calls."""
    S, W = 449, 33
    c = WC.build(dtype, group, S, W, "ragged3", 3, 5, device=dev)
    a = _launch(c, W)
    b = _launch(c, W)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for i in range(3):
        one = _launch(c.batch_slice(i, i + 1), W)
        assert torch.equal(one.view(torch.int16), a[i:i + 1].view(torch.int16)), f"batch entry {i}"


@pytest.mark.parametrize("dtype,group", BIT_GEOMETRIES)
def test_rows_in_front_of_the_window_equal_the_unwindowed_call(dev, dtype, group):
    """Query rows i < W see the same keys with and without the window: within the bound of the (shared) reference on every
    geometry.  In bits on the eight-wave kernel, for EVERY row i < W: such a row's workgroup starts at q_lo <= i < W, so its first
    key step is the token range's as without a window; its wave's first row is <= i, so the wave skips no step; the window term of
    the mask is never true for it; and a rescale another row of the wave triggers multiplies it by exp2(0).  For bf16 group 4
    (prefill32_kernel) only the bound is asserted: in the leading steps of an item the windowed instantiation recomputes P on its
    rescale path, which is meant to reproduce the speculative values but is not shown here to do so in bits."""
    S, W = 449, 193
    for kind in ("none", "left"):
        c = WC.build(dtype, group, S, W, kind, 1, 23, device=dev)
        win_o, _ = c.check_output(_launch(c, W))
        plain_o, _ = c.check_output(_launch(c, 0, entry="plain"))
        r = WC.reference(c, W)
        rows = slice(0, W)
        ex = AC.elementwise_excess(plain_o[:, rows], r.out[:, rows], r.A[:, rows], dtype, r.e32[:, rows], r.under[:, rows])
        assert float(ex.max()) <= 0 and float(WC.excess(win_o, r, dtype).max()) <= 0
        if not (dtype == torch.bfloat16 and group == 4):
            assert torch.equal(win_o[:, rows].view(torch.int16), plain_o[:, rows].view(torch.int16)), kind
        assert not torch.equal(win_o[:, W:].view(torch.int16), plain_o[:, W:].view(torch.int16))


def _packed_layer(dev, dtype, D, HQ, HKV, seed, theta=10000.0):
    from slime_amd import ops
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(n, k, generator=g) * k ** -0.5 for n, k in ((HQ * 128, D), (HKV * 128, D), (HKV * 128, D), (D, HQ * 128))]
    return w, ops.pack_llama_attention(*w, HQ, HKV, dtype, dev, theta), g


@pytest.mark.parametrize("dtype,HQ,HKV", [(torch.bfloat16, 8, 2), (torch.float16, 4, 2)], ids=["bf16-group4", "fp16-group2"])
def test_llama_forward_window_equals_forward_and_resid_in_bits(dev, dtype, HQ, HKV):
    """slime_llama_attn_forward_window with window 0, S and S + 5 against slime_llama_attn_forward (T and fp32 output) and
    slime_llama_attn_forward_resid, through ops; a real window differs; a negative one is refused before anything is written."""
    from slime_amd import _lib, ops
    D, B, S = 512, 2, 90
    w, pa, g = _packed_layer(dev, dtype, D, HQ, HKV, 3)
    x = torch.randn(B, S, D, generator=g).to(dtype).to(dev)
    resid = torch.randn(B, S, D, generator=g).to(dtype).to(dev)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[0, :13] = 0
    mask[1, S - 30:] = 0
    mask = mask.to(dev)
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    for out_dtype in (dtype, torch.float32):
        want = ops.llama_attention_forward(pa, x, pos, mask, out_dtype)
        for W in (0, S, S + 5):
            got = ops.llama_attention_forward_window(pa, x, pos, mask, out_dtype, W)
            assert got.dtype == out_dtype and torch.equal(got, want), (out_dtype, W)
        assert not torch.equal(ops.llama_attention_forward_window(pa, x, pos, mask, out_dtype, 7), want)
    want = ops.llama_attention_forward_resid(pa, x, resid, pos, mask)
    for W in (0, S, S + 5):
        assert torch.equal(ops.llama_attention_forward_window(pa, x, pos, mask, dtype, W, resid=resid), want), W
    a = ops.llama_attention_forward_window(pa, x, pos, mask, dtype, 7, resid=resid)
    buf = resid.clone()
    b = ops.llama_attention_forward_window(pa, x, pos, mask, dtype, 7, resid=buf, out=buf)         # in place on the residual stream
    assert b.data_ptr() == buf.data_ptr() and torch.equal(a, b) and not torch.equal(a, want)
    keep = torch.full((B, S, D), 3.0, dtype=dtype, device=dev)
    with pytest.raises(_lib.SlimeHipError, match="window -2"):
        ops.llama_attention_forward_window(pa, x, pos, mask, dtype, -2, out=keep)
    torch.cuda.synchronize()
    assert bool((keep == 3.0).all())


def test_ops_prefill_attention_window(dev):
    """ops.prefill_attention_window on a packed q | k | v buffer against the float64 reference, with a [B, S] mask."""
    from slime_amd import ops
    S, W, HQ, HKV = 130, 40, 4, 2
    c = WC.build(torch.float16, 2, S, W, "ragged3", 3, 77, device=dev, guard="attract")
    q, k, v = c.logical()
    qkv = torch.cat([q.reshape(3, S, -1), k.reshape(3, S, -1), v.reshape(3, S, -1)], -1).contiguous()
    i = torch.arange(S, device=dev)[None]
    mask = ((i >= c.ranges[0][:, None]) & (i < (c.ranges[0] + c.ranges[1])[:, None])).long()
    out = ops.prefill_attention_window(qkv, HQ, HKV, W, mask)
    torch.cuda.synchronize()
    assert float(WC.excess(out.view(3, S, HQ, 128), WC.reference(c, W), torch.float16).max()) <= 0


# ------------------------------------------------------------------------------------------------ layer and model
def _rel(a, b, live):
    err = AC.rel_l2(a[live], b[live])
    worst = float(((a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-6))[live].max())
    return err, worst


def _padded(B, S, padding):
    mask = torch.ones(B, S, dtype=torch.long)
    if padding == "right":
        mask[0, S - 21:] = 0
        mask[1, S - 67:] = 0
    else:
        mask[0, :37] = 0
        mask[1, :5] = 0
    return mask, (mask.cumsum(-1) - 1).clamp(min=0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=DT_ID.get)
@pytest.mark.parametrize("padding", ["left", "right"])
def test_hip_mistral_attention_module_vs_hf(dev, dtype, padding):
    """HipMistralAttention (hidden 512, heads 4 / kv 1, theta 10 000, sliding_window 48, S = 150) against the stock HF
    MistralAttention, fp32, eager, on the CPU, at test_gpu_prefill.py's TOL; the HF pair with and without the window is further
    apart than that, so the case can tell them apart; padded rows are exact zeros."""
    from transformers import MistralConfig
    from transformers.models.mistral import modeling_mistral as M
    from slime_amd.model.language_model import HipMistralAttention
    D, B, S, W = 512, 2, 150, 48
    torch.manual_seed(17)
    mask, pos = _padded(B, S, padding)
    hidden = torch.randn(B, S, D)
    outs = {}
    for sw in (W, None):
        cfg = MistralConfig(hidden_size=D, num_attention_heads=4, num_key_value_heads=1, head_dim=128, intermediate_size=64,
                            num_hidden_layers=1, vocab_size=32, sliding_window=sw, rope_theta=10000.0, attn_implementation="eager")
        torch.manual_seed(18)
        model = M.MistralModel(cfg).eval()
        seen = {}
        h = model.layers[0].self_attn.register_forward_hook(lambda mod, a, kw, out: seen.update(x=kw["hidden_states"], y=out[0]), with_kwargs=True)
        with torch.no_grad():
            model(inputs_embeds=hidden, attention_mask=mask, position_ids=pos, use_cache=False)
        h.remove()
        outs[sw] = (seen["x"].detach(), seen["y"].detach(), model.layers[0].self_attn)
    x, ref, attn = outs[W]
    live = mask.bool()
    assert _rel(outs[None][1], ref, live)[0] > TOL[dtype], "the window must matter at this shape"
    m = HipMistralAttention(D, 4, 1, 128, 10000.0, sliding_window=W, compute_dtype=dtype)
    m.load_state_dict({k: v for k, v in attn.state_dict().items()})
    m.to(dev)
    out, _, _ = m(x.to(dev), attention_mask=mask.to(dev), position_ids=pos.to(dev))
    out = out.cpu()
    err, worst = _rel(out, ref, live)
    print(f"HipMistralAttention {DT_ID[dtype]} {padding}-padded W={W}: rel-L2 {err:.2e}, worst token row {worst:.2e}")
    assert out.dtype == torch.float32 and err < TOL[dtype] and worst < 6 * TOL[dtype]
    assert float(out[~live].abs().max()) == 0.0


@pytest.mark.parametrize("family", ["mistral", "mixtral"])
@pytest.mark.parametrize("padding", ["left", "right"])
def test_patched_attention_inside_hf_mistral_and_mixtral_models(dev, family, padding):
    """replace_{mistral,mixtral}_attn_with_hip_attn inside a stock 2-layer model (hidden 512, heads 4 / kv 1, theta 10 000,
    sliding_window 48, S = 150): the model on the GPU keeps HF's own fp32 norms / MLP / MoE block and its fp32 residual stream --
    the patched attention computes in bf16 and returns fp32 -- against the stock fp32 forward on the CPU at TOL[bf16].  The stock
    pair with and without the window misses that tolerance."""
    import importlib
    import transformers
    from slime_amd.model.language_model import mistral_attention as MA
    M = importlib.import_module(f"transformers.models.{family}.modeling_{family}")
    name = family.capitalize()
    extra = {} if family == "mistral" else {"num_local_experts": 2, "num_experts_per_tok": 2, "experts_implementation": "eager"}
    B, S, W, dtype = 2, 150, 48, torch.bfloat16
    mask, pos = _padded(B, S, padding)
    live = mask.bool()
    refs = {}
    for sw in (W, None):
        cfg = getattr(transformers, name + "Config")(hidden_size=512, num_attention_heads=4, num_key_value_heads=1, head_dim=128,
                                                     intermediate_size=256, num_hidden_layers=2, vocab_size=64, sliding_window=sw,
                                                     rope_theta=10000.0, attn_implementation="eager", **extra)
        torch.manual_seed(29)
        model = getattr(M, name + "Model")(cfg).eval()
        torch.manual_seed(30)
        emb = torch.randn(B, S, 512) * 0.5
        with torch.no_grad():
            refs[sw] = model(inputs_embeds=emb, attention_mask=mask, position_ids=pos, use_cache=False).last_hidden_state
        if sw == W:
            windowed_model = model
    ref = refs[W]
    assert _rel(refs[None], ref, live)[0] > TOL[dtype], "the window must matter at this shape"
    gpu_model = copy.deepcopy(windowed_model).to(dev)
    stock = getattr(M, name + "Attention").forward
    replace, restore = getattr(MA, f"replace_{family}_attn_with_hip_attn"), getattr(MA, f"restore_{family}_attn")
    try:
        replace()
        with torch.no_grad():
            got = gpu_model(inputs_embeds=emb.to(dev), attention_mask=mask.to(dev), position_ids=pos.to(dev), use_cache=False).last_hidden_state
    finally:
        restore()
    assert getattr(M, name + "Attention").forward is stock
    got = got.float().cpu()
    err, worst = _rel(got, ref, live)
    print(f"patched {name}Model ({padding} padding, W={W}) vs stock fp32 CPU forward: rel-L2 {err:.2e}, worst token row {worst:.2e}")
    assert torch.isfinite(got).all() and err < TOL[dtype] and worst < 6 * TOL[dtype]


def test_mistral_7b_slice_full_width_vs_float64_oracle(dev):
    """Mistral-7B's attention sub-layer at full width (hidden 4096, 32 / 8 heads, theta 10 000), one layer, S = 700, W = 256,
    bf16, through HipMistralAttention against the float64 restatement that test_window_attention_cpu.py holds to HF."""
    from slime_amd.model.language_model import HipMistralAttention
    D, HQ, HKV, S, W, dtype = 4096, 32, 8, 700, 256, torch.bfloat16
    g = torch.Generator().manual_seed(41)
    m = HipMistralAttention(D, HQ, HKV, 128, 10000.0, sliding_window=W, compute_dtype=dtype)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * p_.shape[1] ** -0.5)
    w = [getattr(m, n).weight.detach().clone() for n in ("q_proj", "k_proj", "v_proj", "o_proj")]
    hidden = torch.randn(1, S, D, generator=g)
    mask = torch.ones(1, S, dtype=torch.long)
    mask[0, :37] = 0
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    ref = WC.attention_layer_reference(hidden, *w, HQ, HKV, pos, mask, 10000.0, W)
    causal = WC.attention_layer_reference(hidden, *w, HQ, HKV, pos, mask, 10000.0, 0)
    live = mask.bool()
    assert _rel(causal, ref, live)[0] > TOL[dtype], "the window must matter at this shape"
    m.to(dev)
    out, _, _ = m(hidden.to(dev), attention_mask=mask.to(dev), position_ids=pos.to(dev))
    out = out.cpu().double()
    err, worst = _rel(out, ref, live)
    print(f"Mistral-7B slice bf16 S={S} W={W}: rel-L2 {err:.2e}, worst token row {worst:.2e}")
    assert err < TOL[dtype] and worst < 6 * TOL[dtype]
    assert float(out[~live].abs().max()) == 0.0
