"""Sliding-window prefill attention, the part that needs no GPU: (1) the float64 reference of window_attention_conformance.py
equals HF's own MistralAttention / MixtralAttention (eager, float64) -- that pins the semantics  j <= i, i - j < W, rows not
position ids; (2) the Mistral / Mixtral patches' plumbing with the HIP call replaced by a recorder; (3) the refusals of the two
new C entries, on fake pointers; (4) the emulation of the kernel's arithmetic with the right window stays inside the derived
bound on the GPU tests' cases while every wrong window leaves it, and the inputs make the first excluded key count.
"""
import ctypes as C

import pytest
import torch

import attention_conformance as AC
import window_attention_conformance as WC

DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}


# ------------------------------------------------------------------------------------------------ (1) the oracle against HF
def _hf(family):
    import transformers
    from transformers.models.mistral import modeling_mistral
    from transformers.models.mixtral import modeling_mixtral
    if family == "mistral":
        return transformers.MistralConfig, modeling_mistral.MistralModel, {}
    return transformers.MixtralConfig, modeling_mixtral.MixtralModel, {"num_local_experts": 2, "num_experts_per_tok": 1, "experts_implementation": "eager"}


def _masks(B, S):
    left = torch.ones(B, S, dtype=torch.long)
    left[0, :11] = 0
    left[1, :37] = 0
    right = torch.ones(B, S, dtype=torch.long)
    right[0, S - 21:] = 0
    right[1, S - 3:] = 0
    return {"none": None, "left": left, "right": right}


@pytest.mark.parametrize("family,heads,W", [("mistral", h, w) for h in (2, 4) for w in (1, 8, 33)] + [("mixtral", 2, 8), ("mixtral", 4, 33)])
def test_reference_equals_hf_eager_float64(family, heads, W):
    """One decoder layer of the stock model, float64, attn_implementation="eager", S = 70, kv heads 1, theta 10 000; no mask, a
    left-padded and a right-padded [B, S] mask with position ids counted from the first token (so rows and positions differ).
    The layer's self_attn is observed with a hook; the restatement is fed the same input.  Live rows agree to 1e-8; the
    `<=` window and the causal-only mask are off by far more -- the case can tell them apart."""
    Config, Model, extra = _hf(family)
    B, S, dh = 2, 70, 16
    cfg = Config(hidden_size=heads * dh, num_attention_heads=heads, num_key_value_heads=1, head_dim=dh, intermediate_size=32,
                 num_hidden_layers=1, vocab_size=32, sliding_window=W, rope_theta=10000.0, attn_implementation="eager", **extra)
    torch.manual_seed(heads * 100 + W)
    model = Model(cfg).double().eval()
    seen = {}

    def hook(mod, args, kwargs, output):
        seen["x"] = (kwargs["hidden_states"] if "hidden_states" in kwargs else args[0]).detach()
        seen["y"] = output[0].detach()
    attn = model.layers[0].self_attn
    h = attn.register_forward_hook(hook, with_kwargs=True)
    emb = torch.randn(B, S, heads * dh, dtype=torch.float64) * 3.0
    try:
        for name, mask in _masks(B, S).items():
            pos = None if mask is None else (mask.cumsum(-1) - 1).clamp(min=0)
            with torch.no_grad():
                model(inputs_embeds=emb, attention_mask=mask, position_ids=pos, use_cache=False)
            live = torch.ones(B, S, dtype=torch.bool) if mask is None else mask.bool()
            w = [getattr(attn, n).weight.detach() for n in ("q_proj", "k_proj", "v_proj", "o_proj")]
            errs = {}
            for label, win in (("right", W), ("le", W + 1), ("causal", 0)):
                ref = WC.attention_layer_reference(seen["x"], *w, heads, 1, pos, mask, 10000.0, win)
                errs[label] = float((ref - seen["y"])[live].abs().max())
            print(f"{family} heads {heads}/1 W={W} mask={name}: |restatement - HF| right {errs['right']:.1e}, "
                  f"i-j<=W {errs['le']:.1e}, causal {errs['causal']:.1e}")
            assert errs["right"] < 1e-8, (name, errs)
            assert errs["le"] > 1e-3 and errs["causal"] > 1e-3, (name, errs)
    finally:
        h.remove()


def test_layer_reference_without_window_is_the_prefill_oracle():
    """window 0 of the restatement is the project's existing Llama oracle (oracle/prefill_oracle.py), so the GPU tests' window
    cases and the existing Llama cases stand on one definition."""
    from oracle import prefill_oracle as P
    g = torch.Generator().manual_seed(5)
    D, HQ, HKV, S = 256, 2, 1, 40
    w = [torch.randn(n, k, generator=g) * k ** -0.5 for n, k in ((HQ * 128, D), (HKV * 128, D), (HKV * 128, D), (D, HQ * 128))]
    hid = torch.randn(2, S, D, generator=g)
    mask = torch.ones(2, S, dtype=torch.long)
    mask[0, :7] = 0
    mask[1, S - 9:] = 0
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    want = P.llama_attention_forward(hid, *w, HQ, HKV, pos, mask, 10000.0, head_dim=128)
    got = WC.attention_layer_reference(hid, *w, HQ, HKV, pos, mask, 10000.0, 0)
    assert AC.rel_l2(got, want) < 1e-5                        # the oracle is fp32 in places


# ------------------------------------------------------------------------------------------------ (2) patch plumbing
@pytest.mark.parametrize("family", ["mistral", "mixtral"])
@pytest.mark.parametrize("sliding_window", [None, 6])
def test_patch_plumbing_under_installed_transformers(monkeypatch, family, sliding_window):
    """With replace_{mistral,mixtral}_attn_with_hip_attn applied, a stock 2-layer model of the INSTALLED transformers runs end to
    end on the CPU; the recorder standing in for the HIP call sees the un-expanded [B, S] mask, the position ids and
    window == config.sliding_window (0 for None); use_cache=True raises; restore_* puts every patched name back by identity; the
    Llama patch applied and restored in the same process keeps its own five-argument call."""
    import importlib
    from slime_amd import ops
    from slime_amd.model.language_model import llama_attention as L
    from slime_amd.model.language_model import mistral_attention as MA
    from transformers.models.llama import modeling_llama as LM
    Config, Model, extra = _hf(family)
    M = importlib.import_module(f"transformers.models.{family}.modeling_{family}")
    attn_cls = getattr(M, family.capitalize() + "Attention")
    cfg = Config(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=64, num_hidden_layers=2,
                 vocab_size=64, sliding_window=sliding_window, rope_theta=1e6, attn_implementation="eager", **extra)
    model = Model(cfg).eval()
    emb, mask = torch.randn(2, 10, 512), torch.tensor([[1] * 10, [0] * 4 + [1] * 6])
    seen, llama_seen, thetas = [], [], []

    def recorder(pa, hidden, position_ids, attention_mask, out_dtype, window, resid=None, out=None):
        seen.append((None if attention_mask is None else tuple(attention_mask.shape),
                     None if position_ids is None else tuple(position_ids.shape), window, out_dtype))
        return torch.zeros_like(hidden)

    def llama_recorder(pa, hidden, position_ids, attention_mask, out_dtype):
        llama_seen.append(None if attention_mask is None else tuple(attention_mask.shape))
        return torch.zeros_like(hidden)

    def pack(*a, **k):
        thetas.append(a[-1])
        return object()
    monkeypatch.setattr(ops, "llama_attention_forward_window", recorder)
    monkeypatch.setattr(ops, "llama_attention_forward", llama_recorder)
    monkeypatch.setattr(ops, "pack_llama_attention", pack)
    names = [n for n in ("create_causal_mask", "create_sliding_window_causal_mask") if hasattr(M, n)]
    stock = {n: getattr(M, n) for n in names}
    stock_forward, llama_forward = attn_cls.forward, LM.LlamaAttention.forward
    llama_mask = getattr(LM, "create_causal_mask", None)
    replace, restore = getattr(MA, f"replace_{family}_attn_with_hip_attn"), getattr(MA, f"restore_{family}_attn")
    try:
        replace()
        L.replace_llama_attn_with_hip_attn()
        assert attn_cls.forward is not stock_forward and all(getattr(M, n) is not stock[n] for n in names)
        with torch.no_grad():
            out = model(inputs_embeds=emb, attention_mask=mask, use_cache=False).last_hidden_state
            model(inputs_embeds=emb, attention_mask=None, use_cache=False)
        with pytest.raises(NotImplementedError, match="use_cache=False"):
            model(inputs_embeds=emb, attention_mask=mask, use_cache=True)
        with pytest.raises(NotImplementedError, match="never materialises"):
            model.layers[0].self_attn(emb, attention_mask=mask, output_attentions=True)
        lcfg = LM.LlamaConfig(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=64,
                              num_hidden_layers=1, vocab_size=64, attn_implementation="eager")
        with torch.no_grad():
            LM.LlamaModel(lcfg).eval()(inputs_embeds=emb, attention_mask=mask, use_cache=False)
        L.restore_llama_attn()
        with torch.no_grad():                                    # the Mistral patch survives the Llama patch's restore
            model(inputs_embeds=emb, attention_mask=mask, use_cache=False)
    finally:
        L.restore_llama_attn()
        restore()
    W = 0 if sliding_window is None else sliding_window
    assert out.shape == (2, 10, 512) and torch.isfinite(out).all()
    assert seen[:2] == [((2, 10), (1, 10), W, torch.float32)] * 2 and seen[2:4] == [(None, (1, 10), W, torch.float32)] * 2
    assert seen[4:] == seen[:2] and llama_seen == [(2, 10)]
    assert thetas[:2] == [1e6, 1e6]                              # one pack per layer; the Llama model's comes after
    assert attn_cls.forward is stock_forward and all(getattr(M, n) is stock[n] for n in names)
    assert LM.LlamaAttention.forward is llama_forward and getattr(LM, "create_causal_mask", None) is llama_mask
    assert "create_sliding_window_causal_mask" in names or not hasattr(M, "create_sliding_window_causal_mask")
    restore()                                                    # a second restore is a no-op


def test_mistral_patch_refuses_scaled_rope_and_module_defaults():
    from transformers import MistralConfig
    from slime_amd.model.language_model import HipMistralAttention, llama_attention as L, mistral_attention as MA
    assert L._rope_theta(MistralConfig(rope_theta=1e6)) == 1e6
    sc = MistralConfig(rope_scaling={"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                     "original_max_position_embeddings": 8192})
    with pytest.raises(NotImplementedError, match="rope_type"):
        L._rope_theta(sc, MA.MISTRAL_ROPE_THETA)
    m = HipMistralAttention(512, 4, 1, sliding_window=None)
    assert sorted(n for n, _ in m.named_parameters()) == ["k_proj.weight", "o_proj.weight", "q_proj.weight", "v_proj.weight"]
    assert MA._window(None) == 0 and MA._window(4096) == 4096 and HipMistralAttention().sliding_window is None
    with pytest.raises(ValueError, match="sliding_window"):
        HipMistralAttention(512, 4, 1, sliding_window=0)
    with pytest.raises(NotImplementedError, match="no KV cache"):
        m(torch.zeros(1, 4, 512), use_cache=True)
    with pytest.raises(NotImplementedError, match="never materialises"):
        m(torch.zeros(1, 4, 512), output_attentions=True)


# ------------------------------------------------------------------------------------------------ (3) refusals, host only
FAKE = 0x7F0000001000                  # 16- and 256-byte aligned, never dereferenced: every call below is refused before a launch


def _prefill_args(**kw):
    a = dict(q=FAKE, q_bs=40 * 512, q_rs=512, k=FAKE + 4096, k_bs=40 * 256, k_rs=256, v=FAKE + 8192, v_bs=40 * 256, v_rs=256,
             o=FAKE + 12288, o_bs=40 * 512, o_rs=512, batch=1, n_heads=4, n_kv_heads=2, head_dim=128, S=40, kv_start=None, kv_len=None,
             dtype=0)
    a.update(kw)
    return list(a.values())


PREFILL_REFUSALS = [
    (dict(q=None), "null pointer"), (dict(batch=0), "empty shape"), (dict(batch=65536), "empty shape"), (dict(S=0), "empty shape"),
    (dict(head_dim=64), "head_dim 64"), (dict(n_heads=7), "7 query heads / 2 kv heads"), (dict(n_heads=6), "group size 3"),
    (dict(n_heads=64), "group size 32"), (dict(q_rs=516), "multiples of 8"), (dict(o_bs=40 * 512 + 4), "multiples of 8"),
    (dict(o=FAKE + 8), "16-byte aligned"), (dict(kv_start=FAKE), "come together"), (dict(dtype=2), "dtype 2"),
    (dict(n_heads=2, S=65536 * 256), "sequence too long")]


@pytest.mark.parametrize("change,needle", PREFILL_REFUSALS, ids=[n.replace(" ", "_") for _, n in PREFILL_REFUSALS])
@pytest.mark.parametrize("window", [0, 8])
def test_prefill_window_entry_reproduces_every_refusal(change, needle, window):
    from slime_amd import _lib
    lib = _lib.load()
    if "dtype" not in change:
        change = dict(change, dtype=_lib.BF16)
    args = _prefill_args(**change)
    rc0 = lib.slime_prefill_attention(*args, None)
    msg0 = lib.slime_last_error().decode()
    rc1 = lib.slime_prefill_attention_window(*args, window, None)
    msg1 = lib.slime_last_error().decode()
    assert rc0 == rc1 == -1 and needle in msg0 and msg1 == msg0, (msg0, msg1)


def test_prefill_window_negative_is_refused_by_name():
    from slime_amd import _lib
    lib = _lib.load()
    rc = lib.slime_prefill_attention_window(*_prefill_args(dtype=_lib.BF16), -1, None)
    msg = lib.slime_last_error().decode()
    assert rc == -1 and "window -1" in msg, msg
    rc = lib.slime_prefill_attention_window(*_prefill_args(dtype=_lib.BF16, q=None), -3, None)      # ... before anything else
    assert rc == -1 and "window -3" in lib.slime_last_error().decode()


def _desc(**kw):
    from slime_amd import _lib
    d = _lib.LlamaAttnDesc()
    f = dict(hidden=512, n_heads=4, n_kv_heads=2, head_dim=128, dtype=_lib.BF16, w_qkv=FAKE, w_o=FAKE, inv_freq=FAKE)
    f.update(kw)
    for k, v in f.items():
        setattr(d, k, v)
    return d


LLAMA_REFUSALS = [
    (dict(dtype=2), {}, "dtype must be BF16 or F16"), (dict(head_dim=64), {}, "heads"), (dict(n_heads=5), {}, "heads"),
    (dict(hidden=192), {}, "multiple of 128"), (dict(w_qkv=None), {}, "missing weights"), (dict(inv_freq=None), {}, "missing weights"),
    ({}, dict(hidden=None), "bad input"), ({}, dict(pos=None), "bad input"), ({}, dict(batch=0), "bad input"), ({}, dict(S=0), "bad input"),
    ({}, dict(ws=None), "workspace"), ({}, dict(ws_bytes=16), "workspace"), ({}, dict(ws=FAKE + 8), "workspace")]


@pytest.mark.parametrize("with_resid", [False, True], ids=["forward", "resid"])
@pytest.mark.parametrize("dchange,achange,needle", LLAMA_REFUSALS, ids=[f"{i}-{n.split()[0]}" for i, (_, _, n) in enumerate(LLAMA_REFUSALS)])
def test_llama_window_entry_reproduces_every_refusal(dchange, achange, needle, with_resid):
    from slime_amd import _lib
    lib = _lib.load()
    d = _desc(**dchange)
    a = dict(hidden=FAKE, pos=FAKE, batch=1, S=40, out=FAKE + 65536, ws=FAKE + (1 << 20), ws_bytes=1 << 30)
    a.update(achange)
    resid = FAKE + (1 << 19) if with_resid else None
    if with_resid:
        rc0 = lib.slime_llama_attn_forward_resid(C.byref(d), a["hidden"], a["pos"], None, None, a["batch"], a["S"], resid, a["out"],
                                                 a["ws"], a["ws_bytes"], None)
    else:
        rc0 = lib.slime_llama_attn_forward(C.byref(d), a["hidden"], a["pos"], None, None, a["batch"], a["S"], a["out"], d.dtype,
                                           a["ws"], a["ws_bytes"], None)
    msg0 = lib.slime_last_error().decode()
    for window in (0, 8):
        rc1 = lib.slime_llama_attn_forward_window(C.byref(d), a["hidden"], a["pos"], None, None, a["batch"], a["S"], resid, a["out"],
                                                  d.dtype, window, a["ws"], a["ws_bytes"], None)
        msg1 = lib.slime_last_error().decode()
        assert rc0 == rc1 and rc0 in (-1, -2) and needle in msg0 and msg1 == msg0, (rc0, rc1, msg0, msg1)


def test_llama_window_entry_own_refusals():
    from slime_amd import _lib
    lib = _lib.load()
    d = _desc()
    tail = (FAKE + (1 << 20), 1 << 30, None)

    def call(resid, out, out_dtype, window, desc=d, hidden=FAKE):
        rc = lib.slime_llama_attn_forward_window(None if desc is None else C.byref(desc), hidden, FAKE, None, None, 1, 40, resid, out,
                                                 out_dtype, window, *tail)
        return rc, lib.slime_last_error().decode()
    rc, msg = call(None, FAKE + 65536, _lib.BF16, -1)
    assert rc == -1 and "window -1" in msg, msg
    rc, msg = call(FAKE + 4096, FAKE + 65536, _lib.BF16, -7)
    assert rc == -1 and "window -7" in msg, msg
    assert call(None, FAKE, _lib.BF16, 8, desc=None)[0] == -1 and call(None, None, _lib.BF16, 8)[0] == -1
    rc, msg = call(None, FAKE + 65536, _lib.F16, 8)                       # the plain entry's out-dtype rule
    assert rc == -1 and "operand type or F32" in msg
    rc, msg = call(FAKE + 4096, FAKE + 65536, _lib.F32, 8)                # the residual entry stores the operand type only
    assert rc == -1 and "operand type" in msg
    rc, msg = call(FAKE + 4096, FAKE, _lib.BF16, 8)                       # ... and out must not alias the layer's input rows
    assert rc == -1 and "alias" in msg


def test_signatures_of_the_two_entries():
    from slime_amd import _lib
    base, win = _lib._SIGNATURES["slime_prefill_attention"], _lib._SIGNATURES["slime_prefill_attention_window"]
    assert win[0] is base[0] and win[1] == base[1][:-1] + [C.c_int] + base[1][-1:]                 # ... dtype, window, stream
    resid, lw = _lib._SIGNATURES["slime_llama_attn_forward_resid"], _lib._SIGNATURES["slime_llama_attn_forward_window"]
    assert lw[1] == resid[1][:9] + [C.c_int, C.c_int] + resid[1][9:]                                # ... resid, out, out_dtype, window, ws
    assert {"slime_prefill_attention_window", "slime_llama_attn_forward_window"} <= set(_lib.header_symbols())
    assert _lib.ABI_VERSION == 7 and _lib.load().slime_abi_version() == 7


# ------------------------------------------------------------------------------------------------ (4) emulation and mutants
def _check_case(c, W, what):
    """The right window inside the bound; every mutant whose key set differs from the right one on this case outside it; the
    input condition.  Returns the set of mutants that were real on this case."""
    r = WC.reference(c, W)
    scores = WC.raw_scores(c)
    ex = float(WC.excess(WC.emulate(c, W, scores=scores), r, c.dtype).max())
    assert ex <= 0, f"{what}: the emulation with the right window exceeds the bound by {ex:.3e}"
    right = WC.live_mask(c.B, c.n_q, W, c.ranges, "cpu")[0]
    real = set()
    for rule in WC.MUTANT_RULES:
        if torch.equal(WC.live_mask(c.B, c.n_q, W, c.ranges, "cpu", rule)[0], right):
            continue                                            # the same key set on this case: not a mutant here
        real.add(rule)
        ex = float(WC.excess(WC.emulate(c, W, rule, scores=scores), r, c.dtype).max())
        assert ex > 0, f"{what}: mutant {rule} stays inside the bound"
    # input condition: W and W + 1 differ by more than 8 x the bound in every 16-row block that has an excluded key in range
    r1 = WC.reference(c, W + 1)
    margin = (r1.out - r.out).abs() - 8.0 * AC.bound(r.out, r.A, c.dtype, r.e32, r.under)           # [B, S, H, dh]
    lo, hi = WC._bounds(None if c.ranges is None else (c.ranges[0].tolist(), c.ranges[1].tolist()), c.B, c.n_q)
    for b in range(c.B):
        for blk in WC.blocks_with_excluded_key(c.n_q, W, lo[b], hi[b]):
            assert float(margin[b, blk * 16:blk * 16 + 16].max()) > 0, f"{what}: batch {b} block {blk}: the excluded key carries no weight"
    return real


@pytest.mark.parametrize("dtype,group,S", [pytest.param(dt, g, S, id=f"{DT_ID[dt]}-group{g}-S{S}")
                                           for dt in (torch.bfloat16, torch.float16) for g in WC.EIGHT_WAVE_GROUPS[dt] for S in WC.EIGHT_WAVE_S])
def test_emulation_and_mutants_eight_wave_cases(dtype, group, S):
    """Every case test_gpu_window_attention.py walks on the eight-wave kernel -- the same (dtype, group, S) parameters, the same
    builder, seeds and gains -- except the guard kind, which lies outside the logical tensors.  At every S > 1 each of the six
    mutants is real on at least one case."""
    real = set()
    for W, kind, B, seed in WC.eight_wave_cases(dtype, group, S):
        c = WC.build(dtype, group, S, W, kind, B, seed)
        real |= _check_case(c, W, f"{DT_ID[dtype]} group {group} S={S} W={W} ranges={kind}")
    assert S == 1 or real == set(WC.MUTANT_RULES), real


@pytest.mark.parametrize("S", WC.PREFILL32_S)
def test_emulation_and_mutants_group4_bf16_cases(S):
    """The same for the group-4 bf16 list (Mistral's geometry, prefill32_kernel), two kv heads."""
    real = set()
    for W, kind, B, seed in WC.prefill32_cases(S):
        c = WC.build(torch.bfloat16, 4, S, W, kind, B, seed)
        real |= _check_case(c, W, f"bf16 group 4 S={S} W={W} ranges={kind}")
    assert real == set(WC.MUTANT_RULES), real


@pytest.mark.parametrize("W,ranged", WC.MANY_ITEMS)
def test_emulation_and_mutants_many_items_case(W, ranged):
    """... and for the 8 kv heads x batch 4 x S = 600 case (320 items: the seam between a windowed item and the next)."""
    real = _check_case(WC.build_many_items(W, ranged), W, f"bf16 32/8 heads B=4 S=600 W={W} ranges={ranged}")
    assert real == set(WC.MUTANT_RULES), real
