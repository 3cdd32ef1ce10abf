"""CPU tests: slicer / pre-processing host logic against golden vectors produced by the reference,
the C-ABI surface of the built library, and config/builder error behaviour.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_library_exports_exactly_the_header():
    """The product library exports every function include/slime_hip.h declares and NOTHING else (no diagnostic hooks, no
    kernel stubs); the hooks live in the separate -DSLIME_DIAG build."""
    from slime_amd import _lib
    lib = _lib.load()
    syms = set(_lib.header_symbols())
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"libslime_hip.so does not export {s}"
    assert lib.slime_abi_version() == _lib.ABI_VERSION == 7
    assert _exported(_lib.LIB_PATH) == syms
    assert set(_lib._SIGNATURES) == syms, "slime_amd/_lib.py binds exactly the header's functions"
    if os.path.exists(_lib.DIAG_LIB_PATH):
        extra = _exported(_lib.DIAG_LIB_PATH) - syms
        assert extra == set(_lib._DIAG_SIGNATURES), extra


def test_vit_check_refuses_geometries_the_front_end_cannot_run():
    """the fused front end's limits are checked when a tower is PACKED (slime_vit_check, host-only -- no GPU needed), with
    the limit named: CLIP-L/14-336 and -224 pass, a 448 / 14 tower (32 patches per side), a 340-pixel image (not a multiple of 8
    ... nor of the patch) and head_dim 80 do not."""
    import ctypes as C
    from slime_amd import _lib
    lib = _lib.load()

    def desc(image=336, patch=14, hidden=1024, heads=16, inter=4096):
        d = _lib.VitDesc()
        d.hidden, d.inter, d.heads, d.layers_run, d.image, d.patch = hidden, inter, heads, 2, image, patch
        d.kpad, d.dtype, d.eps = (3 * patch * patch + 63) // 64 * 64, _lib.BF16, 1e-5
        for name, _ in _lib.VitDesc._fields_:
            if isinstance(getattr(d, name), (type(None),)) and name != "patch_w":
                setattr(d, name, 0x1000)                          # any non-null address: the check never dereferences
        return d

    assert lib.slime_vit_check(C.byref(desc())) == 0
    assert lib.slime_vit_check(C.byref(desc(image=224))) == 0
    for bad, word in ((desc(image=448), "patches per side"), (desc(image=340, patch=10), "multiple of the patch"),
                      (desc(heads=12), "head_dim"), (desc(hidden=512, heads=8), "hidden=512")):
        assert lib.slime_vit_check(C.byref(bad)) == -1
        assert word in lib.slime_last_error().decode(), lib.slime_last_error()
    missing = desc()
    missing.w_fc2, missing.w_fc2_frag = None, None
    assert lib.slime_vit_check(C.byref(missing)) == -1 and "missing layer weights" in lib.slime_last_error().decode()


def test_grid_tables_match_reference():
    from slime_amd import mm_utils as M, process_image as P
    g = np.load(os.path.join(GOLDEN, "slicer_grid.npz"))
    pts = [(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]
    for (w, h), grid, uhd, sl, sbr in zip(g["sizes"], g["grid"], g["uhd"], g["slices"], g["select_best_resolution"]):
        size = (int(w), int(h))
        assert M.select_best_resolution_uhd(size, (336, 336)) == tuple(uhd), size
        assert M.get_anyres_image_grid_shape(size, PIN, 336) == tuple(grid), size
        assert M.get_anyres_image_grid_shape(size, pts, 336) == tuple(grid), size
        assert P.cal_num_of_slices(*size) == tuple(sl), size
        assert M.select_best_resolution(size, pts) == tuple(sbr), size
    # probes recorded in SURVEY.md 8(a-1)
    assert M.get_anyres_image_grid_shape((336, 336), PIN, 336) == (1, 2)
    assert M.get_anyres_image_grid_shape((4000, 300), PIN, 336) == (7, 1)


@pytest.mark.parametrize("mode", ["anyres", "pad", "any_res", "pad_then_devide"])
def test_process_images_matches_reference_pixels(mode):
    """Bit-exact per-crop checksums and sampled pixels of ``process_images`` for every slicing mode."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    g = np.load(os.path.join(GOLDEN, "slicer_pixels.npz"))
    proc = ClipImageProcessor()
    assert np.allclose(proc.image_mean, g["image_mean"]) and np.allclose(proc.image_std, g["image_std"])
    cfg = SimpleNamespace(image_aspect_ratio=mode, image_grid_pinpoints=PIN)
    for i, (w, h) in enumerate(g["img_specs"]):
        arr = np.random.default_rng(100 + i).integers(0, 256, (int(h), int(w), 3), dtype=np.uint8)
        out = M.process_images([Image.fromarray(arr, "RGB")], proc, cfg)
        out = out[0] if out.dim() == 5 else out
        if out.dim() == 3:
            out = out.unsqueeze(0)
        assert tuple(out.shape) == tuple(g[f"img{i}_{mode}_shape"]), (i, mode)
        flat = out.reshape(out.shape[0], -1).double()
        assert np.array_equal(flat[:, g["sample_idx"]].float().numpy(), g[f"img{i}_{mode}_samples"]), (i, mode)
        assert np.allclose(flat.sum(1).numpy(), g[f"img{i}_{mode}_sum"], rtol=0, atol=1e-6), (i, mode)
        assert np.allclose((flat * flat).sum(1).numpy(), g[f"img{i}_{mode}_sumsq"], rtol=1e-12), (i, mode)


def test_process_images_stacks_or_lists():
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    proc = ClipImageProcessor()
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    a = Image.fromarray(np.zeros((672, 672, 3), np.uint8))
    b = Image.fromarray(np.zeros((1344, 1344, 3), np.uint8))
    same = M.process_images([a, a], proc, cfg)
    assert isinstance(same, torch.Tensor) and tuple(same.shape) == (2, 5, 3, 336, 336)
    mixed = M.process_images([a, b], proc, cfg)
    assert isinstance(mixed, list) and mixed[0].shape[0] == 5 and mixed[1].shape[0] == 1 + 6
    with pytest.raises(Exception):
        M.get_anyres_image_grid_shape((10, 10), "not a list", 336)


def test_builders_reject_unknown_types():
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    from slime_amd.model.multimodal_projector.builder import build_vision_projector
    from slime_amd.model.multimodal_resampler.builder import build_vision_sampler, IdentityMap
    with pytest.raises(ValueError, match="Unknown vision tower"):
        build_vision_tower(SimpleNamespace(mm_vision_tower="not/a/tower", mm_vision_select_layer=-2))
    with pytest.raises(ValueError, match="Unknown projector type"):
        build_vision_projector(SimpleNamespace(mm_projector_type="bogus", mm_hidden_size=128, hidden_size=256))
    assert isinstance(build_vision_sampler(SimpleNamespace(mm_resampler_type=None)), IdentityMap)
    assert isinstance(build_vision_sampler(SimpleNamespace(mm_resampler_type="identity")), IdentityMap)


def test_tower_module_contract_without_gpu():
    """delay_load keeps config only; state-dict keys follow HF (both prefix generations load)."""
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    from slime_amd import weights as W
    args = SimpleNamespace(mm_vision_tower="synthetic:7", mm_vision_select_layer=-2, mm_vision_select_feature="patch")
    t = build_vision_tower(args, delay_load=True)
    assert not t.is_loaded and t.hidden_size == 1024 and t.num_patches == 576 and t.num_patches_per_side == 24
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    m = HipCLIPVisionModel(W.TINY)
    sd = W.make_tower_state_dict(W.TINY, seed=3)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    missing, unexpected = m.load_state_dict(W.strip_tower_prefix(sd), strict=False)      # transformers 5.x names
    assert not missing and not unexpected
    assert set(m.state_dict().keys()) == set(sd.keys())
    bad = SimpleNamespace(mm_vision_tower="synthetic:7", mm_vision_select_layer=-2, mm_vision_select_feature="nope")
    t2 = build_vision_tower(bad, delay_load=True)
    with pytest.raises(ValueError, match="Unexpected select feature"):
        t2._keep_cls()


def test_product_has_no_cpu_path():
    """The HIP path must fail loudly rather than fall back: CPU tensors are rejected."""
    from slime_amd import ops, _lib, weights as W
    with pytest.raises((_lib.SlimeHipError, AssertionError, RuntimeError)):
        pt = ops.pack_tower(W.make_tower_state_dict(W.TINY, seed=1), W.TINY, torch.bfloat16, "cpu")
        ops.tower_forward(pt, torch.zeros(1, 3, 336, 336))


def test_adapter_state_dict_roundtrip():
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    from slime_amd import weights as W
    cfg = default_slime_config("synthetic:1", hidden_size=256, mm_hidden_size=128)
    enc = SlimeVisualEncoder(cfg)
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    enc.model.mm_projector.load_state_dict(W.sub_state(asd, "mm_projector."), strict=True)
    enc.model.sampler.load_state_dict(W.sub_state(asd, "sampler."), strict=True)
    keys = {"mm_projector." + k for k in enc.model.mm_projector.state_dict()} | {"sampler." + k for k in enc.model.sampler.state_dict()}
    assert keys == set(asd.keys())
    assert enc.model.mm_projector.w_gate.dtype == torch.bfloat16 and enc.model.sampler.post_qformer.pos_embed.dtype == torch.float16
    assert enc.model.has_sampler and enc.model.sampler.grid_size == 12


@pytest.mark.parametrize("sizes", [(672, 336), (1344, 336), (640, 672), (1080, 567), (300, 2352), (4000, 336),
                                   (336, 337), (53, 336), (7, 3), (1, 336)])
def test_resample_tables_match_oracle(sizes):
    """Host half of the device slicer: the C ABI's Pillow coefficient tables (pure host function, no GPU)
    equal the oracle's restatement bit for bit."""
    from slime_amd import ops
    from oracle import pil_resample as R
    bounds, kk = ops.resample_tables(*sizes)
    xmin, cnt, fixed = R.coefficients(*sizes)
    assert np.array_equal(bounds[:, 0], xmin) and np.array_equal(bounds[:, 1], cnt)
    assert np.array_equal(kk, fixed)


def test_training_mode_is_rejected_not_silently_detached():
    """the HIP adapter has no backward; training-mode use with trainable adapter parameters raises (before any
    device work) instead of silently freezing the adapter; eval mode / no_grad / frozen parameters pass the guard."""
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config, _require_inference
    enc = SlimeVisualEncoder(default_slime_config("synthetic:1", hidden_size=256, mm_hidden_size=128))
    assert not enc.training
    _require_inference(enc.get_model())                       # eval mode: fine
    enc.train()
    with pytest.raises(RuntimeError, match="inference-only"):
        enc.encode_images(torch.zeros(1, 3, 336, 336), input_ids=torch.zeros(1, 4, dtype=torch.long), split_sizes=[1])
    with torch.no_grad():
        _require_inference(enc.get_model())
    enc.get_model().mm_projector.requires_grad_(False)
    enc.get_model().sampler.requires_grad_(False)
    _require_inference(enc.get_model())


def test_tower_checkpoint_key_mismatch_raises():
    """a checkpoint with another naming scheme / a partial one must not run on uninitialised weights."""
    from slime_amd import weights as W
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel, check_tower_keys
    m = HipCLIPVisionModel(W.TINY)
    sd = W.make_tower_state_dict(W.TINY, seed=3)
    ok = {k: v for k, v in sd.items() if "post_layernorm" not in k}
    check_tower_keys(m.load_state_dict(ok, strict=False), "ok")                    # the dead post_layernorm may be absent
    part = {k: v for k, v in sd.items() if "layers.1." not in k}
    with pytest.raises(RuntimeError, match="missing"):
        check_tower_keys(m.load_state_dict(part, strict=False), "partial")
    renamed = {k.replace("self_attn.q_proj", "attn.in_proj_q"): v for k, v in sd.items()}     # open_clip-like names
    with pytest.raises(RuntimeError, match="unexpected"):
        check_tower_keys(m.load_state_dict(renamed, strict=False), "renamed")


def test_resampler_pack_regenerates_nan_pos_embed():
    """ADVICE r1 / sampler.py:150-154: a stored pos_embed with NaN is replaced by the sincos table at pack time."""
    from slime_amd import ops, weights as W
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    sd = dict(W.sub_state(asd, "sampler.post_qformer."))
    good = ops.pack_resampler(sd, 128, 1, 576, torch.bfloat16, "cpu")
    bad = dict(sd)
    bad["pos_embed"] = sd["pos_embed"].clone()
    bad["pos_embed"][3, 5] = float("nan")
    fixed = ops.pack_resampler(bad, 128, 1, 576, torch.bfloat16, "cpu")
    ref = dict(sd)
    ref["pos_embed"] = torch.from_numpy(W.sincos_pos_embed_2d(128, 12)).to(sd["pos_embed"].dtype)
    want = ops.pack_resampler(ref, 128, 1, 576, torch.bfloat16, "cpu")
    for k in ("q_proj", "pos_k"):
        assert torch.isfinite(fixed.tensors[k].float()).all()
        assert torch.equal(fixed.tensors[k], want.tensors[k])
    assert torch.isfinite(good.tensors["q_proj"].float()).all()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_splice_plan_matches_reference(name):
    """Row f-2, host half: the integer splice plan reproduces the reference's prepare_inputs_labels_for_multimodal outputs
    (tests/golden/prefill.npz) -- labels, mask, position ids bit for bit, and the embeddings once the plan is applied."""
    import prefill_fixture as F
    from slime_amd.model.llava_arch import splice_plan
    c = F.splice_case(F.load(), name)
    am = None if c["attention_mask"] is None else c["attention_mask"].numpy()
    lb = None if c["labels"] is None else c["labels"].numpy()
    src, lab, mask, pos = splice_plan(c["input_ids"].numpy(), am, lb, [f.shape[0] for f in c["feats"]], c["max_length"], c["padding_side"])
    allf = torch.cat(c["feats"], 0)
    emb = torch.zeros(src.shape + (c["table"].shape[1],))
    s = torch.from_numpy(src)
    emb[s >= 0] = c["table"][s[s >= 0]]
    emb[s <= -2] = allf[-2 - s[s <= -2]]
    assert torch.equal(emb, c["out_embeds"])
    if c["out_mask"] is not None:
        assert np.array_equal(mask, c["out_mask"].numpy()) and np.array_equal(lab, c["out_labels"].numpy())
        assert np.array_equal(pos, c["out_position_ids"].numpy())
    with pytest.raises(ValueError, match="fewer image features"):
        splice_plan(c["input_ids"].numpy(), am, lb, [f.shape[0] for f in c["feats"]][:-1], c["max_length"], c["padding_side"])


def test_splice_plan_validates_ids_under_the_mask_only():
    """the reference drops padding through the attention mask BEFORE embed_tokens (llava_arch.py:361-373), so a pad id
    past the vocabulary is legal under mask 0; every id that is embedded must lie in [0, vocab) -- id -1 would otherwise be read as
    padding and an id <= -2 as an image-feature row (silent corruption where nn.Embedding raises)."""
    from slime_amd.model.llava_arch import splice_plan
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    ids = np.array([[5, IMAGE_TOKEN_INDEX, 7, 99999], [1, 2, 3, 4]])
    am = np.array([[1, 1, 1, 0], [1, 1, 1, 1]])
    src, _, mask, _ = splice_plan(ids, am, None, [2, 0], None, "right", vocab_size=100)       # pad id 99999 is masked out: fine
    assert src[0].tolist() == [5, -2, -3, 7] and mask[0].tolist() == [1, 1, 1, 1]
    for bad in (100, 99999, -1, -2, -7):
        ids2 = ids.copy(); ids2[1, 2] = bad
        with pytest.raises(IndexError, match="index out of range"):
            splice_plan(ids2, am, None, [2, 0], None, "right", vocab_size=100)
    ids3 = ids.copy(); ids3[1, 2] = -7
    splice_plan(ids3, am, None, [2, 0], None, "right")                                         # no vocabulary given: plan only (oracle tests)


def test_hf_attention_patch_plumbing_under_installed_transformers(monkeypatch):
    """VERDICT r3 missing #4, host half (no GPU): with ``replace_llama_attn_with_hip_attn`` applied, a stock 2-layer HF ``LlamaModel``
    of the INSTALLED transformers runs end to end -- the patched forward returns as many values as ``LlamaDecoderLayer`` unpacks, the
    [B, S] key-padding mask reaches it un-expanded, position ids arrive, and ``restore_llama_attn`` puts everything back.  The HIP
    call itself is replaced by a recorder here; tests/test_gpu_prefill.py runs the real thing against the fp32 CPU forward."""
    import torch
    from transformers.models.llama import modeling_llama as M
    from transformers import LlamaConfig
    from slime_amd import ops
    from slime_amd.model.language_model import llama_attention as L
    cfg = LlamaConfig(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=256,
                      num_hidden_layers=2, rope_theta=500000.0, vocab_size=64, attn_implementation="eager")
    assert L._rope_theta(cfg) == 500000.0 and L._self_attn_return_arity(M) in (2, 3)
    model = M.LlamaModel(cfg).eval()
    emb, mask = torch.randn(2, 10, 512), torch.tensor([[1] * 10, [0] * 4 + [1] * 6])
    seen = []

    def recorder(pa, hidden, position_ids, attention_mask, out_dtype):
        seen.append((None if attention_mask is None else tuple(attention_mask.shape), None if position_ids is None else tuple(position_ids.shape)))
        return torch.zeros_like(hidden)
    monkeypatch.setattr(ops, "llama_attention_forward", recorder)
    monkeypatch.setattr(ops, "pack_llama_attention", lambda *a, **k: object())
    stock = M.LlamaAttention.forward
    stock_mask = getattr(M, "create_causal_mask", None)
    try:
        L.replace_llama_attn_with_hip_attn()
        with torch.no_grad():
            out = model(inputs_embeds=emb, attention_mask=mask, use_cache=False).last_hidden_state
            model(inputs_embeds=emb, attention_mask=None, use_cache=False)
        with pytest.raises(NotImplementedError, match="use_cache=False"):
            model(inputs_embeds=emb, attention_mask=mask, use_cache=True)
        # positional extras are mapped by the INSTALLED signature (4.48+: hidden_states, position_embeddings, attention_mask;
        # before: hidden_states, attention_mask, position_ids) -- the mask must be recognised as the mask wherever it sits
        import inspect
        names = list(inspect.signature(stock).parameters)[2:]
        vals = {"attention_mask": mask, "position_ids": torch.arange(10)[None], "position_embeddings": (torch.zeros(1), torch.zeros(1))}
        n_pos = max(i for i, n in enumerate(names) if n in ("attention_mask", "position_ids")) + 1
        before = len(seen)
        with torch.no_grad():
            model.layers[0].self_attn(emb, *[vals.get(n) for n in names[:n_pos]])
        assert len(seen) == before + 1 and seen[-1][0] == (2, 10) and seen[-1][1] in (None, (1, 10))
        with pytest.raises(TypeError, match="positional"):
            model.layers[0].self_attn(emb, *([None] * (len(names) + 1)))
    finally:
        L.restore_llama_attn()
    assert out.shape == (2, 10, 512) and torch.isfinite(out).all()
    assert seen[:2] == [((2, 10), (1, 10))] * 2 and seen[2:4] == [(None, (1, 10))] * 2      # two layers per forward
    assert M.LlamaAttention.forward is stock and getattr(M, "create_causal_mask", None) is stock_mask
    sc = LlamaConfig(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, rope_scaling={"rope_type": "llama3", "factor": 8.0,
                     "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    with pytest.raises(NotImplementedError, match="rope_type"):
        L._rope_theta(sc)


def test_gather_chunk_cost_model():
    """slime_amd.dist.choose_chunk: one tower pass + one all-gather at every per-rank size BASELINE's configs produce (round 2's
    fixed chunk of 3 doubled a 9-crop shard's tower time); micro-batches only where the modelled transfer exceeds a second pass."""
    from slime_amd import dist as D
    prof = D.tower_latency_profile()                                     # slime_amd/data/tower_latency_mi355x_vitl336_bf16.json
    T = prof["ms"]
    assert prof["device"] == "MI355X" and prof["dtype"] == "bf16" and T[1] == 1.87 and T[40] == 14.44
    for n in (1, 5, 9, 17, 34, 40, 68):
        assert abs(D.tower_ms(n) - (T[n] if n in T else D.tower_ms(n))) < 1e-9
    assert D.tower_ms(0) == 0.0 and D.tower_ms(11) == pytest.approx((T[10] + T[12]) / 2)
    assert D.tower_ms(60) == pytest.approx(T[40] + prof["ms_per_crop_beyond"] * 20)
    # the curve is a profile of ONE device / tower / dtype; for anything else the policy decides nothing (chunk 0)
    assert D.profile_applies(prof, "AMD Instinct MI355X", "CLIP-ViT-L/14-336", "bf16") and D.profile_applies(prof)
    assert not D.profile_applies(prof, "AMD Instinct MI300X") and not D.profile_applies(prof, None, None, "fp16")
    # equality on canonical keys, not substrings -- 'float16' is not 'bfloat16', 'MI35' is not 'MI355X'
    assert not D.profile_applies(prof, None, None, "float16") and not D.profile_applies(prof, None, None, "f16")
    assert D.profile_applies(prof, None, None, "torch.bfloat16") and D.profile_applies(prof, None, None, "bfloat16")
    assert not D.profile_applies(prof, "MI35") and not D.profile_applies(prof, "AMD Instinct MI355") and D.profile_applies(prof, "mi355x")
    assert not D.profile_applies(prof, None, "CLIP-ViT-L/14") and D.profile_applies(prof, None, "clip-vit-l/14-336 (fp16 run)")
    assert D.choose_chunk(400, 8) > 0 and D.choose_chunk(400, 8, device_name="AMD Instinct MI300X") == 0
    flat = {"device": "MI355X", "model": None, "dtype": None, "ms": {1: 0.1, 100: 10.0}, "ms_per_crop_beyond": 0.1}
    assert D.choose_chunk(34, 8, profile=flat) > 0                        # no per-pass floor in this curve: micro-batches pay early
    assert all(D.tower_ms(a) <= D.tower_ms(b) for a, b in zip(range(1, 80), range(2, 81)))          # monotone
    assert D.gather_ms(9, 1) == 0.0 and D.gather_ms(9, 8) == pytest.approx(0.03 + 7 * 9 * 576 * 1024 * 2 / 100e6)
    for per, world in ((40, 1), (20, 2), (10, 4), (5, 8), (34, 2), (17, 4), (9, 8), (1, 8)):
        assert D.choose_chunk(per, world) == 0, (per, world)
    big = D.choose_chunk(400, 8)
    assert 0 < big < 400
    # the choice is the argmin of the model it documents
    one = D.tower_ms(400) + D.gather_ms(400, 8)
    sizes = [min(big, 400 - i) for i in range(0, 400, big)]
    assert sum(D.tower_ms(x) for x in sizes) + D.gather_ms(sizes[-1], 8) < one


def test_position_ids_broadcast_and_token_ranges_host_logic():
    """HF hands [1, S] / None position ids to every attention layer; ops._position_ids materialises the broadcast and
    rejects shapes that do not broadcast.  ops.token_ranges: contiguous runs only, cached per mask OBJECT."""
    import torch
    from slime_amd import ops
    B, S = 3, 7
    want = torch.arange(S, dtype=torch.int32)[None].expand(B, S)
    for pid in (None, torch.arange(S), torch.arange(S)[None], torch.arange(S)[None].expand(B, S)):
        got = ops._position_ids(pid, B, S, "cpu")
        assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, want)
    for bad in (torch.arange(S)[None].expand(2, S), torch.arange(S + 1), torch.zeros(B, S, 1)):
        with pytest.raises(ValueError, match="broadcast"):
            ops._position_ids(bad, B, S, "cpu")
    m = torch.tensor([[1, 1, 1, 0, 0], [0, 0, 1, 1, 1], [0, 0, 0, 0, 0]])
    st, ln = ops.token_ranges(m)
    assert st.tolist() == [0, 2, 0] and ln.tolist() == [3, 3, 0]
    assert ops.token_ranges(m)[0] is st
    m[0, 3] = 1
    assert ops.token_ranges(m)[1].tolist() == [4, 3, 0]
    with pytest.raises(ValueError, match="contiguous"):
        ops.token_ranges(torch.tensor([[1, 0, 1, 1]]))
    assert ops.token_ranges(None) == (None, None)


def _prefill32_schedule(n_kv, batch, nqb, G):
    """The item walk of prefill32.inc (load_item): workgroup w of G takes item r G + w in even rounds and r G + mirror(w) in odd
    ones; item L = kv head L % n_kv, sequence (L / n_kv) % batch, query block nqb - 1 - L / (n_kv batch) (heaviest first)."""
    n_items = n_kv * batch * nqb
    rounds = -(-n_items // G)
    out = []
    for w in range(G):
        wm = ((((G >> 3) - 1 - (w >> 3)) << 3) | (w & 7)) if G % 8 == 0 else G - 1 - w
        mine = []
        for r in range(rounds):
            L = r * G + (wm if r & 1 else w)
            if L < n_items:
                rest = L // n_kv
                mine.append((L % n_kv, rest % batch, nqb - 1 - rest // batch))
        out.append(mine)
    return out


@pytest.mark.parametrize("n_kv,batch,nqb,G", [(8, 8, 19, 256), (8, 1, 145, 256), (8, 3, 24, 256), (2, 2, 4, 16), (1, 40, 4, 160),
                                              (8, 12, 24, 248), (8, 5, 7, 250), (1, 1, 3, 3)])
def test_prefill32_snake_schedule_covers_every_item_once_and_balances(n_kv, batch, nqb, G):
    """Round 3's persistent prefill attention launches min(items, CUs) workgroups and lets each walk its items by arithmetic alone
    (no counter).  Properties of that walk, restated from prefill32.inc: every (kv head, sequence, query block) exactly once; a
    workgroup's items get lighter from round to round; with G a multiple of 8 a workgroup stays on one kv head when n_kv divides 8
    (XCD = workgroup id mod 8: the K/V of a head stay in one L2); the causal work (2 (qb + 1) key steps per item) of the fullest
    workgroup is within 4 % of the mean at the bench shapes."""
    sched = _prefill32_schedule(n_kv, batch, nqb, G)
    flat = [it for mine in sched for it in mine]
    assert len(flat) == n_kv * batch * nqb and len(set(flat)) == len(flat)
    for w, mine in enumerate(sched):
        assert all(a[2] >= b[2] for a, b in zip(mine, mine[1:]))                  # heaviest first
        if G % 8 == 0 and 8 % n_kv == 0:
            assert all(it[0] == w % n_kv for it in mine)
    steps = [sum(2 * (qb + 1) for _, _, qb in mine) for mine in sched]
    if (n_kv, batch, nqb, G) in ((8, 8, 19, 256), (8, 1, 145, 256)):             # bench.py --config 4 / 5: 98 vs 95.0, 686 vs 661.6 steps
        assert max(steps) <= 1.04 * sum(steps) / G                               # snake order ~ longest-processing-time first


def _xcd_rows_deal(tiles_m, tiles_n, n_fast=True):
    """gemm.hip:xcd_rows_tile restated: workgroup b of the padded grid -> (row tile, column tile) or None (surplus workgroup)."""
    grid = 8 * ((tiles_m + 7) // 8) * tiles_n
    q, r = tiles_m >> 3, tiles_m & 7
    out = []
    for b in range(grid):
        xcd, j = b & 7, b >> 3
        first = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        cnt = q + (1 if xcd < r else 0)
        if j >= cnt * tiles_n:
            out.append(None)
        elif n_fast:
            out.append((first + j // tiles_n, j % tiles_n))
        else:
            out.append((first + j % cnt, j // cnt))
    return out


@pytest.mark.parametrize("tiles_m,tiles_n", [(46, 4), (91, 4), (1, 4), (3, 4), (8, 4), (12, 1), (23, 4), (181, 4), (46, 16)])
def test_xcd_owned_rows_deal_covers_every_tile_once_and_keeps_a_row_tile_in_one_l2(tiles_m, tiles_n):
    """Round 4's tile deal of the ping-pong GEMM (fc2: 46 x 4 tiles at the 20-crop half batch): every tile exactly once; all column
    tiles of a row tile run on ONE XCD (workgroup id mod 8), back to back, so the activation panel crosses the fabric once; an XCD
    owns a contiguous run of row tiles, as even as 8 allows; surplus workgroups of the padded grid are < 8 x tiles_n."""
    for n_fast in (True, False):
        deal = _xcd_rows_deal(tiles_m, tiles_n, n_fast)
        real = [t for t in deal if t is not None]
        assert len(real) == tiles_m * tiles_n and len(set(real)) == len(real)
        assert len(deal) - len(real) < 8 * tiles_n
        owner = {}
        for b, t in enumerate(deal):
            if t is not None:
                assert owner.setdefault(t[0], b & 7) == b & 7
        per_xcd = [sorted(tm for tm, x in owner.items() if x == xcd) for xcd in range(8)]
        assert all(rows == list(range(rows[0], rows[0] + len(rows))) for rows in per_xcd if rows)
        assert max(map(len, per_xcd)) - min(map(len, per_xcd)) <= 1
    deal = _xcd_rows_deal(tiles_m, tiles_n, True)
    for b, t in enumerate(deal):                                   # N fastest: the column tiles of a row tile are 8 workgroup ids apart
        if t is not None and t[1] + 1 < tiles_n:
            assert deal[b + 8] == (t[0], t[1] + 1)


@pytest.mark.parametrize("tiles_m,tiles_n", [(91, 16), (91, 12), (91, 4), (181, 16), (46, 4), (5, 4), (8, 3), (1, 1), (23, 16), (108, 16)])
def test_balanced_xcd_row_deal_covers_every_tile_once_and_is_even(tiles_m, tiles_n):
    """Round 5's rejected balanced XCD row deal of the direct-B GEMM (FINDINGS.md), restated: workgroup b runs on XCD
    b & 7; every (row tile, column tile) exactly once, surplus workgroups exit; the XCDs' tile counts differ by at most the rounding of
    the left-over share; a whole-owned row tile's column tiles all sit on ONE XCD."""
    q, r = tiles_m >> 3, tiles_m & 7
    own, left = q * tiles_n, r * tiles_n
    per = (left + 7) >> 3
    grid = 8 * (own + per)
    seen, per_xcd = {}, [0] * 8
    for b in range(grid):
        xcd, j = b & 7, b >> 3
        if j < own:
            t = (xcd * q + j % q, j // q)
        else:
            e = (j - own) + xcd * per
            if j - own >= per or e >= left:
                continue
            t = (8 * q + e % r, e // r)
        assert t not in seen and t[0] < tiles_m and t[1] < tiles_n
        seen[t] = xcd
        per_xcd[xcd] += 1
    assert len(seen) == tiles_m * tiles_n
    assert max(per_xcd) - min(per_xcd) <= per                        # e.g. 91 x 16: 182 tiles on every XCD
    for tm in range(8 * q):
        assert len({seen[(tm, tn)] for tn in range(tiles_n)}) == 1


@pytest.mark.parametrize("heads,batch,qsplit", [(16, 20, 2), (16, 5, 2), (16, 40, 2), (16, 3, 2), (16, 20, 1), (12, 7, 2), (16, 9, 3)])
def test_attention_partner_redeal_is_a_bijection_and_pairs_share_an_xcd(heads, batch, qsplit):
    """attention.hip:attn64r_kernel's re-deal (round 4): launch-order id L -> (head, crop, query part).  Every triple exactly once;
    when heads x crops is a multiple of 8 the parts of one (crop, head) are ids 8 apart: same XCD, neighbours in dispatch order."""
    seen = {}
    for L in range(heads * batch * qsplit):
        h, b, z = L % heads, (L // heads) % batch, L // (heads * batch)
        if qsplit > 1 and (heads * batch) % 8 == 0:
            j = L >> 3
            p = (j // qsplit) * 8 + (L & 7)
            z, h, b = j % qsplit, p % heads, p // heads
        assert (h, b, z) not in seen and h < heads and b < batch and z < qsplit
        seen[(h, b, z)] = L
    assert len(seen) == heads * batch * qsplit
    if qsplit > 1 and (heads * batch) % 8 == 0:
        for (h, b, z), L in seen.items():
            if z + 1 < qsplit:
                assert seen[(h, b, z + 1)] == L + 8


def test_ctypes_mirrors_match_the_header_layout(tmp_path):
    """slime_amd/_lib.py mirrors the header's argument structs and enums by hand.  A C program compiled against include/slime_hip.h
    prints sizeof / offsetof of every struct field and the enum values; the ctypes classes must agree field by field (a field added
    to one side only, or in another order, would silently shift every later pointer)."""
    import re
    import shutil
    import subprocess
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    pairs = {"slime_gemm_args": _lib.GemmArgs, "slime_vit_desc": _lib.VitDesc, "slime_resampler_desc": _lib.ResamplerDesc,
             "slime_mlp_desc": _lib.MlpDesc, "slime_llama_attn_desc": _lib.LlamaAttnDesc, "slime_probe": _lib.Probe}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {']
    for cname, cls in pairs.items():
        assert re.search(r"}\s*" + cname + r"\s*;", text), cname
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    epi_block = text[text.index("SLIME_EPI_BIAS_T"):]
    epi_block = epi_block[:epi_block.index("}")]                                  # the epilogue enum's body
    enums = ["SLIME_BF16", "SLIME_F16", "SLIME_F32", "SLIME_U8", "SLIME_ABI_VERSION"] + list(dict.fromkeys(re.findall(r"SLIME_EPI_[A-Z0-9_]+", epi_block)))
    for e in enums:
        lines.append(f'printf("{e} %d\\n", (int){e});')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == __import__("ctypes").sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert (int(got["SLIME_BF16"]), int(got["SLIME_F16"]), int(got["SLIME_F32"]), int(got["SLIME_U8"])) == (_lib.BF16, _lib.F16, _lib.F32, _lib.U8)
    assert int(got["SLIME_ABI_VERSION"]) == _lib.ABI_VERSION
    epi = [e for e in enums if e.startswith("SLIME_EPI_")]
    assert len(epi) == 9
    for e in epi:
        assert int(got[e]) == getattr(_lib, e[len("SLIME_"):]), e


def test_weight_residency_policy(monkeypatch):
    """ops.pack_static (round 5): a weight whose fragment-order image exists is resident ONCE -- the row-major tensor is dropped --
    unless SLIME_KEEP_ROW_MAJOR=1; a weight the library cannot run from its image alone keeps its row-major tensor; and
    packed_weight_bytes counts every tensor once.  (The packing itself is a device kernel: a stand-in here.)"""
    import torch
    from slime_amd import ops
    made = []

    def fake_pack(w):
        if w is None or w.shape[-2] % 64 or w.shape[-1] % 64:
            return None
        made.append(tuple(w.shape))
        return w.clone()
    monkeypatch.setattr(ops, "pack_b_frag", fake_pack)
    monkeypatch.delenv("SLIME_KEEP_ROW_MAJOR", raising=False)
    T = {"w_a": torch.zeros(2, 128, 64, dtype=torch.bfloat16), "w_b": torch.zeros(96, 64, dtype=torch.bfloat16), "bias": torch.zeros(128)}
    ops.pack_static(T, ("w_a", "w_b"))
    assert T["w_a"] is None and T["w_a_frag"] is not None            # one copy: the fragment image
    assert T["w_b"] is not None and T["w_b_frag"] is None            # 96 rows: not packable, stays row-major
    assert ops.packed_weight_bytes(T) == 2 * 128 * 64 * 2 + 96 * 64 * 2 + 128 * 4
    assert ops.packed_weight_bytes(T, T) == ops.packed_weight_bytes(T)          # a tensor shared by two packs counts once
    monkeypatch.setenv("SLIME_KEEP_ROW_MAJOR", "1")
    T2 = {"w_a": torch.zeros(128, 64, dtype=torch.bfloat16)}
    ops.pack_static(T2, ("w_a",))
    assert T2["w_a"] is not None and T2["w_a_frag"] is not None and ops.keep_row_major()
    with pytest.raises(ValueError, match="static operand"):
        ops.gemm(torch.zeros(4, 64), None, None, 0)


@pytest.mark.parametrize("nw,nh,merge", [(2, 2, True), (2, 3, True), (4, 4, True), (1, 2, True), (2, 2, False)])
def test_adapter_row_map_restates_the_spatial_merge(nw, nh, merge):
    """rowwise.hip: adapter_row_map_kernel (round 5), restated: GEMM row r of projection[2]'s output [global rows of every image | local
    rows of every image] -> row of the [images, stride, H] token buffer.  Held against the oracle's spatial_merge (llava_arch.py:235-244)
    and the flat order (:233-234): scattering row ids through the map must reproduce cat(global, merged local) per image."""
    import torch
    from oracle import slime_oracle as O
    images, P, g = 3, 576, 12
    n_local, q = nw * nh, g * g
    stride = P + n_local * q + 5                                      # a wider token buffer: the extra rows stay untouched
    rows_g, rows_l, per = images * P, images * n_local * q, n_local * q
    dst = []
    for r in range(rows_g + rows_l):                                  # the kernel's arithmetic
        if r < rows_g:
            dst.append((r // P) * stride + r % P)
        else:
            qq = r - rows_g
            b, rr = qq // per, qq % per
            d = rr
            if merge:
                qx, qy, k = rr % g, (rr // g) % g, rr // (g * g)
                gx, gy = k % nw, k // nw
                d = ((gy * g + qy) * nw + gx) * g + qx
            dst.append(b * stride + P + d)
    assert len(set(dst)) == len(dst)                                  # a scatter without collisions
    buf = torch.full((images * stride, 1), -1.0)
    buf[torch.tensor(dst)] = torch.arange(rows_g + rows_l, dtype=torch.float32)[:, None]
    buf = buf.view(images, stride)
    for b in range(images):
        glob = torch.arange(b * P, (b + 1) * P, dtype=torch.float32)
        loc = torch.arange(rows_g + b * per, rows_g + (b + 1) * per, dtype=torch.float32).view(n_local, q, 1)
        want_loc = O.spatial_merge(loc, nw, nh, g).view(-1) if merge else loc.view(-1)
        assert torch.equal(buf[b, :P], glob) and torch.equal(buf[b, P:P + per], want_loc) and bool((buf[b, P + per:] == -1).all())


@pytest.mark.parametrize("dt,bits", [(torch.bfloat16, 16), (torch.float16, 19)])
def test_split_residual_stream_keeps_the_stated_bits(dt, bits):
    """The split residual stream (ABI 7: hi = T(c) + ONE signed byte) as arithmetic, on the CPU, through the torch
    restatement of csrc/common.h (ops.resid_split / ops.resid_join): over the tower's 46 residual updates against an fp32 stream fed the
    same increments.  The byte is the floor of the pattern distance from hi in units of 2^SH, read back at its cell's centre, so every
    update loses at most ulp(hi) / 512 -- 2^-bits of |c| (bf16 16 bits, fp16 19) -- in EVERY case (ties, binade boundaries, either
    sign), without bias, and the drift of the whole chain stays two orders below the 2^-9 / 2^-12 operand rounding the MFMAs apply to hi."""
    from slime_amd import ops
    g = torch.Generator().manual_seed(0)
    h32 = torch.randn(64, 1024, generator=g) * 1.5
    h32[:, 7] *= 60.0                                                 # an outlier channel
    h32[0, :8] = torch.tensor([0.0, -0.0, 1.0, -2.0, 1.0 - 2.0 ** -9, 2.0 + 2.0 ** -7, -(1.0 + 2.0 ** -8), 3e-5])   # exact values, ties at a binade seam, a small one
    hi, lo = ops.resid_split(h32, dt)
    assert lo.dtype == torch.int8 and torch.equal(hi, h32.to(dt))
    worst, mean_err = 0.0, 0.0
    for step in range(46):
        delta = torch.randn(64, 1024, generator=g) * 0.25
        h32 = h32 + delta
        c = delta + ops.resid_join(hi, lo)                            # the epilogue: acc + (bias + join(hi, lo8))
        hi, lo = ops.resid_split(c, dt)
        assert torch.equal(hi, c.to(dt))                              # the GEMM operand is T(c), whatever the lower part is
        back = ops.resid_join(hi, lo)
        ulp = torch.maximum(hi.float().abs(), torch.tensor(2.0 ** -120)).log2().floor().exp2() * 2.0 ** -(7 if dt == torch.bfloat16 else 10)
        # below fp16's normal range (|hi| < 2^-14) hi's spacing is fixed at 2^-24 while the byte counts cells of hi's fp32 pattern: there the
        # stream keeps what hi keeps (|c - hi| <= 2^-25, the old 16-bit lower part bottomed out at the same spacing) -- six orders below the stream's values
        normal = hi.float().abs() >= (2.0 ** -14 if dt == torch.float16 else 2.0 ** -120)
        err = (back - c).abs()
        assert bool((err[normal] <= (ulp / 512)[normal]).all())       # half a cell of ulp(hi) / 256, in every case
        assert bool((err[normal] <= (c.abs() * 2.0 ** -bits)[normal]).all()) and bool((err[~normal] <= 2.0 ** -25).all())
        mean_err += float((back.double() - c.double()).mean() / c.abs().double().mean())
        worst = max(worst, float((back.double() - h32.double()).norm() / h32.double().norm()))
    assert worst < (6e-5 if dt == torch.bfloat16 else 8e-6)           # end of chain vs the fp32 stream: << 2^-9 = 2e-3 / 2^-12 = 2.4e-4
    assert abs(mean_err / 46) < 2.0 ** -(bits + 4)                    # centre-of-cell read-back: no systematic drift


def test_fragment_staging_feeds_the_same_operands_as_row_major_staging():
    """gemm.hip, round 5, restated on the host: the LDS-staged kernels stage a B tile either from the row-major image (LDS row rho holds
    weight row nphys(rho), its eight 16-byte k-chunks XOR-swizzled) or by copying whole fragments of the slime_gemm_pack_b image (LDS =
    [16-row block][k-step][lane]).  For every lane of every fragment read both forms must hand the MFMA the same weight row and the same
    eight k -- that is why the two are bit-identical -- and frag_piece_offset must address the documented unit
    ((t K/32 + s) 4 + f) 64 + lane of the image."""
    import numpy as np
    N, K = 256, 192                                                   # 4 fragment tiles of 64 rows, 6 k-steps = 3 k-tiles
    W = (np.arange(N * K, dtype=np.int64)).reshape(N, K)              # element id = n K + k
    KS = K // 32
    img = np.empty((N // 64, KS, 4, 64, 8), dtype=np.int64)           # include/slime_hip.h: out[((t KS + s) 4 + f) 64 + lane] (16-byte units)
    for t in range(N // 64):
        for s in range(KS):
            for f in range(4):
                for lane in range(64):
                    row = 64 * t + 32 * (f >> 1) + 8 * ((lane & 15) >> 2) + 4 * (f & 1) + (lane & 3)
                    img[t, s, f, lane] = W[row, 32 * s + 8 * (lane >> 4): 32 * s + 8 * (lane >> 4) + 8]
    flat = img.reshape(-1, 8)                                         # one row per 16-byte unit

    def frag_piece_offset(blk, ks):                                   # bytes, relative to the tile's first fragment (gemm.hip)
        return (((blk >> 2) * (K >> 5) + ks) * 4 + (blk & 3)) * 1024
    for ktile in range(K // 64):
        for blk in range(N // 16):                                    # 16-row MFMA block of the tile = 4 t + f
            for ks in range(2):                                       # k-step inside the 64-wide k-tile
                unit0 = (frag_piece_offset(blk, ks) + ktile * 8192) // 16
                assert unit0 == (((blk >> 2) * KS + 2 * ktile + ks) * 4 + (blk & 3)) * 64
                for lane in range(64):
                    lq, li = lane >> 4, lane & 15
                    got = flat[unit0 + lane]                          # whole-fragment copy: LDS[block][ks][lane] = image unit, read by lane `lane`
                    # the row-major form: LDS row rho = 16 blk + li holds weight row nphys(rho); the lane reads chunk 4 ks + lq of the k-tile
                    rho = 16 * blk + li
                    nl = rho & 15
                    nphys = (rho & ~31) + 8 * (nl >> 2) + 4 * ((rho >> 4) & 1) + (nl & 3)
                    k0 = 64 * ktile + 32 * ks + 8 * lq
                    assert np.array_equal(got, W[nphys, k0:k0 + 8]), (ktile, blk, ks, lane)
