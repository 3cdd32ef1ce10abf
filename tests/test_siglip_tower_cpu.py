"""SigLIP vision towers without a GPU (helpers: tests/siglip_tower_conformance.py).

  1. ABI: the new entries' prototypes and SLIME_EPI_BIAS_GELU_TANH_T == 9 against the header through a C compiler; ABI version and
     ``slime_vit_desc`` as they were.
  2. Refusals of ``slime_siglip_*`` and ``slime_patch_embed_plain``, all before any device work: non-NULL cls / pre_ln_*, bad
     geometry, no output, workspace.
  3. Loader: a SigLIP directory written here (prefixed / flat keys, nested ``vision_config``, ``delay_load``, ``head.*`` present and
     absent); the named pack-time refusals; ``cls_patch``; builder routing (a CLIP directory still yields ``CLIPVisionTower``).
  4. ``SiglipImageProcessor`` bit-equal to transformers' PIL backend on non-square images; ``process_images`` in every mode; the
     device mode that would centre-crop refuses this processor.
  5. The per-element bound of fold + tanh-GELU: the share of pre-activations in [-5, -2.5], the exact reference and the fp32
     emulation inside, the erf and quick restatements outside, both dtypes.
  6. The float64 replay of the packed tower against HF ``SiglipVisionModel`` under a derived bound, with broken variants.
"""
import ctypes as C
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import gemm_conformance as GC
import siglip_tower_conformance as S
import tower_conformance as TC

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}

# ------------------------------------------------------------------------------------------------ 1. ABI
PROTOS = {
    "slime_siglip_check": ("int", ["const slime_vit_desc*"]),
    "slime_siglip_workspace_bytes": ("size_t", ["const slime_vit_desc*", "int"]),
    "slime_siglip_ksplit_workspace_bytes": ("size_t", ["const slime_vit_desc*", "int", "const slime_vit_ksplit*"]),
    "slime_siglip_forward": ("int", ["const slime_vit_desc*", "const void*", "int", "int", "void*", "int", "float*", "float*",
                                     "const slime_vit_ksplit*", "void*", "size_t", "void*"]),
    "slime_patch_embed_plain": ("int", ["const void*", "int", "const void*", "const float*", "float*", "void*", "void*", "float*", "int",
                                        "int", "int", "int", "int", "int", "void*"]),
}


def _ctype_for(decl):
    from slime_amd import _lib
    return {"const slime_vit_desc*": C.POINTER(_lib.VitDesc), "const slime_vit_ksplit*": C.POINTER(_lib.VitKsplit), "int": C.c_int,
            "size_t": C.c_size_t}.get(decl, C.c_void_p)


def test_new_entries_and_the_epilogue_code_mirror_the_header(tmp_path):
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"']
    for name, (res, args) in PROTOS.items():
        r, a = _lib._SIGNATURES[name]
        assert r is _ctype_for(res) and list(a) == [_ctype_for(d) for d in args], name
        # an assignment between function pointer types of different parameter lists does not compile under -Werror
        lines.append(f'static {res} (*const p_{name})({", ".join(args)}) = {name};')
    lines += ['int main(void) {', 'printf("tanh %d\\n", (int)SLIME_EPI_BIAS_GELU_TANH_T);',
              'printf("split %d\\n", (int)SLIME_EPI_BIAS_RESID_SPLIT_LN);', 'printf("abi %d\\n", (int)SLIME_ABI_VERSION);',
              'printf("desc %zu\\n", sizeof(slime_vit_desc));', 'printf("opts %zu\\n", sizeof(slime_vit_opts));',
              'return ' + " || ".join(f"p_{n} == 0" for n in PROTOS) + ';', '}']
    src = tmp_path / "siglip.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Werror", "-c", "-o", str(tmp_path / "siglip.o"), str(src)], check=True)       # the prototypes
    probe = tmp_path / "probe.c"
    text = src.read_text()
    for name in PROTOS:
        text = text.replace(f"= {name};", "= 0;")
    probe.write_text(text)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(probe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["tanh"]) == _lib.EPI_BIAS_GELU_TANH_T == S.EPI_BIAS_GELU_TANH_T == 9 and int(got["split"]) == 8
    assert int(got["abi"]) == _lib.ABI_VERSION == _lib.load().slime_abi_version() == 7
    assert int(got["desc"]) == C.sizeof(_lib.VitDesc) and len(_lib.VitDesc._fields_) == 29
    assert int(got["opts"]) == C.sizeof(_lib.VitOpts) and [f for f, _ in _lib.VitOpts._fields_] == ["act"]
    assert set(PROTOS) <= set(_lib.header_symbols())


# ------------------------------------------------------------------------------------------------ 2. refusals
def _desc(image=384, patch=16, hidden=1024, heads=16, inter=4096, layers=2):
    """A SigLIP descriptor over fake addresses (the checks never dereference): cls / pre_ln_* NULL, as the convention says."""
    from slime_amd import _lib
    d = _lib.VitDesc()
    d.hidden, d.inter, d.heads, d.layers_run, d.image, d.patch = hidden, inter, heads, layers, image, patch
    d.kpad, d.dtype, d.eps = (3 * patch * patch + 63) // 64 * 64, _lib.BF16, 1e-6
    for name, tp in _lib.VitDesc._fields_:
        if tp is C.c_void_p and name not in ("patch_w", "cls", "pre_ln_w", "pre_ln_b"):
            setattr(d, name, 0x1000)
    return d


def _err():
    from slime_amd import _lib
    return _lib.load().slime_last_error().decode()


def test_siglip_check_geometry_and_the_null_convention():
    from slime_amd import _lib
    lib = _lib.load()
    for image, hidden, heads, inter in ((224, 768, 12, 3072), (256, 768, 12, 3072), (384, 768, 12, 3072), (256, 1024, 16, 4096),
                                        (384, 1024, 16, 4096)):                                   # the five released patch-16 geometries
        assert lib.slime_siglip_check(C.byref(_desc(image=image, hidden=hidden, heads=heads, inter=inter))) == 0, _err()
    for field in ("cls", "pre_ln_w", "pre_ln_b"):
        d = _desc()
        setattr(d, field, 0x1000)
        assert lib.slime_siglip_check(C.byref(d)) == -1 and field in _err() and "NULL" in _err(), _err()
    assert lib.slime_vit_check(C.byref(_desc())) == -1 and "missing embedding weights" in _err()    # and the CLIP entries want them
    for bad, word in ((_desc(hidden=1152, heads=16, inter=4304, image=378, patch=14), "hidden=1152"),       # so400m-patch14
                      (_desc(heads=8), "head_dim"), (_desc(image=512), "patches per side"), (_desc(inter=4304), "multiple of 128"),
                      (_desc(image=380), "not a multiple of patch"), (_desc(patch=32, image=384), "16-bit offset table")):
        assert lib.slime_siglip_check(C.byref(bad)) == -1
        assert word in _err(), _err()
    d = _desc()
    d.pos = None
    assert lib.slime_siglip_check(C.byref(d)) == -1 and "missing embedding weights" in _err()
    assert lib.slime_siglip_check(None) == -1 and "null descriptor" in _err()


def test_siglip_forward_refusals_need_no_device():
    from slime_amd import _lib
    lib = _lib.load()
    d, px = _desc(), 0x1000

    def call(desc, out=0x2000, hidden=None, states=None, ks=None, ws=None, nbytes=0, n=1, pix=_lib.F32, odt=_lib.F32):
        return lib.slime_siglip_forward(desc, px, pix, n, out, odt, hidden, states, ks, ws, nbytes, None)

    assert call(C.byref(d), out=None) == -1 and "no output requested" in _err()
    assert call(None) == -1 and "null descriptor" in _err()
    assert call(C.byref(d), n=0) == -1 and "bad input" in _err()
    assert call(C.byref(d), odt=_lib.U8) == -1 and "out dtype" in _err()
    for field in ("cls", "pre_ln_w", "pre_ln_b"):
        bad = _desc()
        setattr(bad, field, 0x1000)
        assert call(C.byref(bad)) == -1 and field in _err()
    assert call(C.byref(_desc(image=512))) == -1 and "patches per side" in _err()
    ks = _lib.VitKsplit(2, 1, 99, 1)
    assert call(C.byref(d), ks=C.byref(ks)) == -1 and "fc1=99" in _err()
    # a valid call up to the workspace: refused there (SLIME_EWORKSPACE = -2), still before any launch
    need = lib.slime_siglip_workspace_bytes(C.byref(d), 1)
    assert call(C.byref(d)) == -2 and "workspace" in _err() and str(need) in _err()
    assert call(C.byref(d), ws=0x10000, nbytes=need - 1) == -2 and call(C.byref(d), ws=0x10010, nbytes=need) == -2
    # the size is that of S = P rows: one row per crop fewer than the CLIP layout's at the same geometry
    P, D, F = 576, 1024, 4096
    rows = lambda M: sum((b + 255) // 256 * 256 for b in (M * D, M * D * 2, max(M * F * 2, (M * 3 * D * 2 + 255) // 256 * 256 + M * D * 2),
                                                        M * (D // 64) * 8))
    assert need == rows(P) and lib.slime_siglip_workspace_bytes(C.byref(d), 3) == rows(3 * P)
    ks = _lib.VitKsplit(2, 1, 2, 4)
    part = max(lib.slime_gemm_ksplit_workspace_bytes(P, n_, s) for n_, s in ((3 * D, 2), (D, 1), (F, 2), (D, 4)))
    assert lib.slime_siglip_ksplit_workspace_bytes(C.byref(d), 1, C.byref(ks)) == need + part
    assert lib.slime_siglip_workspace_bytes(None, 1) == 0 and lib.slime_siglip_workspace_bytes(C.byref(d), 0) == 0
    # the primitive: the same geometry limits, named
    pe = lambda image=384, patch=16, kpad=768, D=1024, x16=0x3000, pos=0x4000: lib.slime_patch_embed_plain(
        px, _lib.F32, 0x2000, pos, None, x16, None, None, _lib.BF16, 1, image, patch, kpad, D, None)
    assert pe(image=512) == -1 and "patches per side" in _err()
    assert pe(kpad=704) == -1 and "kpad" in _err()
    assert pe(x16=None) == -1 and "no output requested" in _err()
    assert pe(pos=None) == -1 and "bad input" in _err()
    assert pe(D=512) == -1 and "D=512" in _err()


def test_gemm_accepts_the_new_epilogue_code_and_still_refuses_unknown_ones():
    """Argument checks only (fake pointers; every call ends at a refusal that precedes the launch)."""
    from slime_amd import _lib
    lib = _lib.load()
    g = _lib.GemmArgs(A=0x1000, lda=64, B=0x2000, bias=0x3000, C=0x4000, ldc=128, M=4, N=128, K=64, dtype=_lib.BF16,
                      epilogue=_lib.EPI_BIAS_GELU_TANH_T, ln_stats=0x5000, ln_groups=2, ln_colsum=0x6000, ln_eps=1e-6)
    assert lib.slime_gemm_ex(C.byref(g), None) == -1 and "ln_groups=2" in _err()      # past the fold's allow-list: the next check speaks
    g.epilogue = _lib.EPI_BIAS_F32
    assert lib.slime_gemm_ex(C.byref(g), None) == -1 and "BIAS_GELU_TANH_T" in _err()  # the allow-list names the new form
    g.epilogue, g.ln_stats, g.dtype = 10, None, _lib.F32
    assert lib.slime_gemm_ksplit(C.byref(g), 1, None, 0, None) == -1 and "dtype" in _err()
    g.K, g.lda = 128, 128
    assert lib.slime_gemm_ksplit(C.byref(g), 2, None, 0, None) == -1 and "unknown epilogue 10" in _err()


# ------------------------------------------------------------------------------------------------ 3. loader
LOADER_CFGS = {"128": (64, 16, 128, 256, 2), "768": (64, 16, 768, 1536, 1)}        # image, patch, D, inter, layers


def _tower(path, feature="patch", **kw):
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    return build_vision_tower(SimpleNamespace(mm_vision_tower=str(path), mm_vision_select_layer=-2, mm_vision_select_feature=feature), **kw)


@pytest.mark.parametrize("head", [True, False], ids=["head", "no_head"])
@pytest.mark.parametrize("keys", ["prefixed", "flat"])
@pytest.mark.parametrize("nested", [False, True], ids=["flat_config", "vision_config"])
@pytest.mark.parametrize("geom", sorted(LOADER_CFGS))
def test_siglip_tower_loads_from_hf_directory(tmp_path, geom, nested, keys, head):
    from slime_amd import weights as W
    from slime_amd.image_processor import SiglipImageProcessor
    from slime_amd.model.multimodal_encoder.siglip_encoder import SigLipVisionTower
    cfg = S.siglip_config(*LOADER_CFGS[geom])
    sd = W.make_siglip_state_dict(cfg, seed=21, head=head)
    assert any("head." in k for k in sd) == head and cfg.seq_len == cfg.num_patches == 16
    S.write_hf_dir(tmp_path, sd if keys == "prefixed" else W.strip_tower_prefix(sd), cfg, nested)
    t = _tower(tmp_path)
    assert isinstance(t, SigLipVisionTower) and t.is_loaded and t.config == cfg and t.hidden_size == cfg.hidden_size
    assert t.num_patches == 16 and t.num_patches_per_side == 4 and t.select_feature == "patch"
    assert isinstance(t.image_processor, SiglipImageProcessor) and t.image_processor.crop_size == {"height": 64, "width": 64}
    got = t.vision_tower.state_dict()
    assert not any("head." in k or "class_embedding" in k or "pre_layrnorm" in k for k in got)
    for k, v in sd.items():
        if "head." not in k:
            assert torch.equal(got[k], v), k
    d = _tower(tmp_path, delay_load=True)
    assert not d.is_loaded and d.config == cfg and d.hidden_size == cfg.hidden_size and d.num_patches == 16
    d.load_model()
    assert d.is_loaded and torch.equal(d.vision_tower.state_dict()["vision_model.embeddings.patch_embedding.bias"],
                                       sd["vision_model.embeddings.patch_embedding.bias"])


REFUSED = {"hidden_act": (dict(hidden_act="gelu"), ("'gelu'", "gelu_pytorch_tanh")),
           "head_dim": (dict(hidden_size=1152, num_attention_heads=16), ("head_dim=72", "64")),
           "grid": (dict(image_size=512), ("32 patches per side", "24")),
           "inter": (dict(intermediate_size=4304), ("intermediate_size=4304", "128"))}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_unsupported_siglip_towers_are_refused_by_name(tmp_path, what):
    """so400m-patch14 (head_dim 72, intermediate 4304, 27 per side) and base-patch16-512 are out of scope: refused when loaded and
    when packed, before any device work, the offending value named."""
    import dataclasses
    from slime_amd import ops, weights as W
    over, words = REFUSED[what]
    good = S.siglip_config(*LOADER_CFGS["128"])
    bad = dataclasses.replace(W.SiglipVisionConfig(), **over) if what != "hidden_act" else dataclasses.replace(good, **over)
    with pytest.raises(ValueError) as e:
        ops.check_siglip_config(bad)
    assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ValueError, match=words[0]):
        ops.pack_siglip_tower({}, bad, torch.bfloat16, "cpu")
    S.write_hf_dir(tmp_path, W.make_siglip_state_dict(good, seed=21), good, False, **over)
    with pytest.raises(ValueError, match=words[0]):
        _tower(tmp_path)
    assert getattr(_tower(tmp_path, delay_load=True).config, list(over)[0]) == list(over.values())[0]   # the config itself is readable
    ops.check_siglip_config(good)


def test_cls_patch_raises_at_construction_and_the_builder_routes(tmp_path):
    import gelu_tower_conformance as G
    from slime_amd import weights as W
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower, is_siglip_tower
    from slime_amd.model.multimodal_encoder.clip_encoder import CLIPVisionTower
    from slime_amd.model.multimodal_encoder.siglip_encoder import SigLipVisionTower
    sig, clip = tmp_path / "sig", tmp_path / "clip"
    sig.mkdir(), clip.mkdir()
    cfg = S.siglip_config(*LOADER_CFGS["128"])
    S.write_hf_dir(sig, W.make_siglip_state_dict(cfg, seed=21), cfg)
    for delay in (False, True):
        with pytest.raises(ValueError, match="cls_patch"):
            _tower(sig, feature="cls_patch", delay_load=delay)
    ccfg = G.vision_config(56, 14, 128, 256, 2, act="quick_gelu")
    G.write_hf_dir(clip, W.make_tower_state_dict(ccfg, seed=21), ccfg)
    t = _tower(clip)
    assert type(t) is CLIPVisionTower and t.config == ccfg and not is_siglip_tower(str(clip))
    assert type(_tower(clip, feature="cls_patch")) is CLIPVisionTower
    # a checkpoint of the other layout does not load silently (shapes or keys: torch's or the loader's RuntimeError)
    G.write_hf_dir(clip, W.make_siglip_state_dict(cfg, seed=21), ccfg)
    with pytest.raises(RuntimeError):
        _tower(clip)
    S.write_hf_dir(sig, W.make_tower_state_dict(ccfg, seed=21), cfg)
    with pytest.raises(RuntimeError):
        _tower(sig)
    # ... nor one with the right shapes and a class token / pre-LayerNorm on top
    extra = dict(W.make_siglip_state_dict(cfg, seed=21), **{"vision_model.embeddings.class_embedding": torch.zeros(128),
                                                          "vision_model.pre_layrnorm.weight": torch.ones(128)})
    S.write_hf_dir(sig, extra, cfg)
    with pytest.raises(RuntimeError, match="SigLIP ViT layout"):
        _tower(sig)
    # names: the stand-in, hub-style names (local cache only: absent here), everything else where it went before
    assert is_siglip_tower("synthetic-siglip:5") and is_siglip_tower("google/siglip-large-patch16-384") and not is_siglip_tower("synthetic:5")
    args = lambda name: SimpleNamespace(mm_vision_tower=name, mm_vision_select_layer=-2, mm_vision_select_feature="patch")
    d = build_vision_tower(args("synthetic-siglip:5"), delay_load=True)
    assert type(d) is SigLipVisionTower and d.config == W.SIGLIP_L_384 and d.num_patches == 576 and d.hidden_size == 1024
    assert type(build_vision_tower(args("synthetic:5"), delay_load=True)) is CLIPVisionTower
    with pytest.raises(FileNotFoundError, match="offline"):
        build_vision_tower(args("google/siglip-large-patch16-384"))
    with pytest.raises(ValueError, match="Unknown vision tower"):
        build_vision_tower(args("facebook/dinov2-large"))


def test_pos_prime_is_one_fp32_addition_and_the_layers_fold_as_pack_tower_does():
    from slime_amd import ops, weights as W
    cfg = S.siglip_config(*LOADER_CFGS["128"])
    sd = W.make_siglip_state_dict(cfg, seed=4)
    flat = W.strip_tower_prefix(sd)
    T = ops.siglip_host_tensors(sd, cfg, torch.bfloat16, 2)
    assert set(T) == {"patch_w", "pos", "w_qkv", "b_qkv", "colsum_qkv", "w_o", "b_o", "w_fc1", "b_fc1", "colsum_fc1", "w_fc2", "b_fc2"}
    want = flat["embeddings.position_embedding.weight"] + flat["embeddings.patch_embedding.bias"][None]
    assert T["pos"].dtype == torch.float32 and T["pos"].shape == (16, 128) and torch.equal(T["pos"], want)
    assert T["patch_w"].shape == (128, 768) and T["patch_w"].dtype == torch.bfloat16         # kpad = 3 * 16^2: no zero column
    assert torch.equal(T["patch_w"], flat["embeddings.patch_embedding.weight"].reshape(128, 768).to(torch.bfloat16))
    # the layer tensors are tower_host_tensors' of a CLIP state dict with the same layers
    clip = dict(flat)
    clip.update({"embeddings.class_embedding": torch.zeros(128), "pre_layrnorm.weight": torch.ones(128), "pre_layrnorm.bias": torch.zeros(128)})
    ref = ops.tower_host_tensors(clip, W.VisionConfig(128, 256, 2, 2, 64, 16, 1e-6), torch.bfloat16, 2)
    for k in T:
        if k not in ("pos", "patch_w"):
            assert torch.equal(T[k], ref[k]), k
    assert ops.siglip_host_tensors(sd, cfg, None, 1)["pos"].dtype == torch.float64


# ------------------------------------------------------------------------------------------------ 4. image processor
def _images():
    from PIL import Image
    rng = np.random.RandomState(5)
    return [Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in ((300, 200), (97, 411), (64, 64), (500, 167))]


@pytest.mark.parametrize("size,resample", [(64, 3), (224, 3), (384, 3), (96, 2)])
def test_image_processor_is_bit_equal_to_transformers_pil_backend(tmp_path, size, resample):
    from transformers import SiglipImageProcessorPil
    from slime_amd import weights as W
    from slime_amd.image_processor import SiglipImageProcessor
    cfg = S.siglip_config(size, 16, 128, 256, 1) if size % 16 == 0 else None
    hf = SiglipImageProcessorPil(size={"height": size, "width": size}, resample=resample)
    ours = SiglipImageProcessor(size, resample=resample)
    if cfg is not None:                                     # read from the file the loader reads
        S.write_hf_dir(tmp_path, {"x": torch.zeros(1)}, cfg, resample=resample)
        ours = SiglipImageProcessor.from_pretrained(str(tmp_path))
    assert ours.crop_size == {"height": size, "width": size} and ours.size["shortest_edge"] == size
    assert ours.image_mean == [0.5] * 3 and ours.image_std == [0.5] * 3 and int(ours.resample) == resample
    ims = _images()
    for im in ims:
        a = ours.preprocess(im, return_tensors="pt")["pixel_values"]
        b = hf(im, return_tensors="pt")["pixel_values"]
        assert a.shape == b.shape == (1, 3, size, size) and a.dtype == b.dtype and torch.equal(a, b), im.size
    assert torch.equal(ours(ims, return_tensors="pt")["pixel_values"], hf(ims, return_tensors="pt")["pixel_values"])


def test_process_images_in_every_mode_and_the_device_refusal():
    """Host process_images: every view of every mode is the processor's own result on that view (so: resized to size x size, never
    centre-cropped); the bare device mode (shortest edge + centre crop) refuses this processor before touching a device."""
    from slime_amd import mm_utils as MU
    from slime_amd.image_processor import SiglipImageProcessor
    proc = SiglipImageProcessor(336)                        # the modes' fixed 336 geometry
    ims = _images()[:2]
    bg = tuple(int(x * 255) for x in proc.image_mean)
    one = lambda v: proc.preprocess(v, return_tensors="pt")["pixel_values"][0]
    for mode in ("pad", "pad_then_devide", "any_res", "anyres", None):
        cfg = SimpleNamespace(image_aspect_ratio=mode, image_grid_pinpoints="[(336, 672), (672, 336), (672, 672)]")
        out = MU.process_images(ims, proc, cfg)
        for i, im in enumerate(ims):
            views = {"pad": lambda: [MU.expand2square(im, bg)], "pad_then_devide": lambda: MU.process_image_naive(im, bg),
                     "any_res": lambda: MU.process_image_any_res(im, bg),
                     "anyres": lambda: [MU.anyres_canvas(im, proc)[0]] + MU.divide_to_patches(MU.anyres_canvas(im, proc)[1], 336),
                     None: lambda: [im]}[mode]()
            got = out[i] if out[i].dim() == 4 else out[i][None]
            assert got.shape == (len(views), 3, 336, 336), (mode, got.shape)
            for j, v in enumerate(views):
                assert torch.equal(got[j], one(v)), (mode, i, j)
    # the bare mode of a non-square image is NOT the centre crop
    from slime_amd.image_processor import ClipImageProcessor
    clip = ClipImageProcessor(336, 336, proc.image_mean, proc.image_std)
    assert not torch.equal(one(ims[0]), clip.preprocess(ims[0])["pixel_values"][0])
    with pytest.raises(ValueError, match="centre"):
        MU.process_images_device(ims, proc, SimpleNamespace(image_aspect_ratio=None), "cpu")
    with pytest.raises(ValueError, match="resample"):
        MU.process_images_device(ims, SiglipImageProcessor(336, resample=2), SimpleNamespace(image_aspect_ratio="pad"), "cpu")


# ------------------------------------------------------------------------------------------------ 5. the epilogue's bound
def _sample_shapes():
    ms = sorted(set(GC.m_table(64)) | set(GC.m_table(128)))
    return [(m, (128, 256)[i % 2], (64, 192)[(i // 2) % 2]) for i, m in enumerate(ms)] + [(17, 128, 2112)]


def test_the_form_is_not_in_the_shared_tables_and_the_three_forms_differ_in_the_tail():
    assert S.FORM not in GC.FORMS and S.FORM not in GC.WAVE_FORMS and S.FORM not in GC.OUT_T_FORMS
    c = S.make_case("random", torch.bfloat16, 5, 128, 64)
    f = c.arg_fields("B")
    assert c.epilogue == f["epilogue"] == 9 and c.fold and c.form == S.FORM and f["ln_stats"] and f["ln_colsum"] and f["ln_groups"] == 1
    # x sigmoid(2 c u) is F.gelu(approximate='tanh') and 0.5 x (1 + tanh(c u)) (float64)
    x = torch.linspace(-12.0, 12.0, 48001, dtype=torch.float64)
    want = torch.nn.functional.gelu(x, approximate="tanh")
    assert float((S.gelu_tanh64(x) - want).abs().max()) < 1e-14
    assert float((0.5 * x * (1 + torch.tanh(S.SQRT_2_PI * (x + S.CUBIC * x ** 3))) - want).abs().max()) < 1e-14
    # in TAIL the two functions (float64, nothing of the library in it) are at least 7 ulp of bf16 and 20 ulp of fp16 apart -- the
    # minimum, 7.2 / 20.2, is at x = -5, where fp16's results are subnormal; one rounding moves a result by half an ulp
    t = torch.linspace(S.TAIL[0], S.TAIL[1], 2501, dtype=torch.float64)
    gap = (S.gelu_tanh64(t) - GC._gelu64(t)).abs()
    for dt, n in ((torch.bfloat16, 7), (torch.float16, 20)):
        assert float((gap / GC._ulp_T(S.gelu_tanh64(t), dt)).min()) >= n, dt
    assert 1.12 < S.tanh_gelu_max_slope() <= S.TANH_GELU_LIPSCHITZ


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_exact_reference_and_emulation_inside_the_bound_restatements_outside(dtype):
    """Every case: at least TAIL_SHARE of the pre-activations in [-5, -2.5]; the exact float64 value rounded once and the fp32
    emulation of the kernel inside the bound; the erf and the quick form -- exact, rounded once: no other error -- outside it."""
    worst = {None: 0.0, "emulate": 0.0}
    least = {v: float("inf") for v in S.VARIANTS}
    for kind in ("random", "tails"):
        for n, (M, N, K) in enumerate(_sample_shapes()):
            c = S.make_case(kind, dtype, M, N, K, guard=("nan", "attract")[n % 2], seed=n)
            r = S.reference(c)
            share = S.tail_share(r)
            assert share >= S.TAIL_SHARE, f"{kind} {M}x{N}x{K}: only {share:.3f} of the pre-activations in {S.TAIL}"
            assert float(r.out.abs().max()) < GC.HALF_MAX[dtype]
            for key, outs in ((None, S.restate64(c, r)), ("emulate", S.emulate(c))):
                ratio, msg = S.check(c, r, outs)
                assert msg is None, f"{key} {kind} M={M} N={N} K={K}: {msg}"
                worst[key] = max(worst[key], ratio)
            for v in S.VARIANTS:
                for outs in (S.restate64(c, r, v), S.emulate(c, v)):
                    ratio, msg = S.check(c, r, outs)
                    assert msg is not None and ratio > 1.0, f"{v} stays inside the bound on {kind} {M}x{N}x{K} ({dtype})"
                    least[v] = min(least[v], ratio)
    print(f"\n{S.FORM} {DT_ID[dtype]}: worst |err| / bound: exact {worst[None]:.3f}, emulation {worst['emulate']:.3f}; "
          + ", ".join(f"{v} at least {least[v]:.1f}" for v in S.VARIANTS))
    assert worst[None] < 1.0 and worst["emulate"] < 1.0


# ------------------------------------------------------------------------------------------------ 6. float64 replay vs HF
REPLAY_GEOMS = {"128": (80, 16, 128, 256, 3), "768": (64, 16, 768, 1536, 2)}       # image, patch, D, inter, layers (g = 5: odd, g = 4)
N_CROPS = 2
FACTOR = 100.0             # how far outside the bound a wrong variant has to lie behind the first layer (test_gelu_tower_cpu's condition)
_cache = {}


def _replay_case(name):
    if name not in _cache:
        from slime_amd import ops, weights as W
        cfg = S.siglip_config(*REPLAY_GEOMS[name])
        sd = W.make_siglip_state_dict(cfg, seed=7)
        px = W.synthetic_pixels(N_CROPS, seed=3, image_size=cfg.image_size)
        L = cfg.num_hidden_layers
        flat = W.strip_tower_prefix(sd)
        host = ops.siglip_host_tensors(sd, cfg, None, L)
        host["pos_without_bias"] = flat["embeddings.position_embedding.weight"].double()
        _cache[name] = dict(cfg=cfg, sd=sd, flat=flat, px=px, host=host,
                            hf64=[h.reshape(-1, cfg.hidden_size) for h in S.hf_states(cfg, sd, px, torch.float64)],
                            hf32=[h.double().reshape(-1, cfg.hidden_size) for h in S.hf_states(cfg, sd, px, torch.float32)])
    return _cache[name]


def _excess(got, want, bound):
    return float(((got - want).abs() / bound).max()) if bool(torch.isfinite(got).all()) else float("inf")


@pytest.mark.parametrize("name", sorted(REPLAY_GEOMS))
def test_float64_replay_of_the_siglip_tower_vs_hf(name):
    """``replay_siglip`` on the float64 backend over the unrounded host tensors (pos + bias fold, LayerNorm fold, tanh form) against
    HF SiglipVisionModel: every state inside the running bound at 2^-53 + 2^-53 (HF in float64) and at 2^-53 + 2^-24 (HF as it
    stands); the broken variants outside it by FACTOR at the first state they touch."""
    c = _replay_case(name)
    cfg, L, D = c["cfg"], c["cfg"].num_hidden_layers, c["cfg"].hidden_size
    res = S.replay_siglip(S.TorchBackend(None), c["host"], cfg, c["px"], L, want_hidden=True, want_states=True)
    assert len(res["states"]) == L + 1 and torch.equal(res["hidden"], res["states"][L]) and torch.equal(res["out"], res["hidden"])
    assert res["out"].shape == (N_CROPS * cfg.num_patches, D)
    bd64 = S.siglip_error_bound(c["flat"], c["host"], cfg, c["px"], L, TC.U64)
    bd32 = S.siglip_error_bound(c["flat"], c["host"], cfg, c["px"], L, TC.U32)
    x64 = max(_excess(res["states"][i], c["hf64"][i], bd64[i]) for i in range(L + 1))
    x32 = max(_excess(res["states"][i], c["hf32"][i], bd32[i]) for i in range(L + 1))
    print(f"\nD={D}: |replay - HF| / bound: float64 {x64:.3g}, fp32 {x32:.3g}")
    assert x64 <= 1.0 and x32 <= 1.0, (x64, x32)
    # the other two activations: the same embeddings, outside the bound behind the first layer
    for act in ("erf", "quick"):
        bad = S.replay_siglip(S.TorchBackend(None, act), c["host"], cfg, c["px"], L, want_states=True)
        assert torch.equal(bad["states"][0], res["states"][0])
        x = _excess(bad["states"][1], c["hf64"][1], bd64[1])
        print(f"  {act} form: state 1 at {x:.3g} bounds")
        assert x > FACTOR, (act, x)
    # the conv bias left out of pos': the embeddings themselves
    bad = S.replay_siglip(S.TorchBackend(None), c["host"], cfg, c["px"], L, want_states=True, broken="bias_not_folded")
    assert _excess(bad["states"][0], c["hf64"][0], bd64[0]) > FACTOR
    # fc1 of layer l with layer l + 1's folded weights
    bad = S.replay_siglip(S.TorchBackend(None), c["host"], cfg, c["px"], L, want_states=True, broken="fold_off_by_one_layer")
    assert torch.equal(bad["states"][0], res["states"][0]) and _excess(bad["states"][1], c["hf64"][1], bd64[1]) > FACTOR
    # a class-row offset of one in the output
    # (judged on the embeddings, layers_run = 0, where the running bound has not grown yet)
    emb = S.replay_siglip(S.TorchBackend(None), c["host"], cfg, c["px"], 0)
    bad = S.replay_siglip(S.TorchBackend(None), c["host"], cfg, c["px"], 0, broken="class_row_offset")
    assert _excess(emb["out"], c["hf64"][0], bd64[0]) <= 1.0 and torch.equal(emb["out"], res["states"][0])
    assert _excess(bad["out"], c["hf64"][0], bd64[0]) > FACTOR and torch.equal(bad["out"][:-1], emb["out"][1:])


def test_hf_loads_the_synthetic_state_dict_completely_and_runs_the_tanh_form():
    """The yardstick is loaded key for key, head included (hf_model asserts it); its activation is the tanh form."""
    c = _replay_case("128")
    m = S.hf_model(c["cfg"], c["sd"])
    assert m.config.hidden_act == "gelu_pytorch_tanh" and len(c["hf32"]) == c["cfg"].num_hidden_layers + 1
    assert c["hf32"][0].shape == (N_CROPS * 25, 128)
