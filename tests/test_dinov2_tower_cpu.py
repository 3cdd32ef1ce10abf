"""DINOv2 vision towers without a GPU (helpers: tests/dinov2_tower_conformance.py).

  1. ABI: the new entries' prototypes against the header through a C compiler; ABI version and ``slime_vit_desc`` as they were.
     Refusals of ``slime_dinov2_*`` and ``slime_patch_embed_prefix``, all before any device work: a missing prefix table, non-NULL
     pre_ln_*, n_prefix outside 1..17, bad geometry, no output, workspace (its size derived here for S = n_prefix + P rows); the
     named refusals of ``ops.check_dinov2_config``.
  2. The float64 replay of the packed tower (prefix rows, interpolated table, conv-bias fold, LayerScale fold) against HF
     ``Dinov2Model`` and ``Dinov2WithRegistersModel`` under a derived bound, with broken variants; the fp16 bound for small lambda.
  3. Loader: a DINOv2 directory written here (bare / prefixed keys, flat / nested config, with / without preprocessor_config.json,
     mask_token / layernorm present or absent); CLIP and SigLIP directories do not load as DINOv2 and keep their own classes.
  4. ``Dinov2ImageProcessor`` bit-equal to transformers' ``BitImageProcessorPil`` on non-square images.
"""
import ctypes as C
import dataclasses
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dinov2_tower_conformance as DV
import tower_conformance as TC

# ------------------------------------------------------------------------------------------------ 1. ABI and refusals
PROTOS = {
    "slime_dinov2_check": ("int", ["const slime_vit_desc*", "int"]),
    "slime_dinov2_workspace_bytes": ("size_t", ["const slime_vit_desc*", "int", "int"]),
    "slime_dinov2_ksplit_workspace_bytes": ("size_t", ["const slime_vit_desc*", "int", "int", "const slime_vit_ksplit*"]),
    "slime_dinov2_forward": ("int", ["const slime_vit_desc*", "int", "const void*", "int", "int", "void*", "int", "int", "float*", "float*",
                                     "const slime_vit_ksplit*", "void*", "size_t", "void*"]),
    "slime_patch_embed_prefix": ("int", ["const void*", "int", "const void*", "const float*", "int", "const float*", "float*", "void*",
                                         "void*", "float*", "int", "int", "int", "int", "int", "int", "void*"]),
}


def _ctype_for(decl):
    from slime_amd import _lib
    return {"const slime_vit_desc*": C.POINTER(_lib.VitDesc), "const slime_vit_ksplit*": C.POINTER(_lib.VitKsplit), "int": C.c_int,
            "size_t": C.c_size_t}.get(decl, C.c_void_p)


def test_new_entries_mirror_the_header(tmp_path):
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"']
    for name, (res, args) in PROTOS.items():
        r, a = _lib._SIGNATURES[name]
        assert r is _ctype_for(res) and list(a) == [_ctype_for(d) for d in args], name
        # an assignment between function pointer types of different parameter lists does not compile under -Werror
        lines.append(f'static {res} (*const p_{name})({", ".join(args)}) = {name};')
    lines += ['int main(void) {', 'printf("gelu %d\\n", (int)SLIME_EPI_BIAS_GELU_T);', 'printf("abi %d\\n", (int)SLIME_ABI_VERSION);',
              'printf("desc %zu\\n", sizeof(slime_vit_desc));', 'printf("ks %zu\\n", sizeof(slime_vit_ksplit));',
              'return ' + " || ".join(f"p_{n} == 0" for n in PROTOS) + ';', '}']
    src = tmp_path / "dinov2.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Werror", "-c", "-o", str(tmp_path / "dinov2.o"), str(src)], check=True)       # the prototypes
    probe = tmp_path / "probe.c"
    text = src.read_text()
    for name in PROTOS:
        text = text.replace(f"= {name};", "= 0;")
    probe.write_text(text)
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(probe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True).stdout.splitlines())
    assert int(got["gelu"]) == _lib.EPI_BIAS_GELU_T
    assert int(got["abi"]) == _lib.ABI_VERSION == _lib.load().slime_abi_version() == 7
    assert int(got["desc"]) == C.sizeof(_lib.VitDesc) and len(_lib.VitDesc._fields_) == 29
    assert int(got["ks"]) == C.sizeof(_lib.VitKsplit)
    assert set(PROTOS) <= set(_lib.header_symbols())


def _desc(image=224, patch=14, hidden=1024, heads=16, inter=4096, layers=2):
    """A DINOv2 descriptor over fake addresses (the checks never dereference): cls set (the prefix table), pre_ln_* NULL."""
    from slime_amd import _lib
    d = _lib.VitDesc()
    d.hidden, d.inter, d.heads, d.layers_run, d.image, d.patch = hidden, inter, heads, layers, image, patch
    d.kpad, d.dtype, d.eps = (3 * patch * patch + 63) // 64 * 64, _lib.BF16, 1e-6
    for name, tp in _lib.VitDesc._fields_:
        if tp is C.c_void_p and name not in ("patch_w", "pre_ln_w", "pre_ln_b"):
            setattr(d, name, 0x1000)
    return d


def _err():
    from slime_amd import _lib
    return _lib.load().slime_last_error().decode()


def test_dinov2_check_geometry_and_the_descriptor_convention():
    from slime_amd import _lib
    lib = _lib.load()
    for image, hidden, heads, inter in ((224, 768, 12, 3072), (224, 1024, 16, 4096), (336, 768, 12, 3072), (336, 1024, 16, 4096)):
        for npre in (1, 5, 17):
            assert lib.slime_dinov2_check(C.byref(_desc(image=image, hidden=hidden, heads=heads, inter=inter)), npre) == 0, _err()
    for field in ("pre_ln_w", "pre_ln_b"):
        d = _desc()
        setattr(d, field, 0x1000)
        assert lib.slime_dinov2_check(C.byref(d), 5) == -1 and field in _err() and "NULL" in _err(), _err()
    d = _desc()
    d.cls = None
    assert lib.slime_dinov2_check(C.byref(d), 5) == -1 and "cls is required" in _err() and "prefix table" in _err(), _err()
    for npre in (0, -1, 18):
        assert lib.slime_dinov2_check(C.byref(_desc()), npre) == -1 and f"n_prefix={npre}" in _err() and "1..17" in _err(), _err()
    for bad, word in ((_desc(hidden=1536, heads=24, inter=6144), "hidden=1536"),                    # the giant model's width
                      (_desc(heads=8), "head_dim"), (_desc(image=448), "patches per side"), (_desc(image=392), "patches per side"),
                      (_desc(inter=4304), "multiple of 128"), (_desc(image=220), "not a multiple of patch"),
                      (_desc(image=238), "multiple of the patch 14 and of 8"),
                      (_desc(image=518), "multiple of the patch 14 and of 8"), (_desc(image=378), "multiple of the patch 14 and of 8")):
        assert lib.slime_dinov2_check(C.byref(bad), 5) == -1
        assert word in _err(), _err()
    d = _desc()
    d.pos = None
    assert lib.slime_dinov2_check(C.byref(d), 1) == -1 and "missing embedding weights" in _err()
    assert lib.slime_dinov2_check(None, 1) == -1 and "null descriptor" in _err()
    # the other families' entries keep their own conventions over the same struct
    assert lib.slime_siglip_check(C.byref(_desc())) == -1 and "cls must be NULL" in _err()
    assert lib.slime_vit_check(C.byref(_desc())) == -1 and "missing embedding weights" in _err()


def test_dinov2_forward_refusals_need_no_device_and_the_workspace_is_that_of_s_rows():
    from slime_amd import _lib
    lib = _lib.load()
    d, px = _desc(), 0x1000

    def call(desc, npre=5, out=0x2000, hidden=None, states=None, ks=None, ws=None, nbytes=0, n=1, pix=_lib.F32, odt=_lib.F32, keep=0):
        return lib.slime_dinov2_forward(desc, npre, px, pix, n, out, odt, keep, hidden, states, ks, ws, nbytes, None)

    assert call(C.byref(d), out=None) == -1 and "no output requested" in _err()
    assert call(None) == -1 and "null descriptor" in _err()
    assert call(C.byref(d), n=0) == -1 and "bad input" in _err()
    assert call(C.byref(d), odt=_lib.U8) == -1 and "out dtype" in _err()
    for npre in (0, 18):
        assert call(C.byref(d), npre=npre) == -1 and f"n_prefix={npre}" in _err()
    for field in ("pre_ln_w", "pre_ln_b"):
        bad = _desc()
        setattr(bad, field, 0x1000)
        assert call(C.byref(bad)) == -1 and field in _err()
    bad = _desc()
    bad.cls = None
    assert call(C.byref(bad)) == -1 and "cls is required" in _err()
    assert call(C.byref(_desc(image=448))) == -1 and "patches per side" in _err()
    ks = _lib.VitKsplit(2, 1, 99, 1)
    assert call(C.byref(d), ks=C.byref(ks)) == -1 and "fc1=99" in _err()
    # a valid call up to the workspace: refused there (SLIME_EWORKSPACE = -2), still before any launch
    need = lib.slime_dinov2_workspace_bytes(C.byref(d), 5, 1)
    assert call(C.byref(d)) == -2 and "workspace" in _err() and str(need) in _err()
    assert call(C.byref(d), ws=0x10000, nbytes=need - 1) == -2 and call(C.byref(d), ws=0x10010, nbytes=need) == -2
    # the size is that of S = n_prefix + P rows per crop
    P, D, F = 256, 1024, 4096
    rows = lambda M: sum((b + 255) // 256 * 256 for b in (M * D, M * D * 2, max(M * F * 2, (M * 3 * D * 2 + 255) // 256 * 256 + M * D * 2),
                                                        M * (D // 64) * 8))
    for npre in (1, 5, 17):
        assert lib.slime_dinov2_workspace_bytes(C.byref(d), npre, 1) == rows(npre + P)
        assert lib.slime_dinov2_workspace_bytes(C.byref(d), npre, 3) == rows(3 * (npre + P))
    assert lib.slime_dinov2_workspace_bytes(C.byref(d), 1, 1) == lib.slime_vit_workspace_bytes(C.byref(d), 1)      # cls + P: the CLIP layout's
    ks = _lib.VitKsplit(2, 1, 2, 4)
    part = max(lib.slime_gemm_ksplit_workspace_bytes(5 + P, n_, s) for n_, s in ((3 * D, 2), (D, 1), (F, 2), (D, 4)))
    assert lib.slime_dinov2_ksplit_workspace_bytes(C.byref(d), 5, 1, C.byref(ks)) == need + part
    assert lib.slime_dinov2_workspace_bytes(None, 5, 1) == 0 and lib.slime_dinov2_workspace_bytes(C.byref(d), 5, 0) == 0
    assert lib.slime_dinov2_workspace_bytes(C.byref(d), 0, 1) == 0 and lib.slime_dinov2_workspace_bytes(C.byref(d), 18, 1) == 0
    # the primitive: the same geometry limits, named, and its own two
    pe = lambda image=224, patch=14, kpad=640, D=1024, x16=0x3000, pos=0x4000, prefix=0x5000, npre=5: lib.slime_patch_embed_prefix(
        px, _lib.F32, 0x2000, prefix, npre, pos, None, x16, None, None, _lib.BF16, 1, image, patch, kpad, D, None)
    assert pe(image=448) == -1 and "patches per side" in _err()
    assert pe(kpad=576) == -1 and "kpad" in _err()
    assert pe(x16=None) == -1 and "no output requested" in _err()
    assert pe(pos=None) == -1 and "bad input" in _err()
    assert pe(D=512) == -1 and "D=512" in _err()
    assert pe(prefix=None) == -1 and "prefix table is required" in _err()
    for npre in (0, 18):
        assert pe(npre=npre) == -1 and f"n_prefix={npre}" in _err() and "1..17" in _err()


REFUSED = {"swiglu": (dict(use_swiglu_ffn=True), ("use_swiglu_ffn", "giant")),
           "hidden_act": (dict(hidden_act="gelu_pytorch_tanh"), ("'gelu_pytorch_tanh'", "'gelu'")),
           "head_dim": (dict(hidden_size=1024, num_attention_heads=8), ("head_dim=128", "64")),
           "width": (dict(hidden_size=384, num_attention_heads=6), ("hidden_size=384", "768")),           # ViT-S/14
           "grid": (dict(image_size=448), ("32 patches per side", "24")),
           "not_patch_multiple": (dict(image_size=230), ("run size 230", "multiple of patch_size 14")),
           "not_multiple_of_8": (dict(image_size=238), ("run size 238", "of 8")),
           "registers": (dict(num_register_tokens=17, model_type="dinov2_with_registers"), ("num_register_tokens=17", "16"))}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_unsupported_dinov2_towers_are_refused_by_name(tmp_path, what):
    """Refused when checked, when packed and when loaded, before any device work, the offending field or value named."""
    from slime_amd import ops, weights as W
    over, words = REFUSED[what]
    bad = dataclasses.replace(W.DINOV2_L_224, **over)
    with pytest.raises(ValueError) as e:
        ops.check_dinov2_config(bad)
    assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ValueError, match=words[0]):
        ops.pack_dinov2_tower({}, bad, torch.bfloat16, "cpu")
    ops.check_dinov2_config(W.DINOV2_L_224), ops.check_dinov2_config(W.DINOV2_L_REG4_224)
    # from a directory: the config says it, the constructor refuses (delay_load too: nothing is read beyond the two json files)
    good = DV.dinov2_config(56, 128, 1, 4 if "registers" in what else 0, 5)
    run = over.get("image_size", 56)
    dir_over = {k: v for k, v in over.items() if k not in ("image_size", "model_type")}
    DV.write_hf_dir(tmp_path, W.make_dinov2_state_dict(good, seed=21), dataclasses.replace(good, image_size=run), **dir_over)
    for delay in (False, True):
        with pytest.raises(ValueError, match=words[0]):
            _tower(tmp_path, delay_load=delay)


def test_pack_refuses_other_dtypes_and_the_select_layer_range():
    from slime_amd import ops, weights as W
    cfg = DV.dinov2_config(56, 128, 2)
    sd = W.make_dinov2_state_dict(cfg, seed=1)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.dinov2_host_tensors(sd, cfg, torch.float32)
    with pytest.raises(ValueError, match="bf16 or fp16"):
        ops.pack_dinov2_tower(sd, cfg, torch.float32, "cpu")
    with pytest.raises(ValueError, match="out of range"):
        ops.dinov2_host_tensors(sd, cfg, None, 3)
    with pytest.raises(ValueError, match="register tokens"):
        ops.dinov2_host_tensors(W.make_dinov2_state_dict(DV.dinov2_config(56, 128, 2, 2), seed=1), DV.dinov2_config(56, 128, 2, 4), None)


# ------------------------------------------------------------------------------------------------ 2. float64 replay vs HF
# name -> (run size, D, layers, registers, table grid): tiny towers (D 128, 2 heads, 2 layers) whose table is for a 5 x 5 grid, run on
# 4 x 4; and a table that fits the run grid (no interpolation)
REPLAY = {"plain": (56, 128, 2, 0, 5), "reg4": (56, 128, 2, 4, 5), "reg1_same_grid": (42, 128, 2, 1, 3)}
N_CROPS = 2
FACTOR = 100.0             # how far outside the bound a wrong variant has to lie at the first state it touches (test_siglip_tower_cpu's)
_cache = {}


def _replay_case(name):
    if name not in _cache:
        from slime_amd import ops, weights as W
        cfg = DV.dinov2_config(*REPLAY[name])
        sd = W.make_dinov2_state_dict(cfg, seed=7)
        px = W.synthetic_pixels(N_CROPS, seed=3, image_size=cfg.image_size)
        L = cfg.num_hidden_layers
        _cache[name] = dict(cfg=cfg, sd=sd, px=px, host=ops.dinov2_host_tensors(sd, cfg, None, L),
                            hf64=[h.reshape(-1, cfg.hidden_size) for h in DV.hf_states(cfg, sd, px, torch.float64)],
                            hf32=[h.double().reshape(-1, cfg.hidden_size) for h in DV.hf_states(cfg, sd, px, torch.float32)])
    return _cache[name]


def _excess(got, want, bound):
    """max |got - want| / bound; a row whose bound is zero (a register token in the embeddings: a copy) must be equal."""
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    d = (got - want).abs()
    r = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max())


def test_the_synthetic_lambdas_are_log_uniform_in_1e_4_to_1():
    from slime_amd import weights as W
    sd = W.make_dinov2_state_dict(DV.dinov2_config(56, 128, 2, 4, 5), seed=7)
    lam = torch.cat([v for k, v in sd.items() if "lambda1" in k])
    assert lam.numel() == 4 * 128 and float(lam.min()) >= 1e-4 and float(lam.max()) <= 1.0
    q = torch.log10(lam)
    assert float(q.min()) < -3.8 and float(q.max()) > -0.2 and -2.3 < float(q.mean()) < -1.7       # both ends reached, the mean at 1e-2


@pytest.mark.parametrize("name", sorted(REPLAY))
def test_float64_replay_of_the_dinov2_tower_vs_hf(name):
    """``replay_dinov2`` on the float64 backend over the unrounded host tensors against HF: every state inside the running bound at
    2^-53 + 2^-53 (HF in float64) and at 2^-53 + 2^-24 (HF as it stands); the broken variants outside it by FACTOR at the first
    state they touch."""
    c = _replay_case(name)
    cfg, L, D = c["cfg"], c["cfg"].num_hidden_layers, c["cfg"].hidden_size
    R, S_, P = cfg.num_register_tokens, cfg.seq_len, cfg.num_patches
    be = DV.TorchBackend(None)
    res = DV.replay_dinov2(be, c["host"], cfg, c["px"], L, keep_prefix=1, want_hidden=True, want_states=True)
    assert len(res["states"]) == L + 1 and torch.equal(res["hidden"], res["states"][L]) and torch.equal(res["out"], res["hidden"])
    assert res["out"].shape == (N_CROPS * S_, D) and c["hf64"][0].shape == (N_CROPS * S_, D)
    patches = DV.replay_dinov2(be, c["host"], cfg, c["px"], L)["out"]
    assert torch.equal(patches.view(N_CROPS, P, D), res["hidden"].view(N_CROPS, S_, D)[:, cfg.n_prefix:])       # keep_prefix = 0
    bd64 = DV.dinov2_error_bound(c["sd"], c["host"], cfg, c["px"], L, TC.U64)
    bd32 = DV.dinov2_error_bound(c["sd"], c["host"], cfg, c["px"], L, TC.U32)
    x64 = max(_excess(res["states"][i], c["hf64"][i], bd64[i]) for i in range(L + 1))
    x32 = max(_excess(res["states"][i], c["hf32"][i], bd32[i]) for i in range(L + 1))
    worst = max(float((res["states"][i] - c["hf64"][i]).abs().max()) for i in range(L + 1))
    print(f"\n{name}: |replay - HF| / bound: float64 {x64:.3g}, fp32 {x32:.3g}; worst |replay - HF float64| {worst:.3g}")
    assert x64 <= 1.0 and x32 <= 1.0, (x64, x32)
    first_touched = {"layerscale_not_folded": 1, "lambdas_swapped": 1, "registers_with_position": 0, "antialias_swapped": 0,
                     "bias_not_folded": 0}
    for v in DV.HOST_BROKEN:
        if (v == "registers_with_position" and R == 0) or (v == "antialias_swapped" and cfg.grid == cfg.table_grid):
            continue                                        # no register rows / no interpolation to get wrong
        bad = DV.replay_dinov2(be, DV.broken_host(c["sd"], cfg, L, v), cfg, c["px"], L, keep_prefix=1, want_states=True)["states"]
        i = first_touched[v]
        assert all(torch.equal(bad[j], res["states"][j]) for j in range(i)), v
        x = _excess(bad[i], c["hf64"][i], bd64[i])
        print(f"  {v}: state {i} at {x:.3g} bounds")
        assert x > FACTOR, (v, x)
    # fc1 of layer l with layer l + 1's folded weights
    bad = DV.replay_dinov2(be, c["host"], cfg, c["px"], L, keep_prefix=1, want_states=True, broken="fold_off_by_one_layer")["states"]
    assert torch.equal(bad[0], res["states"][0]) and _excess(bad[1], c["hf64"][1], bd64[1]) > FACTOR
    # the patch gather one row early (judged on the embeddings, layers_run = 0, where the running bound has not grown yet)
    sel = lambda t: t.view(N_CROPS, S_, D)[:, cfg.n_prefix:].reshape(-1, D)
    emb = DV.replay_dinov2(be, c["host"], cfg, c["px"], 0)
    bad = DV.replay_dinov2(be, c["host"], cfg, c["px"], 0, broken="prefix_offset_by_one")
    assert _excess(emb["out"], sel(c["hf64"][0]), sel(bd64[0])) <= 1.0
    assert _excess(bad["out"], sel(c["hf64"][0]), sel(bd64[0])) > FACTOR and torch.equal(bad["out"][1:P], emb["out"][:P - 1])


def test_the_prefix_rows_and_the_table_are_hfs_own_values():
    """Row 0 = cls + pos[0] (one fp32 addition), the registers as they are, pos' = F.interpolate with HF's arguments + the conv bias;
    antialias follows the model class and changes the table; equal grids skip the interpolation."""
    from slime_amd import ops, weights as W
    for name in ("plain", "reg4"):
        c = _replay_case(name)
        cfg, sd = c["cfg"], c["sd"]
        T = ops.dinov2_host_tensors(sd, cfg, torch.bfloat16, 2)
        assert set(T) == {"patch_w", "cls", "pos", "w_qkv", "b_qkv", "colsum_qkv", "w_o", "b_o", "w_fc1", "b_fc1", "colsum_fc1", "w_fc2", "b_fc2"}
        table = sd["embeddings.position_embeddings"]
        assert T["cls"].dtype == torch.float32 and T["cls"].shape == (cfg.n_prefix, 128)
        assert torch.equal(T["cls"][0], sd["embeddings.cls_token"][0, 0] + table[0, 0])
        if cfg.num_register_tokens:
            assert torch.equal(T["cls"][1:], sd["embeddings.register_tokens"][0])
        want = torch.nn.functional.interpolate(table[:, 1:].reshape(1, 5, 5, 128).permute(0, 3, 1, 2), size=(4, 4), mode="bicubic",
                                               align_corners=False, antialias=cfg.antialias).permute(0, 2, 3, 1).reshape(16, 128)
        assert T["pos"].dtype == torch.float32 and torch.equal(T["pos"], want + sd["embeddings.patch_embeddings.projection.bias"][None])
        other = ops.dinov2_pos_table(table, 4, not cfg.antialias)
        assert not torch.equal(other, want)
        assert T["patch_w"].shape == (128, 640) and T["patch_w"].dtype == torch.bfloat16 and not bool(T["patch_w"][:, 588:].any())
        # LayerScale: row j of the Linear times lambda[j], rounded once to T; the bias in fp32
        lam, Wo, bo = (sd["encoder.layer.1." + k].double() for k in ("layer_scale1.lambda1", "attention.output.dense.weight",
                                                                   "attention.output.dense.bias"))
        assert torch.equal(T["w_o"][1], (Wo * lam[:, None]).float().to(torch.bfloat16)) and torch.equal(T["b_o"][1], (bo * lam).float())
        lam, W2 = (sd["encoder.layer.0." + k].double() for k in ("layer_scale2.lambda1", "mlp.fc2.weight"))
        assert torch.equal(T["w_fc2"][0], (W2 * lam[:, None]).float().to(torch.bfloat16))
        # the run size as an argument
        T2 = ops.dinov2_host_tensors(sd, cfg, None, 0, image_size=70)
        assert T2["pos"].shape == (25, 128) and T2["pos"].dtype == torch.float64 and set(T2) == {"patch_w", "cls", "pos"}
        assert torch.equal(T2["pos"], table[0, 1:].double() + sd["embeddings.patch_embeddings.projection.bias"].double()[None])
    c = _replay_case("reg1_same_grid")
    T = ops.dinov2_host_tensors(c["sd"], c["cfg"], torch.float16, 0)
    assert torch.equal(T["pos"], c["sd"]["embeddings.position_embeddings"][0, 1:] + c["sd"]["embeddings.patch_embeddings.projection.bias"][None])


@pytest.mark.parametrize("name", ["plain", "reg4"])
def test_fp16_small_lambda_bound_holds_on_the_rounded_tensors(name):
    """A folded weight lambda w below 2^-14 lands on the fp16 subnormal grid (spacing 2^-24): the rounding to T moves it by at most
    2^-25, whatever its size -- not by 2^-11 of itself.  (The pack rounds float64 -> fp32 -> fp16: the fp32 step adds at most 2^-24
    of the weight, 2^-38 here.)  Over a row of the GEMM that moves an element of h by at most 2^-25 sum_k |a_k|.  bf16 has no such
    range at these sizes: its error stays relative, 2^-8."""
    from slime_amd import ops
    c = _replay_case(name)
    cfg, L = c["cfg"], c["cfg"].num_hidden_layers
    T16 = ops.dinov2_host_tensors(c["sd"], cfg, torch.float16, L)
    Tb = ops.dinov2_host_tensors(c["sd"], cfg, torch.bfloat16, L)
    be = DV.TorchBackend(None)
    n_small = 0
    for w in ("w_o", "w_fc2"):
        exact = c["host"][w]
        f32 = exact.float().double()
        small = exact.abs() < 2.0 ** -14
        n_small += int(small.sum())
        err = (T16[w].double() - exact).abs()
        assert bool(((T16[w].double() - f32).abs()[small] <= 2.0 ** -25).all())                   # the rounding to fp16 itself
        assert bool((err[small] <= 2.0 ** -25 + 2.0 ** -24 * exact.abs()[small]).all())            # ... and from the float64 value
        assert bool((err[~small] <= (2.0 ** -11 + 2.0 ** -24) * exact.abs()[~small]).all())
        assert float((err[small] / exact.abs()[small].clamp_min(1e-300)).max()) > 2.0 ** -11       # the relative bound does NOT hold there
        assert bool(((Tb[w].double() - exact).abs() <= (2.0 ** -8 + 2.0 ** -24) * exact.abs()).all())
    assert n_small > 1000, n_small                            # the synthetic lambdas reach the range
    # the consequence, on the activations the GEMMs see: ctx / ff rows of the float64 replay through the subnormal-range weights only
    res = DV.replay_dinov2(be, c["host"], cfg, c["px"], 1, keep_prefix=1, want_hidden=True)
    g = torch.Generator().manual_seed(5)
    for w, K in (("w_o", cfg.hidden_size), ("w_fc2", cfg.intermediate_size)):
        a = torch.randn(64, K, generator=g, dtype=torch.float64) * float(res["hidden"].abs().mean())
        exact = c["host"][w][0]
        small = exact.abs() < 2.0 ** -14
        dw = torch.where(small, T16[w][0].double() - exact, torch.zeros_like(exact))
        moved = (a @ dw.t()).abs()
        assert bool((moved <= (2.0 ** -25 + 2.0 ** -38) * a.abs().sum(-1, keepdim=True)).all())


# ------------------------------------------------------------------------------------------------ 3. loader
def _tower(path, feature="patch", **kw):
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    return build_vision_tower(SimpleNamespace(mm_vision_tower=str(path), mm_vision_select_layer=-2, mm_vision_select_feature=feature), **kw)


@pytest.mark.parametrize("extras", [True, False], ids=["mask_and_layernorm", "without"])
@pytest.mark.parametrize("keys", ["bare", "dinov2.", "vision_model."])
@pytest.mark.parametrize("nested", [False, True], ids=["flat_config", "vision_config"])
@pytest.mark.parametrize("prep", [True, False], ids=["preprocessor", "no_preprocessor"])
@pytest.mark.parametrize("registers", [0, 4])
def test_dinov2_tower_loads_from_hf_directory(tmp_path, registers, prep, nested, keys, extras):
    from slime_amd import weights as W
    from slime_amd.image_processor import Dinov2ImageProcessor
    from slime_amd.model.multimodal_encoder.dinov2_encoder import Dinov2VisionTower
    # with a preprocessor_config.json the run size is its crop_size (56: a 4 x 4 grid under a table for 5 x 5, config.json's image_size
    # 70); without, config.json's image_size (56: the table's own grid)
    cfg = DV.dinov2_config(56, 128, 2, registers, 5 if prep else 4)
    sd = W.make_dinov2_state_dict(cfg, seed=21)
    if not extras:
        sd = {k: v for k, v in sd.items() if "mask_token" not in k and not k.startswith("layernorm.")}
    saved = sd if keys == "bare" else {keys + k: v for k, v in sd.items()}
    DV.write_hf_dir(tmp_path, saved, cfg, nested, preprocessor=prep)
    t = _tower(tmp_path)
    assert isinstance(t, Dinov2VisionTower) and t.is_loaded and t.config == cfg and t.hidden_size == 128
    side = 4
    assert t.config.image_size == side * 14 and t.num_patches == side * side and t.num_patches_per_side == side
    assert t.config.n_prefix == 1 + registers and t.config.antialias == (registers > 0) and t.select_feature == "patch"
    assert isinstance(t.image_processor, Dinov2ImageProcessor) and t.image_processor.crop_size == {"height": side * 14, "width": side * 14}
    assert t.image_processor.image_mean == [0.485, 0.456, 0.406] and t.image_processor.size["shortest_edge"] == side * 14 * 256 // 224
    got = t.vision_tower.state_dict()
    assert ("vision_model.embeddings.register_tokens" in got) == (registers > 0)
    for k, v in sd.items():
        assert torch.equal(got["vision_model." + k], v), k
    d = _tower(tmp_path, delay_load=True)
    assert not d.is_loaded and d.config == cfg and d.hidden_size == 128 and d.num_patches == side * side
    d.load_model()
    assert d.is_loaded and torch.equal(d.vision_tower.state_dict()["vision_model.embeddings.cls_token"], sd["embeddings.cls_token"])


def test_cls_patch_and_the_builder_routes(tmp_path):
    import gelu_tower_conformance as G
    import siglip_tower_conformance as S
    from slime_amd import weights as W
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower, is_dinov2_tower, is_siglip_tower
    from slime_amd.model.multimodal_encoder.clip_encoder import CLIPVisionTower
    from slime_amd.model.multimodal_encoder.dinov2_encoder import Dinov2VisionTower
    from slime_amd.model.multimodal_encoder.siglip_encoder import SigLipVisionTower
    dirs = {k: tmp_path / k for k in ("plain", "reg", "clip", "sig")}
    for p in dirs.values():
        p.mkdir()
    plain, reg = DV.dinov2_config(56, 128, 2, 0, 5), DV.dinov2_config(56, 128, 2, 4, 5)
    DV.write_hf_dir(dirs["plain"], W.make_dinov2_state_dict(plain, seed=21), plain)
    DV.write_hf_dir(dirs["reg"], W.make_dinov2_state_dict(reg, seed=21), reg)
    # 'cls_patch': class token + patches without registers; refused at construction with them (delay_load too)
    t = _tower(dirs["plain"], feature="cls_patch")
    assert type(t) is Dinov2VisionTower and t.select_feature == "cls_patch" and t._keep_cls()
    for delay in (False, True):
        with pytest.raises(ValueError, match="cls_patch"):
            _tower(dirs["reg"], feature="cls_patch", delay_load=delay)
        with pytest.raises(ValueError, match="Unexpected select feature"):
            _tower(dirs["plain"], feature="cls", delay_load=delay)
    # feature_select on an HF-like output
    hs = SimpleNamespace(hidden_states=[torch.arange(2 * 21 * 3.0).view(2, 21, 3)] * 3)
    r = _tower(dirs["reg"], delay_load=True)
    assert torch.equal(r.feature_select(hs), hs.hidden_states[0][:, 5:]) and torch.equal(t.feature_select(hs), hs.hidden_states[0])
    # the other families' directories keep their classes, and their checkpoints do not load as DINOv2 (nor the reverse)
    ccfg = G.vision_config(56, 14, 128, 256, 2, act="quick_gelu")
    G.write_hf_dir(dirs["clip"], W.make_tower_state_dict(ccfg, seed=21), ccfg)
    scfg = S.siglip_config(64, 16, 128, 256, 2)
    S.write_hf_dir(dirs["sig"], W.make_siglip_state_dict(scfg, seed=21), scfg)
    assert type(_tower(dirs["clip"])) is CLIPVisionTower and type(_tower(dirs["sig"])) is SigLipVisionTower
    assert not is_dinov2_tower(str(dirs["clip"])) and not is_dinov2_tower(str(dirs["sig"])) and is_dinov2_tower(str(dirs["reg"]))
    assert not is_siglip_tower(str(dirs["reg"]))
    from slime_amd.model.multimodal_encoder.dinov2_encoder import _read_dinov2_config
    for other in ("clip", "sig"):
        with pytest.raises(ValueError, match="not a DINOv2 tower"):
            _read_dinov2_config(str(dirs[other]))
        with pytest.raises(ValueError, match="not a DINOv2 tower"):
            Dinov2VisionTower(str(dirs[other]), SimpleNamespace(mm_vision_select_layer=-2))
    DV.write_hf_dir(dirs["plain"], W.strip_tower_prefix(W.make_tower_state_dict(ccfg, seed=21)), plain)        # CLIP weights under a DINOv2 config
    with pytest.raises(RuntimeError, match="DINOv2 ViT layout"):
        _tower(dirs["plain"])
    DV.write_hf_dir(dirs["plain"], W.make_dinov2_state_dict(reg, seed=21), plain)           # register tokens the config does not announce
    with pytest.raises(RuntimeError, match="DINOv2 ViT layout"):
        _tower(dirs["plain"])
    G.write_hf_dir(dirs["clip"], W.make_dinov2_state_dict(plain, seed=21), ccfg)            # DINOv2 weights under a CLIP config
    with pytest.raises(RuntimeError):
        _tower(dirs["clip"])
    # names: the stand-in; a hub-style name is resolved from the local cache only (absent here: unknown, as before)
    assert is_dinov2_tower("synthetic-dinov2:5") and is_dinov2_tower("facebook/dinov2-large") and not is_dinov2_tower("synthetic:5")
    assert not is_dinov2_tower("synthetic-siglip:5") and not is_siglip_tower("synthetic-dinov2:5")
    args = lambda name: SimpleNamespace(mm_vision_tower=name, mm_vision_select_layer=-2, mm_vision_select_feature="patch")
    d = build_vision_tower(args("synthetic-dinov2:5"), delay_load=True)
    assert type(d) is Dinov2VisionTower and d.config == W.DINOV2_L_REG4_224 and d.num_patches == 256 and d.num_patches_per_side == 16
    assert d.hidden_size == 1024 and d.config.n_prefix == 5 and d.config.table_grid == 37 and d.config.image_size == 224 and d.config.antialias
    assert type(build_vision_tower(args("synthetic:5"), delay_load=True)) is CLIPVisionTower
    assert type(build_vision_tower(args("synthetic-siglip:5"), delay_load=True)) is SigLipVisionTower
    with pytest.raises(ValueError, match="Unknown vision tower: facebook/dinov2-large"):
        build_vision_tower(args("facebook/dinov2-large"))


def test_the_synthetic_state_dict_has_hfs_keys_and_hf_loads_it_completely():
    """The yardstick is loaded key for key (hf_model asserts it), both classes; its activation is the exact GELU."""
    for name in ("plain", "reg4"):
        c = _replay_case(name)
        m = DV.hf_model(c["cfg"], c["sd"])
        assert m.config.hidden_act == "gelu" and set(m.state_dict()) == set(c["sd"])
        assert type(m).__name__ == ("Dinov2WithRegistersModel" if name == "reg4" else "Dinov2Model")
        assert c["hf32"][0].shape == (N_CROPS * c["cfg"].seq_len, 128) and len(c["hf32"]) == 3


# ------------------------------------------------------------------------------------------------ 4. image processor
def _images():
    from PIL import Image
    rng = np.random.RandomState(5)
    return [Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in ((300, 200), (97, 411), (64, 64), (500, 167))]


@pytest.mark.parametrize("size,crop,resample", [(256, 224, 3), (64, 56, 3), (384, 336, 3), (128, 112, 2)])
def test_image_processor_is_bit_equal_to_transformers_pil_backend(tmp_path, size, crop, resample):
    from transformers import BitImageProcessorPil
    from slime_amd.image_processor import Dinov2ImageProcessor, IMAGENET_MEAN, IMAGENET_STD
    hf = BitImageProcessorPil(size={"shortest_edge": size}, crop_size={"height": crop, "width": crop}, resample=resample,
                              image_mean=list(IMAGENET_MEAN), image_std=list(IMAGENET_STD))
    ours = Dinov2ImageProcessor(size, crop, resample=resample)
    if resample == 3:                                       # read from the file the loader reads
        DV.write_hf_dir(tmp_path, {"x": torch.zeros(1)}, DV.dinov2_config(crop, 128, 1))
        ours = Dinov2ImageProcessor.from_pretrained(str(tmp_path))
    assert ours.crop_size == {"height": crop, "width": crop} and ours.size["shortest_edge"] == size
    assert ours.image_mean == list(IMAGENET_MEAN) and ours.image_std == list(IMAGENET_STD) and int(ours.resample) == resample
    ims = _images()
    for im in ims:
        a = ours.preprocess(im, return_tensors="pt")["pixel_values"]
        b = hf(im, return_tensors="pt")["pixel_values"]
        assert a.shape == b.shape == (1, 3, crop, crop) and a.dtype == b.dtype and torch.equal(a, b), im.size
    assert torch.equal(ours(ims, return_tensors="pt")["pixel_values"], hf(ims, return_tensors="pt")["pixel_values"])
    assert Dinov2ImageProcessor().crop_size == {"height": 224, "width": 224} and Dinov2ImageProcessor().size == {"shortest_edge": 256}
