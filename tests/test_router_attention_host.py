"""Host side of the attention text-guided router (mm_resampler_type='qformer'): the float64 oracle against the reference's recorded
numbers, module construction and checkpoint loading, the pack-time algebra, the C ABI mirror, every refusal that returns before a
launch (reached with made-up, aligned, never dereferenced pointers), and the derived bounds of the two new row kernels against torch
fp32 emulations and broken variants.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import router_attention_oracle as RA
from slime_amd import _lib, ops, weights as W

GOLDEN, CASES, golden, golden_case = RA.GOLDEN, RA.CASES, RA.golden, RA.golden_case
FAKE = 0x10000
EINVAL = -1


# ------------------------------------------------------------------------------------------------ oracle against the reference
def test_golden_file_holds_the_issue_cases():
    g = golden()
    assert tuple(g["cases"].tolist()) == CASES and os.path.getsize(GOLDEN) < 1 << 20
    shapes = {n: (golden_case(g, n)["x"].shape, golden_case(g, n)["text"].shape[0], int(golden_case(g, n)["mask"].sum())) for n in CASES}
    assert shapes == {"h256_t288": ((288, 256), 24, 17), "h256_single_key": ((144, 256), 24, 1), "h512_left_pad": ((432, 512), 40, 29)}
    left = golden_case(g, "h512_left_pad")["mask"]
    assert left[0] == 0 and left[-1] == 1                                    # left padded: the zero rows are in front


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference(name):
    g = golden()
    c = golden_case(g, name)
    temp, topp = float(g["temp"]), float(g["topp"])
    logit = RA.logits(c["sd"], c["x"], c["text"], c["mask"])
    scores = torch.softmax(logit / temp, -1)
    e_logit, e_scores = RA.rel_l2(logit, c["logit"]), RA.rel_l2(scores, c["scores"])
    print(f"{name}: oracle vs reference rel-L2 logit {e_logit:.2e} scores {e_scores:.2e}")
    assert e_logit <= 1e-5 and e_scores <= 1e-5
    # the selection on the reference's own fp32 scores, as TextGuidedSampler.forward runs it
    assert torch.equal(RA.select(c["scores"], topp, temp), c["kept"])


# ------------------------------------------------------------------------------------------------ construction and loading
def _cfg(H=256, kind="qformer"):
    from slime_amd.model.llava_arch import default_slime_config
    return default_slime_config("synthetic:1", hidden_size=H, mm_hidden_size=128, mm_resampler_type=kind)


def test_qformer_sampler_constructs_with_the_reference_state_dict():
    from slime_amd.model.multimodal_resampler.builder import build_vision_sampler, TextGuidedRouterAttention, TextGuidedSampler
    g = golden()
    s = build_vision_sampler(_cfg())
    assert isinstance(s.selector, TextGuidedRouterAttention)
    sd = s.selector.state_dict()
    assert list(sd.keys()) == g["state_keys"].tolist()
    assert [",".join(str(n) for n in v.shape) for v in sd.values()] == g["state_shapes"].tolist()
    assert list(W.make_router_attention_state_dict(256).keys()) == g["state_keys"].tolist()
    assert not hasattr(build_vision_sampler(_cfg(kind="cosine")), "selector")
    with pytest.raises(NotImplementedError):
        TextGuidedSampler("spatial", _cfg())
    with pytest.raises(ValueError, match="multiple of 128"):
        build_vision_sampler(_cfg(H=192))


def test_checkpoint_round_trip_strict(tmp_path):
    from slime_amd.model.builder import load_adapter_checkpoint
    from slime_amd.model.llava_arch import SlimeVisualEncoder
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    rsd = W.make_router_attention_state_dict(256, seed=5)
    asd.update({"sampler.selector." + k: v for k, v in rsd.items()})
    torch.save({"model." + k: v for k, v in asd.items() if k.startswith("mm_projector.")}, os.path.join(tmp_path, "mm_projector.bin"))
    torch.save({"model." + k: v for k, v in asd.items() if k.startswith("sampler.")}, os.path.join(tmp_path, "sampler.bin"))
    enc = SlimeVisualEncoder(_cfg())
    sel = enc.get_model().sampler.selector
    sel._packed["stale"] = object()
    load_adapter_checkpoint(enc, str(tmp_path), strict=True)
    assert not sel._packed                                                   # loading clears the pack cache
    for k, v in rsd.items():
        assert torch.equal(sel.state_dict()[k], v), k
    # a checkpoint without the selector is refused under strict=True (a cosine checkpoint does not fit a qformer model)
    torch.save({"model." + k: v for k, v in asd.items() if k.startswith("sampler.post_qformer.")}, os.path.join(tmp_path, "sampler.bin"))
    with pytest.raises(RuntimeError, match="missing"):
        load_adapter_checkpoint(SlimeVisualEncoder(_cfg()), str(tmp_path), strict=True)


# ------------------------------------------------------------------------------------------------ pack-time algebra
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pack_time_algebra(dtype):
    H = 256
    sd = W.make_router_attention_state_dict(H, seed=9)
    T = ops.router_attention_host_tensors(sd, H, dtype)
    s = 128 ** -0.5 * ops.LOG2E
    in_w, in_b = sd["cross_attn.in_proj_weight"], sd["cross_attn.in_proj_bias"]
    assert torch.equal(T["w_q"], (in_w[:H] * s).to(dtype)) and torch.equal(T["b_q"], in_b[:H] * s)          # the folded q scale
    assert T["w_kv"].shape == (2 * H, H) and torch.equal(T["w_kv"][:H], in_w[H:2 * H].to(dtype)) and torch.equal(T["w_kv"][H:], in_w[2 * H:].to(dtype))
    assert torch.equal(T["b_kv"], in_b[H:])
    assert T["w_1"].shape == (128, H) and T["b_1"].shape == (128,) and T["w_2"].shape == (128,)             # H / 4 = 64 padded to 128
    assert torch.equal(T["w_1"][:64], sd["prob_proj.0.weight"].to(dtype)) and torch.equal(T["w_2"][:64], sd["prob_proj.2.weight"].view(-1))
    assert not T["w_1"][64:].any() and not T["b_1"][64:].any() and not T["w_2"][64:].any()
    assert float(T["b_2"]) == float(sd["prob_proj.2.bias"])
    assert ops.router_attention_host_tensors(W.make_router_attention_state_dict(512), 512, dtype)["w_1"].shape == (128, 512)   # no padding
    # the packed form computes the oracle's logits: float64 on the packed (rounded) tensors, q in log2 units
    g = torch.Generator().manual_seed(1)
    x, text = torch.randn(40, H, generator=g), torch.randn(6, H, generator=g)
    st = RA.stages(sd, x, text, None, operand_dtype=dtype)
    q = st["xq"] @ T["w_q"].double().T + T["b_q"].double()
    kv = st["tk"] @ T["w_kv"].double().T + T["b_kv"].double()
    assert torch.allclose(q / (s), st["q"], rtol=2e-2, atol=2e-2) and torch.allclose(kv[:, :H], st["k"], atol=1e-12) and torch.allclose(kv[:, H:], st["v"], atol=1e-12)
    att = torch.softmax((q.view(40, 2, 128).transpose(0, 1) @ kv[:, :H].reshape(6, 2, 128).transpose(0, 1).transpose(1, 2)) * math.log(2.0), -1)
    ctx = (att @ kv[:, H:].reshape(6, 2, 128).transpose(0, 1)).transpose(0, 1).reshape(40, H)
    assert RA.rel_l2(ctx, st["ctx"]) < 2e-2                                                                # the scale was rounded to T with Wq
    h = st["y"] @ T["w_1"].double().T + T["b_1"].double()
    logit = torch.relu(h) @ T["w_2"].double() + float(T["b_2"])
    assert torch.allclose(logit, st["logit"], atol=1e-12)                                                  # the padding adds exactly 0
    for bad in (192, 0, 8320):
        with pytest.raises(ValueError, match="multiple of 128"):
            ops.router_attention_host_tensors(sd, bad, dtype)


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_names_and_version():
    names = _lib.header_symbols()
    for n in ("slime_router_attn_workspace_bytes", "slime_router_attn_scores", "slime_ln_gather", "slime_router_prob_head"):
        assert n in names and n in _lib._SIGNATURES
    assert _lib.ABI_VERSION == 7 and _lib.load().slime_abi_version() == 7
    assert len(_lib._SIGNATURES["slime_router_attn_scores"][1]) == 16


def test_desc_mirror_matches_the_header_layout(tmp_path):
    """_lib.RouterAttnDesc against slime_router_attn_desc: sizeof / offsetof printed by a C program compiled against the header."""
    import re
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(slime_router_attn_desc));']
    for fname, _ in _lib.RouterAttnDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(slime_router_attn_desc, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.RouterAttnDesc)
    body = text[:text.index("} slime_router_attn_desc")]
    body = body[body.rindex("typedef struct"):]
    assert re.findall(r"\b([a-zA-Z_0-9]+)\s*[,;]", body) == [f for f, _ in _lib.RouterAttnDesc._fields_]     # every field, in order
    for fname, _ in _lib.RouterAttnDesc._fields_:
        assert int(got[fname]) == getattr(_lib.RouterAttnDesc, fname).offset, fname


# ------------------------------------------------------------------------------------------------ refusals (no launch)
def _desc(**over):
    d = _lib.RouterAttnDesc()
    d.H, d.heads, d.N1, d.dtype, d.eps, d.b_2 = 256, 2, 128, _lib.BF16, 1e-5, 0.0
    for f, _ in _lib.RouterAttnDesc._fields_:
        if f not in ("H", "heads", "N1", "dtype", "eps", "b_2") and not f.endswith("_frag"):
            setattr(d, f, FAKE)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _scores(lib, d, n_rows=(5, 0, 3), n_keys=(2, 0, 4), **over):
    B = len(n_rows)
    a = dict(tokens=FAKE, token_rows=100, tok_idx=FAKE, n_rows_host=(C.c_int * B)(*n_rows), text=FAKE, text_rows=30, key_idx=FAKE,
             n_keys_host=(C.c_int * B)(*n_keys), B=B, T_max=max(n_rows), temp=1.0, scores=FAKE, ws=None, ws_bytes=0, stream=None)
    a.update(over)
    rc = lib.slime_router_attn_scores(C.byref(d), *a.values())
    return rc, lib.slime_last_error().decode()


def test_library_refusals_come_before_any_launch():
    lib = _lib.load()
    for H in (192, 8320, 0):
        rc, msg = _scores(lib, _desc(H=H, heads=max(H // 128, 1)))
        assert rc == EINVAL and f"H={H}" in msg, msg
    rc, msg = _scores(lib, _desc(heads=3))
    assert rc == EINVAL and "heads=3" in msg
    rc, msg = _scores(lib, _desc(N1=64))
    assert rc == EINVAL and "N1=64" in msg
    rc, msg = _scores(lib, _desc(dtype=_lib.F32))
    assert rc == EINVAL and "dtype" in msg
    rc, msg = _scores(lib, _desc(w_o=None))
    assert rc == EINVAL and "missing weights" in msg
    rc, msg = _scores(lib, _desc(), n_rows=(4097, 1), n_keys=(1, 1))
    assert rc == EINVAL and "T_max=4097" in msg and "4096" in msg
    rc, msg = _scores(lib, _desc(), n_rows=(5, 0, 3), n_keys=(2, 0, 0))
    assert rc == EINVAL and "image 2" in msg and "no valid text key" in msg
    rc, msg = _scores(lib, _desc(), tokens=FAKE + 8)
    assert rc == EINVAL and "aligned" in msg
    rc, msg = _scores(lib, _desc(ln_q_w=FAKE + 4))
    assert rc == EINVAL and "aligned" in msg
    rc, msg = _scores(lib, _desc(), temp=0.0)
    assert rc == EINVAL and "temperature" in msg
    rc, msg = _scores(lib, _desc())                                          # everything valid but the workspace: still no launch
    assert rc == -2 and "workspace" in msg
    assert lib.slime_router_attn_workspace_bytes(C.byref(_desc()), 8, 6) % 256 == 0
    assert lib.slime_router_attn_workspace_bytes(C.byref(_desc()), 0, 6) == 0
    # the primitives
    assert lib.slime_ln_gather(FAKE, 10, None, 4, 192, FAKE, FAKE, 1e-5, FAKE, _lib.BF16, None) == EINVAL and "D=192" in lib.slime_last_error().decode()
    assert lib.slime_ln_gather(FAKE, 10, None, 4, 8320, FAKE, FAKE, 1e-5, FAKE, _lib.BF16, None) == EINVAL
    assert lib.slime_ln_gather(FAKE + 4, 10, None, 4, 256, FAKE, FAKE, 1e-5, FAKE, _lib.BF16, None) == EINVAL
    nr = (C.c_int * 2)(3, 4)
    assert lib.slime_router_prob_head(FAKE, 8, 128, FAKE, 0.0, nr, 2, 4, 1.0, FAKE, FAKE, None) == EINVAL and "cover 7 rows" in lib.slime_last_error().decode()
    assert lib.slime_router_prob_head(FAKE, 7, 100, FAKE, 0.0, nr, 2, 4, 1.0, FAKE, FAKE, None) == EINVAL


def test_python_refusals_raise_value_error_on_the_host():
    pra = ops.pack_router_attention(W.make_router_attention_state_dict(256), 256, torch.bfloat16, "cpu")
    assert pra.N1 == 128 and pra.heads == 2 and pra.desc.H == 256
    tokens, text = torch.zeros(5000, 256), torch.zeros(2, 6, 256)
    with pytest.raises(ValueError, match="no valid text key"):
        ops.router_attention_scores(pra, tokens, [0, 10], [4, 4], text, torch.tensor([[1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]), 1.0)
    with pytest.raises(ValueError, match="4096"):
        ops.router_attention_scores(pra, tokens, [0, 0], [4097, 4], text, None, 1.0)
    with pytest.raises(ValueError, match="multiple of 128"):
        ops.pack_router_attention(W.make_router_attention_state_dict(256), 192, torch.bfloat16, "cpu")
    # an image without tokens may have no key: it is skipped, not refused
    tok, keys, n_keys = ops._router_attention_plan([7, 20], [3, 0], 6, np.array([[0, 0, 1, 1, 0, 1], [0] * 6], dtype=bool))
    assert tok.tolist() == [7, 8, 9] and keys.tolist() == [2, 3, 5] and n_keys == [3, 0]
    tok, keys, n_keys = ops._router_attention_plan([0, 5], [2, 1], 3, None)
    assert keys.tolist() == [0, 1, 2, 3, 4, 5] and n_keys == [3, 3]


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [128, 256, 512, 4096, 5120, 8192])
def test_ln_gather_bound_holds_for_the_emulation_and_not_for_one_pass(D, dtype):
    src, idx, w, b = RA.ln_gather_inputs(D)
    assert idx.numel() > src.shape[0] and len(set(idx.tolist())) < src.shape[0]          # repeats and skips
    want, bd = RA.ln_gather_bound(src.double()[idx], w, b, dtype)
    ratio, msg = RA.RC.check("ln_gather", RA.emulate_ln_gather(src, idx, w, b, dtype), want, bd)
    assert msg is None, msg
    assert ratio > 0.02                                                      # the bound is not vacuous
    r2, msg2 = RA.RC.check("one pass", RA.emulate_ln_gather(src, idx, w, b, dtype, one_pass=True), want, bd)
    assert msg2 is not None and "worst element" in msg2                      # |mean| = 1000 sigma: E[x^2] - mu^2 leaves the bound
    assert RA.ln_gather_depth(D) == 4 * math.ceil(D / 256) + 6


@pytest.mark.parametrize("N1", [128, 1024])
def test_head_bound_holds_for_the_emulation_and_not_without_the_bias(N1):
    h, w2, b2 = RA.head_inputs(N1, 37)
    want, bd = RA.head_bound(h, w2, b2)
    ratio, msg = RA.RC.check("head", RA.emulate_head(h, w2, b2), want, bd)
    assert msg is None, msg
    _, msg2 = RA.RC.check("no bias", RA.emulate_head(h, w2, b2, drop_bias=True), want, bd)
    assert msg2 is not None
    # zero padding of w2 contributes exactly 0 whatever h holds there
    hp = torch.cat([h, 1e6 * torch.ones(37, 128)], 1)
    assert torch.equal(RA.emulate_head(hp, torch.cat([w2, torch.zeros(128)]), b2), RA.emulate_head(h, w2, b2))
