#!/usr/bin/env python3
"""Generate tests/golden/router_attention.npz by running the REFERENCE's attention router (build container only; CPU; seconds).

    python tools/make_golden_router_attention.py

Loads ``slime_amd.weights.make_router_attention_state_dict`` into the reference's ``TextGuidedSampler('qformer', cfg)``
(llava/model/multimodal_resampler/builder.py:222-281), runs its eval path in fp32 and stores, per case: the inputs (bf16-exact
values, kept as their 16-bit patterns to stay under the size limit for a committed file), the fp32 logits (output of ``prob_proj``),
the selector's scores, the kept indices, and the reference's OWN same-dtype drift -- rel-L2 and max-abs of the scores of the module
cast to bf16 / fp16 (inputs cast likewise) against its fp32 run.  The drift measures the reference, not this project's code; the GPU
tests bound the HIP path by it.  Also the state-dict key list with shapes.  Only numbers are written; nothing of the reference
travels.  The archive is written with fixed timestamps, so a rerun reproduces the committed file bit for bit.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from slime_amd import weights as W          # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "router_attention.npz")
TOPP, TEMP = 0.95, 1.0
# name, H, T, L, mask pattern ("right" / "left" padded), valid keys, seeds
CASES = (("h256_t288", 256, 288, 24, "right", 17, 31),
         ("h256_single_key", 256, 144, 24, "right", 1, 32),
         ("h512_left_pad", 512, 432, 40, "left", 29, 33))


def case_inputs(H, T, L, side, n_valid, seed):
    """bf16-exact fp32 inputs: local tokens ~ N(0, 1), text ~ N(0, 1) with ZERO rows at the padded positions (as
    get_pure_text_embedding leaves them), the mask as int64."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16).float()
    text = torch.randn(L, H, generator=g).to(torch.bfloat16).float()
    mask = torch.zeros(L, dtype=torch.int64)
    if side == "left":
        mask[L - n_valid:] = 1
    else:
        mask[:n_valid] = 1
    text[mask == 0] = 0.0
    return x, text, mask


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    assert torch.equal(t.to(torch.bfloat16).float(), t)
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def run_reference(sampler, x, text, mask):
    """-> (logit, scores, kept indices) of one eval-mode call, in the module's dtype."""
    got = {}
    hook = sampler.selector.prob_proj.register_forward_hook(lambda m, i, o: got.__setitem__("logit", o.detach().squeeze(-1)))
    with torch.no_grad():
        scores = sampler.selector(x, text, mask)
        kept_rows = sampler(x, text, mask)
    hook.remove()
    # forward returns the kept ROWS (ascending index order); the rows are distinct random vectors: recover their indices
    eq = (kept_rows.unsqueeze(1) == x.unsqueeze(0)).all(-1)
    assert bool((eq.sum(1) == 1).all())
    return got["logit"], scores, eq.float().argmax(1)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (a rerun is bit-identical)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    from oracle.make_golden import import_reference
    import_reference()
    from llava.model.multimodal_resampler.builder import TextGuidedSampler
    torch.manual_seed(0)
    torch.set_num_threads(1)                                   # one summation order, whatever the machine
    rec = {"topp": np.float64(TOPP), "temp": np.float64(TEMP), "cases": np.array([c[0] for c in CASES])}
    for name, H, T, L, side, n_valid, seed in CASES:
        cfg = SimpleNamespace(mm_resampler_dim=144, mm_resampler_topp=TOPP, mm_resampler_temp=TEMP, hidden_size=H, mm_hidden_size=128,
                              pad_token_id=0)
        sampler = TextGuidedSampler("qformer", cfg).eval()
        sd = W.make_router_attention_state_dict(H, seed=seed)
        sampler.selector.load_state_dict(sd, strict=True)
        x, text, mask = case_inputs(H, T, L, side, n_valid, seed + 100)
        logit, scores, kept = run_reference(sampler, x, text, mask)
        # one valid key: every query attends to it with weight 1, so every token gets the same logit (scores = 1 / T) by construction
        assert logit.dtype == torch.float32 and (n_valid == 1 or float(scores.std() * T) > 1e-3), "degenerate scores"
        rec.update({f"{name}.H": np.int64(H), f"{name}.seed": np.int64(seed), f"{name}.x_bf16": bf16_bits(x), f"{name}.text_bf16": bf16_bits(text),
                    f"{name}.mask": mask.numpy(), f"{name}.logit": logit.numpy(), f"{name}.scores": scores.numpy(), f"{name}.kept": kept.numpy()})
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            low = TextGuidedSampler("qformer", cfg).eval()
            low.selector.load_state_dict(sd, strict=True)
            low = low.to(dt)
            _, s_low, _ = run_reference(low, x.to(dt), text.to(dt), mask)
            d = s_low.double() - scores.double()
            rec[f"{name}.drift_{tag}"] = np.array([float(d.norm() / scores.double().norm()), float(d.abs().max())])
            print(f"{name} {tag}: rel-L2 {rec[f'{name}.drift_{tag}'][0]:.3e} max-abs {rec[f'{name}.drift_{tag}'][1]:.3e}")
        if name == CASES[0][0]:
            ref_sd = sampler.selector.state_dict()
            rec["state_keys"] = np.array(list(ref_sd.keys()))
            rec["state_shapes"] = np.array([",".join(str(n) for n in v.shape) for v in ref_sd.values()])
        print(f"{name}: kept {kept.numel()} of {T}, scores in [{float(scores.min()):.3e}, {float(scores.max()):.3e}]")
    write_npz(OUT, rec)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
