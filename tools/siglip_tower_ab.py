#!/usr/bin/env python
"""What a SigLIP tower costs next to the CLIP tower of the same build.

  1. fc1 alone at the SigLIP production shape (M = 11520 = 20 crops x 576, N = 4096, K = 1024), LayerNorm fold consumer on the
     direct-B kernel (what the tower launches), epilogue SLIME_EPI_BIAS_GELU_TANH_T against SLIME_EPI_BIAS_QUICKGELU_T, bf16 and
     fp16.  Each leg's kernel is proven by slime_gemm_kernel_name first and its output checked against an fp32 torch evaluation.
  2. a synthetic siglip-large-patch16-384 (23 layers run, S = 576, the plain front end) against the synthetic CLIP-L/14-336 tower
     (23 layers, S = 577) through the models' ``encode`` (one stream at 5 crops, the two-stream split at 40), bf16 and fp16.

One process; the legs of a comparison are alternated ROUNDS times after a warm-up of all of them (tools/gelu_fold_ab.py's loop).
Per leg the median and the spread of the per-round medians; a ratio is reported with the larger spread of its two legs beside it.
There is no pass mark.

    python tools/siglip_tower_ab.py [--steps 20] [--rounds 3] [--warmup 5] [--iters 20] [--out FILE]   (default: profiles/siglip_tower_ab.txt)
"""
import argparse
import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch

from gelu_fold_ab import alternate, sclk

M, N, K = 11520, 4096, 1024
CROPS = (5, 40)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="GEMM launches per timed step")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "siglip_tower_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, ops, weights as W
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    from slime_amd.model.multimodal_encoder.siglip_encoder import HipSiglipVisionModel
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream
    lines = [f"SigLIP tower against the CLIP tower, same build: fc1 with the LayerNorm fold at M = {M}, N = {N}, K = {K} (tanh-form GELU vs "
             f"quick-GELU), and synthetic siglip-large-patch16-384 vs CLIP-L/14-336, 23 layers each, over {CROPS[0]} and {CROPS[1]} crops",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             f"{a.iters} launches per GEMM step, HIP events per step, legs alternated in one process",
             f"sclk before the run: {sclk()}"]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g) + 0.5 * torch.randn(M, 1, generator=g)
    w = torch.randn(N, K, generator=g) * (2 * K) ** -0.5 * 2.0
    bias = torch.randn(N, generator=g) * 0.02
    epis = {"quick-GELU": _lib.EPI_BIAS_QUICKGELU_T, "tanh GELU": _lib.EPI_BIAS_GELU_TANH_T}
    flops = 2.0 * M * N * K
    for dt, tname in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        x16, w16 = x.to(dt).to(dev), w.to(dt).to(dev)
        xg = x16.double().view(M, K // 64, 64)
        stats = torch.stack([xg.sum(-1), (xg * xg).sum(-1)], -1).float().contiguous()
        colsum = w16.double().sum(1).float().contiguous()
        b = bias.to(dev)
        wf = ops.pack_b_frag(w16)
        out = torch.empty(M, N, dtype=dt, device=dev)
        mu = x16.double().mean(1, keepdim=True)
        rstd = (x16.double().var(1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
        pre = (((x16.double() - mu) * rstd).float() @ w16.float().t() + b)
        refs = {"quick-GELU": pre * torch.sigmoid(1.702 * pre), "tanh GELU": torch.nn.functional.gelu(pre, approximate="tanh")}
        legs = {}
        for ename, epi in epis.items():
            kern = ops.gemm_kernel_name(M, N, K, dt, epi, True)
            assert "gemm_db_kernel" in kern, kern
            args = _lib.GemmArgs(A=x16.data_ptr(), lda=K, B=None, bias=b.data_ptr(), C=out.data_ptr(), ldc=N, M=M, N=N, K=K,
                                 dtype=ops.dtype_code(dt), epilogue=epi, ln_stats=stats.data_ptr(), ln_groups=K // 64,
                                 ln_colsum=colsum.data_ptr(), ln_eps=1e-6, B_frag=wf.data_ptr())

            def step(args=args):
                for _ in range(a.iters):
                    _lib.check(lib.slime_gemm_ex(C.byref(args), stream()), "slime_gemm_ex")

            _lib.check(lib.slime_gemm_ex(C.byref(args), stream()), "slime_gemm_ex")
            torch.cuda.synchronize()
            err = float((out.float() - refs[ename]).norm() / refs[ename].norm())
            assert err < {torch.bfloat16: 8e-3, torch.float16: 1.2e-3}[dt], (ename, err)
            legs[f"{ename:10s} {kern}"] = step
        res = alternate(legs, a.rounds, a.steps, a.warmup)
        lines.append(f"fc1 {tname} direct-B:")
        per = []
        for k, (med, lo, hi) in res.items():
            us = med / a.iters * 1e3
            per.append((us, (hi - lo) / a.iters * 1e3))
            lines.append(f"    {k:50s} {us:8.2f} us / launch  {flops / us / 1e6:7.1f} TF/s  round medians {lo / a.iters * 1e3:.2f} .. {hi / a.iters * 1e3:.2f} us")
        (q, sq), (e, se) = per
        lines.append(f"    tanh / quick = {e / q:.4f}  ({e - q:+.2f} us; largest spread of the two legs {max(sq, se):.2f} us)")
        del x16, w16, wf, out, pre, refs
        torch.cuda.empty_cache()
    # ---- the towers
    csd = W.make_tower_state_dict(W.CLIP_L_336, seed=1234)
    ssd = W.make_siglip_state_dict(W.SIGLIP_L_384, seed=1234, head=False)
    for dt, tname in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        clip, sig = HipCLIPVisionModel(W.CLIP_L_336, dt), HipSiglipVisionModel(W.SIGLIP_L_384, dt)
        clip.load_state_dict(csd)
        sig.load_state_dict(ssd)
        clip.to(dev).to(dt)
        sig.to(dev).to(dt)
        for n in CROPS:
            pc = W.synthetic_pixels(n, seed=44, image_size=336).to(dev).to(dt)
            ps = W.synthetic_pixels(n, seed=44, image_size=384).to(dev).to(dt)
            legs = {"CLIP-L/14-336 (S = 577)": lambda: clip.encode(pc, -2), "siglip-large-patch16-384 (S = 576)": lambda: sig.encode(ps, -2)}
            res = alternate(legs, a.rounds, a.steps, a.warmup)
            streams = 2 if n >= clip.split_min_crops else 1
            lines.append(f"tower {tname}, 23 layers, {n} crops, {streams} stream(s):")
            for k, (med, lo, hi) in res.items():
                lines.append(f"    {k:36s} {med:8.3f} ms / pass   round medians {lo:.3f} .. {hi:.3f} ms")
            (c, cl, ch), (s, sl, sh) = res["CLIP-L/14-336 (S = 577)"], res["siglip-large-patch16-384 (S = 576)"]
            lines.append(f"    SigLIP / CLIP = {s / c:.4f}  ({s - c:+.3f} ms; largest spread of the two legs {max(ch - cl, sh - sl):.3f} ms)")
            del pc, ps
        del clip, sig
        torch.cuda.empty_cache()
    lines.append(f"sclk after the run: {sclk()}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
