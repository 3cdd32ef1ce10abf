#!/usr/bin/env python
"""What an exact-GELU tower (HF ``hidden_act='gelu'``: the OpenCLIP family) costs next to the quick-GELU tower of the same build.

  1. fc1 alone at the production shape (M = 11540 = 20 crops x 577, N = 4096, K = 1024), LayerNorm fold consumer, epilogue
     SLIME_EPI_BIAS_GELU_T against SLIME_EPI_BIAS_QUICKGELU_T: the direct-B kernel (fragment-order weights: what the tower launches)
     and the stream kernel (row-major weights only), bf16 and fp16.  Each leg's kernel is proven by slime_gemm_kernel_name first, and
     both outputs are checked against an fp32 torch evaluation of the same rounded operands.
  2. the 23-layer ViT-L/14-336 tower over 20 crops on one stream, the same synthetic weights packed with each activation.

One process; the legs of a comparison are alternated ROUNDS times after a warm-up of all of them.  A GEMM step is ITERS launches
between two HIP events (one launch is ~0.1 ms: too short a window on its own), a tower step is one pass.  Per leg the median and the
spread of the per-round medians; a ratio is reported with the larger spread of its two legs beside it.  There is no pass mark.

    python tools/gelu_fold_ab.py [--steps 20] [--rounds 4] [--warmup 5] [--iters 20] [--out FILE]   (default: profiles/gelu_fold_ab.txt)
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

M, N, K = 11540, 4096, 1024
CROPS = 20


def sclk():
    try:
        o = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        got = [ln.split("(")[-1].split(")")[0] for ln in o.splitlines() if "sclk" in ln]
        return got[0] if got else "?"
    except Exception as e:                   # the clock is context for the reader, not an input of the measurement
        return f"? ({type(e).__name__})"


def alternate(legs, rounds, steps, warmup):
    """legs: name -> callable that enqueues one step.  -> name -> (median ms per step, min and max of the per-round medians)."""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for s0, s1 in evs:
                s0.record()
                fn()
                s1.record()
            torch.cuda.synchronize()
            times[k].append([s0.elapsed_time(s1) for s0, s1 in evs])
    out = {}
    for k, rounds_ in times.items():
        rm = [statistics.median(x) for x in rounds_]
        out[k] = (statistics.median([t for x in rounds_ for t in x]), min(rm), max(rm))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="GEMM launches per timed step")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gelu_fold_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, ops, weights as W
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream().cuda_stream
    lines = [f"exact GELU against quick-GELU, same build: fc1 with the LayerNorm fold at M = {M}, N = {N}, K = {K}, and the 23-layer "
             f"ViT-L/14-336 tower over {CROPS} crops",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             f"{a.iters} launches per GEMM step, HIP events per step, legs alternated in one process",
             f"sclk before the run: {sclk()}"]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g) + 0.5 * torch.randn(M, 1, generator=g)
    w = torch.randn(N, K, generator=g) * (2 * K) ** -0.5 * 2.0
    bias = torch.randn(N, generator=g) * 0.02
    epis = {"quick-GELU": _lib.EPI_BIAS_QUICKGELU_T, "exact GELU": _lib.EPI_BIAS_GELU_T}
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
        rstd = (x16.double().var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
        pre = (((x16.double() - mu) * rstd).float() @ w16.float().t() + b)
        refs = {"quick-GELU": pre * torch.sigmoid(1.702 * pre), "exact GELU": torch.nn.functional.gelu(pre)}
        for kname, frag in (("direct-B", wf), ("stream", None)):
            legs = {}
            for ename, epi in epis.items():
                kern = ops.gemm_kernel_name(M, N, K, dt, epi, frag is not None)
                assert ("gemm_db_kernel" if frag is not None else "gemm_w4_kernel") in kern, kern
                args = _lib.GemmArgs(A=x16.data_ptr(), lda=K, B=w16.data_ptr(), bias=b.data_ptr(), C=out.data_ptr(), ldc=N, M=M, N=N, K=K,
                                     dtype=ops.dtype_code(dt), epilogue=epi, ln_stats=stats.data_ptr(), ln_groups=K // 64,
                                     ln_colsum=colsum.data_ptr(), ln_eps=1e-5, B_frag=None if frag is None else frag.data_ptr())

                def step(args=args):
                    for _ in range(a.iters):
                        _lib.check(lib.slime_gemm_ex(C.byref(args), stream()), "slime_gemm_ex")

                _lib.check(lib.slime_gemm_ex(C.byref(args), stream()), "slime_gemm_ex")
                torch.cuda.synchronize()
                err = float((out.float() - refs[ename]).norm() / refs[ename].norm())
                assert err < {torch.bfloat16: 8e-3, torch.float16: 1.2e-3}[dt], (kname, ename, err)
                legs[f"{ename:10s} {kern}"] = step
            res = alternate(legs, a.rounds, a.steps, a.warmup)
            lines.append(f"fc1 {tname} {kname}:")
            per = []
            for k, (med, lo, hi) in res.items():
                us = med / a.iters * 1e3
                per.append((us, (hi - lo) / a.iters * 1e3))
                lines.append(f"    {k:70s} {us:8.2f} us / launch  {flops / us / 1e6:7.1f} TF/s  round medians {lo / a.iters * 1e3:.2f} .. {hi / a.iters * 1e3:.2f} us")
            (q, sq), (e, se) = per
            lines.append(f"    exact / quick = {e / q:.4f}  (+{e - q:.2f} us; largest spread of the two legs {max(sq, se):.2f} us)")
        del x16, w16, wf, out, pre, refs
        torch.cuda.empty_cache()
    # ---- the tower
    import dataclasses
    sd = W.strip_tower_prefix(W.make_tower_state_dict(W.CLIP_L_336, seed=1234))
    px = W.synthetic_pixels(CROPS, seed=44)
    for dt, tname in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        towers = {"quick-GELU": ops.pack_tower(sd, W.CLIP_L_336, dt, dev),
                  "exact GELU": ops.pack_tower(sd, dataclasses.replace(W.CLIP_L_336, hidden_act="gelu"), dt, dev)}
        p = px.to(dev).to(dt)
        outs = {k: torch.empty(CROPS, 576, 1024, dtype=dt, device=dev) for k in towers}
        legs = {k: (lambda pt=pt, o=outs[k]: ops.tower_forward(pt, p, out_dtype=dt, out=o)) for k, pt in towers.items()}
        res = alternate(legs, a.rounds, a.steps, a.warmup)
        d = float((outs["exact GELU"].float() - outs["quick-GELU"].float()).norm() / outs["quick-GELU"].float().norm())
        lines.append(f"tower {tname}, 23 layers, {CROPS} crops, one stream (the two activations' features differ by rel-L2 {d:.2e}):")
        for k, (med, lo, hi) in res.items():
            lines.append(f"    {k:12s} {med:8.3f} ms / pass   round medians {lo:.3f} .. {hi:.3f} ms")
        (q, ql, qh), (e, el, eh) = res["quick-GELU"], res["exact GELU"]
        lines.append(f"    exact / quick = {e / q:.4f}  (+{e - q:.3f} ms; largest spread of the two legs {max(qh - ql, eh - el):.3f} ms)")
        del towers, outs
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
