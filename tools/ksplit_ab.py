#!/usr/bin/env python
"""A/B of the opt-in deterministic split-K GEMM (slime_gemm_ksplit / ``k_split``) against the unsplit path, on the shapes a tower
pass over 1 / 5 / 9 crops launches.  Needs the GPU; there is no fallback.

Stand-alone: the tower's own calls (fragment-order weight image alone, the epilogue the layer uses) at ViT-L widths, bf16 --
out_proj M x 1024 x 1024 and fc2 M x 1024 x 4096 (BIAS_RESID_SPLIT_LN) at M = 577 / 2885 / 5193, qkv M x 3072 x 1024 (LayerNorm
fold, BIAS_T) and fc1 M x 4096 x 1024 (fold, BIAS_QUICKGELU_T) at M = 577 -- with splits 1 / 2 / 4.  splits = 1 IS slime_gemm_ex.
A timed sample is BATCH back-to-back launches between two HIP events (the launches are 10-60 us: one launch per event pair would
time the events); operands stay in the caches between launches, for every leg alike.
Tower: HipCLIPVisionModel.encode over 1 / 5 / 9 crops, 24-layer ViT-L/14-336 (23 run), ``k_split=None`` against the tuples of
CANDIDATES (qkv, out_proj, fc1, fc2).

One process; every leg warmed up, then the legs of a group ALTERNATED ``--rounds`` times; per leg the median over all samples and the
spread of the per-round medians.  A leg "wins" only where its gain over the unsplit leg exceeds the larger of the two spreads.

    python tools/ksplit_ab.py [--rounds 5] [--steps 20] [--out FILE]        (default: profiles/ksplit_ab.txt)
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

BATCH = 20
CANDIDATES = [(1, 1, 1, 2), (1, 1, 1, 4), (1, 2, 1, 2), (1, 2, 1, 4), (2, 2, 2, 4), (2, 4, 2, 8)]


def sclk():
    try:
        o = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        got = [ln.split("(")[-1].split(")")[0] for ln in o.splitlines() if "sclk" in ln]
        return got[0] if got else "?"
    except Exception as e:                   # the clock is context for the reader, not an input of the measurement
        return f"? ({type(e).__name__})"


def alternate(legs, rounds, steps, warmup, batch):
    """legs: name -> callable.  Returns name -> (median ms per call, min and max of the per-round medians)."""
    for fn in legs.values():
        for _ in range(warmup * batch):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for e0, e1 in evs:
                e0.record()
                for _ in range(batch):
                    fn()
                e1.record()
            torch.cuda.synchronize()
            per_round[k].append([e0.elapsed_time(e1) / batch for e0, e1 in evs])
    out = {}
    for k, rs in per_round.items():
        rm = [statistics.median(r) for r in rs]
        out[k] = (statistics.median([t for r in rs for t in r]), min(rm), max(rm))
    return out


def report(lines, title, res, base, unit, scale):
    lines.append(title)
    lines.append(f"    {'leg':22s} {'median ' + unit:>11s} {'round medians min .. max':>28s} {'spread':>8s} {'vs unsplit':>11s}  verdict")
    b_med, b_lo, b_hi = res[base]
    for k, (med, lo, hi) in res.items():
        spread = max(hi - lo, b_hi - b_lo)
        gain = b_med - med
        verdict = "" if k == base else ("wins" if gain > spread else ("loses" if -gain > spread else "within the spread"))
        lines.append(f"    {k:22s} {med * scale:11.2f} {lo * scale:13.2f} .. {hi * scale:<12.2f} {(hi - lo) * scale:8.2f} {med / b_med:11.3f}  {verdict}")


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "ksplit_ab.txt"))
    a = ap.parse_args()
    assert a.rounds >= 3 and a.steps >= 10, "at least 3 alternations of 10 samples per leg"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, ops, weights as W
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    lib = _lib.load()
    lines = [f"k-split A/B: device {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs, "
             f"csrc {_lib.csrc_digest()}, bf16, ViT-L widths",
             f"{a.warmup} warm-up + {a.rounds} rounds x {a.steps} samples per leg, legs of a group alternated in one process; a stand-alone sample = "
             f"{BATCH} back-to-back launches between two HIP events",
             f"sclk before the run: {sclk()}"]

    # ---- stand-alone launches ------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    D, F = 1024, 4096

    def operand(n, k):
        w = (torch.randn(n, k, generator=g, device=dev) * k ** -0.5).to(dt)
        return ops.pack_b_frag(w), w.float().sum(1).contiguous(), torch.randn(n, generator=g, device=dev) * 0.02

    shapes = [("out_proj", M, D, D, "resid") for M in (577, 2885, 5193)] + [("fc2", M, D, F, "resid") for M in (577, 2885, 5193)]
    shapes += [("qkv", 577, 3 * D, D, "fold_t"), ("fc1", 577, F, D, "fold_gelu")]
    for name, M, N, K, kind in shapes:
        wf, colsum, bias = operand(N, K)
        x = torch.randn(M, K, generator=g, device=dev).to(dt)
        ws_bytes = lib.slime_gemm_ksplit_workspace_bytes(M, N, 4)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        ws = ws[(-ws.data_ptr()) % 256:][:ws_bytes]
        # the argument block is built once and the C entry called directly: per launch the host then spends a ctypes call, well
        # under the 10-60 us of the kernels (the ops wrappers allocate an output per call)
        ga = _lib.GemmArgs(A=x.data_ptr(), lda=K, B=None, bias=bias.data_ptr(), M=M, N=N, K=K, dtype=_lib.BF16, B_frag=wf.data_ptr())
        if kind == "resid":
            hi, lo = ops.resid_split(torch.randn(M, N, generator=g, device=dev), dt)
            st_out = torch.empty(M, N // 64, 2, device=dev)
            epi = _lib.EPI_BIAS_RESID_SPLIT_LN
            ga.C, ga.ldc, ga.lo8, ga.ldlo, ga.stats_out = hi.data_ptr(), N, lo.data_ptr(), N, st_out.data_ptr()
        else:
            xs = x.float().view(M, K // 64, 64)
            stats = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).contiguous()
            out = torch.empty(M, N, dtype=dt, device=dev)
            epi = _lib.EPI_BIAS_T if kind == "fold_t" else _lib.EPI_BIAS_QUICKGELU_T
            ga.C, ga.ldc, ga.ln_stats, ga.ln_groups, ga.ln_colsum, ga.ln_eps = out.data_ptr(), N, stats.data_ptr(), K // 64, colsum.data_ptr(), 1e-5
        ga.epilogue = epi
        stream = torch.cuda.current_stream().cuda_stream
        legs = {}
        for s in (1, 2, 4):
            _lib.check(lib.slime_gemm_ksplit(C.byref(ga), s, ws.data_ptr(), ws_bytes, stream), "slime_gemm_ksplit")
            legs[f"splits={s}"] = (lambda s=s: lib.slime_gemm_ksplit(C.byref(ga), s, ws.data_ptr(), ws_bytes, stream))
        res = alternate(legs, a.rounds, a.steps, a.warmup, BATCH)
        unsplit = ops.gemm_kernel_name(M, N, K, dt, epi, True)
        report(lines, f"{name}: M={M} N={N} K={K}  (unsplit kernel: {unsplit})", res, "splits=1", "us", 1e3)
        del ws

    # ---- the tower --------------------------------------------------------------------------------------------------------------
    vm = HipCLIPVisionModel(W.CLIP_L_336)
    vm.load_state_dict(W.make_tower_state_dict(W.CLIP_L_336, seed=1234))
    vm.to(dev).to(dt)
    for n in (1, 5, 9):
        px = W.synthetic_pixels(n, seed=3).to(dev).to(dt)

        def leg(ks):
            def run():
                vm.k_split = ks
                return vm.encode(px)
            return run
        legs = {"k_split=None": leg(None)}
        for ks in CANDIDATES:
            legs["k_split=" + ",".join(map(str, ks))] = leg(ks)
        ref = legs["k_split=None"]().float()
        worst = max(float((fn().float() - ref).norm() / ref.norm()) for fn in legs.values())
        res = alternate(legs, a.rounds, a.steps, a.warmup, 1)
        report(lines, f"tower, {n} crop(s), encode() ({'two streams' if n >= vm.split_min_crops else 'one stream'}); worst rel-L2 of a split "
                      f"leg's features to the unsplit leg's: {worst:.2e}", res, "k_split=None", "ms", 1.0)
    vm.k_split = None
    lines.append(f"sclk after the run: {sclk()}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
