#!/usr/bin/env python3
"""A/B timing for the sliding-window prefill attention (32 query / 8 kv heads, head_dim 128, bf16: Llama-3 / Mistral-7B), one
process, alternating legs, HIP events around >= 0.2 s of calls per sample:

  (a) slime_prefill_attention (no window) on a library built from the PARENT commit (--parent-lib) against this tree's, at
      8 x 1216 and 1 x 9280 -- with a second, independent series of the parent library as the spread ("parent again": what two
      runs of the very same code differ by on this box);
  (b) slime_prefill_attention_window at 1 x 9280 and 1 x 6000, W = 4096, beside the unwindowed call of this tree and beside
      W = S - 1 (the windowed kernel with next to no window), with the ratio of 32-key steps computed from the geometry beside
      the ratios of times.

  python tools/window_prefill_ab.py --parent-lib /path/to/parent/libslime_hip.so [--rounds 7] > profiles/window_prefill_ab.txt

Outputs are compared too: (a) must be bit-equal between the two libraries; (b) W >= S must be bit-equal to the unwindowed call.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slime_amd import _lib, ops  # noqa: E402

HQ, HKV = 32, 8
N = (HQ + 2 * HKV) * 128


def key_steps(S, W, rows):
    """32-key steps a kernel working on blocks of ``rows`` query rows has to visit: per block, from the step of the first key its
    first row sees to the step of its last row's own key (W = 0: from key 0)."""
    n = 0
    for q_lo in range(0, S, rows):
        q_hi = min(S, q_lo + rows)
        first = 0 if W <= 0 else max(0, q_lo - W + 1) >> 5
        n += ((q_hi - 1) >> 5) - first + 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    parent = C.CDLL(a.parent_lib)
    sig = _lib._SIGNATURES["slime_prefill_attention"]
    parent.slime_prefill_attention.restype, parent.slime_prefill_attention.argtypes = sig
    dt = torch.bfloat16
    st = torch.cuda.current_stream().cuda_stream
    print(f"device {torch.cuda.get_device_name(0)}; csrc {_lib.csrc_digest()}; {a.rounds} rounds, >= 0.2 s (>= {a.calls} calls) per sample, "
          f"median [min .. max] ms per call")

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def sample(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n = max(a.calls, min(1000, int(200.0 / max(timed(fn, 3), 1e-3))))          # at least 0.2 s of work per sample
        return timed(fn, n)

    def series(legs):
        t = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():                      # alternating legs inside one process
                t[k].append(sample(fn))
        return t

    def show(name, xs):
        print(f"    {name:34s} {statistics.median(xs):8.4f} [{min(xs):8.4f} .. {max(xs):8.4f}]")
        return statistics.median(xs)

    for B, S, part_a, part_b in ((8, 1216, True, False), (1, 9280, True, True), (1, 6000, False, True)):
        torch.manual_seed(S)
        qkv = (torch.randn(B, S, N, device=dev) * 0.5).to(dt)
        qkv[..., :HQ * 128] *= 0.1
        o = torch.empty((B, S, HQ * 128), dtype=dt, device=dev)
        p = qkv.data_ptr()
        head = (p, S * N, N, p + HQ * 256, S * N, N, p + (HQ + HKV) * 256, S * N, N, o.data_ptr(), S * HQ * 128, HQ * 128, B, HQ, HKV, 128, S,
                None, None, ops.dtype_code(dt))

        def plain(l=lib):
            rc = l.slime_prefill_attention(*head, st)
            assert rc == 0, rc

        def windowed(W):
            _lib.check(lib.slime_prefill_attention_window(*head, W, st), "slime_prefill_attention_window")

        plain(parent)
        torch.cuda.synchronize()
        o_parent = o.clone()
        o.zero_()
        plain(lib)
        torch.cuda.synchronize()
        o_tree = o.clone()
        if part_a:
            print(f"\n(a) unwindowed slime_prefill_attention, B={B} S={S}: outputs parent vs this tree bit-equal: {bool(torch.equal(o_parent, o_tree))}")
            t = series({"parent": lambda: plain(parent), "this tree": lambda: plain(lib), "parent again": lambda: plain(parent)})
            mp, mt, mp2 = show("parent build", t["parent"]), show("this tree", t["this tree"]), show("parent build again (spread)", t["parent again"])
            print(f"    this tree / parent {mt / mp:.4f}; parent again / parent {mp2 / mp:.4f}; "
                  f"parent's own range over both series {max(t['parent'] + t['parent again']) / min(t['parent'] + t['parent again']):.4f}")
        if part_b:
            W = 4096
            o.zero_()
            windowed(S)
            torch.cuda.synchronize()
            same = bool(torch.equal(o, o_tree))
            print(f"\n(b) windowed slime_prefill_attention_window, B={B} S={S} W={W} (W >= S bit-equal to the unwindowed call: {same})")
            t = series({"unwindowed": lambda: plain(lib), "windowed": lambda: windowed(W), "windowed, W = S - 1": lambda: windowed(S - 1)})
            mu, mw, mf = show("unwindowed (prefill32_kernel)", t["unwindowed"]), show(f"W = {W} (prefill32_kernel, WIN)", t["windowed"]), \
                show("W = S - 1 (prefill32_kernel, WIN)", t["windowed, W = S - 1"])
            s64, s64w = key_steps(S, 0, 64), key_steps(S, W, 64)
            print(f"    32-key steps from the geometry, 64-row blocks: {s64w} of {s64} = {s64w / s64:.4f} (the window removes {1 - s64w / s64:.1%})")
            print(f"    time W = {W} / unwindowed {mw / mu:.4f}; time W = {W} / W = S - 1 (same kernel, nearly no window) {mw / mf:.4f}")


if __name__ == "__main__":
    main()
