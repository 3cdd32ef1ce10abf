#!/usr/bin/env python3
"""Time the step's router, cosine against attention (mm_resampler_type 'cosine' / 'qformer'), at B = 8 images, T = 576 local
tokens, L = 64 text tokens (48 valid), H = 4096, bf16 operands: ``ops.router_select_batched_device`` against
``ops.router_attention_select_batched_device`` on the same token buffer, HIP events per call (each call ends with the read of the B
kept counts, so the host sync is inside the figure), legs alternated.  Writes profiles/router_attention_ab.txt.  No threshold is
attached: the attention router does 4 GEMMs and B attention launches where the cosine router does two HBM passes.

    python tools/router_attention_ab.py
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slime_amd import _lib, ops, weights as W          # noqa: E402

B, T, L, VALID, H, P = 8, 576, 64, 48, 4096, 576
ROUNDS, STEPS, WARMUP = 4, 20, 5


def main():
    _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    rows = P + T
    tokens = torch.randn(B * rows, H, generator=g).to(dev)
    off, n_rows = [b * rows + P for b in range(B)], [T] * B
    text = torch.randn(B, L, H, generator=g)
    mask = torch.zeros(B, L, dtype=torch.int64)
    mask[:, :VALID] = 1
    text[mask == 0] = 0.0
    text_d, mask_d = text.to(dev), mask.to(dev)
    pra = ops.pack_router_attention(W.make_router_attention_state_dict(H, seed=7), H, torch.bfloat16, dev)
    legs = {"cosine": lambda: ops.router_select_batched_device(tokens, off, n_rows, text_d, mask_d, 0.95, 1.0),
            "attention (host mask)": lambda: ops.router_attention_select_batched_device(pra, tokens, off, n_rows, text_d, mask, 0.95, 1.0),
            "attention (device mask)": lambda: ops.router_attention_select_batched_device(pra, tokens, off, n_rows, text_d, mask_d, 0.95, 1.0)}
    for fn in legs.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    med = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, fn in legs.items():
            ts = []
            for _ in range(STEPS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                st = fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            med[name].append(statistics.median(ts))
    lines = [f"router A/B: B={B} T={T} L={L} ({VALID} valid keys) H={H} bf16; {ROUNDS} rounds x {STEPS} calls per leg, alternated; ms per call",
             f"device: {torch.cuda.get_device_name(0)}; csrc {_lib.csrc_digest()}; kept counts of the last call: {st.counts}"]
    for name, m in med.items():
        lines.append(f"{name:26s} median of round medians {statistics.median(m):8.3f} ms   (round medians {min(m):.3f} .. {max(m):.3f})")
    out = "\n".join(lines) + "\n"
    print(out, end="")
    with open(os.path.join(ROOT, "profiles", "router_attention_ab.txt"), "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
