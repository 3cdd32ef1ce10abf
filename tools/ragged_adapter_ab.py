#!/usr/bin/env python
"""A/B of the two programs a RAGGED batch can take through ``SlimeVisualEncoder.encode_visual``: the ragged fused adapter
(``fused_adapter=True``: slime_adapter_forward_ragged on the tower's 16-bit features) against the per-module sequence
(``fused_adapter=False``: fp32 hand-over, two index_select copies, GatedBlock + post_qformer + MLP sequences, one merge_rows
launch per image) -- what such a batch ran before the ragged entry point existed.

SliME-8B dims, synthetic weights, bf16, 8 images with the local-crop grids GRIDS below (30 local + 8 global = 38 crops).  One
process, HIP events around every step, the legs alternated ROUNDS times after a warm-up of every leg; per leg the median step and
the spread of the per-round medians.  Two tower-only legs (the tower handing over T / fp32 features, as the two programs ask it
to) give the adapter's share by subtraction.  The outputs of the two programs are compared on the same input first.

    python tools/ragged_adapter_ab.py [--steps 20] [--rounds 4] [--warmup 5] [--out FILE]   (default: profiles/ragged_adapter_ab.txt)
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

GRIDS = [(2, 1), (1, 3), (2, 2), (2, 2), (3, 2), (1, 2), (2, 3), (3, 1)]
SIZES = [(672, 336), (336, 1008), (672, 672), (672, 672), (1008, 700), (336, 336), (700, 1008), (1008, 336)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_adapter_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, mm_utils as M, weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = default_slime_config("synthetic:1234")
    assert [tuple(M.get_anyres_image_grid_shape(s, cfg.image_grid_pinpoints, 336)) for s in SIZES] == GRIDS
    enc = SlimeVisualEncoder(cfg)
    enc.load_visual_state(W.make_tower_state_dict(W.CLIP_L_336, seed=1234), W.make_adapter_state_dict(W.ADAPTER_8B, seed=4321))
    enc.to(dev)
    tower = enc.get_vision_tower()
    tower.vision_tower.to(dt)
    counts = [1 + nw * nh for nw, nh in GRIDS]
    images = W.synthetic_pixels(sum(counts), seed=77).to(dev).to(dt)

    def step(fused):
        cfg.fused_adapter = fused
        return enc.encode_visual(images, counts, SIZES, merge="spatial")

    legs = {
        "fused (ragged call)": lambda: step(True),
        "per-module sequence": lambda: step(False),
        "tower only, T features": lambda: tower(images, out_dtype=dt),
        "tower only, fp32 features": lambda: tower(images, out_dtype=torch.float32),
    }
    lines = [f"ragged adapter A/B: {len(GRIDS)} images, grids {GRIDS}, {sum(counts)} crops, bf16, SliME-8B dims, synthetic weights",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             "HIP events per step, legs alternated in one process"]
    # same input, both programs: the outputs agree to the operand type's rounding (the fused program hands over T features, as the
    # reference's tower does; the per-module one fp32 features)
    fo, mo = step(True), step(False)
    torch.cuda.synchronize()
    num = sum(float((f[0].double() - m[0].double()).pow(2).sum() + (f[1].double() - m[1].double()).pow(2).sum()) for f, m in zip(fo, mo))
    den = sum(float(m[0].double().pow(2).sum() + m[1].double().pow(2).sum()) for m in mo)
    lines.append(f"outputs, fused vs per-module, all token rows: rel-L2 {(num / den) ** 0.5:.3e}")
    del fo, mo
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [[] for _ in range(a.rounds)] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            for s0, s1 in evs:
                s0.record()
                fn()
                s1.record()
            torch.cuda.synchronize()
            times[k][r] = [s0.elapsed_time(s1) for s0, s1 in evs]
    med = {}
    lines.append(f"{'leg':28s} {'median ms':>10s} {'round medians (min .. max)':>30s} {'spread':>8s}")
    for k, rounds in times.items():
        rm = [statistics.median(x) for x in rounds]
        med[k] = statistics.median([t for x in rounds for t in x])
        lines.append(f"{k:28s} {med[k]:10.3f} {min(rm):14.3f} .. {max(rm):<12.3f} {max(rm) - min(rm):8.3f}")
    ad_f = med["fused (ragged call)"] - med["tower only, T features"]
    ad_m = med["per-module sequence"] - med["tower only, fp32 features"]
    lines.append(f"adapter alone (step - its tower leg): fused {ad_f:.3f} ms, per-module {ad_m:.3f} ms")
    lines.append(f"step: fused / per-module = {med['fused (ragged call)'] / med['per-module sequence']:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
