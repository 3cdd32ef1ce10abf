#!/usr/bin/env python
"""What a DINOv2 tower costs, next to the CLIP tower of the same build at the same run size.

  1. (default) a synthetic DINOv2 ViT-L/14 with 4 registers run at 224 (23 layers run, S = 261, the prefix front end, LayerScale folded
     into out_proj / fc2) against the synthetic CLIP-L/14 tower at 224 (23 layers, S = 257) through the models' ``encode``, at 5
     crops (one stream) and 20 crops (the two-stream split), bf16 and fp16.  One process; the legs of a comparison are alternated
     ROUNDS times after a warm-up of all of them (tools/gelu_fold_ab.py's loop).  Per leg the median and the spread of the per-round
     medians; a ratio is reported with the larger spread of its two legs beside it.
  2. ``--trace CROPS``: nothing but warm-up + ``--steps`` passes of the DINOv2 tower (bf16, one stream): the program of a
     ``rocprofv3 --kernel-trace --stats -- python tools/dinov2_tower_ab.py --trace 5`` run of its own.
  3. ``--kernel-stats CSV``: per-kernel calls and average time from that run's ``*kernel_stats.csv``, appended to ``--out``.

There is no pass mark.

    python tools/dinov2_tower_ab.py [--steps 20] [--rounds 3] [--warmup 5] [--out FILE]   (default: profiles/dinov2_tower_ab.txt)
"""
import argparse
import csv
import dataclasses
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

CROPS = (5, 20)
SELECT = -2


def towers(dt, dev):
    from slime_amd import weights as W
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    from slime_amd.model.multimodal_encoder.dinov2_encoder import HipDinov2VisionModel
    ccfg = dataclasses.replace(W.CLIP_L_336, image_size=224)
    clip, dino = HipCLIPVisionModel(ccfg, dt), HipDinov2VisionModel(W.DINOV2_L_REG4_224, dt)
    clip.load_state_dict(W.make_tower_state_dict(ccfg, seed=1234))
    dino.load_state_dict(W.make_dinov2_state_dict(W.DINOV2_L_REG4_224, seed=1234))
    clip.to(dev).to(dt)
    dino.to(dev).to(dt)
    return clip, dino


def kernel_stats(path, out, label):
    """Calls and average duration per kernel of a rocprofv3 ``--stats`` csv, largest total first."""
    rows = list(csv.DictReader(open(path)))
    key = lambda names: next(k for k in rows[0] if k.lower().replace("_", "") in names)
    name, calls, total, avg = key(("name", "kernelname")), key(("calls",)), key(("totaldurationns",)), key(("averagens",))
    rows.sort(key=lambda r: -float(r[total]))
    whole = sum(float(r[total]) for r in rows)
    lines = [f"per-kernel times, {label} (rocprofv3 --kernel-trace --stats, a run of its own; pack-time kernels included):",
             f"    {'kernel':78s} {'calls':>6s} {'avg us':>9s} {'share':>6s}"]
    for r in rows:
        if float(r[total]) < 0.002 * whole:
            continue
        lines.append(f"    {r[name][:78]:78s} {int(float(r[calls])):6d} {float(r[avg]) / 1e3:9.2f} {100 * float(r[total]) / whole:5.1f}%")
    text = "\n".join(lines)
    print(text)
    with open(out, "a") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, metavar="CROPS")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV")
    ap.add_argument("--label", default="DINOv2 ViT-L/14-224 + 4 registers, bf16")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "dinov2_tower_ab.txt"))
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out, a.label)
    import torch
    from gelu_fold_ab import alternate, sclk
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, weights as W
    dev = torch.device("cuda:0")
    if a.trace:
        _, dino = towers(torch.bfloat16, dev)
        dino.two_streams = False
        px = W.synthetic_pixels(a.trace, seed=44, image_size=224).to(dev).to(torch.bfloat16)
        for _ in range(a.warmup + a.steps):
            dino.encode(px, SELECT)
        torch.cuda.synchronize()
        return
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    lines = [f"DINOv2 tower against the CLIP tower, same build, same run size: synthetic DINOv2 ViT-L/14 + 4 registers at 224 (S = 261) vs "
             f"CLIP-L/14 at 224 (S = 257), 23 layers each, over {CROPS[0]} and {CROPS[1]} crops",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             f"HIP events per step, legs alternated in one process",
             f"sclk before the run: {sclk()}"]
    for dt, tname in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        clip, dino = towers(dt, dev)
        for n in CROPS:
            px = W.synthetic_pixels(n, seed=44, image_size=224).to(dev).to(dt)
            legs = {"CLIP-L/14-224 (S = 257)": lambda: clip.encode(px, SELECT), "DINOv2-L/14-224 + 4 reg (S = 261)": lambda: dino.encode(px, SELECT)}
            res = alternate(legs, a.rounds, a.steps, a.warmup)
            streams = 2 if n >= clip.split_min_crops else 1
            lines.append(f"tower {tname}, 23 layers, {n} crops, {streams} stream(s):")
            for k, (med, lo, hi) in res.items():
                lines.append(f"    {k:36s} {med:8.3f} ms / pass   round medians {lo:.3f} .. {hi:.3f} ms")
            (c, cl, ch), (s, sl, sh) = res["CLIP-L/14-224 (S = 257)"], res["DINOv2-L/14-224 + 4 reg (S = 261)"]
            lines.append(f"    DINOv2 / CLIP = {s / c:.4f}  ({s - c:+.3f} ms; largest spread of the two legs {max(ch - cl, sh - sl):.3f} ms)")
            del px
        del clip, dino
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
