#!/usr/bin/env python
"""A/B of the two programs a batch of DIFFERENTLY sized images can take through the device slicer: the job-table slicer
(``mm_utils.process_images_gpu_ragged``: slime_slice_jobs, two launches and one table upload for the batch) against the per-image
loop over ``mm_utils.process_anyres_image_gpu`` (up to four resample launches, a zeroed canvas, two tile+normalise launches and a
torch.cat per image) -- what such a batch ran before the job table existed.

Eight device-resident uint8 images of the sizes SIZES below (2 to 6 local crops each: the slicing rule never gives fewer than 2),
real CLIP processor (crop 336), bf16 output, coefficient tables warm.  One process, the legs alternated ROUNDS times after a warm-up
of both; per step a pair of HIP events (device time from the first launch to the last kernel's end) and a host clock around the step
ending in a synchronise (wall time: what the caller waits for).  Per leg the median step and the spread of the per-round medians.
The outputs of the two programs are compared on the same input first (they must be equal).

    python tools/ragged_slicer_ab.py [--steps 200] [--rounds 4] [--warmup 10] [--out FILE]   (default: profiles/ragged_slicer_ab.txt)
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

SIZES = [(336, 336), (1600, 300), (1000, 150), (400, 1100), (640, 480), (500, 900), (1008, 700), (1920, 1080)]
PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ragged_slicer_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    proc = ClipImageProcessor()
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    n_local = [M.anyres_geometry(s, 336)[6] for s in SIZES]
    assert len(set(SIZES)) == 8
    images = [torch.from_numpy(np.random.default_rng(i).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(dev) for i, (w, h) in enumerate(SIZES)]

    def loop():
        return [M.process_anyres_image_gpu(im, proc, PIN, dev, dt) for im in images]

    def ragged():
        return M.process_images_gpu_ragged(images, proc, cfg, dev, dt)[0]

    legs = {"per-image loop": loop, "job table (ragged call)": ragged}
    lines = [f"ragged slicer A/B: {len(SIZES)} device-resident images {SIZES}, local crops {n_local}, {sum(n_local) + len(SIZES)} crops, bf16 output",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             "HIP events (device) and host clock to synchronise (wall) per step, legs alternated in one process"]
    same = torch.equal(torch.cat(loop()), ragged())
    lines.append(f"outputs, job table vs per-image loop, all crops: {'identical' if same else 'DIFFERENT'}")
    assert same
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    dev_ms = {k: [[] for _ in range(a.rounds)] for k in legs}
    wall_ms = {k: [[] for _ in range(a.rounds)] for k in legs}
    for r in range(a.rounds):
        for k, fn in (list(legs.items()) if r % 2 == 0 else list(legs.items())[::-1]):
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                wall_ms[k][r].append((time.perf_counter() - t0) * 1e3)
                dev_ms[k][r].append(e0.elapsed_time(e1))
    med = {}
    lines.append(f"{'leg':26s} {'what':8s} {'median ms':>10s} {'round medians (min .. max)':>30s} {'spread':>8s}")
    for k in legs:
        for what, t in (("device", dev_ms[k]), ("wall", wall_ms[k])):
            rm = [statistics.median(x) for x in t]
            med[k, what] = statistics.median([v for x in t for v in x])
            lines.append(f"{k:26s} {what:8s} {med[k, what]:10.4f} {min(rm):14.4f} .. {max(rm):<12.4f} {max(rm) - min(rm):8.4f}")
    for what in ("device", "wall"):
        lines.append(f"{what}: job table / per-image loop = {med['job table (ragged call)', what] / med['per-image loop', what]:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
