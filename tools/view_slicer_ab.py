#!/usr/bin/env python
"""A/B of the three programs an image can take through the 'pad', 'pad_then_devide', 'any_res' and bare-processor (None) modes of
``process_images``:

  host        ``mm_utils.process_images`` (PIL on the CPU, one process) -- no device work; the pixels it returns still have to be
              uploaded, which is not counted;
  view jobs   ``mm_utils.process_images_device`` from HOST uint8 pixels: the H2D copy of the raw image, one table upload and two
              launches (``slime_view_jobs``);
  composed    the same result from the primitives that existed before the view jobs, from the same host pixels: a torch fill and paste
              of the padded field, ``ops.resize_bicubic_u8``, ``ops.tile_normalize`` per view.  BICUBIC modes only (there is no
              LANCZOS single-size resize), so 'pad_then_devide' has no composed leg.

Per mode, image size (640 x 480, 1920 x 1080) and batch (1, 8): the three results are compared first (they must be equal), the legs
are warmed up, then alternated ROUNDS times in one process; per step a host clock around the call ending in a device synchronise
(wall time: what the caller waits for).  Per leg the median step and the spread of the per-round medians.  The host leg takes fewer
steps: it is two to three orders of magnitude slower.

    python tools/view_slicer_ab.py [--steps 30] [--host-steps 3] [--rounds 3] [--warmup 5] [--out FILE]
                                                                                   (default: profiles/view_slicer_ab.txt)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from PIL import Image

SIZES = [(640, 480), (1920, 1080)]
BATCHES = [1, 8]
MODES = ["pad", "pad_then_devide", "any_res", None]


def peak_clock_mhz():
    """The device's peak engine clock (hipDeviceGetAttribute, hipDeviceAttributeClockRate = 5, in kHz): torch's device properties do
    not carry it on ROCm."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        v = ctypes.c_int(0)
        if hip.hipDeviceGetAttribute(ctypes.byref(v), 5, 0) == 0 and v.value > 0:
            return v.value / 1e3
    except OSError:
        pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "view_slicer_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.host_steps >= 1 and a.rounds >= 3, "at least 20 timed device steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, mm_utils as M, ops
    from slime_amd.image_processor import ClipImageProcessor
    dev = torch.device("cuda:0")
    proc = ClipImageProcessor()
    crop = proc.crop_size["height"]
    bg = tuple(int(x * 255) for x in proc.image_mean)
    bg_t = torch.tensor(bg, dtype=torch.uint8, device=dev)

    def composed(mode, pixels):
        views = []
        for px in pixels:
            img = px.to(dev, non_blocking=True)
            for spec in M.view_jobs_for(mode, (img.shape[1], img.shape[0]), crop, bg):
                x0, y0, w, h = spec.box
                field = img[y0:y0 + h, x0:x0 + w]
                if spec.field != (w, h):
                    padded = bg_t.expand(spec.field[1], spec.field[0], 3).contiguous()
                    padded[spec.paste[1]:spec.paste[1] + h, spec.paste[0]:spec.paste[0] + w] = field
                    field = padded
                big = ops.resize_bicubic_u8(field, *spec.out)
                wx, wy = spec.windows[:2]
                views.append(ops.tile_normalize(big[wy:wy + crop, wx:wx + crop].contiguous(), crop, proc.image_mean, proc.image_std, torch.float32))
        return torch.cat(views)

    props = torch.cuda.get_device_properties(0)
    clock = peak_clock_mhz()
    lines = [f"view slicer A/B: process_images modes {MODES} at {SIZES}, batch {BATCHES}, fp32 output, random RGB images",
             f"device {torch.cuda.get_device_name(0)}, {props.multi_processor_count} CUs, peak clock {f'{clock:.0f} MHz' if clock else 'not reported'}; "
             f"host: {os.cpu_count()} logical CPUs, torch threads {torch.get_num_threads()}; csrc {_lib.csrc_digest()}",
             f"{a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per device leg ({a.host_steps} per round for the host leg), host clock to "
             "synchronise (wall) per step, legs alternated in one process; device legs start from HOST uint8 pixels (H2D included)",
             f"{'mode':16s} {'size':>10s} {'batch':>5s} {'leg':10s} {'median ms':>10s} {'round medians (min .. max)':>30s} {'vs host':>9s} {'vs composed':>12s}"]
    for mode in MODES:
        cfg = SimpleNamespace(image_aspect_ratio=mode)
        for (w, h) in SIZES:
            for batch in BATCHES:
                arrs = [np.random.default_rng(1000 + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i in range(batch)]
                pils = [Image.fromarray(x, "RGB") for x in arrs]
                pixels = [torch.from_numpy(x).pin_memory() for x in arrs]
                legs = {"host": lambda: M.process_images(pils, proc, cfg),
                        "view jobs": lambda: M.process_images_device(pixels, proc, cfg, dev)}
                if mode != "pad_then_devide":
                    legs["composed"] = lambda: composed(mode, pixels)
                ref = legs["host"]()
                ref = torch.cat(list(ref)) if mode in ("any_res", "pad_then_devide") else ref
                for k in list(legs)[1:]:
                    got = legs[k]()
                    got = torch.cat(list(got)) if (k == "view jobs" and mode in ("any_res", "pad_then_devide")) else got
                    assert torch.equal(got.cpu().reshape(ref.shape), ref), (mode, (w, h), batch, k)
                for k in list(legs)[1:]:
                    for _ in range(a.warmup):
                        legs[k]()
                torch.cuda.synchronize()
                wall = {k: [[] for _ in range(a.rounds)] for k in legs}
                for r in range(a.rounds):
                    for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                        for _ in range(a.host_steps if k == "host" else a.steps):
                            t0 = time.perf_counter()
                            legs[k]()
                            torch.cuda.synchronize()
                            wall[k][r].append((time.perf_counter() - t0) * 1e3)
                med = {k: statistics.median([v for x in wall[k] for v in x]) for k in legs}
                for k in legs:
                    rm = [statistics.median(x) for x in wall[k]]
                    vs_host = f"{med['host'] / med[k]:8.1f}x"
                    vs_comp = f"{med['composed'] / med[k]:11.2f}x" if "composed" in legs else f"{'-':>12s}"
                    lines.append(f"{str(mode):16s} {f'{w}x{h}':>10s} {batch:5d} {k:10s} {med[k]:10.4f} {min(rm):14.4f} .. {max(rm):<12.4f} {vs_host} {vs_comp}")
                print("\n".join(lines[-len(legs):]), flush=True)
    lines.append("'vs host' / 'vs composed': that leg's median over this leg's (above 1: this leg is faster).  Results equal across the legs "
                 "on every row (checked before timing).")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
