#!/usr/bin/env python
"""A/B of the two programs ``prepare_inputs_labels_for_multimodal`` has between the router and the LLM's input embeddings:
``fused_splice=False`` (per image index_select + cat + cast, one cat of all feature rows, ``slime_splice_rows``; the text embeddings for
the router by per-sequence lookups and cats) against ``fused_splice=True`` (``slime_splice_routed``: one launch from the router's device
arrays; the text embeddings from ``pure_text_plan`` and one launch).

SliME-8B dims, synthetic weights, bf16 images and a bf16 128256 x 4096 embedding table, 8 images with the local-crop grids of
tools/ragged_adapter_ab.py (30 local + 8 global = 38 crops), one 64-token prompt per image.  One process; first the outputs of the two
programs are compared bit for bit on the same input; then the legs are alternated ROUNDS times after a warm-up of every leg, HIP
events around every step; per leg the median step and the spread of the per-round medians.  A third leg, ``encode_visual`` (tower +
fused adapter, no router, no glue), gives the share of everything behind the adapter by subtraction.

    python tools/routed_splice_ab.py [--steps 20] [--rounds 4] [--warmup 5] [--out FILE]   (default: profiles/routed_splice_ab.txt)
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ragged_adapter_ab import GRIDS, SIZES

PROMPT, VOCAB = 64, 128256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "routed_splice_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, mm_utils as M, weights as W
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = default_slime_config("synthetic:1234")
    assert [tuple(M.get_anyres_image_grid_shape(s, cfg.image_grid_pinpoints, 336)) for s in SIZES] == GRIDS
    embed = torch.nn.Embedding(VOCAB, cfg.hidden_size, device=dev, dtype=dt)
    with torch.no_grad():
        embed.weight.copy_(torch.randn(VOCAB, cfg.hidden_size, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) * 0.02)
    enc = SlimeVisualEncoder(cfg, embed_tokens=embed)
    enc.load_visual_state(W.make_tower_state_dict(W.CLIP_L_336, seed=1234), W.make_adapter_state_dict(W.ADAPTER_8B, seed=4321))
    enc.to(dev)
    enc.get_vision_tower().vision_tower.to(dt)
    counts = [1 + nw * nh for nw, nh in GRIDS]
    pixels = W.synthetic_pixels(sum(counts), seed=77).to(dev).to(dt)
    images = list(torch.split(pixels, counts, dim=0))
    n = len(GRIDS)
    ids = torch.randint(3, VOCAB, (n, PROMPT), generator=torch.Generator().manual_seed(4))
    ids[:, 5] = IMAGE_TOKEN_INDEX
    am = torch.ones_like(ids)
    am[::2, -6:] = 0                                                  # right padding of different lengths
    ids, am = ids.to(dev), am.to(dev)
    lab, pos = ids.clone(), torch.arange(PROMPT, device=dev).expand(n, PROMPT).contiguous()

    def step(fused):
        cfg.fused_splice = fused
        return enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, images, image_sizes=SIZES)

    legs = {
        "fused_splice=False": lambda: step(False),
        "fused_splice=True": lambda: step(True),
        "encode_visual": lambda: enc.encode_visual(pixels, counts, SIZES, merge="spatial"),
    }
    lines = [f"routed splice A/B: {n} images, grids {GRIDS}, {sum(counts)} crops, {PROMPT}-token prompts, bf16 images, bf16 table "
             f"{VOCAB} x {cfg.hidden_size}, SliME-8B dims, synthetic weights",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             "HIP events per step, legs alternated in one process"]
    off, on = step(False), step(True)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in ((off[i], on[i]) for i in (1, 2, 4, 5)))
    same = same and torch.equal(off[4].view(torch.int16), on[4].view(torch.int16))
    lines.append(f"outputs, fused_splice=True vs False (embeds {tuple(on[4].shape)} {on[4].dtype}, labels, mask, position ids): "
                 f"{'bit-identical' if same else 'DIFFERENT'}")
    assert same, "the two programs differ"
    del off, on
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
    med, spread = {}, {}
    lines.append(f"{'leg':28s} {'median ms':>10s} {'round medians (min .. max)':>30s} {'spread':>8s}")
    for k, rounds in times.items():
        rm = [statistics.median(x) for x in rounds]
        med[k] = statistics.median([t for x in rounds for t in x])
        spread[k] = max(rm) - min(rm)
        lines.append(f"{k:28s} {med[k]:10.3f} {min(rm):14.3f} .. {max(rm):<12.3f} {spread[k]:8.3f}")
    g_off, g_on = med["fused_splice=False"] - med["encode_visual"], med["fused_splice=True"] - med["encode_visual"]
    lines.append(f"behind the adapter (step - encode_visual: text embeddings, router, glue, splice): off {g_off:.3f} ms, on {g_on:.3f} ms")
    diff = med["fused_splice=False"] - med["fused_splice=True"]
    noise = max(spread["fused_splice=False"], spread["fused_splice=True"])
    verdict = "a gain" if diff > noise else "a loss" if -diff > noise else "inside the spread of the round medians: no difference shown"
    lines.append(f"step: off - on = {diff:.3f} ms (on / off = {med['fused_splice=True'] / med['fused_splice=False']:.4f}); "
                 f"largest spread of the two legs {noise:.3f} ms -> {verdict}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
