#!/usr/bin/env python
"""A/B of the two programs behind the projector of a LLaVA-NeXT style model (no sampler, ``mm_patch_merge_type='spatial_unpad'``):

  leg A  ``prepare_inputs_labels_for_multimodal`` as shipped: the merge is a host plan, ``slime_splice_merged`` moves every row from the
         projector's fp32 output into the padded embedding tensor in one launch;
  leg B  the materialising program, written here from existing pieces: ``encode_images`` (cast to the images' dtype, split per image),
         a per-image torch merge (view / permute / unpad slice / cat of the zero column and of the base crop), ``torch.cat`` of all
         images, ``splice_plan`` + ``slime_splice_rows``.

LLaVA-NeXT dims: CLIP-L/336, mlp2x_gelu 1024 -> 4096, synthetic weights, bf16 images, a bf16 128256 x 4096 embedding table, the 8 image
sizes of tools/ragged_adapter_ab.py (30 local + 8 global = 38 crops), one 64-token prompt per image.  One process; first the two
outputs are compared bit for bit; then the legs are alternated ROUNDS times after a warm-up of both, HIP events around every step; per
leg the median step and the spread of the per-round medians.

    python tools/merged_splice_ab.py [--steps 20] [--rounds 4] [--warmup 5] [--out FILE]   (default: profiles/merged_splice_ab.txt)
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "merged_splice_ab.txt"))
    a = ap.parse_args()
    assert a.steps >= 20 and a.rounds >= 3, "at least 20 timed steps per leg and 3 alternations"
    assert torch.cuda.is_available(), "this measurement needs the GPU (no fallback)"
    from slime_amd import _lib, mm_utils as M, ops, weights as W
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config, splice_plan, unpad_window
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    cfg = default_slime_config("synthetic:1234", mm_resampler_type=None, mm_projector_type="mlp2x_gelu", mm_patch_merge_type="spatial_unpad")
    assert [tuple(M.get_anyres_image_grid_shape(s, cfg.image_grid_pinpoints, 336)) for s in SIZES] == GRIDS
    embed = torch.nn.Embedding(VOCAB, cfg.hidden_size, device=dev, dtype=dt)
    with torch.no_grad():
        embed.weight.copy_(torch.randn(VOCAB, cfg.hidden_size, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) * 0.02)
    enc = SlimeVisualEncoder(cfg, embed_tokens=embed)
    enc.load_visual_state(W.make_tower_state_dict(W.CLIP_L_336, seed=1234), None)
    asd = W.sub_state(W.make_adapter_state_dict(W.ADAPTER_8B, seed=4321), "mm_projector.")
    enc.get_model().mm_projector.load_state_dict({k[len("projection."):]: v for k, v in asd.items() if k.startswith("projection.")})
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
    table = embed.weight.detach()
    side = enc.get_vision_tower().num_patches_per_side

    def merged():
        return enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, images, image_sizes=SIZES)

    def materialised():
        ids_np, am_np, lab_np = ids.cpu().numpy(), am.cpu().numpy(), lab.cpu().numpy()     # as leg A: ids, mask, labels to the host first
        feats, _ = enc.encode_images(pixels, ids, counts, am, None, SIZES, labels=lab)           # [1 + n_i, 576, H] of the images' dtype
        per_image = []
        for f, size, (nw, nh) in zip(feats, SIZES, GRIDS):
            raster = f[1:].view(nh, nw, side, side, -1).permute(0, 2, 1, 3, 4).reshape(nh * side, nw * side, -1)
            r0, r1, c0, c1 = unpad_window(size, nh * side, nw * side)
            kept = raster[r0:r1, c0:c1]
            kept = torch.cat([kept, torch.zeros_like(kept[:, :1])], dim=1)                         # a zero row ends every raster row
            per_image.append(torch.cat([f[0], kept.reshape(-1, kept.shape[-1])], dim=0))
        src, l2, m2, p2 = splice_plan(ids_np, am_np, lab_np, [f.shape[0] for f in per_image], None, "right", vocab_size=VOCAB)
        B, T = src.shape
        emb = ops.splice_rows(table, torch.cat(per_image, 0), torch.from_numpy(src).reshape(-1).to(dev), table.dtype).view(B, T, -1)
        return None, torch.from_numpy(p2).to(dev), torch.from_numpy(m2).to(dev), None, emb, torch.from_numpy(l2).to(dev)

    legs = {"A merged splice": merged, "B materialising": materialised}
    H = cfg.hidden_size
    rows = sum(counts) * side * side
    lines = [f"merged splice A/B: {n} images, grids {GRIDS}, {sum(counts)} crops, {PROMPT}-token prompts, bf16 images, bf16 table "
             f"{VOCAB} x {H}, CLIP-L/336 + mlp2x_gelu 1024 -> {H}, spatial_unpad, synthetic weights",
             f"device {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}, {a.warmup} warm-up + {a.rounds} rounds x {a.steps} steps per leg, "
             "HIP events per step, legs alternated in one process"]
    ya, yb = merged(), materialised()
    torch.cuda.synchronize()
    same = all(torch.equal(ya[i], yb[i]) for i in (1, 2, 4, 5)) and torch.equal(ya[4].view(torch.int16), yb[4].view(torch.int16))
    lines.append(f"outputs, A vs B (embeds {tuple(ya[4].shape)} {ya[4].dtype}, labels, mask, position ids): "
                 f"{'bit-identical' if same else 'DIFFERENT'}")
    assert same, "the two programs differ"
    kept = int(ya[2].sum()) - int(am.sum()) + n
    lines.append(f"projector rows {rows} x {H}: leg B's cast writes {rows * H * 2 / 1e6:.1f} MB (reads {rows * H * 4 / 1e6:.1f} MB fp32), its merge "
                 f"and cat each move the {kept} merged rows ({kept * H * 2 / 1e6:.1f} MB) once more; leg A reads the fp32 rows it keeps once")
    del ya, yb
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
    ka, kb = legs.keys()
    diff, noise = med[kb] - med[ka], max(spread.values())
    verdict = "a gain" if diff > noise else "a loss" if -diff > noise else "inside the spread of the round medians: no difference shown"
    lines.append(f"step: B - A = {diff:.3f} ms (A / B = {med[ka] / med[kb]:.4f}); largest spread of the two legs {noise:.3f} ms -> {verdict}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
