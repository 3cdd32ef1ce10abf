#!/usr/bin/env python
"""Writes tests/golden/merge_unsampled.npz: what the REFERENCE computes for the LLaVA-NeXT merge of un-sampled crops
(mm_patch_merge_type 'spatial' / 'spatial_unpad', llava/model/llava_arch.py:122-150 and :274-459).  Runs only where the reference is
present; the file holds data only (integers), no program text.

 (a) ``unpad_*``: the window the reference's ``unpad_image`` keeps, for a sweep of (w, h) over every canvas the uhd slicing rule can
     produce at 24 patches per crop side: ``unpad_canvas`` [n, 2] (cur_h, cur_w), ``unpad_size`` [n, 2] (w, h), ``unpad_window``
     [n, 4] (r0, r1, c0, c1) -- read off an index-coded raster that went through the function.
 (b) ``<case>_*``: the reference's unmodified ``prepare_inputs_labels_for_multimodal`` over a stub model whose ``encode_images``,
     embedding table and ``image_newline`` are position-coded (channel 0: flat crop index of the batch / token id, channel 1: patch
     index, channel 2: marker -- 1 image feature, 2 embedding row, 3 image_newline; a zero row is all zeros).  Per case the inputs and
     the outputs; ``new_input_embeds`` is stored as one integer per row (``marker << 40 | channel0 << 20 | channel1``), differenced
     along the flattened rows (``<case>_codes_delta``: its cumulative sum restores the codes), which compresses to almost nothing.

    python tools/make_golden_merge_unsampled.py [--out tests/golden/merge_unsampled.npz]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn as nn

SIDE, P, CROP = 24, 576, 336
VOCAB = 64
PINPOINTS = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"
M_FEATURE, M_TABLE, M_NEWLINE = 1, 2, 3

# the batch of the GPU tests: 5 + 1 + 7 + 4 = 17 crops; the one-crop image's size is never read
SIZES = [(640, 480), (300, 300), (900, 700), (1000, 333)]
SPLITS = [5, 1, 7, 4]
# with images_mask: padded crops in between, the mask marks exactly the grid's crops (7 + 1 + 7 + 6 = 21 crops)
MASKS = [[1, 1, 1, 0, 1, 1, 0], [1], [1, 1, 1, 1, 1, 1, 1], [1, 0, 1, 1, 0, 1]]
# further sizes of the length table, one image per case
SINGLES = [(480, 640), (700, 300), (336, 336), (500, 500)]


def uhd_canvases():
    """(cur_h, cur_w) in patches of every slice layout the uhd rule chooses from: the factor pairs of 2 .. 7 slices."""
    out = []
    for n in range(2, 8):
        for ws in range(1, n + 1):
            if n % ws == 0:
                out.append(((n // ws) * SIDE, ws * SIDE))
    return out


def unpad_sweep(A):
    canv, size, win = [], [], []
    dims = list(range(100, 2100, 131)) + [333, 336, 480, 500, 640, 672, 700, 900, 1000, 1008]
    for cur_h, cur_w in uhd_canvases():
        coded = torch.arange(cur_h * cur_w).view(1, cur_h, cur_w)
        for w in dims:
            for h in dims:
                kept = A.unpad_image(coded, (w, h))
                assert kept.numel() > 0, (cur_h, cur_w, w, h)
                r0, c0 = divmod(int(kept[0, 0, 0]), cur_w)
                canv.append((cur_h, cur_w))
                size.append((w, h))
                win.append((r0, r0 + kept.shape[1], c0, c0 + kept.shape[2]))
    return np.array(canv, dtype=np.int16), np.array(size, dtype=np.int16), np.array(win, dtype=np.int16)


def stub_model(A, merge_type, side, max_length):
    """The reference's LlavaMetaForCausalLM over position-coded parts; only ``encode_images`` is replaced (by the coded features)."""
    table = torch.zeros(VOCAB, 3)
    table[:, 0] = torch.arange(VOCAB)
    table[:, 2] = M_TABLE
    embed = nn.Embedding(VOCAB, 3)
    with torch.no_grad():
        embed.weight.copy_(table)
    tower = SimpleNamespace(num_patches_per_side=SIDE, num_patches=P, config=SimpleNamespace(image_size=CROP))
    model = SimpleNamespace(embed_tokens=embed, image_newline=torch.tensor([0.0, 0.0, float(M_NEWLINE)]), has_sampler=False,
                            get_vision_tower=lambda: tower)
    cfg = SimpleNamespace(mm_patch_merge_type=merge_type, image_aspect_ratio="anyres", image_grid_pinpoints=PINPOINTS,
                          tokenizer_padding_side=side, tokenizer_model_max_length=max_length)

    class Stub(A.LlavaMetaForCausalLM):
        def __init__(self):
            self.model, self.config, self.device = model, cfg, torch.device("cpu")

        def get_model(self):
            return self.model

        def encode_images(self, images, input_ids=None, split_sizes=None, attention_mask=None, images_mask=None, image_sizes=None,
                          labels=None):
            n = images.shape[0]
            f = torch.zeros(n, P, 3)
            f[:, :, 0] = torch.arange(n, dtype=torch.float32)[:, None]
            f[:, :, 1] = torch.arange(P, dtype=torch.float32)[None, :]
            f[:, :, 2] = M_FEATURE
            return list(torch.split(f, split_sizes, dim=0)), split_sizes

    return Stub()


def pack_codes(emb):
    e = emb.round().to(torch.int64)
    assert torch.equal(e.float(), emb), "the codes are integers"
    return ((e[..., 2] << 40) | (e[..., 0] << 20) | e[..., 1]).numpy()


def text_batch(n_seq, where, seed, length=12):
    """ids [n_seq, length] with the image tokens at ``where[b]`` (a list per sequence), a mask with padding, labels."""
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, VOCAB, size=(n_seq, length)).astype(np.int64)
    am = np.ones_like(ids)
    for b, cols in enumerate(where):
        for c in cols:
            ids[b, c] = IMAGE_TOKEN_INDEX
    am[0, -2:] = 0                                       # right padding behind the last image token of sequence 0
    if n_seq > 2:
        am[2, :1] = 0                                    # a masked token in front of sequence 2
    lab = np.where(ids == IMAGE_TOKEN_INDEX, -100, ids + 1000)
    return ids, am, lab


def run_case(A, out, name, merge_type, side, max_length, splits, sizes, masks, ids, am, lab):
    m = stub_model(A, merge_type, side, max_length)
    images = [torch.zeros(s, 3, 2, 2) for s in splits]              # the stub reads only the crop counts
    imask = None if masks is None else [torch.tensor(x) for x in masks]
    pos = torch.arange(ids.shape[1]).expand(ids.shape[0], -1).contiguous()
    r = m.prepare_inputs_labels_for_multimodal(torch.from_numpy(ids), pos, torch.from_numpy(am), None, torch.from_numpy(lab), images,
                                               image_sizes=sizes, images_mask=imask)
    none_ids, new_pos, new_mask, _, emb, new_lab = r
    assert none_ids is None
    codes = pack_codes(emb.detach())
    meta = dict(merge_type=merge_type, side=side, max_length=max_length, splits=list(splits), sizes=[list(x) for x in sizes], masks=masks,
                ids=ids.tolist(), am=am.tolist(), lab=lab.tolist(), shape=list(codes.shape))
    out[name + "_meta"] = np.array(json.dumps(meta))
    out[name + "_codes_delta"] = np.diff(codes.reshape(-1), prepend=np.int64(0))
    out[name + "_new_lab_delta"] = np.diff(new_lab.numpy().reshape(-1), prepend=np.int64(0))
    out[name + "_new_mask"] = np.packbits(new_mask.numpy().astype(np.uint8).reshape(-1))
    out[name + "_new_pos_delta"] = np.diff(new_pos.numpy().reshape(-1), prepend=np.int64(0))
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "merge_unsampled.npz"))
    a = ap.parse_args()
    from oracle.make_golden import import_reference, REF
    assert os.path.isdir(os.path.join(REF, "llava")), "the reference is not present here"
    import_reference()
    import llava.model.llava_arch as A
    out = {}
    out["unpad_canvas"], out["unpad_size"], out["unpad_window"] = unpad_sweep(A)
    names = []
    ids4, am4, lab4 = text_batch(4, [[3], [5], [4], [9]], seed=1)
    for merge_type in ("spatial", "spatial_unpad"):
        for tag, side, max_length, masked in (("right", "right", None, False), ("mask", "right", None, True), ("left", "left", None, False),
                                              ("left_mask", "left", None, True), ("cut", "right", 400, False), ("cut_left", "left", 400, False)):
            splits = [len(x) for x in MASKS] if masked else SPLITS
            names.append(run_case(A, out, f"{merge_type}_{tag}", merge_type, side, max_length, splits, SIZES, MASKS if masked else None,
                                  ids4, am4, lab4))
        # two image tokens in one sequence, a sequence without one (it still consumes an image: llava_arch.py:369-376)
        ids3, am3, lab3 = text_batch(3, [[2, 7], [4], []], seed=2)
        names.append(run_case(A, out, f"{merge_type}_two_tokens", merge_type, "right", None, SPLITS, SIZES, None, ids3, am3, lab3))
        for k, size in enumerate(SINGLES):                           # the other sizes of the length table, one image each
            ids1, am1, lab1 = text_batch(1, [[1]], seed=10 + k, length=4)
            nw, nh = A.get_anyres_image_grid_shape(size, PINPOINTS, CROP)
            names.append(run_case(A, out, f"{merge_type}_single{k}", merge_type, "right", None, [1 + nw * nh], [size], None, ids1, am1, lab1))
    out["cases"] = np.array(names)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(names)} cases, {out['unpad_window'].shape[0]} unpad windows")


if __name__ == "__main__":
    main()
