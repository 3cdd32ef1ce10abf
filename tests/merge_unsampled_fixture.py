"""Shared by the host and GPU tests of the un-sampled LLaVA-NeXT merge: tests/golden/merge_unsampled.npz (written by
tools/make_golden_merge_unsampled.py from the reference) and the position codes its ``new_input_embeds`` are recorded in.

A code is one integer per output row, ``marker << 40 | a << 20 | b``: marker 1 an image feature (a: flat crop index of the batch,
b: patch index), 2 an embedding row (a: token id), 3 ``image_newline``, 0 a zero row."""
import json
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_unsampled.npz")
SIDE, P = 24, 576
M_FEATURE, M_TABLE, M_NEWLINE = 1, 2, 3

_cache = {}


def load():
    if "g" not in _cache:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def case_names():
    return [str(n) for n in load()["cases"]]


def case(name):
    """One recorded call of the reference's prepare_inputs_labels_for_multimodal: its inputs and its four outputs as int64 arrays."""
    g = load()
    meta = json.loads(str(g[name + "_meta"]))
    B, T = meta["shape"]
    new_mask = np.unpackbits(g[name + "_new_mask"])[:B * T].reshape(B, T).astype(np.int64)
    return SimpleNamespace(name=name, merge_type=meta["merge_type"], side=meta["side"], max_length=meta["max_length"],
                           splits=meta["splits"], sizes=[tuple(s) for s in meta["sizes"]], masks=meta["masks"],
                           ids=np.array(meta["ids"], dtype=np.int64), am=np.array(meta["am"], dtype=np.int64),
                           lab=np.array(meta["lab"], dtype=np.int64),
                           codes=np.cumsum(g[name + "_codes_delta"]).reshape(B, T),
                           new_lab=np.cumsum(g[name + "_new_lab_delta"]).reshape(B, T),
                           new_pos=np.cumsum(g[name + "_new_pos_delta"]).reshape(B, T), new_mask=new_mask)


def decode_src(src, token_rows):
    """The kernel's rule for a ``src`` of ``ops.splice_merged`` (include/slime_hip.h), as position codes; the one extra row is
    ``image_newline``.  A source outside its tensor decodes to -1, which no recorded code equals."""
    src = np.asarray(src, dtype=np.int64)
    k = -2 - src
    out = np.full(src.shape, -1, dtype=np.int64)
    out[src == -1] = 0
    t = src >= 0
    out[t] = (M_TABLE << 40) | (src[t] << 20)
    f = (src <= -2) & (k < token_rows)
    out[f] = (M_FEATURE << 40) | ((k[f] // P) << 20) | (k[f] % P)
    out[(src <= -2) & (k == token_rows)] = M_NEWLINE << 40
    return out


def plan_src(c, cfg, tower, has_newline=True):
    """The composed plan of this repository for a recorded case: (src, labels, mask, position ids, plan lengths, token rows)."""
    from slime_amd.model.llava_arch import merged_src, splice_plan, unsampled_merge_plans
    cfg.mm_patch_merge_type = c.merge_type
    plans = unsampled_merge_plans(c.splits, c.sizes, c.masks, cfg, tower, has_newline)
    lens = [int(p.shape[0]) for p in plans]
    src, lab, mask, pos = splice_plan(c.ids, c.am, c.lab, lens, c.max_length, c.side)
    token_rows = sum(c.splits) * P
    return merged_src(src, plans, token_rows), lab, mask, pos, lens, token_rows


def stand_in_tower(select_feature="patch"):
    return SimpleNamespace(num_patches_per_side=SIDE, num_patches=P, select_feature=select_feature, config=SimpleNamespace(image_size=336))
