"""Multimodal glue for the visual hot path: the build's counterpart of ``LlavaMetaModel`` /
``LlavaMetaForCausalLM.encode_images`` (llava/model/llava_arch.py:28-44,212-269).

Same plugin construction (three builders driven by the same config attribute names), same stage
order and outputs as the reference's ``encode_images`` sampler branch:

    tower(all crops) -> global = mm_projector(crop 0) ; local = mm_projector(post_qformer(crops 1..n))
    -> drop masked crops -> merge ('spatial' raster / 'flat') -> text-guided router -> cat(global, sep, local)

but scheduled for the GPU instead of per image: the reference loops over images in Python and calls the
ViT once per image (llava_arch.py:222); here ALL crops of the batch go through the tower as one batch,
all global views through one GatedBlock launch sequence and all local crops through one
post_qformer + MLP sequence; only the tiny data-dependent tail (merge, router, concat) is per image.
When every image of the batch has the same crop layout (the usual case: one resolution bucket per batch) the
whole adapter -- both experts of the GatedBlock, post_qformer, the shared projection MLP over the stacked rows,
gate mix and spatial merge -- is ONE C-ABI call (``slime_adapter_forward``) on the tower's 16-bit features, as
in the reference, which hands fp16/bf16 features to its adapter.  A batch whose images have different crop counts or
grids (the usual anyres batch) takes the same sequence through ``slime_adapter_forward_ragged``: one flat token buffer,
every image at its own row offset, the router on that buffer directly.  What stays on the per-module sequence, where the
tower hands over fp32 features: ``images_mask``, ``use_local_only`` / ``use_global_only``, non-gated projectors,
``fused_adapter=False`` and more than 64 images in one call.

``SlimeMetaForCausalLM`` can be mixed into an HF causal LM exactly like ``LlavaMetaForCausalLM``
(INTEGRATION.md); ``SlimeVisualEncoder`` is the standalone form used by bench.py and the tests.
"""
from __future__ import annotations

import functools
from abc import ABC, abstractmethod
from typing import Optional, Sequence

import torch
import torch.nn as nn

from .multimodal_encoder.builder import build_vision_tower
from .multimodal_projector.builder import build_vision_projector, GatedBlock, HipMlp, _operand_dtype
from .multimodal_resampler.builder import build_vision_sampler
from .. import ops
from ..constants import IMAGE_TOKEN_INDEX, IGNORE_INDEX
from ..mm_utils import get_anyres_image_grid_shape


def _split_indices(split_sizes, device):
    """Row indices of the global views (crop 0 of every image) and of the local crops in the flat crop
    batch (host-side index math, no device sync)."""
    g, l, off = [], [], 0
    for s in split_sizes:
        g.append(off)
        l.extend(range(off + 1, off + s))
        off += s
    return (torch.tensor(g, dtype=torch.long, device=device), torch.tensor(l, dtype=torch.long, device=device))


def _uniform_layout(split_sizes, image_sizes, cfg, crop: int, merge_type: str):
    """(n_local, nw, nh, merge) when all images share one crop count and one grid, else None."""
    if not split_sizes or any(s != split_sizes[0] for s in split_sizes):
        return None
    n_local = split_sizes[0] - 1
    if n_local == 0:
        return (0, 1, 1, False)
    if merge_type == "flat":
        return (n_local, n_local, 1, False)
    if merge_type != "spatial" or image_sizes is None:
        return None
    grids = {tuple(get_anyres_image_grid_shape(sz, cfg.image_grid_pinpoints, crop)) for sz in image_sizes}
    if len(grids) != 1:
        return None
    nw, nh = next(iter(grids))
    return (n_local, nw, nh, True) if nw * nh == n_local else None


def _ragged_layout(split_sizes, image_sizes, cfg, crop: int, merge_type: str):
    """Per-image crop grids ``[(nw_i, nh_i)]`` for the ragged fused adapter (``(0, 0)``: an image without local crops; 'flat':
    ``(n_i, 1)``), or None when it cannot take the batch: 'spatial' without image sizes, a grid that does not match its image's
    crop count, another merge type, or more images than the call's layout holds."""
    if not split_sizes or len(split_sizes) > ops.RAGGED_MAX_IMAGES or any(s < 1 for s in split_sizes):
        return None
    if merge_type == "flat":
        return [(s - 1, 1) if s > 1 else (0, 0) for s in split_sizes]
    if merge_type != "spatial" or image_sizes is None or len(image_sizes) != len(split_sizes):
        return None
    grids = []
    for s, sz in zip(split_sizes, image_sizes):
        if s == 1:
            grids.append((0, 0))
            continue
        nw, nh = get_anyres_image_grid_shape(sz, cfg.image_grid_pinpoints, crop)
        if nw * nh != s - 1:
            return None
        grids.append((int(nw), int(nh)))
    return grids


def _project_local(projector, comp: torch.Tensor, operand_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``mm_projector`` on the compressed local crops [sum n_i, g*g, D] of a whole batch.  The reference calls the projector
    per image (n_i <= 7 crops), where GatedBlock.forward's test ``x.shape[0] != 576 and x.shape[1] != 576``
    (projector/builder.py:180-181) always takes the plain-MLP return; on the batch-stacked tensor dim 0 is sum n_i and may
    equal 576 by accident, so the MLP is called directly instead of through that shape test."""
    kw = {"operand_dtype": operand_dtype} if operand_dtype is not None else {}
    if isinstance(projector, GatedBlock):
        return projector.projection(comp, out_dtype=torch.float32, **kw)
    if isinstance(projector, HipMlp):
        return projector(comp, out_dtype=torch.float32, **kw)
    return projector(comp, out_dtype=torch.float32)


def _adapter_operand_dtype(model, images: torch.Tensor) -> dict:
    """``{"operand_dtype": T}`` for the adapter modules that take the extension (GatedBlock, HipMlp, Resampler) when the call's
    images are 16-bit: the reference's tower returns features in the input dtype and its adapter computes in it."""
    if images.dtype not in (torch.bfloat16, torch.float16):
        return {}
    from .multimodal_resampler.sampler import Resampler
    from .multimodal_projector.builder import HipLinear
    return {"operand_dtype": images.dtype} if isinstance(model.mm_projector, (GatedBlock, HipMlp, HipLinear, Resampler)) else {}


def _router_operand_dtype(model, images: torch.Tensor) -> dict:
    """``{"operand_dtype": T}`` for the attention router (mm_resampler_type='qformer') when the call's images are 16-bit, as
    ``_adapter_operand_dtype`` does for the adapter; the cosine router computes in fp32 and takes no such argument."""
    if getattr(model.sampler, "router_type", None) != "qformer" or images.dtype not in (torch.bfloat16, torch.float16):
        return {}
    return {"operand_dtype": images.dtype}


def _require_inference(model) -> None:
    """The HIP path has no backward.  The reference's pretrain / finetune stages train mm_projector and sampler through
    this code (train.py:1100-1130); silently detaching them under @torch.no_grad would freeze the adapter without a
    message, so training-mode use is an error here ("inference only")."""
    if not torch.is_grad_enabled():
        return
    for name in ("mm_projector", "sampler"):
        mod = getattr(model, name, None)
        if mod is not None and any(p.requires_grad and p.is_floating_point() for p in mod.parameters()) and mod.training:
            raise RuntimeError(
                f"slime_amd is inference-only: {name} has trainable parameters and autograd is enabled, but the HIP adapter "
                "has no backward.  Call .eval() / .requires_grad_(False), or run under torch.no_grad().")


def _fused_adapter(model, images: torch.Tensor, layout, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None):
    """tower -> slime_adapter_forward for a uniform batch: tokens [B, 576 + n*g*g, H]."""
    n_local, nw, nh, merge = layout
    tower = model.get_vision_tower()
    T = _operand_dtype(images, model.mm_projector.projection[0].weight)
    feats = tower(images, out_dtype=T)
    B = feats.shape[0] // (1 + n_local)
    post = model.sampler.post_qformer.packed(feats.shape[1], T) if n_local else None
    return ops.adapter_forward(model.mm_projector.packed(T), post, feats, B, n_local, nw, nh, merge,
                               int(model.mm_projector.learnable_gated), out_dtype, out)


def _fused_adapter_ragged(model, images: torch.Tensor, grids, merge: bool, out_dtype: torch.dtype):
    """tower -> slime_adapter_forward_ragged: (flat tokens [sum_i (576 + n_i*g*g), H], first row of every image)."""
    tower = model.get_vision_tower()
    T = _operand_dtype(images, model.mm_projector.projection[0].weight)
    feats = tower(images, out_dtype=T)
    post = model.sampler.post_qformer.packed(feats.shape[1], T) if feats.shape[0] > len(grids) else None
    return ops.adapter_forward_ragged(model.mm_projector.packed(T), post, feats, grids, merge,
                                      int(model.mm_projector.learnable_gated), out_dtype)


def _check_token_ids(t, vocab_size):
    """nn.Embedding raises IndexError for an id outside [0, vocab); the splice would instead read id -1 as padding and an id
    <= -2 as an image-feature row.  IMAGE_TOKEN_INDEX is the one legal negative id."""
    import numpy as np
    bad = (t != IMAGE_TOKEN_INDEX) & ((t < 0) | (t >= vocab_size))
    if bad.any():
        raise IndexError(f"input_ids contain token id {int(t[np.argmax(bad)])} outside [0, {vocab_size}) (index out of range in self)")


def splice_plan(input_ids, attention_mask, labels, feat_lens, max_length=None, padding_side: str = "right", vocab_size=None):
    """Index plan of ``prepare_inputs_labels_for_multimodal`` (llava_arch.py:362-459), integer host logic on numpy arrays.
    ``input_ids`` [B, L] int64 (IMAGE_TOKEN_INDEX marks an image), ``attention_mask`` [B, L] or None, ``labels`` [B, L] or
    None, ``feat_lens[j]`` = token rows of image feature j (consumed in order of appearance; a sequence without an image
    token still consumes one feature, of which it uses zero rows: :377-385).
    Returns int64 arrays [B, max_len]: ``src`` (>= 0 token id, -2 - k row k of the concatenated features, -1 padding),
    ``labels`` (IGNORE_INDEX on image and padding rows), ``mask``, ``position_ids``.
    ``vocab_size``: validate the ids that survive the mask (the only ones the reference embeds, :361-373) as nn.Embedding would."""
    import numpy as np
    ids = np.asarray(input_ids, dtype=np.int64)
    B = ids.shape[0]
    am = np.ones_like(ids, dtype=bool) if attention_mask is None else np.asarray(attention_mask) != 0
    lb = np.full_like(ids, IGNORE_INDEX) if labels is None else np.asarray(labels, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(np.asarray(feat_lens, dtype=np.int64))])
    seqs, labs, img = [], [], 0
    for b in range(B):
        t, y = ids[b][am[b]], lb[b][am[b]]                                  # :366-368 drop padding through the mask
        if vocab_size is not None:
            _check_token_ids(t, vocab_size)
        where = np.nonzero(t == IMAGE_TOKEN_INDEX)[0]
        if where.size == 0:                                                 # :376-385
            if img >= len(feat_lens):
                raise ValueError("fewer image features than sequences / image tokens")
            seqs.append(t); labs.append(y); img += 1
            continue
        if img + where.size > len(feat_lens):
            raise ValueError("fewer image features than image tokens")
        ps, pl, prev = [], [], 0
        for w in where:                                                     # :387-411
            ps.append(t[prev:w]); pl.append(y[prev:w])
            n = int(feat_lens[img])
            ps.append(-2 - (starts[img] + np.arange(n, dtype=np.int64)))
            pl.append(np.full(n, IGNORE_INDEX, dtype=np.int64))
            img += 1
            prev = w + 1
        ps.append(t[prev:]); pl.append(y[prev:])
        seqs.append(np.concatenate(ps)); labs.append(np.concatenate(pl))
    if max_length is not None:                                              # :420-424
        seqs = [q[:max_length] for q in seqs]
        labs = [q[:max_length] for q in labs]
    max_len = max(q.shape[0] for q in seqs)                                 # :427
    src = np.full((B, max_len), -1, dtype=np.int64)
    lab = np.full((B, max_len), IGNORE_INDEX, dtype=np.int64)
    mask = np.zeros((B, max_len), dtype=np.int64)
    pos = np.zeros((B, max_len), dtype=np.int64)
    for b, (q, y) in enumerate(zip(seqs, labs)):                            # :435-455
        n = q.shape[0]
        sl = slice(max_len - n, max_len) if padding_side == "left" else slice(0, n)
        src[b, sl], lab[b, sl], mask[b, sl], pos[b, sl] = q, y, 1, np.arange(n)
    return src, lab, mask, pos


def routed_src(src, feat_lens):
    """``splice_plan``'s ``src`` for ``ops.splice_routed``: every entry ``-2 - k`` (row k of the virtual concatenation of the per-image
    features, ``feat_lens[i]`` rows each) becomes ``-2 - (i << 32 | p)``, image i and row p inside its feature; token ids and -1 stay.
    A zero-row feature owns no k, so it is never named."""
    import numpy as np
    src = np.asarray(src, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(np.asarray(feat_lens, dtype=np.int64))]).astype(np.int64)
    out = src.copy()
    m = src <= -2
    k = -2 - src[m]
    if k.size and int(k.max()) >= int(starts[-1]):
        raise ValueError("splice plan names a feature row past the last image")
    img = np.searchsorted(starts, k, side="right") - 1          # the LAST image that starts at or before k: skips zero-row features
    out[m] = -2 - ((img.astype(np.int64) << 32) | (k - starts[img]))
    return out


def unpad_window(original_size, cur_h: int, cur_w: int):
    """``(r0, r1, c0, c1)``: the rows and columns of a ``cur_h x cur_w`` raster that the reference's ``unpad_image`` keeps for an image
    of ``original_size = (width, height)`` (llava_arch.py:122-150) -- its arithmetic restated exactly: Python float division and
    ``int()``, ``padding = (cur - new) // 2`` trimmed from both ends, so an odd remainder keeps one row or column more than ``new``."""
    original_width, original_height = (int(v) for v in original_size)
    cur_h, cur_w = int(cur_h), int(cur_w)
    if original_width / original_height > cur_w / cur_h:
        scale_factor = cur_w / original_width
        new_height = int(original_height * scale_factor)
        padding = (cur_h - new_height) // 2
        r0, r1, _ = slice(padding, cur_h - padding).indices(cur_h)
        return r0, max(r0, r1), 0, cur_w
    scale_factor = cur_h / original_height
    new_width = int(original_width * scale_factor)
    padding = (cur_w - new_width) // 2
    c0, c1, _ = slice(padding, cur_w - padding).indices(cur_w)
    return 0, cur_h, c0, max(c0, c1)


MERGE_ZERO, MERGE_NEWLINE = -1, -2          # entries of a merge plan that name no projector row


@functools.lru_cache(maxsize=4096)
def _grid_of(width: int, height: int, pinpoints: str, crop: int):
    """``get_anyres_image_grid_shape`` per (size, pinpoints, crop): the merge plan runs on the host in front of the step's first launch,
    where parsing the pinpoint string once per image is most of its time."""
    nw, nh = get_anyres_image_grid_shape((width, height), pinpoints, crop)
    return int(nw), int(nh)


def unsampled_merge_plans(split_sizes, image_sizes, images_mask, cfg, tower, has_newline: bool):
    """The LLaVA-NeXT merge of un-sampled crops (llava_arch.py:293-333) as integer host logic: per image an int64 array over its
    feature positions, in the reference's order.  Entry ``k >= 0``: flat token row ``crop * P + patch`` of the batch's projector output
    (all crops of all images, P rows each); ``MERGE_ZERO``: a zero row (the reference's ``zeros_like`` column behind every kept raster
    row, :318-319); ``MERGE_NEWLINE``: ``model.image_newline`` (behind a single-crop image, :327-331).  Every refusal is raised here,
    before any device work."""
    import numpy as np
    merge_type = getattr(cfg, "mm_patch_merge_type", "flat")
    unpad = "unpad" in merge_type
    side = int(tower.num_patches_per_side)
    P = side * side
    rows_per_crop = int(tower.num_patches) + (1 if getattr(tower, "select_feature", "patch") == "cls_patch" else 0)
    if rows_per_crop != P:
        raise ValueError(f"mm_patch_merge_type={merge_type!r} needs {side}x{side} = {P} tower rows per crop, the tower returns "
                         f"{rows_per_crop} (mm_vision_select_feature='cls_patch' is not a raster)")
    multi = any(s > 1 for s in split_sizes)
    if multi and getattr(cfg, "image_aspect_ratio", "square") != "anyres":
        raise NotImplementedError(f"mm_patch_merge_type={merge_type!r} merges several crops only for image_aspect_ratio='anyres', "
                                  f"not {getattr(cfg, 'image_aspect_ratio', 'square')!r} (llava_arch.py:312)")
    if multi and (image_sizes is None or len(image_sizes) != len(split_sizes)):
        raise ValueError(f"mm_patch_merge_type={merge_type!r} needs one image size per image: {len(split_sizes)} images, "
                         f"{'no' if image_sizes is None else len(image_sizes)} image_sizes")
    if images_mask is not None and len(images_mask) != len(split_sizes):
        raise ValueError(f"images_mask has {len(images_mask)} entries for {len(split_sizes)} images")
    patch = np.arange(P, dtype=np.int64)
    plans, crop0 = [], 0
    for i, s in enumerate(split_sizes):
        if s < 1:
            raise ValueError(f"image {i} has no crops")
        base = crop0 * P + patch
        if s == 1:                                                          # :325-331
            if unpad and not has_newline:
                raise ValueError(f"mm_patch_merge_type={merge_type!r}: image {i} has one crop and takes model.image_newline, which "
                                 "this model does not have (it is created when the config names 'unpad' at construction)")
            plans.append(np.concatenate([base, [MERGE_NEWLINE]]).astype(np.int64) if unpad else base)
            crop0 += s
            continue
        local = np.arange(crop0 + 1, crop0 + s, dtype=np.int64)
        if images_mask is not None:                                         # :300-302
            m = images_mask[i]
            m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
            sel = np.nonzero(m[1:])[0]
            if sel.size and int(sel.max()) >= s - 1:
                raise ValueError(f"image {i}: images_mask marks local crop {int(sel.max())} of {s - 1}")
            local = local[sel]
        w_i, h_i = (int(v) for v in image_sizes[i])
        nw, nh = _grid_of(w_i, h_i, str(cfg.image_grid_pinpoints), int(tower.config.image_size))
        if nw * nh != local.shape[0]:
            raise ValueError(f"image {i}: grid {nw}x{nh} does not match {local.shape[0]} local crops")
        # raster[y, x] of the nh*side x nw*side canvas: view(nh, nw, side, side).permute(0, 2, 1, 3)
        raster = (local.reshape(nh, 1, nw, 1) * P + patch.reshape(1, side, 1, side)).reshape(nh * side, nw * side)
        if unpad:                                                           # :314-320
            r0, r1, c0, c1 = unpad_window(image_sizes[i], nh * side, nw * side)
            raster = raster[r0:r1, c0:c1]
            raster = np.concatenate([raster, np.full((raster.shape[0], 1), MERGE_ZERO, dtype=np.int64)], axis=1)
        plans.append(np.concatenate([base, raster.reshape(-1)]))
        crop0 += s
    return plans


def merged_src(src, plans, token_rows: int):
    """``splice_plan``'s ``src`` (built with the plan lengths as ``feat_lens``) for ``ops.splice_merged``: every entry ``-2 - k`` is
    looked up in the concatenated per-image merge plans: a projector row r becomes ``-2 - r``, a zero row -1, the newline row
    ``-2 - token_rows`` (row 0 of ``extra``); token ids and -1 stay."""
    import numpy as np
    src = np.asarray(src, dtype=np.int64)
    allp = np.concatenate([np.asarray(p, dtype=np.int64) for p in plans]) if len(plans) else np.zeros((0,), dtype=np.int64)
    out = src.copy()
    m = src <= -2
    k = -2 - src[m]
    if k.size and int(k.max()) >= allp.shape[0]:
        raise ValueError("splice plan names a feature row past the last image")
    v = allp[k]
    if v.size and int(v.max()) >= token_rows:
        raise ValueError(f"merge plan names projector row {int(v.max())} of {token_rows}")
    out[m] = np.where(v >= 0, -2 - v, np.where(v == MERGE_ZERO, -1, -2 - np.int64(token_rows)))
    return out


def _pure_text_order(ids, padding_side: str = "right", max_len=None):
    """Column of ``ids`` [B, L] behind every row of get_pure_text_embedding's output, -1 for the zero rows that stand in for the
    <image> placeholders (appended; prepended for left padding), cut to ``max_len`` (llava_arch.py:162-210).  int64 [B, L']."""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64)
    rows = []
    for t in ids:
        cols = np.nonzero(t != IMAGE_TOKEN_INDEX)[0].astype(np.int64)
        pad = np.full(t.shape[0] - cols.shape[0], -1, dtype=np.int64)
        row = np.concatenate([pad, cols]) if padding_side == "left" else np.concatenate([cols, pad])
        rows.append(row if max_len is None else row[:max_len])
    return np.stack(rows, 0) if rows else np.zeros((0, 0), dtype=np.int64)


def pure_text_plan(ids, padding_side: str = "right", max_len=None):
    """Source table of ``get_pure_text_embedding`` for one ``ops.splice_rows(table, None, src, dtype)`` launch: int64 [B, L'], a token
    id per text token (padding ids included, as the reference embeds them), -1 (a zero row) per <image> placeholder."""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64)
    order = _pure_text_order(ids, padding_side, max_len)
    return np.where(order >= 0, np.take_along_axis(ids, np.maximum(order, 0), axis=1), -1) if order.size else order


_SPLICE_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


class SlimeMetaModel:
    """Mixin: builds the three hot-path plugins from the config (llava_arch.py:28-44)."""

    def __init__(self, config):
        super(SlimeMetaModel, self).__init__(config)
        if hasattr(config, "mm_vision_tower"):
            self.vision_tower = build_vision_tower(config, delay_load=True)
            self.mm_projector = build_vision_projector(config)
            self.sampler = build_vision_sampler(config)
            t = getattr(config, "mm_resampler_type", None)
            self.has_sampler = t != "identity" and t is not None and t != "spatial"
            if "unpad" in getattr(config, "mm_patch_merge_type", ""):
                # the row 'spatial_unpad' appends to a single-crop image (llava_arch.py:41-44, :327-331); zeros where the reference
                # leaves uninitialised memory: a checkpoint that carries the key overwrites it
                self.image_newline = nn.Parameter(torch.zeros(config.hidden_size))

    def get_vision_tower(self):
        vt = getattr(self, "vision_tower", None)
        return vt[0] if type(vt) is list else vt


class SlimeMetaForCausalLM(ABC):
    @abstractmethod
    def get_model(self):
        ...

    def get_vision_tower(self):
        return self.get_model().get_vision_tower()

    # ------------------------------------------------------------------ text side (router input)
    def get_pure_text_embedding(self, input_ids, attention_mask=None, labels=None):
        """Embeddings of the text tokens with the <image> placeholders removed, zero rows appended
        (or prepended for left padding) in their place (llava_arch.py:162-210)."""
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        embed = self.get_model().embed_tokens
        left = getattr(self.config, "tokenizer_padding_side", "right") == "left"
        embs, masks = [], []
        for ids, am in zip(input_ids, attention_mask):
            keep = ids != IMAGE_TOKEN_INDEX
            n_img = int((~keep).sum())
            e, m = embed(ids[keep]), am[keep]
            if n_img > 0:
                ze = torch.zeros((n_img, e.shape[1]), dtype=e.dtype, device=e.device)
                zm = torch.zeros((n_img,), dtype=m.dtype, device=m.device)
                e, m = (torch.cat((ze, e)), torch.cat((zm, m))) if left else (torch.cat((e, ze)), torch.cat((m, zm)))
            embs.append(e)
            masks.append(m)
        max_len = getattr(self.config, "tokenizer_model_max_length", None)
        if max_len is not None:
            embs, masks = [x[:max_len] for x in embs], [x[:max_len] for x in masks]
        embs, masks = torch.stack(embs, 0), torch.stack(masks, 0)
        assert masks.shape == embs.shape[:2]
        return embs, masks

    def _pure_text_planned(self, input_ids, attention_mask):
        """``get_pure_text_embedding`` as an integer plan on the host and ONE launch (``pure_text_plan`` + ``slime_splice_rows``), for
        the routed path: fp32 embeddings (the router computes in fp32; widening a 16-bit table row is exact) and the mask, both
        on the table's device."""
        import numpy as np
        table = self.get_model().embed_tokens.weight.detach()
        ids = input_ids.detach().cpu().numpy().astype(np.int64)
        _check_token_ids(ids.reshape(-1), table.shape[0])                    # what nn.Embedding would raise on
        side = getattr(self.config, "tokenizer_padding_side", "right")
        max_len = getattr(self.config, "tokenizer_model_max_length", None)
        order = _pure_text_order(ids, side, max_len)
        src = pure_text_plan(ids, side, max_len)
        am = np.ones_like(ids) if attention_mask is None else attention_mask.detach().cpu().numpy()
        mask = np.where(order >= 0, np.take_along_axis(am, np.maximum(order, 0), axis=1), 0)
        B, L = src.shape
        emb = ops.splice_rows(table, None, torch.from_numpy(src).reshape(-1).to(table.device), torch.float32).view(B, L, -1)
        return emb, torch.from_numpy(mask).to(table.device)

    def _splice_routable(self, images) -> bool:
        """``cfg.fused_splice`` asks for it and ``slime_splice_routed`` can take the call: a table and images of a type it converts,
        table and tokens on one device."""
        table = self.get_model().embed_tokens.weight
        return (bool(getattr(self.config, "fused_splice", False)) and table.dtype in _SPLICE_DTYPES and images.dtype in _SPLICE_DTYPES
                and table.device == images.device)

    def _fused_route(self, images, input_ids, split_sizes, attention_mask, images_mask, image_sizes, labels, routable: bool):
        """Tower, fused adapter and batched router for the batches a fused adapter call takes (uniform or ragged crop layouts), else
        None -- decided on the host, before any device work.  Returns ``(tokens2d, local_row_off, n_rows, P, router_state,
        counts)``: the flat fp32 token buffer [rows, H]; image i's local tokens are rows ``local_row_off[i] .. + n_rows[i]``, its
        ``P`` global tokens the rows right before them; the router's device arrays; the kept counts on the host (the step's one
        D2H read).  ``routable``: the text embeddings for the router come from ``_pure_text_planned``."""
        model = self.get_model()
        tower = model.get_vision_tower()
        cfg = self.config
        merge_type = getattr(cfg, "mm_patch_merge_type", "flat")
        fusable = (bool(getattr(cfg, "fused_adapter", True)) and isinstance(model.mm_projector, GatedBlock) and images_mask is None
                   and not getattr(cfg, "use_local_only", False) and not getattr(cfg, "use_global_only", False))
        if not fusable:
            return None
        layout = _uniform_layout(list(split_sizes), image_sizes, cfg, tower.config.image_size, merge_type)
        grids = None
        if layout is None:
            grids = _ragged_layout(list(split_sizes), image_sizes, cfg, tower.config.image_size, merge_type)
        if grids is None and (layout is None or layout[0] == 0):
            return None
        text_emb, text_mask = self._pure_text_planned(input_ids, attention_mask) if routable \
            else self.get_pure_text_embedding(input_ids, attention_mask, labels)
        B, P = len(split_sizes), tower.num_patches
        if grids is None:
            tokens = _fused_adapter(model, images, layout, torch.float32)        # [B, 576 + n*g*g, H] fp32
            rows = tokens.shape[1]
            tokens, off, n_rows = tokens.view(B * rows, -1), [i * rows + P for i in range(B)], [rows - P] * B
        else:
            # ragged batch, same program: one flat fp32 token buffer, image i at rows [row0[i], row0[i] + 576 + n_i*g*g); the
            # router reads its local rows in place (no per-image merge launch, no concatenation)
            tokens, row0 = _fused_adapter_ragged(model, images, grids, merge_type == "spatial", torch.float32)
            q = model.sampler.grid_size ** 2
            off, n_rows = [r + P for r in row0], [nw * nh * q for nw, nh in grids]
        # router: all B images in one launch pair, one D2H for the B kept counts (the reference syncs per image)
        st = model.sampler.select_batched_device(tokens, off, n_rows, text_emb, text_mask, **_router_operand_dtype(model, images))
        return tokens, off, n_rows, P, st, st.counts

    # ------------------------------------------------------------------ the hot path
    def encode_images(self, images, input_ids=None, split_sizes=None, attention_mask=None, images_mask=None,
                      image_sizes=None, labels=None):
        _require_inference(self.get_model())
        with torch.no_grad():
            return self._encode_images(images, input_ids, split_sizes, attention_mask, images_mask, image_sizes, labels)

    def _encode_images(self, images, input_ids, split_sizes, attention_mask, images_mask, image_sizes, labels):
        model = self.get_model()
        tower = model.get_vision_tower()
        cfg = self.config
        merge_type = getattr(cfg, "mm_patch_merge_type", "flat")
        use_local_only = getattr(cfg, "use_local_only", False)
        use_global_only = getattr(cfg, "use_global_only", False)
        out_dtype = images.dtype

        if model.has_sampler and split_sizes is not None:
            B = len(split_sizes)
            routable = self._splice_routable(images)
            fused = self._fused_route(images, input_ids, split_sizes, attention_mask, images_mask, image_sizes, labels, routable)
            if fused is not None and routable:
                # one launch writes every image's [glob | sep | routed] rows into one flat buffer; the per-image tensors are views
                tokens, off, n_rows, P, st, counts = fused
                import numpy as np
                lens = [P + 1 + c for c in counts]
                src = np.concatenate([-2 - ((np.int64(i) << 32) | np.arange(n, dtype=np.int64)) for i, n in enumerate(lens)])
                flat = ops.splice_routed(model.embed_tokens.weight.detach(), int(cfg.seperator), tokens, P, st,
                                         torch.from_numpy(src).to(tokens.device), out_dtype, out_dtype)
                return [f.unsqueeze(0) for f in torch.split(flat, lens, dim=0)], split_sizes
            if fused is not None:
                tokens, off, n_rows, P, st, counts = fused
                sep = model.embed_tokens(torch.tensor(cfg.seperator, dtype=input_ids.dtype, device=input_ids.device))
                sep32 = sep.to(device=tokens.device, dtype=torch.float32).unsqueeze(0)
                outs = []
                for i in range(B):
                    glob = tokens[off[i] - P:off[i]]
                    routed = tokens[off[i]:off[i] + n_rows[i]].index_select(0, st.keep[i, :counts[i]].long())
                    outs.append(torch.cat([glob, sep32, routed], dim=0).to(out_dtype).unsqueeze(0))
                return outs, split_sizes
            sep = model.embed_tokens(torch.tensor(cfg.seperator, dtype=input_ids.dtype, device=input_ids.device))
            text_emb, text_mask = self.get_pure_text_embedding(input_ids, attention_mask, labels)
            feats = tower(images, out_dtype=torch.float32)                      # [sum(1+n_i), 576, D], one batch
            dev = feats.device
            g_idx, l_idx = _split_indices(split_sizes, dev)
            glob = loc = None
            # the adapter's MFMA operands are of the IMAGES' 16-bit type, as in the reference (its tower hands the adapter features
            # in the input dtype, clip_encoder.py:52,56) -- not of a default picked from the fp32 hand-over (round 6: an fp16 call
            # into fp32 adapter parameters ran the adapter on bf16 operands)
            T16 = _adapter_operand_dtype(model, images)
            if not use_local_only:
                glob = model.mm_projector(feats.index_select(0, g_idx), out_dtype=torch.float32, **T16)      # [B,576,H]
            if not use_global_only:
                comp = model.sampler.post_qformer(feats.index_select(0, l_idx), out_dtype=torch.float32, **T16)   # [sum n_i,144,D]
                loc = _project_local(model.mm_projector, comp, T16.get("operand_dtype"))         # [sum n_i,144,H]
            g = model.sampler.grid_size
            merged_list = []
            lstart = 0
            for i in range(B):
                if loc is None:
                    break
                n_i = split_sizes[i] - 1
                li = loc[lstart:lstart + n_i]
                lstart += n_i
                if images_mask is not None and images_mask[0].size(0) - 1 == li.size(0):
                    li = li[torch.nonzero(images_mask[i][1:]).squeeze(1)]    # padded crops (train.py:903-926)
                H = li.shape[-1]
                merged = torch.empty((li.shape[0] * g * g, H), dtype=torch.float32, device=dev)
                if li.shape[0] > 0:
                    if merge_type == "spatial":
                        nw, nh = get_anyres_image_grid_shape(image_sizes[i], cfg.image_grid_pinpoints, tower.config.image_size)
                        if nw * nh != li.shape[0]:
                            raise ValueError(f"image {i}: grid {nw}x{nh} does not match {li.shape[0]} local crops")
                        ops.merge_rows(li.contiguous(), merged, 0, nw, nh, g, True)
                    elif merge_type == "flat":
                        ops.merge_rows(li.contiguous(), merged, 0, li.shape[0], 1, g, False)
                    else:
                        raise NotImplementedError(f"mm_patch_merge_type={merge_type!r}")
                merged_list.append(merged)
            keeps = None
            if merged_list:
                # one ragged concatenation -> one batched router call (one D2H for all kept counts)
                cat = torch.cat(merged_list, 0)
                offs, o = [], 0
                for m_ in merged_list:
                    offs.append(o)
                    o += m_.shape[0]
                keeps = model.sampler.select_batched(cat, offs, [m_.shape[0] for m_ in merged_list], text_emb, text_mask,
                                                     **_router_operand_dtype(model, images))
            outs = []
            for i in range(B):
                pieces = []
                if glob is not None:
                    pieces.append(glob[i])
                if loc is not None:
                    if glob is not None:
                        pieces.append(sep.to(device=dev, dtype=torch.float32).unsqueeze(0))
                    pieces.append(merged_list[i].index_select(0, keeps[i]))
                outs.append(torch.cat(pieces, dim=0).to(out_dtype).unsqueeze(0))
            return outs, split_sizes

        if split_sizes is not None:                                               # no sampler: per-image lists
            return list(torch.split(self._project_crops(images, out_dtype), split_sizes, dim=0)), split_sizes

        T16 = _adapter_operand_dtype(model, images)
        feats = tower(images, out_dtype=torch.float32)
        return model.mm_projector(feats, out_dtype=out_dtype, **T16), split_sizes

    def _project_crops(self, images, out_dtype):
        """Tower and ``mm_projector`` once over all crops of a batch without a sampler (llava_arch.py:257-260): [crops, P, H] of
        ``out_dtype`` (an IdentityMap hands the tower's fp32 features through whatever is asked for)."""
        model = self.get_model()
        T16 = _adapter_operand_dtype(model, images)
        feats = model.get_vision_tower()(images, out_dtype=torch.float32)
        if not isinstance(model.mm_projector, GatedBlock):
            return model.mm_projector(feats, out_dtype=out_dtype, **T16)
        return torch.cat([model.mm_projector(f, out_dtype=out_dtype, **T16) for f in torch.split(feats, 1)], 0)

    def _merged_unsampled(self, images, split_sizes, image_sizes, images_mask):
        """The un-sampled 'spatial' / 'spatial_unpad' branch without its per-image tensors: the merge plans (host; every refusal is
        raised before the device is touched), the projector's fp32 output over all crops as [crops * P, H], and the dtype the
        features of ``encode_images`` carry for this model -- the middle rounding ``slime_splice_merged`` applies."""
        from .multimodal_projector.builder import IdentityMap
        model = self.get_model()
        plans = unsampled_merge_plans(list(split_sizes), image_sizes, images_mask, self.config, model.get_vision_tower(),
                                      getattr(model, "image_newline", None) is not None)
        _require_inference(model)
        with torch.no_grad():
            tokens = self._project_crops(images, torch.float32)
        P = model.get_vision_tower().num_patches
        if tokens.dim() != 3 or tokens.shape[0] != sum(split_sizes) or tokens.shape[1] != P or tokens.dtype != torch.float32:
            raise ValueError(f"mm_projector returned {tuple(tokens.shape)} {tokens.dtype} for {sum(split_sizes)} crops of {P} rows: the "
                             "merged splice needs fp32 [crops, P, H]")
        mid = torch.float32 if isinstance(model.mm_projector, IdentityMap) else images.dtype
        return plans, tokens.reshape(-1, tokens.shape[-1]), mid


    # ------------------------------------------------------------------ splice (the step after the hot path)
    def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images,
                                             image_sizes=None, images_mask=None):
        """Signature, branches and return tuple of llava_arch.py:274-459.  The visual features come from ``encode_images``
        above; the splice itself is an integer plan on the host (``splice_plan``: token ids are a few hundred ints) and ONE
        device launch (``slime_splice_rows``) that writes the whole padded [B, max_len, H] embedding tensor -- embedding
        lookup, image rows, zero padding -- where the reference runs per-sequence embed / split / cat / stack.  Without a sampler,
        'spatial' / 'spatial_unpad' (the LLaVA-NeXT crop merge, :293-333) is part of the same plan: ``unsampled_merge_plans`` names the
        projector row, zero row or ``image_newline`` behind every feature position and ``slime_splice_merged`` moves the rows from the
        projector's fp32 output in that one launch; no per-image feature tensor is built."""
        vision_tower = self.get_vision_tower()
        if vision_tower is None or images is None or input_ids.shape[1] == 1:
            return input_ids, position_ids, attention_mask, past_key_values, None, labels
        merge_type = getattr(self.config, "mm_patch_merge_type", "flat")
        # The ids come to the host once (the splice plan below is integer host logic).  A token id outside the embedding table is
        # rejected HERE, before anything touches the device: the reference's nn.Embedding lookups would hit a device-side assert,
        # which on ROCm aborts the process instead of raising.  Scope as in the reference: the splice embeds only the ids under the
        # attention mask (llava_arch.py:361-373: a pad id past the table is legal there) -- splice_plan checks those --, the
        # text-guided router embeds EVERY non-image id, padding included (get_pure_text_embedding, :162-179).
        ids_np = input_ids.detach().cpu().numpy()
        vocab = self.get_model().embed_tokens.weight.shape[0]
        if getattr(self.get_model(), "has_sampler", False) and ids_np.size:
            _check_token_ids(ids_np.reshape(-1), vocab)
        routed = merged = am_np = lab_np = None
        if type(images) is list or images.ndim == 5:
            if type(images) is list:
                images = [x.unsqueeze(0) if x.ndim == 3 else x for x in images]
            concat_images = torch.cat([im for im in images], dim=0)
            split_sizes = [im.shape[0] for im in images]
            if getattr(self.get_model(), "has_sampler", False) and self._splice_routable(concat_images):
                # cfg.fused_splice: no per-image feature tensors -- the router's device arrays go to the splice launch below
                _require_inference(self.get_model())
                with torch.no_grad():
                    routed = self._fused_route(concat_images, input_ids, split_sizes, attention_mask, images_mask, image_sizes, labels, True)
            feats = []
            if not getattr(self.get_model(), "has_sampler", False) and merge_type.startswith("spatial"):
                # LLaVA-NeXT merge of un-sampled crops (:293-333): a host plan over the projector's rows, no per-image tensors
                # mask and labels come to the host BEFORE the tower is launched: splice_plan then runs under the device work
                am_np = None if attention_mask is None else attention_mask.detach().cpu().numpy()
                lab_np = None if labels is None else labels.detach().cpu().numpy()
                merged = self._merged_unsampled(concat_images, split_sizes, image_sizes, images_mask)
            elif routed is None:
                feats, split_sizes = self.encode_images(concat_images, input_ids, split_sizes, attention_mask, images_mask, image_sizes,
                                                        labels=labels)
            if type(feats) is not list:
                feats = list(torch.split(feats, split_sizes, dim=0))
            flat = []
            for f in feats:
                if f.dim() == 3 and f.shape[0] == 1:                      # sampler branch: [1, 576 + 1 + k, H] (:254-255,322)
                    flat.append(f[0])
                elif merge_type == "flat":                                  # :290-291
                    flat.append(f.flatten(0, 1))
                else:
                    raise ValueError(f"Unexpected mm_patch_merge_type: {merge_type}")
            feats = flat
        else:
            f, _ = self.encode_images(images, input_ids=input_ids, attention_mask=attention_mask, labels=labels)
            feats = [x for x in f]
        if getattr(self.config, "tune_mm_mlp_adapter", False) and getattr(self.config, "mm_use_im_start_end", False):
            raise NotImplementedError

        embed = self.get_model().embed_tokens
        table = embed.weight
        dev = table.device
        feat_lens = [f.shape[0] for f in feats] if routed is None else [routed[3] + 1 + c for c in routed[5]]
        if merged is not None:
            feat_lens = [int(p.shape[0]) for p in merged[0]]
        if merged is None:
            am_np = None if attention_mask is None else attention_mask.detach().cpu().numpy()
            lab_np = None if labels is None else labels.detach().cpu().numpy()
        src, lab, mask, pos = splice_plan(ids_np, am_np, lab_np,
                                          feat_lens, getattr(self.config, "tokenizer_model_max_length", None),
                                          getattr(self.config, "tokenizer_padding_side", "right"), vocab_size=vocab)
        B, T = src.shape
        out_dtype = table.dtype if table.dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32
        if routed is not None:
            # the same plan with (image, position) in place of rows of a concatenation that is never built; the image rows take
            # the rounding to the images' dtype that encode_images gives its features, then the cast to the table's
            tokens, _, _, P, st, _ = routed
            src_d = torch.from_numpy(routed_src(src, feat_lens)).reshape(-1).to(dev)
            new_input_embeds = ops.splice_routed(table.detach(), int(self.config.seperator), tokens, P, st, src_d, concat_images.dtype,
                                                 out_dtype).view(B, T, -1)
        elif merged is not None:
            # the same plan looked up in the per-image merge plans: an image row names a row of the projector's fp32 output, a zero
            # row or image_newline; the projector rows take the rounding encode_images gives its features, then the cast to the table's
            plans, tokens, mid = merged
            newline = getattr(self.get_model(), "image_newline", None)
            extra = None if newline is None else newline.detach()[None].to(dev)
            src_d = torch.from_numpy(merged_src(src, plans, tokens.shape[0])).reshape(-1).to(dev)
            new_input_embeds = ops.splice_merged(table.detach(), tokens, extra, src_d, mid, out_dtype).view(B, T, -1)
        else:
            allf = torch.cat([f.reshape(-1, f.shape[-1]) for f in feats], 0).to(dev) if feats else None
            new_input_embeds = ops.splice_rows(table.detach(), allf, torch.from_numpy(src).reshape(-1).to(dev), out_dtype).view(B, T, -1)
        new_labels = None if labels is None else torch.from_numpy(lab).to(labels.device, labels.dtype)
        new_mask = None if attention_mask is None else torch.from_numpy(mask).to(attention_mask.device, attention_mask.dtype)
        new_pos = None if position_ids is None else torch.from_numpy(pos).to(position_ids.device, position_ids.dtype)
        return None, new_pos, new_mask, past_key_values, new_input_embeds, new_labels


class _Cfg:
    """Attribute bag with the config names the reference persists (llava_arch.py:64-93)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def default_slime_config(vision_tower: str = "synthetic:1234", hidden_size: int = 4096, mm_hidden_size: int = 1024,
                         **over) -> _Cfg:
    """SliME-8B inference configuration (scripts/llama/llama3_8b_sft.sh:14-48)."""
    d = dict(mm_vision_tower=vision_tower, mm_vision_select_layer=-2, mm_vision_select_feature="patch",
             mm_projector_type="gated", mm_hidden_size=mm_hidden_size, hidden_size=hidden_size,
             mm_patch_merge_type="spatial", image_aspect_ratio="anyres", mm_resampler_type="cosine",
             mm_resampler_topp=0.95, mm_resampler_dim=144, mm_resampler_temp=1.0, mm_learnable_gated=-1,
             image_grid_pinpoints="[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]",
             seperator=1919, pad_token_id=0, use_local_only=False, use_global_only=False,
             fused_splice=False)          # opt-in: router output -> embeddings in one launch (slime_splice_routed), bit-identical
    d.update(over)
    return _Cfg(**d)


class _ModelBase(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config


class _VisualModel(SlimeMetaModel, _ModelBase):
    def __init__(self, config, embed_tokens: Optional[nn.Module] = None):
        super().__init__(config)
        self.embed_tokens = embed_tokens


class SlimeVisualEncoder(nn.Module, SlimeMetaForCausalLM):
    """Standalone visual front end: tower + adapter + glue, no LLM.  ``embed_tokens`` (the LLM's
    embedding table) is only needed for the separator token and the text-guided router."""

    def __init__(self, config, embed_tokens: Optional[nn.Module] = None):
        super().__init__()
        self.config = config
        self.model = _VisualModel(config, embed_tokens)
        self.eval()                     # inference front end (a from_pretrained HF model arrives in eval mode as well)

    def get_model(self):
        return self.model

    def load_visual_state(self, tower_sd=None, adapter_sd=None):
        vt = self.get_vision_tower()
        if not vt.is_loaded:
            vt.load_model()
        if tower_sd is not None:
            from .multimodal_encoder.clip_encoder import check_tower_keys
            check_tower_keys(vt.vision_tower.load_state_dict(tower_sd, strict=False), "<state dict>")
        if adapter_sd is not None:
            from ..weights import sub_state
            self.model.mm_projector.load_state_dict(sub_state(adapter_sd, "mm_projector."), strict=True)
            if len(self.model.sampler.state_dict()) > 0:          # IdentityMap (no sampler) has no parameters
                self.model.sampler.load_state_dict(sub_state(adapter_sd, "sampler."), strict=True)
            newline = getattr(self.model, "image_newline", None)
            if newline is not None:                                # train.py:246 saves it next to mm_projector; optional here
                for key in ("image_newline", "model.image_newline"):
                    if key in adapter_sd:
                        v = adapter_sd[key]
                        if tuple(v.shape) != tuple(newline.shape):
                            raise ValueError(f"{key} has shape {tuple(v.shape)}, the model's image_newline {tuple(newline.shape)}")
                        with torch.no_grad():
                            newline.copy_(v)
                        break
        return self

    @torch.no_grad()
    def encode_visual(self, images: torch.Tensor, split_sizes: Sequence[int], image_sizes=None, merge: Optional[str] = None):
        """Router-free form of the sampler branch (what bench.py times): returns per image
        ``(global [576,H], merged_local [n*144,H])`` in fp32."""
        model = self.model
        tower = model.get_vision_tower()
        merge = merge or getattr(self.config, "mm_patch_merge_type", "flat")
        if getattr(self.config, "fused_adapter", True) and isinstance(model.mm_projector, GatedBlock):
            layout = _uniform_layout(list(split_sizes), image_sizes, self.config, tower.config.image_size, merge)
            if layout is not None and layout[0] > 0:
                tokens = _fused_adapter(model, images, layout, torch.float32)
                P = tower.num_patches
                return [(tokens[i, :P], tokens[i, P:]) for i in range(len(split_sizes))]
            grids = None
            if layout is None:
                grids = _ragged_layout(list(split_sizes), image_sizes, self.config, tower.config.image_size, merge)
            if grids is not None:
                tokens, row0 = _fused_adapter_ragged(model, images, grids, merge == "spatial", torch.float32)
                P, q = tower.num_patches, model.sampler.grid_size ** 2
                return [(tokens[r:r + P], tokens[r + P:r + P + nw * nh * q]) for r, (nw, nh) in zip(row0, grids)]
        feats = tower(images, out_dtype=torch.float32)
        dev = feats.device
        g_idx, l_idx = _split_indices(split_sizes, dev)
        T16 = _adapter_operand_dtype(model, images)
        glob = model.mm_projector(feats.index_select(0, g_idx), out_dtype=torch.float32, **T16)
        n_local = feats.shape[0] - len(split_sizes)
        if n_local == 0:
            return [(glob[i], glob.new_zeros((0, glob.shape[-1]))) for i in range(len(split_sizes))]
        comp = model.sampler.post_qformer(feats.index_select(0, l_idx), out_dtype=torch.float32, **T16)
        loc = _project_local(model.mm_projector, comp, T16.get("operand_dtype"))
        g = model.sampler.grid_size
        outs, lstart = [], 0
        for i, s in enumerate(split_sizes):
            n_i = s - 1
            li = loc[lstart:lstart + n_i].contiguous()
            lstart += n_i
            merged = torch.empty((n_i * g * g, li.shape[-1]), dtype=torch.float32, device=dev)
            if n_i > 0:
                if merge == "spatial":
                    nw, nh = get_anyres_image_grid_shape(image_sizes[i], self.config.image_grid_pinpoints,
                                                         tower.config.image_size)
                    ops.merge_rows(li, merged, 0, nw, nh, g, True)
                else:
                    ops.merge_rows(li, merged, 0, n_i, 1, g, False)
            outs.append((glob[i], merged))
        return outs
