"""Minimal CLIP image processor with the attribute surface the reference's ``mm_utils`` touches
(``crop_size['height']``, ``crop_size.values()``, ``size['shortest_edge']``, ``image_mean``,
``preprocess(img, return_tensors='pt')['pixel_values']``) -- the role HF ``CLIPImageProcessor`` plays at
llava/model/multimodal_encoder/clip_encoder.py:30.  Host (CPU, PIL + numpy) code: it runs inside
forked DataLoader workers in the reference (llava/eval/model_vqa_loader.py:78), where HIP cannot.

Arithmetic follows transformers' PIL backend so outputs are bit-identical to it:
resize shortest edge (bicubic, long side ``int(size*long/short)``) -> centre crop (``(h-crop)//2``) ->
``float32(float64(u8) * (1/255))`` -> ``(x - mean32) / std32`` -> CHW.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Sequence, Union

import numpy as np
import torch
from PIL import Image

from .constants import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD


class ClipImageProcessor:
    def __init__(self, size: int = 336, crop_size: int = 336, image_mean: Sequence[float] = OPENAI_CLIP_MEAN,
                 image_std: Sequence[float] = OPENAI_CLIP_STD, rescale_factor: float = 1 / 255):
        self.size: Dict[str, int] = {"shortest_edge": int(size)}
        self.crop_size: Dict[str, int] = {"height": int(crop_size), "width": int(crop_size)}
        self.image_mean: List[float] = [float(v) for v in image_mean]
        self.image_std: List[float] = [float(v) for v in image_std]
        self.rescale_factor = float(rescale_factor)
        self.resample = Image.BICUBIC

    @classmethod
    def from_pretrained(cls, path: str) -> "ClipImageProcessor":
        """Read an HF ``preprocessor_config.json`` from a local directory (no hub access here)."""
        f = os.path.join(path, "preprocessor_config.json")
        if not os.path.isfile(f):
            return cls()
        cfg = json.load(open(f))
        size = cfg.get("size", 336)
        size = size.get("shortest_edge", size.get("height", 336)) if isinstance(size, dict) else size
        crop = cfg.get("crop_size", size)
        crop = crop.get("height", size) if isinstance(crop, dict) else crop
        return cls(size, crop, cfg.get("image_mean", OPENAI_CLIP_MEAN), cfg.get("image_std", OPENAI_CLIP_STD),
                   cfg.get("rescale_factor", 1 / 255))

    # -- pieces -------------------------------------------------------------------------------
    def _resize_center_crop(self, img: Image.Image) -> np.ndarray:
        img = img.convert("RGB")
        w, h = img.size
        s = self.size["shortest_edge"]
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = s, int(s * long / short)
        nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
        if (nw, nh) != (w, h):
            img = img.resize((nw, nh), resample=self.resample)
        arr = np.asarray(img)                                  # HWC uint8
        ch, cw = self.crop_size["height"], self.crop_size["width"]
        top, left = (nh - ch) // 2, (nw - cw) // 2
        if top < 0 or left < 0:                                # smaller than the crop: zero pad (HF center_crop)
            ph, pw = max(ch, nh), max(cw, nw)
            pad = np.zeros((ph, pw, 3), dtype=arr.dtype)
            t0, l0 = -(-(ph - nh) // 2), -(-(pw - nw) // 2)
            pad[t0:t0 + nh, l0:l0 + nw] = arr
            arr, top, left = pad, (ph - ch) // 2, (pw - cw) // 2
        return arr[top:top + ch, left:left + cw]

    def normalize_u8(self, arr: np.ndarray) -> np.ndarray:
        """HWC uint8 -> CHW float32, HF numerics."""
        x = (arr.astype(np.float64) * self.rescale_factor).astype(np.float32)
        x = (x - np.array(self.image_mean, dtype=np.float32)) / np.array(self.image_std, dtype=np.float32)
        return np.ascontiguousarray(x.transpose(2, 0, 1))

    def preprocess(self, images: Union[Image.Image, Sequence[Image.Image]], return_tensors: str = "pt"):
        if isinstance(images, Image.Image):
            images = [images]
        out = [self.normalize_u8(self._resize_center_crop(im)) for im in images]
        if return_tensors == "pt":
            return {"pixel_values": torch.from_numpy(np.stack(out, 0))}
        return {"pixel_values": out}

    __call__ = preprocess


IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class Dinov2ImageProcessor(ClipImageProcessor):
    """The role of HF ``BitImageProcessor``, which the DINOv2 checkpoints name in ``preprocessor_config.json``: resize the shortest
    edge to 256 (bicubic), centre crop 224, rescale, ImageNet mean / std -- the pipeline of the class above with other constants
    (bit-identical to transformers' PIL backend).  ``crop_size`` is the size the tower runs at."""

    def __init__(self, size: int = 256, crop_size: int = 224, image_mean: Sequence[float] = IMAGENET_MEAN,
                 image_std: Sequence[float] = IMAGENET_STD, rescale_factor: float = 1 / 255, resample: int = Image.BICUBIC):
        super().__init__(size, crop_size, image_mean, image_std, rescale_factor)
        self.resample = Image.Resampling(int(resample))

    @classmethod
    def from_pretrained(cls, path: str, default_crop: int = 224) -> "Dinov2ImageProcessor":
        """Read ``preprocessor_config.json`` from a local directory; without one: a centre crop of ``default_crop`` out of a
        shortest edge of 256 / 224 times that (the released checkpoints' ratio)."""
        f = os.path.join(path, "preprocessor_config.json")
        if not os.path.isfile(f):
            return cls(default_crop * 256 // 224, default_crop)
        cfg = json.load(open(f))
        crop = cfg.get("crop_size", default_crop)
        if isinstance(crop, dict):
            if crop.get("height", default_crop) != crop.get("width", crop.get("height", default_crop)):
                raise ValueError(f"Dinov2ImageProcessor: crop_size {crop} is not square (the tower takes one run size)")
            crop = crop.get("height", default_crop)
        size = cfg.get("size", crop * 256 // 224)
        size = size.get("shortest_edge", size.get("height", crop)) if isinstance(size, dict) else size
        return cls(size, crop, cfg.get("image_mean", IMAGENET_MEAN), cfg.get("image_std", IMAGENET_STD),
                   cfg.get("rescale_factor", 1 / 255), cfg.get("resample", Image.BICUBIC))


SIGLIP_MEAN = (0.5, 0.5, 0.5)
SIGLIP_STD = (0.5, 0.5, 0.5)


class SiglipImageProcessor(ClipImageProcessor):
    """The role of HF ``SiglipImageProcessor``: resize to exactly ``(size, size)`` -- the aspect ratio is NOT kept and there is no
    centre crop -- with the resample filter of ``preprocessor_config.json``, then the rescale / normalise arithmetic of the class
    above (bit-identical to transformers' PIL backend).  ``size`` carries ``shortest_edge`` next to ``height`` / ``width`` and
    ``crop_size`` is the output size: the attribute surface ``mm_utils`` touches.  ``do_center_crop`` is False: the device
    pre-processing modes that would resize the shortest edge and cut a centre window refuse this processor (mm_utils)."""
    do_center_crop = False

    def __init__(self, size: int = 384, image_mean: Sequence[float] = SIGLIP_MEAN, image_std: Sequence[float] = SIGLIP_STD,
                 rescale_factor: float = 1 / 255, resample: int = Image.BICUBIC):
        super().__init__(size, size, image_mean, image_std, rescale_factor)
        self.size = {"shortest_edge": int(size), "height": int(size), "width": int(size)}
        self.resample = Image.Resampling(int(resample))

    @classmethod
    def from_pretrained(cls, path: str, default_size: int = 384) -> "SiglipImageProcessor":
        f = os.path.join(path, "preprocessor_config.json")
        if not os.path.isfile(f):
            return cls(default_size)
        cfg = json.load(open(f))
        size = cfg.get("size", default_size)
        if isinstance(size, dict):
            h, w = size.get("height", size.get("shortest_edge", default_size)), size.get("width", size.get("shortest_edge", default_size))
            if h != w:
                raise ValueError(f"SiglipImageProcessor: size {size} is not square (the tower takes one image_size)")
            size = h
        return cls(size, cfg.get("image_mean", SIGLIP_MEAN), cfg.get("image_std", SIGLIP_STD), cfg.get("rescale_factor", 1 / 255),
                   cfg.get("resample", Image.BICUBIC))

    def _resize_center_crop(self, img: Image.Image) -> np.ndarray:
        """(the base class's hook) RGB, then ONE resize to (size, size); an image of that size already is passed through."""
        img = img.convert("RGB")
        s = self.crop_size["height"]
        if img.size != (s, s):
            img = img.resize((s, s), resample=self.resample)
        return np.asarray(img)
