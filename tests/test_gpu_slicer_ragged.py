"""GPU tests of the job-table slicer (slime_slice_jobs; mm_utils.process_images_gpu_ragged): a batch of differently sized images in
two launches.  Every comparison is exact (torch.equal / np.array_equal): against the existing kernels (slime_resize_bicubic_u8 into
a zeroed canvas + slime_tile_normalize, themselves pinned to Pillow by test_gpu_slicer.py), against PIL directly, against the host
slicer and against the reference-generated pixel goldens."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"
CROP = 16
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
SENTINEL = 7.0
OUT_CROPS = 50


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def abi_jobs(dev):
    """The smallest jobs (crop 16) that reach every branch of the two kernels; (name, host pixels, device source, out_w, out_h,
    canvas_w, canvas_h, x0, y0, first_crop).  The first_crop values are out of job order and leave crops 0, 7, 8, 40 and 47 .. 49 to
    nobody."""
    spec = [  # name, (src_h, src_w), (out_h, out_w), (canvas_h, canvas_w), (x0, y0), first_crop
        ("both passes, down-scale, off-centre paste", (37, 23), (20, 14), (32, 48), (5, 3), 41),       # 6 tiles
        ("both passes, up-scale", (9, 7), (32, 16), (32, 16), (0, 0), 1),                              # 2 tiles
        ("horizontal only", (16, 40), (16, 32), (16, 32), (0, 0), 3),                                  # 2
        ("horizontal only, padded, odd row bytes", (11, 9), (11, 13), (16, 16), (2, 4), 38),           # 1
        ("vertical only, aligned rows", (10, 16), (16, 16), (16, 16), (0, 0), 5),                      # 1
        ("vertical only, 21-byte rows, padded", (9, 7), (16, 7), (16, 16), (4, 0), 6),                 # 1
        ("neither pass, padded", (16, 16), (16, 16), (32, 32), (7, 9), 9),                             # 4
        ("neither pass, whole tiles", (16, 32), (16, 32), (16, 32), (0, 0), 39 - 3),                   # 2: crops 36, 37
        ("two segments, second partial", (4, 701), (8, 304), (16, 304), (0, 5), 13),                   # 19: crops 13 .. 31
        ("span over 48 KiB", (4, 17000), (8, 4), (16, 16), (6, 8), 39),                                # 1
        ("unaligned view at the end of its allocation", (5, 50), (7, 20), (16, 32), (12, 9), 32),      # 2
        ("vertical only at the end of its allocation", (5, 6), (16, 6), (16, 16), (10, 0), 34),        # 1
        ("upscale 1x1", (1, 1), (16, 16), (16, 16), (0, 0), 35),                                       # 1
    ]
    jobs = []
    for i, (name, (h, w), (oh, ow), (ch, cw), (x0, y0), first) in enumerate(spec):
        px = _rand(h, w, 1000 + i)
        if "allocation" in name:
            buf = torch.empty((1 + h * w * 3,), dtype=torch.uint8, device=dev)       # the view starts 1 byte in and ends with the storage
            src = buf[1:].view(h, w, 3)
            src.copy_(torch.from_numpy(px))
            assert src.data_ptr() % 16 != 0 and src.data_ptr() + h * w * 3 == buf.data_ptr() + buf.numel()
        else:
            src = torch.from_numpy(px).to(dev)
        jobs.append((name, px, src, ow, oh, cw, ch, x0, y0, first))
    owned = sorted(c for j in jobs for c in range(j[9], j[9] + (j[5] // CROP) * (j[6] // CROP)))
    assert len(owned) == len(set(owned)) and max(owned) < OUT_CROPS
    assert sorted(set(range(OUT_CROPS)) - set(owned)) == [0, 7, 8, 40, 47, 48, 49]
    return jobs


@pytest.fixture(scope="module")
def abi_expected(dev, abi_jobs):
    """Per job, the crops the existing kernels give: resize into a zeroed canvas, then tile + normalise (fp32)."""
    from slime_amd import ops
    want = []
    for name, px, src, ow, oh, cw, ch, x0, y0, first in abi_jobs:
        canvas = torch.zeros((ch, cw, 3), dtype=torch.uint8, device=dev)
        ops.resize_bicubic_u8(src, ow, oh, out=canvas[y0:y0 + oh, x0:x0 + ow])
        want.append(ops.tile_normalize(canvas, CROP, MEAN, STD, torch.float32))
    return want


def _run(ops, dev, jobs, dtype, order=None):
    out = torch.full((OUT_CROPS, 3, CROP, CROP), SENTINEL, dtype=dtype, device=dev)
    table = [j[2:] for j in jobs]
    if order is not None:
        table = [table[i] for i in order]
    ops.slice_jobs(table, CROP, MEAN, STD, out)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_job_table_equals_the_existing_kernels(dev, abi_jobs, abi_expected, dtype):
    """One call with every job: each job's crops equal resize + tile_normalize (the 16-bit results the rounded fp32 ones), crops no
    job owns keep the sentinel."""
    from slime_amd import ops
    out = _run(ops, dev, abi_jobs, dtype)
    owned = torch.zeros(OUT_CROPS, dtype=torch.bool)
    for (name, *_rest, first), want in zip(abi_jobs, abi_expected):
        n = want.shape[0]
        owned[first:first + n] = True
        got = out[first:first + n]
        assert torch.equal(got, want.to(dtype)), (name, int((got.float() != want.to(dtype).float()).sum()))
    assert bool((out[~owned.to(dev)] == SENTINEL).all())


def test_job_table_matches_pillow(dev, abi_jobs):
    """Three of the jobs against PIL directly: Image.resize, paste on black, tile, rescale + normalise in numpy (fp32)."""
    from slime_amd import ops
    out = _run(ops, dev, abi_jobs, torch.float32).cpu().numpy()
    mean, std = np.array(MEAN, dtype=np.float32), np.array(STD, dtype=np.float32)
    checked = 0
    for name, px, src, ow, oh, cw, ch, x0, y0, first in abi_jobs:
        if name not in ("both passes, down-scale, off-centre paste", "two segments, second partial", "span over 48 KiB"):
            continue
        canvas = np.zeros((ch, cw, 3), dtype=np.uint8)
        canvas[y0:y0 + oh, x0:x0 + ow] = np.asarray(Image.fromarray(px, "RGB").resize((ow, oh)))
        norm = ((canvas.astype(np.float64) * (1.0 / 255.0)).astype(np.float32) - mean) / std
        tiles = [norm[y:y + CROP, x:x + CROP].transpose(2, 0, 1) for y in range(0, ch, CROP) for x in range(0, cw, CROP)]
        assert np.array_equal(out[first:first + len(tiles)], np.stack(tiles)), name
        checked += 1
    assert checked == 3


def test_job_order_does_not_change_the_crops(dev, abi_jobs):
    from slime_amd import ops
    a = _run(ops, dev, abi_jobs, torch.float32)
    order = list(np.random.default_rng(3).permutation(len(abi_jobs)))
    assert order != sorted(order)
    b = _run(ops, dev, abi_jobs, torch.float32, order=order)
    assert torch.equal(a, b)


MIXED = [(336, 336), (672, 672), (640, 480), (300, 200), (1000, 150), (823, 823)]     # first: thumbnail resize skipped; second: canvas resize skipped


@pytest.fixture(scope="module")
def mixed_batch():
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    proc = ClipImageProcessor()
    imgs = [Image.fromarray(_rand(h, w, w * 31 + h), "RGB") for w, h in MIXED]
    ref = M.process_images(imgs, proc, cfg)                                   # PIL host path: list of [1 + n_i, 3, 336, 336] fp32
    assert isinstance(ref, list)
    return cfg, proc, imgs, ref


@pytest.mark.parametrize("as_tensors", [False, True])
def test_ragged_slicer_equals_host_slicer(dev, mixed_batch, as_tensors):
    """process_images_gpu_ragged == process_images (PIL) image by image in fp32, bf16 = the rounded host result, split_sizes and
    image_sizes the host's; process_images_gpu on the same mixed batch returns the same list.  PIL inputs and device tensors."""
    from slime_amd import mm_utils as M
    cfg, proc, imgs, ref = mixed_batch
    inputs = [torch.from_numpy(np.array(im)).to(dev) for im in imgs] if as_tensors else imgs
    crops, split, sizes = M.process_images_gpu_ragged(inputs, proc, cfg, dev)
    assert split == [r.shape[0] for r in ref] and sizes == [im.size for im in imgs]
    assert crops.dtype == torch.float32 and tuple(crops.shape) == (sum(split), 3, 336, 336) and crops.device.type == "cuda"
    for i, (g, r) in enumerate(zip(crops.cpu().split(split), ref)):
        assert torch.equal(g, r), i
    crops16, split16, _ = M.process_images_gpu_ragged(inputs, proc, cfg, dev, dtype=torch.bfloat16)
    assert split16 == split and torch.equal(crops16.cpu(), torch.cat(ref).to(torch.bfloat16))
    got = M.process_images_gpu(inputs, proc, cfg, dev)
    assert isinstance(got, list) and len(got) == len(ref) and all(torch.equal(g.cpu(), r) for g, r in zip(got, ref))
    with pytest.raises(NotImplementedError):
        M.process_images_gpu_ragged(inputs, proc, SimpleNamespace(image_aspect_ratio="pad", image_grid_pinpoints=PIN), dev)


def test_ragged_slicer_matches_reference_goldens(dev):
    """The images of tests/golden/slicer_pixels.npz (the reference's own process_images('anyres') pixels) in ONE ragged call: the
    sample and sum assertions of test_device_slicer_matches_reference_goldens."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    g = np.load(os.path.join(GOLDEN, "slicer_pixels.npz"))
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    arrs = [torch.from_numpy(_rand(int(h), int(w), 100 + i)) for i, (w, h) in enumerate(g["img_specs"])]
    crops, split, _ = M.process_images_gpu_ragged(arrs, ClipImageProcessor(), cfg, dev)
    for i, out in enumerate(crops.cpu().split(split)):
        assert tuple(out.shape) == tuple(g[f"img{i}_anyres_shape"])
        flat = out.reshape(out.shape[0], -1).double()
        assert np.array_equal(flat[:, g["sample_idx"]].float().numpy(), g[f"img{i}_anyres_samples"]), i
        assert np.allclose(flat.sum(1).numpy(), g[f"img{i}_anyres_sum"], rtol=0, atol=1e-6), i


def test_more_than_64_images_split_invisibly(dev, monkeypatch):
    """70 small images of two alternating sizes (crop 32 processor: 3 and 5 crops each): two library calls, one result -- every
    image's crops equal process_anyres_image_gpu's."""
    from slime_amd import mm_utils as M, ops
    from slime_amd.image_processor import ClipImageProcessor
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    proc = ClipImageProcessor(size=32, crop_size=32)
    sizes = [(40, 30), (70, 50)]
    arrs = [torch.from_numpy(_rand(sizes[i % 2][1], sizes[i % 2][0], 500 + i)).to(dev) for i in range(70)]
    calls = []
    real = ops.slice_jobs
    monkeypatch.setattr(ops, "slice_jobs", lambda jobs, *a, **kw: (calls.append(len(jobs)), real(jobs, *a, **kw))[1])
    crops, split, got_sizes = M.process_images_gpu_ragged(arrs, proc, cfg, dev)
    assert calls == [128, 12] and got_sizes == [sizes[i % 2] for i in range(70)]
    assert split == [3, 5] * 35 and crops.shape[0] == sum(split)
    for i, (a, got) in enumerate(zip(arrs, crops.split(split))):
        assert torch.equal(got, M.process_anyres_image_gpu(a, proc, PIN, dev)), i


def test_ragged_crops_feed_encode_images(dev):
    """Hand-over: the flat crops, split_sizes and image_sizes of a three-image mixed batch go straight into
    SlimeVisualEncoder.encode_images (tiny synthetic tower / adapter); the output is identical to feeding the host-sliced pixels."""
    from test_gpu_modules import _tiny_encoder
    from slime_amd import mm_utils as M
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    dtype = torch.bfloat16
    torch.manual_seed(0)
    embed = nn.Embedding(2000, 256).to(dev)
    enc, _, _ = _tiny_encoder(dev, dtype, embed=embed)
    proc = enc.get_vision_tower().image_processor
    cfg = SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=PIN)
    imgs = [Image.fromarray(_rand(h, w, 70 + i), "RGB") for i, (w, h) in enumerate([(336, 336), (640, 480), (300, 900)])]
    crops, split, sizes = M.process_images_gpu_ragged(imgs, proc, cfg, dev, dtype=dtype)
    host = torch.cat(M.process_images(imgs, proc, cfg)).to(dev).to(dtype)
    assert len(set(split)) > 1 and torch.equal(crops, host)
    ids = torch.randint(3, 1900, (3, 12), device=dev)
    ids[:, 4] = IMAGE_TOKEN_INDEX
    am = torch.ones_like(ids)
    a, ss_a = enc.encode_images(crops, input_ids=ids, split_sizes=split, attention_mask=am, image_sizes=sizes)
    b, ss_b = enc.encode_images(host, input_ids=ids, split_sizes=split, attention_mask=am, image_sizes=sizes)
    assert ss_a == ss_b == split and len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
