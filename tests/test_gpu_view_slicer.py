"""GPU tests of the view-job slicer (slime_view_jobs; ops.view_jobs, mm_utils.process_images_device): the 'pad', 'pad_then_devide',
'any_res' and bare-processor modes of process_images on the device.  Every comparison is exact (torch.equal / np.array_equal):
against the host process_images, against Pillow on the materialised padded field, and against the reference-generated pixel goldens
(whose checksum keeps the atol of test_device_slicer_matches_reference_goldens)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"
MODES = ["pad", "pad_then_devide", "any_res", None]
SIZES = [(300, 200), (200, 300),     # padding on either axis, upscale
         (336, 336),                 # no pass at all
         (322, 200),                 # the 1023-row Lanczos
         (37, 50),                   # tiny source, every tap clipped
         (1000, 30),                 # the field is almost all background
         (640, 480), (672, 672)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _cfg(mode):
    return SimpleNamespace(image_aspect_ratio=mode, image_grid_pinpoints=PIN)


_HOST = {}


def _host(mode, size):
    """(pixels, process_images([image])[0]) of the random image of ``size`` under ``mode``: computed once, never modified."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    key = (mode, size)
    if key not in _HOST:
        w, h = size
        px = _rand(h, w, w * 31 + h)
        ref = M.process_images([Image.fromarray(px, "RGB")], ClipImageProcessor(), _cfg(mode))
        assert isinstance(ref, torch.Tensor) and ref.shape[0] == 1 and ref.dtype == torch.float32
        _HOST[key] = (px, ref)
    return _HOST[key]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_modes_equal_the_host_path(dev, mode, size):
    """process_images_device == process_images bit for bit in fp32, == the rounded host result in bf16 / fp16; PIL inputs and device
    uint8 tensors."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    proc = ClipImageProcessor()
    px, ref = _host(mode, size)
    got = M.process_images_device([Image.fromarray(px, "RGB")], proc, _cfg(mode), dev)
    assert isinstance(got, torch.Tensor) and got.device.type == "cuda" and got.dtype == torch.float32 and got.shape == ref.shape
    assert torch.equal(got.cpu(), ref), int((got.cpu() != ref).sum())
    t = torch.from_numpy(px).to(dev)
    assert torch.equal(M.process_images_device([t], proc, _cfg(mode), dev).cpu(), ref)
    for dtype in (torch.bfloat16, torch.float16):
        got16 = M.process_images_device([t], proc, _cfg(mode), dev, dtype=dtype)
        assert got16.dtype == dtype and torch.equal(got16.cpu(), ref.to(dtype)), dtype


def test_padding_takes_part_in_the_resampling():
    """The 300 x 200 'pad' case tells "pad, then resize" (the definition) from "resize, then pad": the host results differ, so the
    comparison above is not blind to the order.  (CPU only; it guards the test, not the kernel.)"""
    from slime_amd.image_processor import ClipImageProcessor
    from slime_amd.process_image import expand2square
    proc = ClipImageProcessor()
    bg = tuple(int(m * 255) for m in proc.image_mean)
    px, ref = _host("pad", (300, 200))
    img = Image.fromarray(px, "RGB")
    late = expand2square(img.resize((336, 224)), bg)
    assert late.size == (336, 336) and not np.array_equal(proc.normalize_u8(np.asarray(late)), ref[0].numpy())


@pytest.mark.parametrize("mode", ["pad", "any_res", "pad_then_devide"])
def test_modes_match_reference_goldens(dev, mode):
    """The six images of tests/golden/slicer_pixels.npz (the reference's own process_images pixels), per mode: shapes equal, samples
    equal exactly, sums within the atol of test_device_slicer_matches_reference_goldens."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    g = np.load(os.path.join(GOLDEN, "slicer_pixels.npz"))
    proc = ClipImageProcessor()
    assert len(g["img_specs"]) == 6
    for i, (w, h) in enumerate(g["img_specs"]):
        out = M.process_images_device([torch.from_numpy(_rand(int(h), int(w), 100 + i))], proc, _cfg(mode), dev).cpu()
        out = out[0] if out.dim() == 5 else out
        assert tuple(out.shape) == tuple(g[f"img{i}_{mode}_shape"]), (i, mode)
        flat = out.reshape(out.shape[0], -1).double()
        assert np.array_equal(flat[:, g["sample_idx"]].float().numpy(), g[f"img{i}_{mode}_samples"]), (i, mode)
        assert np.allclose(flat.sum(1).numpy(), g[f"img{i}_{mode}_sum"], rtol=0, atol=1e-6), (i, mode)


@pytest.mark.parametrize("mode", MODES)
def test_batch_of_different_sizes(dev, mode):
    """One call over images of different sizes: the return type (stacked tensor or list) and the values are process_images'."""
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    proc = ClipImageProcessor()
    sizes = [(300, 200), (37, 50), (640, 480), (336, 336)]
    imgs = [Image.fromarray(_rand(h, w, 900 + i), "RGB") for i, (w, h) in enumerate(sizes)]
    ref = M.process_images(imgs, proc, _cfg(mode))
    got = M.process_images_device(imgs, proc, _cfg(mode), dev)
    assert isinstance(ref, list) == (mode == "any_res")                       # 640 x 480 has more slices than the small ones
    if isinstance(ref, list):
        assert isinstance(got, list) and len(got) == len(ref)
        for a, b in zip(got, ref):
            assert a.device.type == "cuda" and torch.equal(a.cpu(), b)
        assert all(a.untyped_storage().data_ptr() == got[0].untyped_storage().data_ptr() for a in got)   # views of one buffer
    else:
        assert isinstance(got, torch.Tensor) and got.shape == ref.shape and torch.equal(got.cpu(), ref)


def test_more_than_128_jobs_split_invisibly(dev, monkeypatch):
    """19 'any_res' images of 1344 x 1344 (7 views each: 133 jobs, two library calls -- 17 such images are only 119) of two
    alternating contents: every image's crops equal the host's."""
    from slime_amd import _lib, mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    proc = ClipImageProcessor()
    px = [_rand(1344, 1344, 40), _rand(1344, 1344, 41)]
    ref = [M.process_images([Image.fromarray(p, "RGB")], proc, _cfg("any_res"))[0] for p in px]
    assert ref[0].shape == (7, 3, 336, 336) and not torch.equal(ref[0], ref[1])
    calls = []
    lib = _lib.load()
    real = lib.slime_view_jobs
    monkeypatch.setattr(lib, "slime_view_jobs", lambda t, d, n, *a: (calls.append(n), real(t, d, n, *a))[1])
    arrs = [torch.from_numpy(px[i % 2]).to(dev) for i in range(19)]
    got = M.process_images_device(arrs, proc, _cfg("any_res"), dev)
    assert calls == [128, 5] and got.shape == (19, 7, 3, 336, 336)
    got = got.cpu()
    for i in range(19):
        assert torch.equal(got[i], ref[i % 2]), i


def test_anyres_is_process_images_gpu(dev):
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    proc = ClipImageProcessor()
    imgs = [Image.fromarray(_rand(h, w, 60 + i), "RGB") for i, (w, h) in enumerate([(300, 200), (640, 480)])]
    a = M.process_images_device(imgs, proc, _cfg("anyres"), dev)
    b = M.process_images_gpu(imgs, proc, _cfg("anyres"), dev)
    assert type(a) is type(b) and len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ---- the primitive ---------------------------------------------------------------------------------------------------------------------
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
BG = (122, 116, 104)
SENTINEL = (255, 0, 255)


def _pillow_view(img, spec, crop):
    """The definition: materialise the field, Image.resize, crop the windows, normalise (fp32) -> [n, 3, crop, crop]."""
    from slime_amd.image_processor import ClipImageProcessor
    x0, y0, w, h = spec.box
    field = np.empty((spec.field[1], spec.field[0], 3), dtype=np.uint8)
    field[:] = np.array(spec.bg, dtype=np.uint8)
    field[spec.paste[1]:spec.paste[1] + h, spec.paste[0]:spec.paste[0] + w] = img[y0:y0 + h, x0:x0 + w]
    big = np.asarray(Image.fromarray(field, "RGB").resize(spec.out, Image.LANCZOS if spec.filter == 1 else Image.BICUBIC))
    assert big.shape[:2] == (spec.out[1], spec.out[0])
    wx, wy, step, nx, ny = spec.windows
    proc = ClipImageProcessor(image_mean=MEAN, image_std=STD)
    return torch.from_numpy(np.stack([proc.normalize_u8(big[wy + j * step:wy + j * step + crop, wx + i * step:wx + i * step + crop])
                                      for j in range(ny) for i in range(nx)]))


def _specs():
    """(name, image (w, h), ViewSpec) at crop 16: every branch of the two kernels.  The images are filled with SENTINEL outside the
    box, so a byte read from outside the box changes the result."""
    from slime_amd.ops import ViewSpec as V
    return [
        ("both passes, padded left/right, bicubic", (40, 50), V((0, 0, 40, 50), (50, 50), (5, 0), BG, (23, 29), 0, (1, 2, 5, 2, 3))),
        ("both passes, padded top/bottom, lanczos up-scale", (50, 20), V((0, 0, 50, 20), (50, 50), (0, 15), BG, (64, 61), 1, (0, 3, 21, 3, 3))),
        ("vertical only (out_w == field_w), padded, 150-byte rows", (30, 40), V((0, 0, 30, 40), (50, 40), (10, 0), BG, (50, 64), 0, (1, 2, 7, 5, 7))),
        ("vertical only, lanczos down-scale, aligned rows", (64, 90), V((0, 0, 64, 90), (64, 100), (0, 4), BG, (64, 33), 1, (0, 0, 16, 4, 2))),
        ("horizontal only (out_h == field_h), padded both ways", (30, 30), V((0, 0, 30, 30), (50, 40), (10, 6), BG, (80, 40), 0, (3, 1, 11, 6, 3))),
        ("horizontal only, lanczos down-scale", (90, 16), V((0, 0, 90, 16), (100, 16), (7, 0), BG, (37, 16), 1, (0, 0, 7, 4, 1))),
        ("no pass, padded: a copy of the field", (20, 30), V((0, 0, 20, 30), (40, 40), (13, 7), BG, (40, 40), 0, (0, 0, 6, 5, 5))),
        ("box at an odd byte offset inside a larger image, both passes", (64, 48), V((5, 3, 21, 17), (31, 31), (5, 9), BG, (40, 45), 0, (0, 0, 12, 3, 3))),
        ("box inside a larger image, vertical only", (64, 48), V((7, 1, 21, 17), (21, 23), (0, 3), BG, (21, 40), 1, (5, 0, 8, 1, 4))),
        ("box inside a larger image, horizontal only", (64, 48), V((9, 30, 21, 17), (27, 17), (3, 0), BG, (50, 17), 0, (0, 1, 17, 3, 1))),
        ("box inside a larger image, copy", (64, 48), V((43, 31, 21, 17), (21, 17), (0, 0), BG, (21, 17), 0, (5, 1, 16, 1, 1))),
        ("two segments, windows start past the first", (100, 60), V((0, 0, 100, 60), (110, 60), (4, 0), BG, (900, 330), 0, (301, 5, 290, 2, 2))),
        ("span over 48 KiB: direct loads", (17000, 4), V((3, 0, 16990, 4), (17000, 8), (5, 2), BG, (16, 16), 0, (0, 0, 16, 1, 1))),
        ("1 x 1 box on a field", (3, 3), V((1, 1, 1, 1), (3, 3), (1, 1), BG, (16, 16), 1, (0, 0, 16, 1, 1))),
    ]


def test_view_jobs_primitive_matches_pillow(dev):
    """ops.view_jobs at crop 16, all jobs in ONE call, the output pre-filled with NaN: every job's crops equal the definition
    (Pillow on the materialised field -- so the SENTINEL pixels around a box did not leak in); owned crops hold no NaN; crops no job
    owns are untouched.  The first_crop values run against the job order and leave gaps; one image is a strided view, one is not
    packed."""
    from slime_amd import ops
    specs = _specs()
    total = sum(s.crops for _, _, s in specs) + 5
    out = torch.full((total, 3, 16, 16), float("nan"), dtype=torch.float32, device=dev)
    jobs, want, first = [], [], total
    for i, (name, (w, h), spec) in enumerate(specs):
        img = np.empty((h, w, 3), dtype=np.uint8)
        img[:] = np.array(SENTINEL, dtype=np.uint8)
        x0, y0, bw, bh = spec.box
        img[y0:y0 + bh, x0:x0 + bw] = _rand(bh, bw, 2000 + i)
        first -= spec.crops + (1 if i % 3 == 0 else 0)                          # a gap before some jobs
        t = torch.from_numpy(img).to(dev)
        if i == 0:                                                                # rows of a wider buffer: used as it is, stride > row
            wide = torch.zeros((h, w + 5, 3), dtype=torch.uint8, device=dev)
            wide[:, :w] = t
            t = wide[:, :w]
            assert not t.is_contiguous() and t.stride(1) == 3
        elif i == 2:                                                              # every second pixel of a buffer: view_jobs packs a copy
            sparse = torch.zeros((h, 2 * w, 3), dtype=torch.uint8, device=dev)
            sparse[:, ::2] = t
            t = sparse[:, ::2]
            assert t.stride(1) == 6
        jobs.append((t, spec, first))
        want.append((name, first, _pillow_view(img, spec, 16)))
    assert first == 0
    ops.view_jobs(jobs, 16, MEAN, STD, out)
    got = out.cpu()
    owned = torch.zeros(total, dtype=torch.bool)
    for name, first, ref in want:
        mine = got[first:first + ref.shape[0]]
        owned[first:first + ref.shape[0]] = True
        assert not torch.isnan(mine).any(), name
        assert torch.equal(mine, ref), (name, int((mine != ref).sum()))
    assert int((~owned).sum()) == 5 and bool(torch.isnan(got[~owned]).all())
    # the 16-bit outputs are the rounded fp32 ones
    for dtype in (torch.bfloat16, torch.float16):
        out16 = torch.zeros((total, 3, 16, 16), dtype=dtype, device=dev)
        ops.view_jobs(jobs, 16, MEAN, STD, out16)
        assert torch.equal(out16.cpu()[owned], got[owned].to(dtype)), dtype


def test_overlapping_windows_of_an_unresized_field(dev):
    """Step 308 on a 1024 x 1024 field at crop 336: nine overlapping windows, no resampling pass -- the crops are the normalised
    pixels themselves; a tenth crop nobody owns keeps its NaN."""
    from slime_amd import ops
    from slime_amd.ops import ViewSpec as V
    img = _rand(1024, 1024, 77)
    spec = V((0, 0, 1024, 1024), (1024, 1024), (0, 0), BG, (1024, 1024), 1, (0, 0, 308, 3, 3))
    out = torch.full((10, 3, 336, 336), float("nan"), dtype=torch.float32, device=dev)
    ops.view_jobs([(torch.from_numpy(img).to(dev), spec, 1)], 336, MEAN, STD, out)
    got = out.cpu()
    assert torch.equal(got[1:], _pillow_view(img, spec, 336)) and bool(torch.isnan(got[0]).all())


def test_pad_crops_feed_encode_images(dev):
    """Hand-over: process_images_device(..., 'pad') feeds straight into SlimeVisualEncoder.encode_images (tiny synthetic tower /
    adapter); the output is identical to feeding the host-preprocessed pixels moved to the device."""
    from test_gpu_modules import _tiny_encoder
    from slime_amd import mm_utils as M
    dtype = torch.bfloat16
    enc, _, _ = _tiny_encoder(dev, dtype)
    proc = enc.get_vision_tower().image_processor
    imgs = [Image.fromarray(_rand(h, w, 70 + i), "RGB") for i, (w, h) in enumerate([(300, 200), (336, 336), (37, 50)])]
    crops = M.process_images_device(imgs, proc, _cfg("pad"), dev, dtype=dtype)
    host = M.process_images(imgs, proc, _cfg("pad")).to(dev).to(dtype)
    assert crops.shape == (3, 3, 336, 336) and torch.equal(crops, host)
    a, _ = enc.encode_images(crops)
    b, _ = enc.encode_images(host)
    assert a.shape == b.shape and a.shape[0] == 3 and torch.equal(a, b)
