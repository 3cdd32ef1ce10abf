"""CPU tests of the view-job slicer's host side (slime_resample_*_ex, slime_view_jobs_plan / slime_view_jobs, mm_utils.view_jobs_for):
the LANCZOS tables against Pillow through an integer two-pass emulation, the BICUBIC tables against the existing functions, the job
geometry of every mode against the host functions, the plan, the argument checks (all of which run before any launch) and the
ctypes mirror of the job struct.  Everything is exact.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN

CROP = 16
SEG = 256            # output pixels per workgroup of the horizontal pass (slicer.hip)
PRECISION_BITS = 32 - 8 - 2
BG = (122, 116, 104)
# the (src, dst) sizes of test_gpu_slicer.py's CASES
RESIZE_CASES = [((672, 672), (336, 336)), ((1344, 1344), (336, 336)), ((640, 480), (672, 504)), ((1920, 1080), (1008, 567)),
                ((300, 200), (672, 448)), ((4000, 300), (2352, 177)), ((500, 336), (336, 336)), ((336, 500), (336, 226)),
                ((37, 53), (336, 336)), ((1000, 1000), (672, 672)), ((673, 672), (672, 672)), ((336, 336), (336, 336)),
                ((20000, 9), (64, 9)), ((5, 3), (1, 1)), ((1, 1), (336, 336)), ((5000, 5000), (336, 336))]


def test_ex_tables_with_bicubic_are_the_existing_tables():
    """slime_resample_ksize_ex / slime_resample_coeffs_ex with SLIME_FILTER_BICUBIC return exactly what slime_resample_ksize /
    slime_resample_coeffs return, on every (in -> out) pair of test_gpu_slicer.py's cases (the 20000 -> 64 one takes the malloc
    path); an unknown filter is refused."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    pairs = sorted({(s[i], d[i]) for s, d in RESIZE_CASES for i in (0, 1)})
    assert (20000, 64) in pairs and len(pairs) > 20
    for n_in, n_out in pairs:
        ks = lib.slime_resample_ksize(n_in, n_out)
        assert lib.slime_resample_ksize_ex(n_in, n_out, _lib.FILTER_BICUBIC) == ks
        b0, k0 = np.empty((n_out, 2), np.int32), np.empty((n_out, ks), np.int32)
        assert lib.slime_resample_coeffs(n_in, n_out, b0.ctypes.data, k0.ctypes.data) == 0
        b1, k1 = ops.resample_tables(n_in, n_out, _lib.FILTER_BICUBIC)
        b2, k2 = ops.resample_tables(n_in, n_out)
        assert np.array_equal(b0, b1) and np.array_equal(k0, k1) and np.array_equal(b0, b2) and np.array_equal(k0, k2), (n_in, n_out)
    assert lib.slime_resample_ksize_ex(300, 1024, 2) == 0
    b, k = np.empty((4, 2), np.int32), np.empty((4, 64), np.int32)
    assert lib.slime_resample_coeffs_ex(8, 4, 2, b.ctypes.data, k.ctypes.data) == -1
    assert "SLIME_FILTER_LANCZOS" in lib.slime_last_error().decode()
    # Pillow's kernel size for LANCZOS: support 3.0
    assert lib.slime_resample_ksize_ex(300, 1024, _lib.FILTER_LANCZOS) == 7 and lib.slime_resample_ksize_ex(1344, 1024, _lib.FILTER_LANCZOS) == 9


def _pass(img, bounds, kk, axis):
    """One pass of ImagingResample (8 bpc) over ``axis`` of an [H, W, 3] uint8 array, in integers."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for o in range(bounds.shape[0]):
        lo, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(kk[o, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


@pytest.mark.parametrize("src,dst", [((300, 300), (1024, 1024)), ((322, 322), (1024, 1023)), ((1344, 1344), (1024, 1024)),
                                     ((50, 50), (1024, 1024)), ((37, 37), (64, 64))])
def test_lanczos_tables_reproduce_pillow(src, dst):
    """The LANCZOS tables of slime_resample_coeffs_ex driven through a numpy restatement of Pillow's two integer passes (horizontal,
    rounded to uint8, then vertical) equal Image.resize(dst, Image.LANCZOS) bit for bit."""
    from slime_amd import _lib, ops
    (w, h), (ow, oh) = src, dst
    img = np.random.default_rng(w * 131 + ow).integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.LANCZOS))
    bh, kh = ops.resample_tables(w, ow, _lib.FILTER_LANCZOS)
    bv, kv = ops.resample_tables(h, oh, _lib.FILTER_LANCZOS)
    assert kh.shape[1] == _lib.load().slime_resample_ksize_ex(w, ow, _lib.FILTER_LANCZOS)
    got = _pass(_pass(img, bh, kh, 1), bv, kv, 0)
    assert got.shape == ref.shape and np.array_equal(got, ref)


def _sizes():
    g = np.load(os.path.join(GOLDEN, "slicer_pixels.npz"))
    return [tuple(int(v) for v in s) for s in g["img_specs"]] + [(322, 200), (37, 50), (1000, 30)]


@pytest.mark.parametrize("mode", ["pad", "pad_then_devide", "any_res", None])
def test_view_jobs_for_matches_the_host_functions(mode):
    """mm_utils.view_jobs_for against what the host path does to a blank image of each size: the number of crops, and per job the
    field (the squared view process_image_any_res / process_image_naive / expand2square hand to the processor, the image itself for
    the bare processor) and the resized size (crop x crop for a view the processor resizes, resize_image's size for the LANCZOS
    job, _resize_center_crop's size for the bare processor)."""
    from slime_amd import _lib, mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    from slime_amd.process_image import process_image_any_res, process_image_naive, expand2square, resize_image
    proc = ClipImageProcessor()
    sizes = _sizes()
    assert len(sizes) == 9
    for size in sizes:
        img = Image.new("RGB", size, (255, 255, 255))
        jobs = M.view_jobs_for(mode, size, 336, BG)
        n_crops = sum(j.crops for j in jobs)
        if mode == "pad":
            views = [expand2square(img, BG)]
        elif mode == "any_res":
            views = process_image_any_res(img, BG)
        elif mode == "pad_then_devide":
            views = process_image_naive(img, BG)
        else:
            views = [img]
        assert n_crops == len(views), (mode, size)
        for j in jobs:
            assert all(c == b for c, b in zip(j.bg, BG))
        if mode == "pad_then_devide":
            sq = expand2square(img, BG)
            big = resize_image(sq, 1024)
            assert len(jobs) == 2 and jobs[0].field == jobs[1].field == sq.size
            assert jobs[0].out == (336, 336) and jobs[0].filter == _lib.FILTER_BICUBIC
            assert jobs[1].out == big.size and jobs[1].filter == _lib.FILTER_LANCZOS and jobs[1].crops == len(views) - 1 == 9
            assert jobs[1].windows[:3] == (0, 0, 308) and all(v.size == (336, 336) for v in views[1:])
            # the paste: the white image on the bg field
            assert sq.getbbox() == (0, 0) + sq.size                                   # bg is not black
            px, py = jobs[1].paste
            assert sq.crop((px, py, px + size[0], py + size[1])).getextrema() == ((255, 255),) * 3
            if size == (322, 200):
                assert jobs[1].out == (1024, 1023)
        elif mode in ("pad", "any_res"):
            assert len(jobs) == len(views)
            for j, v in zip(jobs, views):
                assert j.field == v.size and j.out == (336, 336) and j.filter == _lib.FILTER_BICUBIC and j.windows == (0, 0, 336, 1, 1)
                x0, y0, w, h = j.box
                px, py = j.paste
                assert v.crop((px, py, px + w, py + h)).getextrema() == ((255, 255),) * 3       # the box lies where PIL pasted it
                assert (w, h) == v.size or v.getpixel((0, 0)) == BG or v.getpixel((v.size[0] - 1, v.size[1] - 1)) == BG
                assert 0 <= x0 and 0 <= y0 and x0 + w <= size[0] and y0 + h <= size[1]
            if mode == "any_res":                                                      # the boxes are slice_image_any_res's, in its order
                bw, bh = M.cal_num_of_slices(*size)
                W, H = size
                want = [(i * W // bw, j * H // bh, (i + 1) * W // bw, (j + 1) * H // bh) for j in range(bh) for i in range(bw)]
                assert [(b[0], b[1], b[0] + b[2], b[1] + b[3]) for b in (j.box for j in jobs[1:])] == want and jobs[0].box == (0, 0, W, H)
        else:
            (j,) = jobs
            w, h = size
            short, long = (w, h) if w <= h else (h, w)
            nl = int(336 * long / short)
            assert j.field == size and j.paste == (0, 0) and j.box == (0, 0, w, h)
            assert j.out == ((336, nl) if w <= h else (nl, 336)) and j.filter == _lib.FILTER_BICUBIC
            assert j.windows == ((j.out[0] - 336) // 2, (j.out[1] - 336) // 2, 336, 1, 1)
            assert proc._resize_center_crop(img).shape == (336, 336, 3)


def test_pad_then_devide_height_follows_the_reference_expression():
    """int(float(S) * float(1024 / float(S))) is 1023, not 1024, for 2504 of the sides below 20000; the window count comes from the real
    height and stays 3 x 3."""
    from slime_amd import mm_utils as M
    short = [s for s in range(1, 20000) if M.view_jobs_for("pad_then_devide", (s, s), 336, BG)[1].out[1] == 1023]
    assert len(short) == 2504 and short[:4] == [49, 98, 103, 107] and {161, 187, 322, 347} <= set(short) and 336 not in short
    assert M.view_jobs_for("pad_then_devide", (322, 200), 336, BG)[1].out == (1024, 1023)
    assert M.view_jobs_for("pad_then_devide", (322, 200), 336, BG)[1].windows == (0, 0, 308, 3, 3)
    with pytest.raises(ValueError, match="336"):
        M.view_jobs_for("pad_then_devide", (322, 200), 224, BG)


def test_device_path_needs_shortest_edge_equal_to_crop():
    from types import SimpleNamespace
    from slime_amd import mm_utils as M
    from slime_amd.image_processor import ClipImageProcessor
    with pytest.raises(ValueError, match="shortest_edge 384.*336x336"):
        M.process_images_device([Image.new("RGB", (40, 30))], ClipImageProcessor(size=384, crop_size=336),
                                SimpleNamespace(image_aspect_ratio="pad"), "cpu")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def _job(img=(40, 50), box=None, field=None, paste=(0, 0), out=(16, 16), filt=0, win=(0, 0, 16, 1, 1), first_crop=0, tables=True,
         stride=None):
    """A job with dummy non-null addresses (the functions under test never dereference them) and the right ksize values.  Sizes are
    (w, h); box (x0, y0, w, h); win (x0, y0, step, nx, ny)."""
    from slime_amd import _lib
    lib = _lib.load()
    J = _lib.ViewJob()
    box = (0, 0) + img if box is None else box
    field = box[2:] if field is None else field
    J.img, J.img_stride, J.img_h, J.img_w = 0x1000, (img[0] * 3 if stride is None else stride), img[1], img[0]
    J.box_x0, J.box_y0, J.box_w, J.box_h = box
    (J.field_w, J.field_h), (J.paste_x, J.paste_y) = field, paste
    J.bg[0], J.bg[1], J.bg[2] = BG
    (J.out_w, J.out_h), J.filter = out, filt
    J.win_x0, J.win_y0, J.win_step, J.win_nx, J.win_ny = win
    J.first_crop = first_crop
    if tables and out[0] != field[0]:
        J.bounds_h, J.kk_h, J.ksize_h = 0x2000, 0x3000, lib.slime_resample_ksize_ex(field[0], out[0], filt)
    if tables and out[1] != field[1]:
        J.bounds_v, J.kk_v, J.ksize_v = 0x4000, 0x5000, lib.slime_resample_ksize_ex(field[1], out[1], filt)
    return J


def _table(jobs):
    from slime_amd import _lib
    t = (_lib.ViewJob * len(jobs))()
    for i, j in enumerate(jobs):
        C.memmove(C.byref(t[i]), C.byref(j), C.sizeof(_lib.ViewJob))
    return t


def _plan(table, crop=CROP):
    from slime_amd import _lib
    tmp = C.c_size_t(12345)
    rc = _lib.load().slime_view_jobs_plan(table, len(table), crop, C.byref(tmp))
    return rc, tmp.value


def test_plan_lays_out_intermediates_and_workgroups():
    """slime_view_jobs_plan: an intermediate [field_h, out_w, 3] only for jobs that run both passes, at 16-byte aligned, disjoint
    offsets, tmp_bytes = the sum of the 16-byte-rounded sizes; h_block0 / v_block0 = exclusive prefix sums of the workgroup counts
    restated here: launch 1 has ceil(columns the windows cover / 256) * field_h workgroups for a both-pass job and none otherwise,
    launch 2 one per window row, win_nx * win_ny * crop."""
    jobs = [
        _job((40, 50), field=(50, 50), paste=(5, 0), out=(16, 16)),                                     # both passes
        _job((16, 16), out=(16, 16), first_crop=1),                                                     # neither
        _job((40, 50), out=(40, 32), win=(3, 0, 8, 2, 3), first_crop=2),                                # vertical only, 6 windows
        _job((700, 9), out=(1024, 20), filt=1, win=(0, 0, 308, 3, 1), first_crop=8),                    # both, 3 segments (632 + 16 columns)
        _job((40, 16), out=(32, 16), win=(16, 0, 16, 1, 1), first_crop=11),                             # horizontal only
        _job((30, 30), box=(3, 4, 20, 10), field=(20, 20), paste=(0, 5), out=(600, 17), win=(300, 1, 16, 1, 1), first_crop=12),  # both, 1 segment
    ]
    t = _table(jobs)
    rc, tmp_bytes = _plan(t)
    assert rc == 0
    ranges, h0, v0, total = [], 0, 0, 0
    for J in t:
        both = J.out_w != J.field_w and J.out_h != J.field_h
        assert (J.h_block0, J.v_block0) == (h0, v0)
        if both:
            size = J.field_h * J.out_w * 3
            assert J.tmp_offset % 16 == 0
            ranges.append((J.tmp_offset, J.tmp_offset + size))
            total += (size + 15) // 16 * 16
            cols = (J.win_nx - 1) * J.win_step + CROP
            h0 += (cols + SEG - 1) // SEG * J.field_h
        else:
            assert J.tmp_offset == 0
        v0 += J.win_nx * J.win_ny * CROP
    assert len(ranges) == 3 and tmp_bytes == total and h0 == 50 + 3 * 9 + 20
    ranges.sort()
    assert ranges[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] <= tmp_bytes
    rc, tmp_bytes = _plan(_table([jobs[1], jobs[2], jobs[4]]))
    assert rc == 0 and tmp_bytes == 0


def test_view_jobs_checks_its_arguments_on_the_host():
    """slime_view_jobs returns SLIME_EINVAL naming the limit for every refusal the header lists, and SLIME_EWORKSPACE for a short or
    misaligned tmp, all before anything is launched (every pointer here is a dummy)."""
    from slime_amd import _lib
    lib = _lib.load()
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)

    def run(jobs, plan=True, n=None, out_crops=64, out_dtype=_lib.F32, tmp=0x6000, tmp_bytes=1 << 30, crop=CROP):
        t = _table(jobs)
        if plan:
            _plan(t, crop)                      # may itself refuse (then slime_view_jobs must refuse too)
        rc = lib.slime_view_jobs(t, 0x7000, len(jobs) if n is None else n, crop, mean, std, 0x8000, out_crops, out_dtype, tmp, tmp_bytes, None)
        return rc, lib.slime_last_error().decode()

    good = _job((40, 50), field=(50, 50), paste=(5, 0), out=(20, 24), win=(2, 3, 2, 2, 3))

    def bad_ksize(vertical):
        J = _job((40, 50), out=(20, 24))
        if vertical:
            J.ksize_v += 1
        else:
            J.ksize_h -= 1
        return J

    lanczos_with_bicubic_ksize = _job((40, 50), out=(20, 24), filt=0)
    lanczos_with_bicubic_ksize.filter = 1
    unplanned = _job((40, 50), out=(20, 24), first_crop=6)
    cases = [
        (dict(jobs=[good], n=0), "SLIME_VIEW_MAX_JOBS = 128"),
        (dict(jobs=[_job((16, 16), first_crop=i) for i in range(129)], out_crops=200), "SLIME_VIEW_MAX_JOBS = 128"),
        (dict(jobs=[_job((0, 50), box=(0, 0, 4, 4))]), "empty image, box, field or output"),
        (dict(jobs=[_job((40, 50), box=(0, 0, 0, 4), field=(16, 16))]), "empty image, box, field or output"),
        (dict(jobs=[_job((40, 50), field=(50, 0))]), "empty image, box, field or output"),
        (dict(jobs=[_job((40, 50), out=(16, 0))]), "empty image, box, field or output"),
        (dict(jobs=[_job((40, 50), box=(30, 0, 11, 50))]), "leaves the 50x40 image"),
        (dict(jobs=[_job((40, 50), box=(0, 41, 40, 10))]), "leaves the 50x40 image"),
        (dict(jobs=[_job((40, 50), box=(-1, 0, 40, 50))]), "leaves the 50x40 image"),
        (dict(jobs=[_job((40, 50), field=(50, 50), paste=(11, 0))]), "leaves the 50x50 field"),
        (dict(jobs=[_job((40, 50), field=(50, 50), paste=(0, 1))]), "leaves the 50x50 field"),
        (dict(jobs=[_job((40, 50), field=(50, 50), paste=(-1, 0))]), "leaves the 50x50 field"),
        (dict(jobs=[_job((40, 50), out=(20, 24), win=(5, 0, 16, 1, 1))]), "leave the 24x20 resized image"),
        (dict(jobs=[_job((40, 50), out=(20, 24), win=(0, 0, 8, 1, 3))]), "leave the 24x20 resized image"),
        (dict(jobs=[_job((40, 50), out=(20, 24), win=(0, -1, 8, 1, 1))]), "leave the 24x20 resized image"),
        (dict(jobs=[_job((40, 50), win=(0, 0, 16, 0, 1))]), "must be positive"),
        (dict(jobs=[_job((40, 50), win=(0, 0, 16, 1, -2))]), "must be positive"),
        (dict(jobs=[_job((40, 50), win=(0, 0, 0, 1, 1))]), "must be positive"),
        (dict(jobs=[_job((40, 50), filt=2, tables=False)]), "filter 2 is not SLIME_FILTER_BICUBIC / SLIME_FILTER_LANCZOS"),
        (dict(jobs=[_job((40, 50), out=(20, 50), win=(0, 0, 16, 1, 1), tables=False)]), "horizontal tables missing"),
        (dict(jobs=[_job((40, 50), out=(40, 24), tables=False)]), "vertical tables missing"),
        (dict(jobs=[bad_ksize(False)]), "horizontal tables missing or ksize"),
        (dict(jobs=[bad_ksize(True)]), "vertical tables missing or ksize"),
        (dict(jobs=[lanczos_with_bicubic_ksize]), "horizontal tables missing or ksize 9 != 13"),
        (dict(jobs=[good, _job((16, 16), first_crop=5)]), "overlap"),
        (dict(jobs=[_job((16, 16), first_crop=3), _job((40, 50), out=(20, 24), win=(0, 0, 2, 2, 3), first_crop=0)]), "overlap"),
        (dict(jobs=[good], out_crops=5), "outside the output's [0, 5)"),
        (dict(jobs=[_job((16, 16), first_crop=-1)]), "outside the output's"),
        (dict(jobs=[_job((40, 50), stride=119)]), "row stride 119 smaller than a row of 120"),
        (dict(jobs=[good], out_dtype=_lib.U8), "not F32 / BF16 / F16"),
        (dict(jobs=[_job((16, 16)), unplanned], plan=False), "slime_view_jobs_plan"),
        (dict(jobs=[_job((70000, 70000), out=(70000, 70000), win=(0, 0, 1, 50000, 50000))], out_crops=1 << 40), "more than 2^31 - 1 workgroups"),
    ]
    for kw, word in cases:
        rc, msg = run(**kw)
        assert rc == -1, (kw, msg)                                               # SLIME_EINVAL
        assert word in msg, (word, msg)
    # a plan made for another order of the same jobs is not this table's plan
    a, b = _job((40, 50), out=(20, 24), first_crop=0), _job((600, 50), out=(32, 48), first_crop=6)
    t = _table([a, b])
    assert _plan(t)[0] == 0
    swapped = _table([t[1], t[0]])
    assert lib.slime_view_jobs(swapped, 0x7000, 2, CROP, mean, std, 0x8000, 64, _lib.F32, 0x6000, 1 << 30, None) == -1
    assert "slime_view_jobs_plan" in lib.slime_last_error().decode()
    # a valid table passes every argument check and stops at the workspace: nothing was launched
    need = (50 * 20 * 3 + 15) // 16 * 16
    for kw in (dict(tmp_bytes=need - 1), dict(tmp=0), dict(tmp=0x6004)):
        rc, msg = run([good], **kw)
        assert rc == -2 and f"tmp needs {need} bytes" in msg, (kw, rc, msg)      # SLIME_EWORKSPACE
    # the plan refuses what it cannot lay out, naming the same limits
    rc, _ = _plan(_table([_job((40, 50), out=(20, 24), win=(5, 0, 16, 1, 1))]))
    assert rc == -1 and "leave the 24x20 resized image" in lib.slime_last_error().decode()


def test_view_job_mirror_matches_the_header_layout(tmp_path):
    """_lib.ViewJob against slime_view_job: sizeof / offsetof printed by a C program compiled against the header, field by field, the
    job cap and the filter codes."""
    import re
    import shutil
    import subprocess
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"}\s*slime_view_job\s*;", text)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(slime_view_job));', 'printf("max_jobs %d\\n", (int)SLIME_VIEW_MAX_JOBS);',
             'printf("bicubic %d\\n", (int)SLIME_FILTER_BICUBIC);', 'printf("lanczos %d\\n", (int)SLIME_FILTER_LANCZOS);',
             'printf("abi %d\\n", (int)SLIME_ABI_VERSION);']
    for fname, _ in _lib.ViewJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(slime_view_job, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.ViewJob)
    assert int(got["max_jobs"]) == _lib.VIEW_MAX_JOBS == 128
    assert (int(got["bicubic"]), int(got["lanczos"])) == (_lib.FILTER_BICUBIC, _lib.FILTER_LANCZOS) == (0, 1)
    assert int(got["abi"]) == _lib.ABI_VERSION == 7                               # new entry points only
    struct_body = text[:text.index("} slime_view_job")]
    struct_body = struct_body[struct_body.rindex("typedef struct"):]
    declared = [f for f in re.findall(r"\b([a-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", struct_body)]
    assert declared == [f for f, _ in _lib.ViewJob._fields_]                      # every field, in the header's order
    for fname, _ in _lib.ViewJob._fields_:
        assert int(got[fname]) == getattr(_lib.ViewJob, fname).offset, fname
    assert C.sizeof(_lib.ViewJob._fields_[12][1]) == 3 and _lib.ViewJob._fields_[12][0] == "bg"
