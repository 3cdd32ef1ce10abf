"""CPU tests of the job-table slicer's host side (slime_slice_jobs_plan / slime_slice_jobs, mm_utils.anyres_geometry): the plan, the
integer geometry against PIL, the argument checks (all of which run before any launch) and the ctypes mirror of the job struct.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN

PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"
CROP = 16
SEG = 256            # output pixels per workgroup of the horizontal pass (slicer.hip)


def _job(src_h, src_w, out_h, out_w, canvas_h, canvas_w, x0=0, y0=0, first_crop=0, tables=True, stride=None):
    """A job with dummy non-null addresses (the functions under test never dereference them) and the right ksize values."""
    from slime_amd import _lib
    lib = _lib.load()
    J = _lib.SliceJob()
    J.src, J.src_stride, J.src_h, J.src_w = 0x1000, (src_w * 3 if stride is None else stride), src_h, src_w
    J.out_h, J.out_w, J.canvas_h, J.canvas_w, J.x0, J.y0, J.first_crop = out_h, out_w, canvas_h, canvas_w, x0, y0, first_crop
    if tables and out_w != src_w:
        J.bounds_h, J.kk_h, J.ksize_h = 0x2000, 0x3000, lib.slime_resample_ksize(src_w, out_w)
    if tables and out_h != src_h:
        J.bounds_v, J.kk_v, J.ksize_v = 0x4000, 0x5000, lib.slime_resample_ksize(src_h, out_h)
    return J


def _table(jobs):
    from slime_amd import _lib
    t = (_lib.SliceJob * len(jobs))()
    for i, j in enumerate(jobs):
        C.memmove(C.byref(t[i]), C.byref(j), C.sizeof(_lib.SliceJob))
    return t


def _plan(table, crop=CROP):
    from slime_amd import _lib
    tmp = C.c_size_t(12345)
    rc = _lib.load().slime_slice_jobs_plan(table, len(table), crop, C.byref(tmp))
    return rc, tmp.value


def _mixed_jobs():
    """All four pass combinations, twice, interleaved; canvases of 1 to 6 tiles; crop ranges packed in job order."""
    shapes = [
        (37, 23, 20, 14, 32, 48),        # both passes
        (16, 16, 16, 16, 16, 16),        # neither
        (9, 7, 32, 7, 32, 16),           # vertical only
        (4, 701, 8, 304, 16, 304),       # both, two horizontal segments
        (16, 40, 16, 32, 16, 32),        # horizontal only
        (50, 600, 48, 32, 48, 32),       # both
        (20, 20, 20, 20, 32, 32),        # neither, padded
        (5, 5, 5, 16, 16, 16),           # horizontal only
    ]
    jobs, first = [], 0
    for s in shapes:
        jobs.append(_job(*s, first_crop=first))
        first += (s[4] // CROP) * (s[5] // CROP)
    return jobs, first


def test_plan_lays_out_intermediates_and_workgroups():
    """slime_slice_jobs_plan: an intermediate [src_h, out_w, 3] only for jobs that run both passes, at 16-byte aligned, disjoint
    offsets, tmp_bytes = the sum of the 16-byte-rounded sizes; h_block0 / v_block0 = exclusive prefix sums of the workgroup counts
    restated here: launch 1 has ceil(out_w / 256) * src_h workgroups for a both-pass job and none otherwise, launch 2 one per canvas row
    and tile column, canvas_h * (canvas_w / crop)."""
    jobs, _ = _mixed_jobs()
    t = _table(jobs)
    rc, tmp_bytes = _plan(t)
    assert rc == 0
    ranges, h0, v0, total = [], 0, 0, 0
    for J in t:
        both = J.out_w != J.src_w and J.out_h != J.src_h
        assert (J.h_block0, J.v_block0) == (h0, v0)
        if both:
            size = J.src_h * J.out_w * 3
            assert J.tmp_offset % 16 == 0
            ranges.append((J.tmp_offset, J.tmp_offset + size))
            total += (size + 15) // 16 * 16
            h0 += (J.out_w + SEG - 1) // SEG * J.src_h
        else:
            assert J.tmp_offset == 0
        v0 += J.canvas_h * (J.canvas_w // CROP)
    assert len(ranges) == 3 and tmp_bytes == total
    ranges.sort()
    assert ranges[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and ranges[-1][1] <= tmp_bytes
    # no job runs both passes: no tmp at all
    rc, tmp_bytes = _plan(_table([jobs[1], jobs[2], jobs[4]]))
    assert rc == 0 and tmp_bytes == 0


def _sizes():
    g = np.load(os.path.join(GOLDEN, "slicer_grid.npz"))
    return [tuple(int(v) for v in s) for s in g["sizes"]] + [(336, 336), (672, 672), (4000, 300)]


def test_anyres_geometry_matches_pil_and_the_grid_rule():
    """mm_utils.anyres_geometry over the golden grid's 56 sizes and three more: the resized size and paste origin are what
    resize_and_pad_image (PIL, CPU) produces -- the bounding box of a white image on its black canvas --, the canvas is
    get_anyres_image_grid_shape's grid of crops, and n_local is the tile count."""
    from slime_amd import mm_utils as M
    sizes = _sizes()
    assert len(sizes) == 59
    for size in sizes:
        tw, th, nw, nh, x0, y0, n_local = M.anyres_geometry(size, 336)
        assert (tw, th) == tuple(M.select_best_resolution_uhd(size, (336, 336)))
        canvas = M.resize_and_pad_image(Image.new("RGB", size, (255, 255, 255)), (tw, th))
        assert canvas.size == (tw, th)
        assert canvas.getbbox() == (x0, y0, x0 + nw, y0 + nh), size
        gw, gh = M.get_anyres_image_grid_shape(size, PIN, 336)
        assert (gw, gh) == (tw // 336, th // 336) and n_local == gw * gh == len(M.divide_to_patches(canvas, 336)), size


def test_slice_jobs_checks_its_arguments_on_the_host():
    """slime_slice_jobs returns SLIME_EINVAL naming the limit -- job count, canvas not a multiple of crop, paste rectangle outside the
    canvas, missing tables / wrong ksize per pass, crop ranges overlapping or outside the output, stride below a row, output type, a
    table the plan did not fill -- and SLIME_EWORKSPACE for a short tmp, all before anything is launched (dummy pointers)."""
    from slime_amd import _lib
    lib = _lib.load()
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.25, 0.25, 0.25)

    def run(jobs, plan=True, n=None, out_crops=64, out_dtype=_lib.F32, tmp=0x6000, tmp_bytes=1 << 30, crop=CROP):
        t = _table(jobs)
        if plan:
            _plan(t, crop)                      # may itself refuse (then slime_slice_jobs must refuse too)
        rc = lib.slime_slice_jobs(t, 0x7000, len(jobs) if n is None else n, crop, mean, std, 0x8000, out_crops, out_dtype, tmp, tmp_bytes, None)
        return rc, lib.slime_last_error().decode()

    good = _job(37, 23, 20, 14, 32, 48, x0=5, y0=3)

    def bad_ksize(vertical):
        J = _job(37, 23, 20, 14, 32, 48)
        if vertical:
            J.ksize_v += 1
        else:
            J.ksize_h -= 1
        return J

    unplanned = _job(37, 23, 20, 14, 32, 48, first_crop=6)
    cases = [
        (dict(jobs=[good], n=0), "SLIME_SLICE_MAX_JOBS = 128"),
        (dict(jobs=[_job(16, 16, 16, 16, 16, 16, first_crop=i) for i in range(129)], out_crops=200), "SLIME_SLICE_MAX_JOBS = 128"),
        (dict(jobs=[_job(37, 23, 20, 14, 32, 40)]), "not a multiple of crop 16"),
        (dict(jobs=[_job(37, 23, 20, 14, 24, 48)]), "not a multiple of crop 16"),
        (dict(jobs=[_job(37, 23, 20, 14, 32, 48, x0=35)]), "leaves the 32x48 canvas"),
        (dict(jobs=[_job(37, 23, 20, 14, 32, 48, y0=13)]), "leaves the 32x48 canvas"),
        (dict(jobs=[_job(37, 23, 20, 14, 32, 48, x0=-1)]), "leaves the 32x48 canvas"),
        (dict(jobs=[_job(37, 23, 37, 14, 48, 48, tables=False)]), "horizontal tables missing"),
        (dict(jobs=[_job(37, 23, 20, 23, 32, 48, tables=False)]), "vertical tables missing"),
        (dict(jobs=[bad_ksize(False)]), "horizontal tables missing or ksize"),
        (dict(jobs=[bad_ksize(True)]), "vertical tables missing or ksize"),
        (dict(jobs=[good, _job(16, 16, 16, 16, 16, 16, first_crop=5)]), "overlap"),
        (dict(jobs=[_job(16, 16, 16, 16, 16, 16, first_crop=3), _job(37, 23, 20, 14, 32, 48, first_crop=0)]), "overlap"),
        (dict(jobs=[good], out_crops=5), "outside the output's [0, 5)"),
        (dict(jobs=[_job(16, 16, 16, 16, 16, 16, first_crop=-1)]), "outside the output's"),
        (dict(jobs=[_job(37, 23, 20, 14, 32, 48, stride=68)]), "row stride 68 smaller than a row of 69"),
        (dict(jobs=[good], out_dtype=_lib.U8), "not F32 / BF16 / F16"),
        (dict(jobs=[_job(16, 16, 16, 16, 16, 16), unplanned], plan=False), "slime_slice_jobs_plan"),
    ]
    for kw, word in cases:
        rc, msg = run(**kw)
        assert rc == -1, (kw, msg)                                               # SLIME_EINVAL
        assert word in msg, (word, msg)
    # a plan made for another order of the same jobs is not this table's plan
    a, b = _job(37, 23, 20, 14, 32, 48, first_crop=0), _job(50, 600, 48, 32, 48, 32, first_crop=6)
    t = _table([a, b])
    assert _plan(t)[0] == 0
    swapped = _table([t[1], t[0]])
    assert lib.slime_slice_jobs(swapped, 0x7000, 2, CROP, mean, std, 0x8000, 64, _lib.F32, 0x6000, 1 << 30, None) == -1
    assert "slime_slice_jobs_plan" in lib.slime_last_error().decode()
    # a valid table passes every argument check and stops at the workspace: nothing was launched
    need = (37 * 14 * 3 + 15) // 16 * 16
    for kw in (dict(tmp_bytes=need - 1), dict(tmp=0), dict(tmp=0x6004)):
        rc, msg = run([good], **kw)
        assert rc == -2 and f"tmp needs {need} bytes" in msg, (kw, rc, msg)      # SLIME_EWORKSPACE
    # the plan refuses what it cannot lay out, naming the same limits
    rc, _ = _plan(_table([_job(37, 23, 20, 14, 32, 40)]))
    assert rc == -1 and "not a multiple of crop 16" in lib.slime_last_error().decode()


def test_slice_job_mirror_matches_the_header_layout(tmp_path):
    """_lib.SliceJob against slime_slice_job: sizeof / offsetof printed by a C program compiled against the header, field by field,
    and the job cap."""
    import re
    import shutil
    import subprocess
    from slime_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"}\s*slime_slice_job\s*;", text)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {',
             'printf("sizeof %zu\\n", sizeof(slime_slice_job));', 'printf("max_jobs %d\\n", (int)SLIME_SLICE_MAX_JOBS);']
    for fname, _ in _lib.SliceJob._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(slime_slice_job, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.SliceJob)
    assert int(got["max_jobs"]) == _lib.SLICE_MAX_JOBS == 2 * 64
    struct_body = text[:text.index("} slime_slice_job")]
    struct_body = struct_body[struct_body.rindex("typedef struct"):]
    declared = [f for f in re.findall(r"\b([a-z_0-9]+)\s*[,;]", struct_body)]
    assert declared == [f for f, _ in _lib.SliceJob._fields_]                     # every field, in the header's order
    for fname, _ in _lib.SliceJob._fields_:
        assert int(got[fname]) == getattr(_lib.SliceJob, fname).offset, fname
