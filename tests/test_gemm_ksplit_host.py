"""Host side of the opt-in deterministic split-K GEMM (slime_gemm_ksplit, slime_vit_forward_ksplit): the struct mirror, the
workspace queries, every refusal that returns before a launch, and the DERIVED bound of tests/gemm_conformance.py applied to
chunked summation.  No GPU: the refusals are reached with made-up (aligned, never dereferenced) pointer values.

Why the bound of the unsplit GEMM holds unchanged: its accumulation term e (K + 4) S charges one rounding per accumulated product as a
relative weight on S = sum |a_k b_k| + ..., whatever the order of the additions.  A split element sees K / S_ roundings inside its
longest chunk and S_ - 1 in the plane sum, and K / S_ + S_ - 1 <= K for every admissible (K, S_).
"""
import ctypes as C
import re
import shutil
import subprocess

import pytest
import torch

import gemm_conformance as GC

from slime_amd import _lib

FAKE = 0x10000          # a 256-byte aligned address that no refusal path reads


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.slime_last_error().decode()


def test_vit_ksplit_mirror_matches_the_header(tmp_path):
    assert shutil.which("gcc") is not None, "the struct mirror is checked with a C program"
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"}\s*slime_vit_ksplit\s*;", text)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{_lib.HEADER_PATH}"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(slime_vit_ksplit));', 'printf("max %d\\n", (int)SLIME_GEMM_KSPLIT_MAX);']
    for fname, _ in _lib.VitKsplit._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(slime_vit_ksplit, {fname}));')
    lines += ['return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.VitKsplit)
    assert [f for f, _ in _lib.VitKsplit._fields_] == ["qkv", "out_proj", "fc1", "fc2"]
    for fname, _ in _lib.VitKsplit._fields_:
        assert int(got[fname]) == getattr(_lib.VitKsplit, fname).offset, fname
    assert int(got["max"]) == _lib.GEMM_KSPLIT_MAX == 8


def test_gemm_ksplit_workspace_bytes(lib):
    q = lib.slime_gemm_ksplit_workspace_bytes
    for M, N in ((1, 128), (577, 1024), (2885, 4096)):
        assert q(M, N, 1) == 0
        for s in range(2, 9):
            b = q(M, N, s)
            assert b % 256 == 0 and b >= s * ((M + 127) // 128) * 128 * N * 4
            assert b < s * ((M + 127) // 128) * 128 * N * 4 + 256
    # monotone in each argument
    for s in range(1, 8):
        assert q(577, 1024, s) <= q(577, 1024, s + 1)
    ms = [q(m, 1024, 2) for m in range(1, 700)]
    assert ms == sorted(ms) and ms[0] < ms[-1]
    ns = [q(577, n, 2) for n in range(128, 4097, 128)]
    assert ns == sorted(ns) and len(set(ns)) == len(ns)
    # nothing to size outside the range of splits
    assert q(577, 1024, 0) == 0 and q(577, 1024, 9) == 0 and q(0, 1024, 2) == 0


def _tiny_desc():
    d = _lib.VitDesc(hidden=128, inter=512, heads=2, layers_run=2, image=336, patch=14, kpad=640, dtype=_lib.BF16, eps=1e-5)
    for name, _ in _lib.VitDesc._fields_[9:]:
        setattr(d, name, FAKE)
    return d


def test_vit_ksplit_workspace_bytes(lib):
    d = _tiny_desc()
    assert lib.slime_vit_check(C.byref(d)) == 0, _err(lib)
    for n in (1, 3, 9):
        plain = lib.slime_vit_workspace_bytes(C.byref(d), n)
        assert plain > 0
        one = _lib.VitKsplit(1, 1, 1, 1)
        assert lib.slime_vit_ksplit_workspace_bytes(C.byref(d), n, C.byref(one)) == plain
        M = n * 577
        ks = _lib.VitKsplit(2, 2, 2, 4)
        parts = [lib.slime_gemm_ksplit_workspace_bytes(M, 384, 2), lib.slime_gemm_ksplit_workspace_bytes(M, 128, 2),
                 lib.slime_gemm_ksplit_workspace_bytes(M, 512, 2), lib.slime_gemm_ksplit_workspace_bytes(M, 128, 4)]
        assert lib.slime_vit_ksplit_workspace_bytes(C.byref(d), n, C.byref(ks)) == plain + max(parts)      # ONE region, the largest


def _args(M=273, N=128, K=320, epilogue=_lib.EPI_BIAS_F32, **kw):
    f = dict(A=FAKE, lda=K, B=FAKE, bias=FAKE, C=FAKE, ldc=N, M=M, N=N, K=K, dtype=_lib.BF16, epilogue=epilogue)
    f.update(kw)
    return _lib.GemmArgs(**f)


def test_gemm_ksplit_refusals(lib):
    EINVAL, EWORKSPACE = -1, -2
    g = _args()
    need = lib.slime_gemm_ksplit_workspace_bytes(273, 128, 2)
    call = lambda g, s, ws=FAKE, nbytes=1 << 30: lib.slime_gemm_ksplit(C.byref(g), s, ws, nbytes, None)
    for s in (0, -1, 9):
        assert call(g, s) == EINVAL
        assert f"splits={s}" in _err(lib) and "1..8" in _err(lib)
    assert call(g, 6) == EINVAL                          # K = 320: five k-tiles
    assert "splits=6" in _err(lib) and "K / 64 = 5" in _err(lib)
    mix = _args(N=256, K=128, epilogue=_lib.EPI_BIAS_GELU_MIX_T, B_frag=FAKE, A2=FAKE, mix_gates=FAKE)
    assert call(mix, 2) == EINVAL
    assert "BIAS_GELU_MIX_T" in _err(lib) and "direct-B" in _err(lib)
    assert call(g, 2, FAKE, need - 1) == EWORKSPACE
    assert f"need {need}" in _err(lib)
    assert call(g, 2, None, need) == EWORKSPACE
    assert call(g, 2, FAKE + 128, need) == EWORKSPACE
    assert "256-B aligned" in _err(lib)
    # 2 x 2^20 padded rows x 1024 columns of fp32: the partial planes pass what 32-bit offsets reach
    big = _args(M=1 << 20, N=1024, K=128)
    assert lib.slime_gemm_ksplit_workspace_bytes(1 << 20, 1024, 2) == 1 << 33
    assert call(big, 2, FAKE, 1 << 40) == EINVAL
    assert "4 GiB" in _err(lib)
    # the checks of slime_gemm_ex, by the same code and in the same words
    bad = _args(K=96)
    assert call(bad, 2) == EINVAL
    msg = _err(lib)
    assert lib.slime_gemm_ex(C.byref(bad), None) == EINVAL and _err(lib) == msg and "multiple of 64" in msg
    bad = _args(dtype=_lib.F32)
    assert call(bad, 2) == EINVAL and "16-bit MFMA type" in _err(lib)
    bad = _args(epilogue=_lib.EPI_BIAS_RESID_SPLIT_LN)      # lo8 / stats_out missing
    assert call(bad, 2) == EINVAL and "BIAS_RESID_SPLIT_LN needs" in _err(lib)


def test_vit_forward_ksplit_refusals(lib):
    EINVAL, EWORKSPACE = -1, -2
    d = _tiny_desc()

    def call(ks, ws=FAKE, nbytes=1 << 40):
        return lib.slime_vit_forward_ksplit(C.byref(d), FAKE, _lib.F32, 3, FAKE, _lib.F32, 0, None, C.byref(ks) if ks is not None else None,
                                            ws, nbytes, None)
    for field, limit in (("qkv", 2), ("out_proj", 2), ("fc1", 2), ("fc2", 8)):      # hidden 128: two k-tiles; inter 512: eight
        for v in (0, limit + 1):
            ks = _lib.VitKsplit(1, 1, 1, 1)
            setattr(ks, field, v)
            assert call(ks) == EINVAL
            assert f"{field}={v}" in _err(lib) and f"1..{limit}" in _err(lib)
    assert call(None) == EINVAL
    ks = _lib.VitKsplit(2, 2, 2, 4)
    need = lib.slime_vit_ksplit_workspace_bytes(C.byref(d), 3, C.byref(ks))
    assert call(ks, FAKE, need - 1) == EWORKSPACE and f"need {need}" in _err(lib)
    assert call(ks, FAKE + 64, need) == EWORKSPACE


# ------------------------------------------------------------------------------------------------ the bound and chunked summation
KS = ((128, 2), (320, 2), (576, 4), (512, 8))
BROKEN = ("boundary_tile_twice", "boundary_tile_dropped", "last_partial_not_added", "plane_from_previous")


def chunks(K, S):
    """The header's chunk rule: k-tiles [floor(s nk / S), floor((s + 1) nk / S)) of nk = K / 64."""
    nk = K // 64
    return [(s * nk // S, (s + 1) * nk // S) for s in range(S)]


def test_chunk_rule_covers_every_k_tile_once():
    for K in range(64, 4097, 64):
        for S in range(1, min(8, K // 64) + 1):
            ch = chunks(K, S)
            assert ch[0][0] == 0 and ch[-1][1] == K // 64
            assert all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and all(hi > lo for lo, hi in ch)
            assert 64 * max(hi - lo for lo, hi in ch) + S - 1 <= K


def emulate_split(c, S, broken=None):
    """The pair of kernels in torch fp32: every chunk accumulated in 32-wide k-steps from zero, the planes summed ((p0 + p1) + p2)
    + ..., then the epilogue of gemm_conformance.emulate (handed the sum through a one-step accumulation of an exact identity)."""
    A, B = c.buf["A"].win.float(), c.buf["B"].win.float()
    ch = chunks(c.K, S)
    if broken == "boundary_tile_twice":
        ch[0] = (ch[0][0], ch[0][1] + 1)
    if broken == "boundary_tile_dropped":
        ch[1] = (ch[1][0] + 1, ch[1][1])
    planes = []
    for lo, hi in ch:
        p = torch.zeros((c.M, c.N), dtype=torch.float32)
        for k0 in range(64 * lo, 64 * hi, 32):
            p = p + A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].T
        planes.append(p)
    if broken == "plane_from_previous":
        planes[-1] = planes[-2]
    if broken == "last_partial_not_added":
        planes = planes[:-1]
    acc = planes[0]
    for p in planes[1:]:
        acc = acc + p
    return acc


def epilogue_of(c, acc):
    """gemm_conformance.emulate's epilogue on a given accumulator: the case's forms here are linear in acc (bias_f32; resid_split_ln
    = acc + (bias + h), then the integer split), restated from emulate's own lines."""
    bias = c.buf["bias"].win.view(1, -1)
    outs = c.windows()
    if c.form == "bias_f32":
        outs["C"] = acc + bias
        return outs
    assert c.form == "resid_split_ln"
    h = GC.join64(c.buf["C"].win, c.buf["lo8"].win.to(torch.int32), c.dtype).float()
    y = acc + (bias + h)
    hi = y.to(c.dtype)
    sg = y.view(c.M, c.N // 64, 64)
    outs["C"], outs["lo8"] = hi, GC.delta8(y, hi, c.dtype).to(torch.int8)
    outs["stats_out"] = torch.stack([sg.sum(-1), (sg * sg).sum(-1)], -1).view(c.M, 2 * (c.N // 64))
    return outs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("K,S", KS)
@pytest.mark.parametrize("form", ["bias_f32", "resid_split_ln"])
def test_chunked_summation_stays_inside_the_bound(form, K, S, dtype):
    torch.manual_seed(0)
    c = GC.make_case("random", dtype, form, 67, 128, K, outliers=False)
    r = GC.reference(c)
    # the restated epilogue is emulate's: with the unsplit accumulation it reproduces emulate bit for bit
    A, B = c.buf["A"].win.float(), c.buf["B"].win.float()
    acc1 = torch.zeros((c.M, c.N))
    for k0 in range(0, K, 32):
        acc1 = acc1 + A[:, k0:k0 + 32] @ B[:, k0:k0 + 32].T
    want = GC.emulate(c)
    for name, t in epilogue_of(c, acc1).items():
        assert torch.equal(t, want[name]), name
    ratio, msg = GC.check(c, r, epilogue_of(c, emulate_split(c, S)))
    assert msg is None, msg
    assert ratio <= 1.0
    for b in BROKEN:
        ratio_b, msg_b = GC.check(c, r, epilogue_of(c, emulate_split(c, S, b)))
        assert msg_b is not None, f"{b}: stayed inside the bound (worst |err| / bound {ratio_b:.3f})"
