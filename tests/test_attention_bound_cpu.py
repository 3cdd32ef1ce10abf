"""The test of the attention conformance test (tests/attention_conformance.py), without a GPU.

(1) ``emulate`` -- the torch restatement of the kernels' arithmetic, the stand-in for a correct kernel -- stays inside the
    derived element-wise bound on the GPU file's own input generator and shapes, both dtypes, logit gains 1 / 6 / 12, both
    softmax forms ("exact": generic kernel and eight-wave prefill kernel; "lazy": attn64r / prefill32).
    Shapes: every n_kv / n_q edge of the GPU walk at batch 1 x 2 heads (the GPU file runs 2 x 4 up to 20 x 16); left out
    for run time: the 5 / 10 / 17 / 20-crop x 16-head launch-form cases (a host-side launch decision the emulation does
    not have), prefill S = 600 / 1300 at groups 8 and 16, and the cross product of n_q with n_kv.
    Measured here (worst |err| / bound): attention cases bf16 0.46 ("exact") / 0.67 ("lazy"), fp16 0.35 / 0.39; prefill
    cases bf16 0.74, fp16 0.58 (both forms; the worst rows are short causal rows, where one rounding of P is the whole
    error).  The emulation rounds P exactly as the kernels do, so what is left of the bound is its worst-case slack.
(2) every mutant of MUTANTS leaves the bound on at least one element of at least one case (guards as finite attractors).
(3) the reason the element-wise test exists: at a production batch (17 crops x 16 heads x 577 x 577, plain random data,
    the neighbour's rows behind the last key) the two mutants confined to ONE 16-row sub-block of ONE head stay below the
    whole-tensor tolerances of tests/test_gpu_kernels.py (rel-L2 6e-3 bf16, 1.5 * 6e-4 fp16).
"""
import pytest
import torch

import attention_conformance as AC

DTYPES = [torch.bfloat16, torch.float16]
WHOLE_TENSOR_TOL = {torch.bfloat16: 6e-3, torch.float16: 1.5 * 6e-4}


def _attention_cases():
    for nkv in AC.ATTN64_NKV:
        yield dict(dh=64, n_q=nkv if nkv in (257, 577) else 80, n_kv=nkv)
    for nq in AC.ATTN64_NQ:
        yield dict(dh=64, n_q=nq, n_kv=577)
        yield dict(dh=64, n_q=nq, n_kv=200)
    for nkv in AC.ATTN128_NKV:
        yield dict(dh=128, n_q=144, n_kv=nkv, shared_q=True)
    for nq in AC.ATTN128_NQ:
        yield dict(dh=128, n_q=nq, n_kv=576)


def _prefill_cases():
    for group in AC.GROUPS:
        for S in AC.prefill_lengths(group, prefill32=group == 4):
            if S >= 600 and group >= 8:
                continue
            yield group, S


def _check(case, style, worst):
    r = case.reference()
    got = case.emulate(style)
    ratio, ex, idx, g, w = AC.worst(got, r, case.dtype)
    assert ex <= 0, AC.describe_failure(f"emulate({style})", got, r, case.dtype)
    worst[0] = max(worst[0], ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("style", ["exact", "lazy"])
def test_emulation_inside_bound_attention(dtype, style):
    worst = [0.0]
    for n, kw in enumerate(_attention_cases()):
        gain = AC.GAINS[n % 3]
        _check(AC.make_case("random", dtype, B=1, H=2, gain=gain, guard="nan", seed=100 + n, **kw), style, worst)
    for dh, nkv in ((64, 577), (64, 200), (128, 288)):
        for kind in ("onehot", "uniform"):
            _check(AC.make_case(kind, dtype, B=1, H=2, dh=dh, n_q=161, n_kv=nkv, guard="nan", seed=7), style, worst)
    for gain in AC.GAINS:                                         # the CLIP shape at every gain
        _check(AC.make_case("random", dtype, B=1, H=2, dh=64, n_q=577, n_kv=577, gain=gain, guard="nan", seed=9), style, worst)
    print(f"\nemulate({style}) {dtype}: worst |err| / bound over the attention cases = {worst[0]:.3f}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("style", ["exact", "lazy"])
def test_emulation_inside_bound_prefill(dtype, style):
    worst = [0.0]
    for n, (group, S) in enumerate(_prefill_cases()):
        gain = AC.GAINS[n % 3]
        kw = dict(B=1, H=group, HKV=1, dh=128, n_q=S, n_kv=S, gain=gain, causal=True, guard="nan", seed=200 + n)
        _check(AC.make_case("random", dtype, **kw), style, worst)
        kw.update(B=4, ranges=AC.prefill_ranges(S))
        _check(AC.make_case("random" if n % 4 else "onehot", dtype, **kw), style, worst)
    print(f"\nemulate({style}) {dtype}: worst |err| / bound over the prefill cases = {worst[0]:.3f}")
    assert worst[0] <= 1.0


def _mutant_cases(dtype):
    yield "attention 2x4x577x577 dh64 gain 1", AC.make_case("random", dtype, B=2, H=4, dh=64, n_q=577, n_kv=577, guard="attract", seed=4)
    yield "attention uniform 2x4x80x353 dh64", AC.make_case("uniform", dtype, B=2, H=4, dh=64, n_q=80, n_kv=353, guard="attract", seed=5)
    yield "prefill 4x(4/2)x83 gain 1, ranges", AC.make_case("random", dtype, B=4, H=4, HKV=2, dh=128, n_q=83, n_kv=83, causal=True,
                                                            ranges=AC.prefill_ranges(83), guard="attract", seed=6)
    yield "prefill 2x(8/2)x70 gain 6", AC.make_case("random", dtype, B=2, H=8, HKV=2, dh=128, n_q=70, n_kv=70, gain=6.0, causal=True,
                                                    guard="attract", seed=8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_every_mutant_leaves_the_bound(dtype):
    cases = [(name, c, c.reference()) for name, c in _mutant_cases(dtype)]
    for name, c, r in cases:                                      # the cases themselves are clean
        assert AC.worst(c.emulate(), r, dtype)[1] <= 0, name
    print()
    for mname, defect in AC.MUTANTS.items():
        caught = []
        for name, c, r in cases:
            ratio, ex, idx, g, w = AC.worst(c.emulate("exact", defect), r, dtype)
            if ex > 0:
                caught.append((name, ratio, idx))
        assert caught, f"mutant {mname} stays inside the bound on every case ({dtype})"
        name, ratio, (b, i, h, d) = caught[0]
        print(f"{dtype} {mname:36s} caught by [{name}] at (batch {b}, head {h}, row {i}, column {d}): |err| / bound = {ratio:.3g}"
              f"  (+ {len(caught) - 1} more cases)")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_confined_mutants_pass_the_whole_tensor_tolerance(dtype):
    """One sub-block of one (crop, head) wrong, 17 x 16 x 577 x 577 as in test_attention32_launch_forms' largest case."""
    torch.manual_seed(0)
    c = AC.make_case("random", dtype, B=17, H=16, dh=64, n_q=577, n_kv=577, gain=1.0, boost=0.0, guard="neighbour", seed=11)
    refs, clean = [], []
    for b0 in range(0, c.B, 4):
        s = c.batch_slice(b0, min(c.B, b0 + 4))
        refs.append(s.reference())
        clean.append(s.emulate("lazy"))
    r = AC.Ref(*(torch.cat([x[t] for x in refs]) for t in range(4)))
    clean = torch.cat(clean)
    base = AC.rel_l2(clean, r.out)
    print(f"\n{dtype} clean emulation: whole-tensor rel-L2 {base:.2e}, worst |err| / bound {AC.worst(clean, r, dtype)[0]:.3f}")
    first = c.batch_slice(0, 4)
    for mname in AC.CONFINED:
        got = clean.clone()
        got[:4] = first.emulate("lazy", AC.MUTANTS[mname])
        whole = AC.rel_l2(got, r.out)
        cb, ch, blk = AC.MUTANTS[mname].confine
        rows = AC.rel_l2(got[cb, blk * 16:blk * 16 + 16, ch], r.out[cb, blk * 16:blk * 16 + 16, ch])
        ratio, ex, (b, i, h, d), g, w = AC.worst(got, r, dtype)
        print(f"{dtype} {mname:36s} rel-L2 on its 16 rows {rows:.2e}, whole tensor {whole:.2e} (tolerance {WHOLE_TENSOR_TOL[dtype]:.1e}: "
              f"passes), element-wise worst |err| / bound {ratio:.2f} at (batch {b}, head {h}, row {i}, column {d})")
        assert whole < WHOLE_TENSOR_TOL[dtype], "the whole-tensor check was expected to miss this mutant"
        assert rows > 10 * base, "the defect is there"
        assert ex > 0 and (b, h, i // 16) == (cb, ch, blk), "and the element-wise bound points at it, even on plain random data"
