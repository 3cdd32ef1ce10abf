"""Element-wise conformance of the cosine text-guided router on the GPU, through the C ABI: slime_router_scores and
slime_router_scores_batched against the float64 unfactorised reference, probs_out of slime_router_select against the float64 softmax
of the device's own scores, under the DERIVED bounds of tests/router_conformance.py (its docstring holds the derivations; the test of
the bounds themselves is tests/test_router_bound_cpu.py), and the kept set end to end, exactly, on scores separated by construction.

Every operand lives in a padded buffer of its own (gemm_conformance.Padded): NaN around every input, the sentinel byte 0x7B in every
output and in the workspace, guards behind them; the workspaces have exactly the documented sizes (L + H + 4 floats;
slime_router_batched_workspace_floats).  After each call every byte outside the output windows is what it was.  All guards are inside
the test's own allocations; nothing here provokes a fault: a refused call returns before any launch (csrc/router.hip: every
SLIME_REQUIRE of an entry precedes its first hipLaunchKernelGGL), and the refusal tests call only entries that have the check.

What is walked.  Scores: T in {1, 4, 5, 7, 37} x H in {4, 128, 256, 260, 1024} x L in {1, 3, 4, 5, 12}, L = 260 > H = 256,
ceil4(125) == H = 128 and the product shape 1008 x 300 x 4096, each with and without a mask, over random / aligned / cancelling /
zero image row / norms on both sides of eps / zero text row / fully masked inputs; bit for bit: masked-out rows of 1e17 against zeros,
permuted image rows, a second call into a fresh workspace.  The batched entry: B = 4 (an empty image, two overlapping row ranges, row
offset 0, the buffer's last row) in the fused and the ragged layout, with per-image masks and without, L > H, B = 1 -- bit-equal to
the single calls, the padding of [B, T_max] untouched.  probs_out at T in {1, 2, 1023, 1025, 4096} x temp in {0.3, 1, 2} with exact
zeros.  End to end at T in {37, 288, 1008} in three forms.  The refusals of all four entries.

Worst |err| / bound observed on an MI355X (the module prints this table at the end of a run and writes it to the file
SLIME_ROUTER_CONFORMANCE_REPORT names).  These are measurements against the float64 reference, not targets.
    scores, by input kind     random 0.042   aligned 0.054   cancelling 0.023   zero_row 0.018   tiny 0.030   zero_text_row 0.022
    scores, fully masked      0.000 (every score is exactly 0.0)
    scores_batched            0.018 (and bit-equal to the single calls)
    probs_out                 0.515 (scores a dozen text rows can produce)   0.491 (scores over +-200, exact zeros)
The score bound is a worst case linear in the chain lengths, which random roundings stay far inside.  The softmax's has few terms, each
a tight worst case of one rounding: at |z - max z| >= 64 the subtraction alone rounds by up to 64 e of a bound of about 130 e, and one
element in 4096 attains it.  All 29 tests passed on the kernels as they were; the one product change is the entries' refusal of
pointers their 16-byte loads cannot take.  Two references had to be stated more exactly than torch gives them: the selection's
cumulative sum rounds every partial sum to fp32 (torch.cumsum on the CPU carries a double: router_conformance.router_expected), and the
float64 softmax is evaluated on the host (torch's GPU build was 6e-6 off at z - max z = -65).
"""
import json
import math
import os

import pytest
import torch

import gemm_conformance as GC
import rowwise_conformance as RC
import router_conformance as R
from rowwise_conformance import Padded

pytestmark = pytest.mark.gpu

NAN = math.nan
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    """worst |err| / bound per (operation, kind), printed when the module is done (and written to the file
    SLIME_ROUTER_CONFORMANCE_REPORT names, if set)."""
    table = {}
    yield table
    lines = [f"    {k:40s} {v:.3f}" for k, v in sorted(table.items())]
    print("\ncosine router conformance, worst |err| / bound per operation and kind:\n" + "\n".join(lines))
    path = os.environ.get("SLIME_ROUTER_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _note(ratios, key, value):
    ratios[key] = max(ratios.get(key, 0.0), float(value))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inp(t, rows=1, guard=NAN):
    """A copy of an input tensor in a buffer of its own, ``guard`` (NaN) in front of it and behind it."""
    t = t.contiguous()
    return Padded(rows, t.numel() // rows, t.dtype, t.device, pad_cols=0, guard_rows=0, tail=GC.TAIL).fill(t.view(rows, -1), guard)


def _out(rows, width, dtype, dev):
    """An output (or workspace) window of exactly rows x width elements: sentinel bytes everywhere, guard rows and a tail behind."""
    return Padded(rows, width, dtype, dev, pad_cols=0, tail=GC.TAIL)


def _same(p, snap):
    return bool(torch.equal(p.flat.view(torch.uint8), snap.view(torch.uint8)))


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.uint8) == R.SENTINEL_BYTE).all())


class _Operands:
    """img, text, mask of one call in guarded buffers (a mask's guard is 1: a read past it would take a NaN row for valid)."""

    def __init__(self, img, text, mask):
        self.T, self.H = img.shape
        self.L = text.shape[-2]
        self.img, self.text = _inp(img, self.T), _inp(text.reshape(-1, self.H), text.numel() // self.H)
        self.mask = None if mask is None else _inp(mask.reshape(1, -1), 1, guard=1)
        self.snaps = [(p, p.snapshot()) for p in (self.img, self.text, self.mask) if p is not None]

    def unchanged(self):
        return all(_same(p, s) for p, s in self.snaps)

    def mask_ptr(self, b=0):
        return None if self.mask is None else self.mask.ptr() + b * self.L


def _run_scores(lib, ops_, T=None, img_ptr=None, text_ptr=None, mask_ptr=None):
    """slime_router_scores into a fresh sentinel output and a fresh workspace of exactly L + H + 4 floats -> scores [T] (a clone);
    asserts the return code and that nothing outside the two windows, and no input, was written."""
    dev = ops_.img.flat.device
    T = ops_.T if T is None else T
    out, ws = _out(1, T, torch.float32, dev), _out(1, R.single_workspace_floats(ops_.L, ops_.H), torch.float32, dev)
    so, sw = out.snapshot(), ws.snapshot()
    rc = lib.slime_router_scores(img_ptr or ops_.img.ptr(), T, text_ptr or ops_.text.ptr(), ops_.L, mask_ptr if mask_ptr is not None else ops_.mask_ptr(),
                                 ops_.H, out.ptr(), ws.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert out.intact(so), "slime_router_scores: a byte outside the scores window was written"
    assert ws.intact(sw), "slime_router_scores: a byte outside the L + H + 4 floats of workspace was written"
    assert ops_.unchanged(), "slime_router_scores: an input was written"
    return out.win.view(-1).clone()


def _select(lib, scores, temp, topp, want_probs=True):
    """slime_router_select on guarded buffers -> (kept indices int64 on the host, probs [T] or None)."""
    dev, T = scores.device, scores.numel()
    sb = _inp(scores.view(1, T))
    keep, cnt, probs = _out(1, T, torch.int32, dev), _out(1, 1, torch.int32, dev), _out(1, T, torch.float32, dev)
    snaps = [(p, p.snapshot()) for p in (keep, cnt, probs)]
    ss = sb.snapshot()
    rc = lib.slime_router_select(sb.ptr(), T, float(temp), float(topp), keep.ptr(), cnt.ptr(), probs.ptr() if want_probs else None, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    for p, s in snaps:
        assert p.intact(s), "slime_router_select: a byte outside an output window was written"
    assert _same(sb, ss), "slime_router_select: the scores were written"
    n = int(cnt.win.view(-1)[0])
    assert 1 <= n <= T and _is_sentinel(keep.win.view(-1)[n:]), "keep_idx behind keep_count was written"
    if not want_probs:
        assert _same(probs, snaps[2][1])
    return keep.win.view(-1)[:n].cpu().long(), (probs.win.view(-1).clone() if want_probs else None)


# ================================================================================================ 1. scores
ALL_SHAPES = list(R.SCORE_SHAPES) + [R.PRODUCT_SHAPE]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "T%d_L%d_H%d" % s)
def test_scores(dev, ratios, shape):
    """One (T, L, H): every input kind with and without a mask inside the bound (0.0 exactly for a zero image row and a fully masked
    text, whose kept set is arange(n)); for the random kind with a mask the three bit-for-bit properties."""
    from slime_amd import _lib
    lib = _lib.load()
    T, L, H = shape
    for c in R.score_cases(seed=3, shapes=(shape,), device=dev):
        o = _Operands(c.img, c.text, c.mask)
        got = _run_scores(lib, o)
        ratio, msg = R.check_scores(c, got)
        assert msg is None, msg
        _note(ratios, f"scores {c.kind}", ratio)
        if c.kind == "all_masked":
            kept, _ = _select(lib, got, 1.0, 0.5, want_probs=False)
            assert torch.equal(kept, torch.arange(kept.numel())), f"{c.what()}: all scores tied, the lowest indices are kept"
        if c.kind != "random":
            continue
        assert RC.bits_equal(_run_scores(lib, o), got), f"{c.what()}: a second call into a fresh workspace gives other bits"
        perm = torch.randperm(T, generator=torch.Generator().manual_seed(T)).to(dev)
        assert RC.bits_equal(_run_scores(lib, _Operands(c.img[perm], c.text, c.mask)), got[perm]), f"{c.what()}: a score depends on another row"
        if c.mask is not None and L >= 2:
            gone = c.mask.eq(0).nonzero().view(-1)
            big, zero = c.text.clone(), c.text.clone()
            big[gone], zero[gone] = R.BIG, 0.0
            a, b = _run_scores(lib, _Operands(c.img, big, c.mask)), _run_scores(lib, _Operands(c.img, zero, c.mask))
            assert RC.bits_equal(a, b), f"{c.what()}: a masked-out text row of 1e17 changes the scores, first at {RC.first_diff(a, b)}"
            assert RC.bits_equal(b, got), f"{c.what()}: a masked-out text row's finite values change the scores"


# ================================================================================================ 2. the batched entry
BATCHES = [("fused", 12, True, 4), ("fused", 12, False, 4), ("ragged", 12, True, 4), ("ragged", 12, False, 4), ("fused", 260, True, 4),
           ("ragged", 260, False, 4), ("ragged", 12, True, 1)]


@pytest.mark.parametrize("layout,L,masked,B", BATCHES, ids=lambda v: str(v))
def test_batched_scores_equal_single_calls(dev, ratios, layout, L, masked, B):
    """slime_router_scores_batched with a workspace of exactly slime_router_batched_workspace_floats floats: row b of the padded
    [B, T_max] array holds the bits of the single call on image b in its first n_rows[b] elements and the sentinel behind them."""
    from slime_amd import _lib
    lib = _lib.load()
    H = 128
    bc = R.make_batch_case(layout, L, H, masked, B=B, seed=5, device=dev)
    T_max = bc.T_max
    need = lib.slime_router_batched_workspace_floats(B, L, H)
    assert need == R.batched_workspace_floats(B, L, H)
    o = _Operands(bc.tokens, bc.text, bc.mask)
    off = _inp(torch.tensor(bc.row_off, dtype=torch.int64, device=dev).view(1, B), guard=1 << 40)
    cnt = _inp(torch.tensor(bc.n_rows, dtype=torch.int32, device=dev).view(1, B), guard=1 << 20)
    out, ws = _out(B, T_max, torch.float32, dev), _out(1, need, torch.float32, dev)
    so, sw, soff, scnt = out.snapshot(), ws.snapshot(), off.snapshot(), cnt.snapshot()
    rc = lib.slime_router_scores_batched(o.img.ptr(), off.ptr(), cnt.ptr(), B, T_max, o.text.ptr(), L, o.mask_ptr(), H, out.ptr(), ws.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.slime_last_error().decode()
    assert out.intact(so), f"{bc.name}: a byte in front of or behind the [B, T_max] scores was written"
    assert ws.intact(sw), f"{bc.name}: a byte outside the documented workspace was written"
    assert o.unchanged() and _same(off, soff) and _same(cnt, scnt), f"{bc.name}: an input was written"
    got = out.win.clone()
    for b in range(B):
        n = bc.n_rows[b]
        assert _is_sentinel(got[b, n:]), f"{bc.name}: image {b}: an element at or behind n_rows = {n} was written"
        if n == 0:
            continue
        single = _run_scores(lib, o, T=n, img_ptr=o.img.ptr() + bc.row_off[b] * H * 4, text_ptr=o.text.ptr() + b * L * H * 4, mask_ptr=o.mask_ptr(b))
        assert RC.bits_equal(got[b, :n].contiguous(), single), f"{bc.name}: image {b} differs from its single call at {RC.first_diff(got[b, :n].contiguous(), single)}"
        rows = bc.tokens[bc.row_off[b]:bc.row_off[b] + n]
        mb = None if bc.mask is None else bc.mask[b]
        c = R.ScoreCase(n, L, H, "random", rows, bc.text[b], mb)
        ratio, msg = R.check_scores(c, got[b, :n])
        assert msg is None, f"{bc.name}: image {b}: {msg}"
        _note(ratios, "scores_batched random", ratio)


# ================================================================================================ 3. probs_out
@pytest.mark.parametrize("T", R.PROB_T)
def test_probs_out(dev, ratios, T):
    """probs_out against the float64 softmax of the same fp32 scores; the kept set from those probabilities exactly; the spread kind:
    exact zeros below z - max z = -104, kept in ascending index order at top-p = 1 - 2^-20."""
    from slime_amd import _lib
    lib = _lib.load()
    for temp in R.PROB_TEMP:
        for kind in R.PROB_KINDS:
            s = R.prob_scores(T, kind, seed=2).to(dev)
            name = f"probs T={T} temp={temp} {kind}"
            for topp in (0.95, R.TOPP_ALMOST_ONE) if kind == "spread" else (0.95,):
                kept, probs = _select(lib, s, temp, topp)
                ratio, msg = R.check_probs(name, probs, s, temp)
                assert msg is None, msg
                _note(ratios, f"probs {kind}", ratio)
                want = R.router_expected(probs.cpu(), R.f32(topp))
                assert torch.equal(kept, want), f"{name} top-p={topp}: the kept set is not the stable descending sort's"
                if kind == "spread" and T >= 2:
                    assert float(R.probs_reference(s, temp)[2].min()) < -104.0 and bool((probs == 0).any()), name
                    assert R.kept_zeros_are_the_lowest(probs.cpu(), kept), f"{name} top-p={topp}: exact zeros must tie by ascending index"


# ================================================================================================ 4. end to end, exactly
@pytest.mark.parametrize("T", R.SEP_T)
def test_kept_set_equals_the_float64_oracle(dev, T):
    """Scores separated by construction (the margin is asserted on the CPU and again here): the float64 kept set of the oracle's
    router_select, exactly, from the two C entries, ops.router_topp and ops.router_topp_batched."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    for topp, temp in R.SEP_PT:
        img, text, mask, want, margin = R.separated_case(T, topp, temp, device=dev)
        want = want.cpu()
        what = f"separated T={T} top-p={topp} temp={temp}"
        assert margin >= R.MARGIN, (what, margin)
        scores = _run_scores(lib, _Operands(img, text, mask))
        kept, _ = _select(lib, scores, temp, topp, want_probs=False)
        assert torch.equal(kept, want), f"{what}: slime_router_scores + slime_router_select keep {kept.numel()}, the float64 oracle {want.numel()}"
        assert torch.equal(ops.router_topp(img, text, mask, topp, temp).cpu(), want), f"{what}: ops.router_topp"
        tokens = torch.cat([torch.randn(3, img.shape[1], device=dev), img]).contiguous()
        got = ops.router_topp_batched(tokens, [3], [T], text[None], mask[None], topp, temp)
        assert len(got) == 1 and torch.equal(got[0].cpu(), want), f"{what}: ops.router_topp_batched"


# ================================================================================================ 5. refusals
def _refused(lib, rc, needle, outs, what):
    torch.cuda.synchronize()
    assert rc == EINVAL, (what, rc)
    msg = lib.slime_last_error().decode()
    assert needle in msg, (what, msg)
    for p, s in outs:
        assert _same(p, s), f"{what}: a refused call wrote an output"


def test_refusals(dev):
    """Every refusal returns SLIME_EINVAL with the entry (and, for an alignment, the argument) named, and leaves the outputs and the
    workspace untouched: each check precedes the entry's first launch."""
    from slime_amd import _lib
    lib = _lib.load()
    T, L, H, B = 5, 3, 128, 2
    c = R.make_score_case(T, L, H, "random", True, seed=9, device=dev)
    o = _Operands(c.img, c.text, c.mask)
    out, ws = _out(B, T, torch.float32, dev), _out(1, max(R.single_workspace_floats(L, H), R.batched_workspace_floats(B, L, H)) + 4, torch.float32, dev)
    off = _inp(torch.tensor([0, 1], dtype=torch.int64, device=dev).view(1, B), guard=0)
    cnt = _inp(torch.tensor([4, 3], dtype=torch.int32, device=dev).view(1, B), guard=0)
    outs = [(out, out.snapshot()), (ws, ws.snapshot())]
    good = dict(img=o.img.ptr(), T=T, text=o.text.ptr(), L=L, mask=o.mask_ptr(), H=H, scores=out.ptr(), ws=ws.ptr())
    single = [(dict(img=good["img"] + 4), "router_scores: img must be 16-byte aligned"), (dict(text=good["text"] + 4), "router_scores: text must be 16-byte aligned"),
              (dict(ws=good["ws"] + 4), "router_scores: ws must be 16-byte aligned"), (dict(scores=good["scores"] + 2), "router_scores: scores must be 4-byte aligned"),
              (dict(img=good["img"] + 8), "img must be 16-byte"), (dict(ws=good["ws"] + 12), "ws must be 16-byte")]
    single += [(dict(**{k: None}), "router_scores: bad input") for k in ("img", "text", "scores", "ws")]
    single += [(d, "router_scores: bad input") for d in (dict(T=0), dict(T=-1), dict(L=0), dict(L=-3), dict(H=126), dict(H=0), dict(H=-4))]
    for override, needle in single:
        a = dict(good, **override)
        rc = lib.slime_router_scores(a["img"], a["T"], a["text"], a["L"], a["mask"], a["H"], a["scores"], a["ws"], _stream())
        _refused(lib, rc, needle, outs, ("slime_router_scores", override))
    goodb = dict(good, off=off.ptr(), cnt=cnt.ptr(), B=B, T_max=4)
    del goodb["T"]
    batched = [(dict(img=good["img"] + 4), "router_scores_batched: img must be 16-byte aligned"),
               (dict(text=good["text"] + 4), "router_scores_batched: text must be 16-byte aligned"),
               (dict(ws=good["ws"] + 4), "router_scores_batched: ws must be 16-byte aligned"),
               (dict(scores=good["scores"] + 2), "router_scores_batched: scores must be 4-byte aligned")]
    batched += [(dict(**{k: None}), "router_scores_batched: bad input") for k in ("img", "off", "cnt", "text", "scores", "ws")]
    batched += [(d, "router_scores_batched: bad input") for d in (dict(B=0), dict(B=-1), dict(B=65536), dict(T_max=0), dict(T_max=-2), dict(L=0), dict(H=126), dict(H=0))]
    for override, needle in batched:
        a = dict(goodb, **override)
        rc = lib.slime_router_scores_batched(a["img"], a["off"], a["cnt"], a["B"], a["T_max"], a["text"], a["L"], a["mask"], a["H"], a["scores"], a["ws"], _stream())
        _refused(lib, rc, needle, outs, ("slime_router_scores_batched", override))
    # the two selections
    sc = _inp(torch.linspace(-1, 1, B * T, device=dev).view(B, T), B)
    keep, kc, probs = _out(B, T, torch.int32, dev), _out(1, B, torch.int32, dev), _out(1, T, torch.float32, dev)
    outs = [(p, p.snapshot()) for p in (keep, kc, probs)]
    gs = dict(scores=sc.ptr(), T=T, temp=1.0, topp=0.5, keep=keep.ptr(), kc=kc.ptr(), probs=probs.ptr())
    sel = [(dict(**{k: None}), "router_select: null pointer") for k in ("scores", "keep", "kc")]
    sel += [(dict(T=0), "router_select: T=0 outside 1..4096"), (dict(T=-1), "router_select: T=-1 outside 1..4096"), (dict(T=4097), "router_select: T=4097 outside 1..4096"),
            (dict(temp=0.0), "router_select: temperature must be positive"), (dict(temp=-1.0), "router_select: temperature must be positive")]
    for override, needle in sel:
        a = dict(gs, **override)
        rc = lib.slime_router_select(a["scores"], a["T"], a["temp"], a["topp"], a["keep"], a["kc"], a["probs"], _stream())
        _refused(lib, rc, needle, outs, ("slime_router_select", override))
    gb = dict(scores=sc.ptr(), cnt=cnt.ptr(), B=B, T_max=T, temp=1.0, topp=0.5, keep=keep.ptr(), kc=kc.ptr())
    selb = [(dict(**{k: None}), "router_select_batched: bad input") for k in ("scores", "cnt", "keep", "kc")]
    selb += [(dict(B=0), "router_select_batched: bad input"), (dict(T_max=0), "router_select_batched: T_max=0 outside 1..4096"),
             (dict(T_max=4097), "router_select_batched: T_max=4097 outside 1..4096"), (dict(temp=0.0), "router_select_batched: temperature must be positive"),
             (dict(temp=-0.5), "router_select_batched: temperature must be positive")]
    for override, needle in selb:
        a = dict(gb, **override)
        rc = lib.slime_router_select_batched(a["scores"], a["cnt"], a["B"], a["T_max"], a["temp"], a["topp"], a["keep"], a["kc"], _stream())
        _refused(lib, rc, needle, outs, ("slime_router_select_batched", override))
    assert o.unchanged()
    # and the accepted call still runs afterwards
    assert RC.bits_equal(_run_scores(lib, o), _run_scores(lib, o))
