"""Element-wise conformance of ``slime_attention`` and ``slime_prefill_attention`` on the GPU, through the C ABI, against the
float64 reference and the DERIVED bound of tests/attention_conformance.py (its docstring holds the derivation; the test of the
bound itself is tests/test_attention_bound_cpu.py).

Every case lives in padded buffers: row stride = heads * head_dim + 64 elements, batch stride = (rows + 3) row strides.  Each
case runs twice: guard rows (>= n_q, >= n_kv) and guard columns of q / k / v are NaN in the first pass and finite attractors
in the second (a guard key row is a large multiple of the common query direction with v = 1000: a kernel that admits one is
grossly wrong, not subtly); o is pre-filled with a sentinel bit pattern.  After the call the n_q x E window must be finite and
inside the bound element by element, and every other element of o must still be the sentinel (compared as integers).  All
guards are inside the test's own allocations.

What is walked: every dispatch branch of slime_attention (attn64r: head_dim 64 and 321 <= n_kv <= 608; the generic kernel at
head_dim 64 below / above that; the generic kernel at head_dim 128) on both sides of each dispatch, chunk, tail and
query-split edge; slime_prefill_attention at every GQA group size it accepts (1, 2, 4, 8, 16) in both dtypes, bf16 group 4 on
both of its kernels, at the sequence lengths where a workgroup's tiling changes, with and without token ranges; the refusals;
and the two group sizes no model test reaches (MHA, group 8) through HipLlamaAttention.

Worst |err| / bound observed on an MI355X, bf16 / fp16 (the module prints this table at the end of a run):
attn64r 0.67 / 0.46; generic head_dim 64 0.59 / 0.45; generic head_dim 128 0.50 / 0.31; prefill32 0.64 (bf16 only); eight-wave
prefill kernel, groups 1 / 2 / 4 / 8 / 16: 0.53 / 0.66 / 0.62 / 0.70 / 0.67 and 0.55 / 0.56 / 0.56 / 0.60 / 0.63.  All 318 cases
passed on the kernels as they were; the HipLlamaAttention cases measure 5.3e-3 (bf16) / 6.7e-4 (fp16) against 8e-3 / 1.2e-3.
"""
import json
import os

import pytest
import torch

import attention_conformance as AC

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
DT_ID = {torch.bfloat16: "bf16", torch.float16: "fp16"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from slime_amd import _lib
    _lib.load()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ratios():
    """worst |err| / bound per (kernel, dtype), printed when the module is done (and written to the file
    SLIME_CONFORMANCE_REPORT names, if set)."""
    table = {}
    yield table
    lines = [f"    {k:28s} {v:.3f}" for k, v in sorted(table.items())]
    print("\nattention conformance, worst |err| / bound per kernel and dtype:\n" + "\n".join(lines))
    path = os.environ.get("SLIME_CONFORMANCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _attention_branch(dh, n_kv):
    if dh == 128:
        return "attention generic dh128"
    return "attention attn64r" if 321 <= n_kv <= 608 else "attention generic dh64"


def _launch_attention(c):
    from slime_amd import _lib, ops
    lib = _lib.load()
    o = c.new_output()
    rq, rk = c.H * c.dh + AC.PAD_COLS, c.HKV * c.dh + AC.PAD_COLS
    q_bs = 0 if c.shared_q else (c.n_q + AC.PAD_ROWS) * rq
    kv_bs = (c.n_kv + AC.PAD_ROWS) * rk
    _lib.check(lib.slime_attention(c.qbuf.data_ptr(), q_bs, rq, c.kbuf.data_ptr(), kv_bs, rk, c.vbuf.data_ptr(), kv_bs, rk,
                                   o.data_ptr(), (c.n_q + AC.PAD_ROWS) * rq, rq, c.B, c.H, c.dh, c.n_q, c.n_kv,
                                   ops.dtype_code(c.dtype), torch.cuda.current_stream().cuda_stream), "slime_attention")
    torch.cuda.synchronize()
    return o


def _launch_prefill(c, variant=0):
    from slime_amd import _lib, ops
    rq, rk = c.H * c.dh + AC.PAD_COLS, c.HKV * c.dh + AC.PAD_COLS
    S = c.n_q
    o = c.new_output()

    def call(lib):
        start, length = (None, None) if c.ranges is None else (c.ranges[0].data_ptr(), c.ranges[1].data_ptr())
        _lib.check(lib.slime_prefill_attention(c.qbuf.data_ptr(), (S + AC.PAD_ROWS) * rq, rq, c.kbuf.data_ptr(), (S + AC.PAD_ROWS) * rk, rk,
                                               c.vbuf.data_ptr(), (S + AC.PAD_ROWS) * rk, rk, o.data_ptr(), (S + AC.PAD_ROWS) * rq, rq,
                                               c.B, c.H, c.HKV, c.dh, S, start, length, ops.dtype_code(c.dtype),
                                               torch.cuda.current_stream().cuda_stream), "slime_prefill_attention")
        torch.cuda.synchronize()

    if variant == 0:
        call(_lib.load())
    else:
        with _lib.diag() as lib:
            lib.slime_prefill_set_variant(variant)
            try:
                call(lib)
            finally:
                lib.slime_prefill_set_variant(0)
    return o


def _verify(c, o, what, key, ratios):
    win, intact = c.check_output(o)
    r = c.reference()
    assert torch.isfinite(win.float()).all(), AC.describe_failure(what + ": non-finite output", win, r, c.dtype)
    ratio, ex, idx, g, w = AC.worst(win, r, c.dtype)
    print(f"{what}: worst |err| / bound {ratio:.3f}")
    assert ex <= 0, AC.describe_failure(what, win, r, c.dtype)
    assert intact, what + ": an element of o outside the n_q x E window was written"
    k = f"{key} {DT_ID[c.dtype]}"
    ratios[k] = max(ratios.get(k, 0.0), ratio)


def _run_attention(dev, ratios, kind, dtype, **kw):
    for guard in ("nan", "attract"):
        c = AC.make_case(kind, dtype, guard=guard, device=dev, **kw)
        what = (f"slime_attention {kind} {DT_ID[dtype]} B={c.B} H={c.H} dh={c.dh} n_q={c.n_q} n_kv={c.n_kv} gain={kw.get('gain', 1.0)} "
                f"shared_q={c.shared_q} guard={guard}")
        _verify(c, _launch_attention(c), what, _attention_branch(c.dh, c.n_kv), ratios)


# ------------------------------------------------------------------------------------------------ slime_attention, head_dim 64
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("n_kv", AC.ATTN64_NKV)
def test_attention_dh64_key_lengths(dev, ratios, dtype, n_kv):
    """Both sides of the dispatch (320 | 321, 608 | 609), the short-tail switch of attn64r (336 | 337, 352 | 353, 592 | 593,
    576 | 577), fewer keys than one step, the 608-row chunk edge of the generic kernel (1216 | 1217); CLIP-L/14-224 (257) and
    -336 (577) additionally square."""
    gain = AC.GAINS[AC.ATTN64_NKV.index(n_kv) % 3]
    _run_attention(dev, ratios, "random", dtype, B=2, H=4, dh=64, n_q=577, n_kv=n_kv, gain=gain, seed=n_kv)
    if n_kv in (257, 577):
        _run_attention(dev, ratios, "random", dtype, B=2, H=4, dh=64, n_q=n_kv, n_kv=n_kv, gain=AC.GAINS[(n_kv + 1) % 3], seed=n_kv + 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("n_kv", [577, 200])
@pytest.mark.parametrize("n_q", AC.ATTN64_NQ)
def test_attention_dh64_query_lengths(dev, ratios, dtype, n_kv, n_q):
    """One query, a ragged last sub-block, and the query-split edge (40 sub-blocks per workgroup: 640 | 641) on attn64r
    (n_kv = 577) and on the generic kernel (n_kv = 200)."""
    gain = AC.GAINS[AC.ATTN64_NQ.index(n_q) % 3]
    _run_attention(dev, ratios, "random", dtype, B=2, H=4, dh=64, n_q=n_q, n_kv=n_kv, gain=gain, seed=n_q)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("crops", [5, 10, 17, 20])
def test_attention_attn64r_launch_forms(dev, ratios, dtype, crops):
    """attn64r doubles its query split by a rounds-of-CUs rule: 5, 10, 17 and 20 crops x 16 heads fall on both sides of it
    (and 17 x 16 is not a multiple of 8: the XCD re-deal of the partners is off)."""
    _run_attention(dev, ratios, "random", dtype, B=crops, H=16, dh=64, n_q=577, n_kv=577, gain=1.0, seed=crops)
    if crops in (5, 20):
        _run_attention(dev, ratios, "random", dtype, B=crops, H=16, dh=64, n_q=641, n_kv=593, gain=6.0, seed=crops + 1)


# ------------------------------------------------------------------------------------------------ slime_attention, head_dim 128
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shared_q", [True, False], ids=["q_bs=0", "per-batch-q"])
@pytest.mark.parametrize("axis,n", [("kv", n) for n in AC.ATTN128_NKV] + [("q", n) for n in AC.ATTN128_NQ])
def test_attention_dh128(dev, ratios, dtype, shared_q, axis, n):
    """The 288-row chunk edge (287 | 288 | 289), fewer keys than one step, the query-split edge (16 sub-blocks: 256 | 257),
    with shared queries (q_bs = 0, the resampler's layout) and per-batch queries."""
    n_q, n_kv = (144, n) if axis == "kv" else (n, 576)
    gain = AC.GAINS[n % 3]
    _run_attention(dev, ratios, "random", dtype, B=3, H=4, dh=128, n_q=n_q, n_kv=n_kv, gain=gain, shared_q=shared_q, seed=n)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("kind", ["onehot", "uniform"])
@pytest.mark.parametrize("dh,n_kv", [(64, 577), (64, 1217), (128, 577)], ids=["attn64r", "generic64", "generic128"])
def test_attention_onehot_and_uniform(dev, ratios, dtype, kind, dh, n_kv):
    """One query per sub-block aligned with a key late in the sweep (the running reference jumps by ~40 log2 units there), and
    all-equal logits (the output is the mean of v: every key's weight is visible, the first and last key carry -+64)."""
    _run_attention(dev, ratios, kind, dtype, B=2, H=4, dh=dh, n_q=577, n_kv=n_kv, seed=3)


# ------------------------------------------------------------------------------------------------ slime_prefill_attention
def _prefill_params():
    for dtype in DTYPES:
        for group in AC.GROUPS:
            variants = (0, 1) if (group == 4 and dtype == torch.bfloat16) else (0,)
            for variant in variants:
                p32 = group == 4 and dtype == torch.bfloat16
                for S in AC.prefill_lengths(group, prefill32=p32):
                    yield pytest.param(dtype, group, variant, S, id=f"{DT_ID[dtype]}-group{group}-variant{variant}-S{S}")


def _prefill_key(c, variant):
    return "prefill32" if (c.group == 4 and c.dtype == torch.bfloat16 and variant == 0) else f"prefill eight-wave group {c.group}"


def _run_prefill(dev, ratios, kind, dtype, group, variant, S, gain, seed):
    HKV = 2
    for ranged in (False, True):
        for guard in ("nan", "attract"):
            c = AC.make_case(kind, dtype, B=4 if ranged else 2, H=HKV * group, HKV=HKV, dh=128, n_q=S, n_kv=S, gain=gain, causal=True,
                             ranges=AC.prefill_ranges(S) if ranged else None, guard=guard, seed=seed, device=dev)
            what = (f"slime_prefill_attention {kind} {DT_ID[dtype]} heads {c.H}/{c.HKV} (group {group}) variant {variant} S={S} gain={gain} "
                    f"ranges={'yes' if ranged else 'no'} guard={guard}")
            _verify(c, _launch_prefill(c, variant), what, _prefill_key(c, variant), ratios)


@pytest.mark.parametrize("dtype,group,variant,S", list(_prefill_params()))
def test_prefill_attention(dev, ratios, dtype, group, variant, S):
    """Every group size x dtype (bf16 group 4: prefill32 and, as diagnostic variant 1, the eight-wave kernel on the same
    inputs), S on the workgroup's own edges (QB = 256 / group query rows: QB - 1, QB, QB + 1, 2 QB + 17), the 32-key step and
    192-row chunk edges, 600 (and 63 / 64 / 65 / 1300 for prefill32's 64-row items); without token ranges and with four
    sequences -- left-padded, right-padded, a single token, the whole S.  K / V differ per kv head and q per query head, so a
    wrong head mapping is a gross error."""
    gain = AC.GAINS[(S + group) % 3]
    _run_prefill(dev, ratios, "random", dtype, group, variant, S, gain, seed=1000 * group + S)


@pytest.mark.parametrize("dtype,group,variant", [(torch.bfloat16, 4, 0), (torch.bfloat16, 4, 1), (torch.float16, 4, 0),
                                                   (torch.bfloat16, 1, 0), (torch.float16, 16, 0)])
@pytest.mark.parametrize("kind", ["onehot", "uniform"])
def test_prefill_attention_onehot_and_uniform(dev, ratios, dtype, group, variant, kind):
    _run_prefill(dev, ratios, kind, dtype, group, variant, 273, 1.0, seed=17)


@pytest.mark.parametrize("n_heads,n_kv_heads,dtype_code,needle", [
    (6, 2, None, "group size 3"), (64, 2, None, "group size 32"), (7, 2, None, "7 query heads / 2 kv heads"), (8, 2, 2, "dtype 2")])
def test_prefill_attention_refusals(dev, n_heads, n_kv_heads, dtype_code, needle):
    """Group sizes outside {1, 2, 4, 8, 16}, a head count the kv heads do not divide, and a non-16-bit dtype are refused with
    SLIME_EINVAL and a message that names what was refused; nothing is launched (o keeps its sentinel)."""
    from slime_amd import _lib
    lib = _lib.load()
    S = 40
    E, EK = n_heads * 128, n_kv_heads * 128
    q = torch.zeros((1, S, E), dtype=torch.bfloat16, device=dev)
    k = torch.zeros((1, S, EK), dtype=torch.bfloat16, device=dev)
    o = torch.full((1, S, E), AC.SENTINEL, dtype=torch.int16, device=dev)
    rc = lib.slime_prefill_attention(q.data_ptr(), S * E, E, k.data_ptr(), S * EK, EK, k.data_ptr(), S * EK, EK, o.data_ptr(), S * E, E,
                                     1, n_heads, n_kv_heads, 128, S, None, None, _lib.BF16 if dtype_code is None else dtype_code,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1, "SLIME_EINVAL expected"
    assert needle in lib.slime_last_error().decode()
    assert bool((o == AC.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ one level up: the module
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("padding", ["right", "left"])
@pytest.mark.parametrize("n_heads,n_kv_heads", [(8, 8), (16, 2)], ids=["mha-8/8", "group8-16/2"])
def test_llama_attention_module_mha_and_group8(dev, dtype, padding, n_heads, n_kv_heads):
    """HipLlamaAttention / ops.pack_llama_attention at the two group sizes no model test reaches, against
    oracle/prefill_oracle.llama_attention_forward at the per-stage tolerances of DESIGN.md section 2."""
    from slime_amd.model.language_model import HipLlamaAttention
    from oracle import prefill_oracle as P
    D, B, S = 1024, 2, 150
    g = torch.Generator().manual_seed(n_heads + (padding == "left"))
    m = HipLlamaAttention(D, n_heads, n_kv_heads, 128, 500000.0, compute_dtype=dtype)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.copy_(torch.randn(p_.shape, generator=g) * p_.shape[1] ** -0.5)
    w = {n: getattr(m, n).weight.detach().clone() for n in ("q_proj", "k_proj", "v_proj", "o_proj")}
    m.to(dev)
    hidden = torch.randn(B, S, D, generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    if padding == "right":
        mask[0, S - 21:] = 0
        mask[1, S - 67:] = 0
    else:
        mask[0, :37] = 0
        mask[1, :5] = 0
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    out, _, _ = m(hidden.to(dev), attention_mask=mask.to(dev), position_ids=pos.to(dev))
    assert out.dtype == torch.float32 and out.shape == (B, S, D)
    ref = P.llama_attention_forward(hidden, w["q_proj"], w["k_proj"], w["v_proj"], w["o_proj"], n_heads, n_kv_heads, pos, mask, 500000.0,
                                    head_dim=128)
    out = out.cpu()
    err = AC.rel_l2(out, ref)
    print(f"HipLlamaAttention {n_heads}/{n_kv_heads} {DT_ID[dtype]} {padding}-padded: rel-L2 {err:.2e}")
    assert err < {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}[dtype]
    assert float(out[~mask.bool()].abs().max()) == 0.0, "padded positions give zero rows"
