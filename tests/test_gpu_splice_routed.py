"""GPU tests of the routed splice (slime_splice_routed, cfg.fused_splice): the kernel alone on synthetic router arrays against a
CPU restatement of today's path (index_select, cat, .to(mid).to(out), then splice_rows' rule) -- bit for bit, every dtype
combination --, its zeroing backstop, and the opt-in path of encode_images / prepare_inputs_labels_for_multimodal against the
flag-off path on the tiny encoder.  Everything is an equality: the feature claims bit identity, so there is no tolerance."""
import pytest
import torch
import torch.nn as nn

from test_gpu_modules import _tiny_encoder

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
B, P, T_MAX = 3, 5, 7
N_ROWS = (7, 0, 4)
OFF = (5, 17, 22)                     # first local row of every image: P global rows in front of each, images back to back
TOKEN_ROWS = 26
TABLE_ROWS, SEP_ID = 40, 33
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_same_bits(got, want, what=""):
    """torch.equal, and the same bit patterns (torch.equal alone takes -0.0 for +0.0)."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert torch.equal(got, want), what
    assert torch.equal(bits(got), bits(want)), what


_data = {}


def data(H):
    """fp32 tokens [TOKEN_ROWS, H] and an fp32 table [TABLE_ROWS, H], built once per width on the CPU.  The token values carry what a
    rounding can get wrong: +-0, fp32 / bf16 subnormals, values that are subnormal only in fp16, exact round-to-even ties of bf16 and of
    fp16 in both directions, and +-1e5 (infinite in fp16).  No NaN: the sources here never hold one, a NaN's payload after two
    conversions is not specified the same way on both sides, and prefill.hip is built without NaN semantics."""
    if H not in _data:
        g = torch.Generator().manual_seed(100 + H)
        tokens = torch.randn(TOKEN_ROWS, H, generator=g)
        special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3e-39, 1e-6, -3e-6, 6.0e-8, 2.0 ** -25,
                                1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11),
                                1 + 2.0 ** -8 + 2.0 ** -20, 1e5, -1e5, 65504.0, 65520.0, 3.3895e38])
        flat = tokens.view(-1)
        flat[torch.arange(special.numel() * 9) * 7 % flat.numel()] = special.repeat(9)      # spread over rows, local and global ones
        table = torch.randn(TABLE_ROWS, H, generator=g)
        table[SEP_ID, :4] = torch.tensor([1 + 2.0 ** -8, -0.0, 1e5, 1 + 3 * 2.0 ** -11])
        _data[H] = (tokens, table)
    return _data[H]


# keep tables: (counts, kept local indices per image).  Counts 0, 1 and n_rows[b] all occur; entries past the count are filled with
# valid indices, so that nothing a test does can reach outside the token buffer.
KEEPS = [((7, 0, 1), ([0, 1, 2, 3, 4, 5, 6], [], [2])),
         ((1, 0, 4), ([5], [], [0, 1, 2, 3])),
         ((3, 0, 0), ([1, 4, 6], [], []))]


def plan_rows(counts):
    """The rows of one call as ('t', id) | ('z',) | ('f', image, position): text rows, padding and every feature row of every image,
    the images out of order and one of them backwards; 4 does not divide the row count (the last workgroup is partial)."""
    rows = [("t", 3), ("t", 0), ("t", TABLE_ROWS - 1)]
    rows += [("f", 0, p) for p in range(P + 1 + counts[0])] + [("z",)]
    rows += [("f", 2, p) for p in reversed(range(P + 1 + counts[2]))] + [("t", SEP_ID), ("z",)]
    rows += [("f", 1, p) for p in range(P + 1 + counts[1])] + [("t", 7)]
    while len(rows) % 4 != 3:
        rows.append(("z",))
    return rows


def encode(rows):
    return torch.tensor([r[1] if r[0] == "t" else -1 if r[0] == "z" else -2 - ((r[1] << 32) | r[2]) for r in rows], dtype=torch.int64)


def expected(rows, tokens, table, keeps, counts, mid, out):
    """Today's path on the CPU: per image cat([glob, sep32, local.index_select(keep)]).to(mid), then splice_rows' rule into `out`."""
    feats = []
    for b in range(B):
        glob = tokens[OFF[b] - P:OFF[b]]
        routed = tokens[OFF[b]:OFF[b] + N_ROWS[b]].index_select(0, torch.tensor(keeps[b][:counts[b]], dtype=torch.long))
        feats.append(torch.cat([glob, table[SEP_ID].float().unsqueeze(0), routed], 0).to(mid))
    want = torch.zeros(len(rows), tokens.shape[1], dtype=out)
    for r, row in enumerate(rows):
        if row[0] == "t":
            want[r] = table[row[1]].to(out)                   # equal dtypes: a copy; else a cast
        elif row[0] == "f":
            want[r] = feats[row[1]][row[2]].to(out)
    return want


def device_state(dev, keeps, counts, extra_image=None):
    """The router's device arrays.  They hold B + 1 entries while the call is told B: the extra one (an alias of image 0 unless given) is
    what a kernel without the b < B guard would read -- valid memory, valid rows."""
    from slime_amd import ops
    extra = extra_image or (OFF[0], N_ROWS[0], list(range(7)), 7)
    keep = torch.zeros((B + 1, T_MAX), dtype=torch.int32)
    for b in range(B):
        keep[b, :len(keeps[b])] = torch.tensor(keeps[b], dtype=torch.int32)
    keep[B, :len(extra[2])] = torch.tensor(extra[2], dtype=torch.int32)
    st = ops.RouterState(keep.to(dev), torch.tensor(list(counts) + [extra[3]], dtype=torch.int32).to(dev),
                         torch.tensor(list(OFF) + [extra[0]], dtype=torch.int64).to(dev),
                         torch.tensor(list(N_ROWS) + [extra[1]], dtype=torch.int32).to(dev), list(counts))
    return st


def launch(dev, table_d, tokens_d, st, src_d, mid, out, token_rows=TOKEN_ROWS, table_rows=None):
    """The C entry point on a buffer with 4 sentinel rows in front of and behind the rows it may write."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    rows, H = src_d.numel(), tokens_d.shape[1]
    buf = torch.full((rows + 8, H), SENTINEL, dtype=out, device=dev)
    _lib.check(lib.slime_splice_routed(table_d.data_ptr(), ops.dtype_code(table_d.dtype), table_rows or table_d.shape[0], SEP_ID, tokens_d.data_ptr(),
                                       token_rows, st.off.data_ptr(), st.n_rows.data_ptr(), B, P, T_MAX, st.keep.data_ptr(),
                                       st.cnt.data_ptr(), ops.dtype_code(mid), src_d.data_ptr(), buf[4:].data_ptr(), ops.dtype_code(out),
                                       rows, H, torch.cuda.current_stream().cuda_stream), "slime_splice_routed")
    got = buf.cpu()
    assert bool((got[:4] == SENTINEL).all()) and bool((got[-4:] == SENTINEL).all()), "rows outside [0, rows) were written"
    return got[4:-4]


CASES = [(264, t, m, o) for t in DT for m in DT for o in DT] + \
        [(H, t, m, o) for H in (8, 4096) for t in ("bf16", "f32") for m in DT for o in DT]


@pytest.mark.parametrize("H,table_dt,mid_dt,out_dt", CASES, ids=lambda v: str(v))
def test_kernel_matches_todays_path_bit_for_bit(dev, H, table_dt, mid_dt, out_dt):
    """H = 8: the smallest legal row (one 16-byte piece of a 16-bit row); 264: a partial last 64-lane sweep; 4096: the product width."""
    from slime_amd import ops
    tokens, table32 = data(H)
    table = table32.to(DT[table_dt])
    mid, out = DT[mid_dt], DT[out_dt]
    tokens_d, table_d = tokens.to(dev), table.to(dev)
    for counts, keeps in KEEPS:
        rows = plan_rows(counts)
        assert len(rows) > 8 and len(rows) % 4 != 0
        src_d = encode(rows).to(dev)
        st = device_state(dev, keeps, counts)
        got = launch(dev, table_d, tokens_d, st, src_d, mid, out)
        want = expected(rows, tokens, table, keeps, counts, mid, out)
        assert_same_bits(got, want, f"counts {counts}")
        if counts == KEEPS[0][0]:                       # the wrapper makes the same call (B and T_max from the state's shapes)
            st3 = ops.RouterState(st.keep[:B].contiguous(), st.cnt[:B].contiguous(), st.off[:B].contiguous(), st.n_rows[:B].contiguous(),
                                  list(counts))
            assert_same_bits(ops.splice_routed(table_d, SEP_ID, tokens_d, P, st3, src_d, mid, out).cpu(), want, "ops.splice_routed")


@pytest.mark.parametrize("H,out_dt", [(264, "bf16"), (8, "f32")])
def test_backstop_zeroes_what_the_state_does_not_cover(dev, H, out_dt):
    """A row whose source the state does not cover is zeroed, not read: a position past the kept count, a keep index equal to
    n_rows[b], an image number equal to B, a token row past token_rows, a table id past the table.  Every index is chosen so that the
    row a kernel WITHOUT the guard would read lies inside the allocations (it would then write a non-zero row and fail here): this
    checks the guards, it cannot reach out of bounds."""
    tokens, table32 = data(H)
    out = DT[out_dt]
    tokens_d, table_d = tokens.to(dev), table32.to(torch.bfloat16).to(dev)
    assert bool((tokens.abs().sum(1) > 0).all())                     # no token row is all zeros: a zero output row means "not read"
    # image 0: count 2, but entry 2 holds a valid index; entry 1 is n_rows[0] = 7 (token row 12: image 1's first global row);
    # image 1 (no local rows): count 1 with index 0 = n_rows[1] (token row 17); image 2: count 4, all valid
    counts, keeps = (2, 1, 4), ([3, 7, 5], [0], [0, 1, 2, 3])
    rows = [("f", 0, P + 1 + 0), ("f", 0, P + 1 + 1), ("f", 0, P + 1 + 2), ("f", 0, P + 1 + 6),      # ok, idx == n_rows, j >= count twice
            ("f", 1, P + 1 + 0), ("f", 1, P), ("f", 2, P + 1 + 3), ("f", B, 0), ("f", B, P + 1), ("f", B, P),
            ("t", TABLE_ROWS - 2), ("t", TABLE_ROWS - 1), ("f", 2, 0)]                   # the call is told TABLE_ROWS - 1 table rows
    zero = [False, True, True, True, True, False, False, True, True, True, False, True, False]
    src_d = encode(rows).to(dev)
    st = device_state(dev, keeps, counts)
    got = launch(dev, table_d, tokens_d, st, src_d, torch.bfloat16, out, table_rows=TABLE_ROWS - 1)
    ok = [r for r, z in zip(rows, zero) if not z]
    want_ok = expected(ok, tokens, table32.to(torch.bfloat16), ([3], [], [0, 1, 2, 3]), (1, 0, 4), torch.bfloat16, out)
    k = 0
    for r, z in enumerate(zero):
        if z:
            assert bool((bits(got[r]) == 0).all()), f"row {r} {rows[r]} was read"
        else:
            assert_same_bits(got[r], want_ok[k], f"row {r} {rows[r]}")
            k += 1
    # token_rows smaller than the buffer: rows 20.. are outside, so image 2 keeps its first three global rows only
    rows = [("f", 2, p) for p in range(P + 1 + 4)] + [("f", 0, 0), ("z",)]
    got = launch(dev, table_d, tokens_d, st, encode(rows).to(dev), torch.bfloat16, out, token_rows=20)
    want = expected(rows, tokens, table32.to(torch.bfloat16), ([3], [], [0, 1, 2, 3]), (1, 0, 4), torch.bfloat16, out)
    for r, row in enumerate(rows):
        outside = row[0] == "f" and row[1] == 2 and row[2] != P and (OFF[2] - P + row[2] if row[2] < P else OFF[2] + row[2] - P - 1) >= 20
        if outside:
            assert bool((bits(got[r]) == 0).all()), f"row {r} {row} was read"
        else:
            assert_same_bits(got[r], want[r], f"row {r} {row}")


# ------------------------------------------------------------------------------------------------ the opt-in path
PT = 576                                                             # the tiny tower's patches per crop


def _batch(kind, dev, dtype):
    from slime_amd import weights as W
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    if kind == "uniform":                                            # 2 images of (1 + 2) crops, one grid
        counts, sizes, merge = [3, 3], [(672, 336), (672, 336)], "spatial"
    else:                                                            # crop-major order: grids (2, 1), (1, 1), (0, 0)
        counts, sizes, merge = [3, 2, 1], None, "flat"
    px = [W.synthetic_pixels(c, seed=80 + i).to(dev).to(dtype) for i, c in enumerate(counts)]
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, 2000, (len(counts), 12), generator=g)
    ids[:, 4] = IMAGE_TOKEN_INDEX
    ids[-1, 4], ids[-1, 9] = 17, IMAGE_TOKEN_INDEX                   # the last sequence meets its image late
    am = torch.ones_like(ids)
    am[0, -2:] = 0
    pos = torch.arange(12).expand_as(ids).contiguous()
    return counts, sizes, merge, px, ids.to(dev), am.to(dev), ids.clone().to(dev), pos.to(dev)


@pytest.mark.parametrize("kind", ["uniform", "ragged"])
@pytest.mark.parametrize("table_dt", ["bf16", "f32"])
@pytest.mark.parametrize("img_dt", ["bf16", "f16"])
def test_fused_splice_path_equals_the_flag_off_path(dev, monkeypatch, img_dt, table_dt, kind):
    from slime_amd import ops
    dtype = DT[img_dt]
    embed = nn.Embedding(2048, 256)
    embed.weight.data.copy_(torch.randn(2048, 256, generator=torch.Generator().manual_seed(3)) * 0.5)
    embed.to(DT[table_dt])
    counts, sizes, merge, px, ids, am, lab, pos = _batch(kind, dev, dtype)
    enc, _, _ = _tiny_encoder(dev, dtype, embed=embed, mm_patch_merge_type=merge)
    cfg, sampler = enc.config, enc.get_model().sampler
    assert cfg.fused_splice is False                                 # opt-in
    calls = []
    real = ops.splice_routed
    monkeypatch.setattr(ops, "splice_routed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def both(flag):
        cfg.fused_splice = flag
        n0 = len(calls)
        feats, _ = enc.encode_images(torch.cat(px, 0), ids, counts, am, None, sizes, labels=lab)
        out = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=sizes)
        return feats, out, len(calls) - n0

    # a cut inside the last image: its routed rows (uniform: 3 of them survive) / its global rows (ragged: the image has nothing else)
    cut = 9 + PT + 1 + 3 if kind == "uniform" else 9 + PT - 2
    for topp, side, max_len in ((0.95, "right", None), (0.5, "right", None), (0.0, "right", None), (0.95, "left", None),
                                (0.95, "right", cut), (0.5, "left", cut)):
        sampler.topp, cfg.tokenizer_padding_side, cfg.tokenizer_model_max_length = topp, side, max_len
        f0, o0, n_off = both(False)
        f1, o1, n_on = both(True)
        what = f"topp {topp}, {side}, max_len {max_len}"
        assert n_off == 0 and n_on == 2, what                        # one launch per call, and only with the flag
        kept = [f.shape[1] - PT - 1 for f in f0]
        n_local = [(c - 1) * 144 for c in counts]
        assert all(0 <= k <= n for k, n in zip(kept, n_local)), what
        if topp == 0.5:
            assert any(0 < k < n for k, n in zip(kept, n_local)), f"{what}: the gather is the identity ({kept} of {n_local})"
        if max_len == cut and kind == "uniform":
            assert kept[-1] > 3, what
        assert len(f0) == len(f1) == len(counts)
        for a, b in zip(f0, f1):
            assert a.dim() == 3 and a.shape[0] == 1
            assert_same_bits(b.cpu(), a.cpu(), what)
        assert o1[0] is None and o0[0] is None and o1[3] is None
        assert_same_bits(o1[4].cpu(), o0[4].cpu(), what)             # embeds
        assert o1[4].dtype == DT[table_dt] and (max_len is None or o1[4].shape[1] == max_len)
        for i in (1, 2, 5):                                          # position ids, mask, labels
            assert torch.equal(o1[i], o0[i]) and o1[i].dtype == o0[i].dtype, (what, i)
    # the flag is a no-op where no fused adapter call takes the batch
    cfg.fused_adapter = False
    sampler.topp, cfg.tokenizer_padding_side, cfg.tokenizer_model_max_length = 0.5, "right", None
    f0, o0, n_off = both(False)
    f1, o1, n_on = both(True)
    assert n_off == 0 and n_on == 0
    for a, b in zip(f0, f1):
        assert_same_bits(b.cpu(), a.cpu(), "fused_adapter=False")
    assert_same_bits(o1[4].cpu(), o0[4].cpu(), "fused_adapter=False")
    for i in (1, 2, 5):
        assert torch.equal(o1[i], o0[i])
