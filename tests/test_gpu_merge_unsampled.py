"""GPU tests of the un-sampled LLaVA-NeXT merge in the device splice (slime_splice_merged; mm_patch_merge_type 'spatial' /
'spatial_unpad' without a sampler): the kernel alone against a torch restatement -- bit for bit, every dtype combination, the
zeroing backstop, every refusal --, ``prepare_inputs_labels_for_multimodal`` against a yardstick built from ``encode_images``'
per-image features and a torch transcription of the merge rules, the row order against the reference's record
(tests/golden/merge_unsampled.npz), and the branches the feature leaves alone.  Everything is an equality: no tolerance."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import merge_unsampled_fixture as F

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
TOKEN_ROWS, EXTRA_ROWS, TABLE_ROWS = 11, 2, 9           # what the calls are told; every allocation holds one row more
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


# ------------------------------------------------------------------------------------------------ the kernel alone
_data = {}


def data(H):
    """fp32 tokens, table and extra rows, one row more than the calls are told, built once per width on the CPU; the values carry
    what a rounding can get wrong (+-0, subnormals of every format, round-to-even ties of bf16 and fp16, values infinite in fp16).
    No NaN: prefill.hip is built without NaN semantics."""
    if H not in _data:
        g = torch.Generator().manual_seed(200 + H)
        special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 3e-39, 1e-6, -3e-6, 6.0e-8, 2.0 ** -25,
                                1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 3 * 2.0 ** -11),
                                1 + 2.0 ** -8 + 2.0 ** -20, 1e5, -1e5, 65504.0, 65520.0, 3.3895e38])
        out = []
        for rows in (TOKEN_ROWS + 1, TABLE_ROWS + 1, EXTRA_ROWS + 1):
            t = torch.randn(rows, H, generator=g)
            flat = t.view(-1)
            flat[torch.arange(special.numel() * 3) * 5 % flat.numel()] = special.repeat(3)
            t[:, 0] += 0.5                                             # no row is all zeros: a zero output row means "not read"
            out.append(t)
        _data[H] = tuple(out)
    return _data[H]


def plan_rows():
    """('t', id) | ('z',) | ('k', token row) | ('e', extra row): every kind, the token rows out of order; the last two entries of the
    first group resolve outside their tensors -- a token index equal to token_rows + extra_rows and a table id equal to table_rows,
    both inside the allocations (a kernel without the guard would copy a non-zero row, not fault).  4 * k + 1 rows."""
    rows = [("t", 3), ("t", 0), ("t", TABLE_ROWS - 1), ("z",), ("e", 0), ("e", EXTRA_ROWS - 1), ("e", EXTRA_ROWS), ("t", TABLE_ROWS)]
    rows += [("k", k) for k in reversed(range(TOKEN_ROWS))] + [("z",), ("k", 0), ("e", 1), ("t", 5)]
    while len(rows) % 4 != 1:
        rows.append(("k", len(rows) % TOKEN_ROWS))
    return rows


def encode(rows):
    code = {"t": lambda r: r[1], "z": lambda r: -1, "k": lambda r: -2 - r[1], "e": lambda r: -2 - (TOKEN_ROWS + r[1])}
    return torch.tensor([code[r[0]](r) for r in rows], dtype=torch.int64)


def expected(rows, tokens, table, extra, mid, out):
    """The rule of include/slime_hip.h in torch on the CPU."""
    want = torch.zeros(len(rows), tokens.shape[1], dtype=out)
    for r, row in enumerate(rows):
        if row[0] == "t" and row[1] < TABLE_ROWS:
            want[r] = table[row[1]].to(out)                    # equal dtypes: a copy; else one cast
        elif row[0] == "k":
            want[r] = tokens[row[1]].to(mid).to(out)
        elif row[0] == "e" and row[1] < EXTRA_ROWS:
            want[r] = extra[row[1]].to(out)
    return want


def launch(dev, table_d, tokens_d, extra_d, src_d, mid, out):
    """The C entry point on a buffer with 4 sentinel rows in front of and behind the rows it may write."""
    from slime_amd import _lib, ops
    lib = _lib.load()
    rows, H = src_d.numel(), table_d.shape[1]
    buf = torch.full((rows + 8, H), SENTINEL, dtype=out, device=dev)
    _lib.check(lib.slime_splice_merged(table_d.data_ptr(), ops.dtype_code(table_d.dtype), TABLE_ROWS, tokens_d.data_ptr(), TOKEN_ROWS,
                                       ops.dtype_code(mid), extra_d.data_ptr(), ops.dtype_code(extra_d.dtype), EXTRA_ROWS, src_d.data_ptr(),
                                       buf[4:].data_ptr(), ops.dtype_code(out), rows, H, torch.cuda.current_stream().cuda_stream),
               "slime_splice_merged")
    got = buf.cpu()
    assert bool((got[:4] == SENTINEL).all()) and bool((got[-4:] == SENTINEL).all()), "rows outside [0, rows) were written"
    return got[4:-4]


@pytest.mark.parametrize("H", [8, 264])
@pytest.mark.parametrize("out_dt", list(DT))
@pytest.mark.parametrize("mid_dt", list(DT))
@pytest.mark.parametrize("table_dt", list(DT))
def test_kernel_matches_the_torch_restatement_bit_for_bit(dev, table_dt, mid_dt, out_dt, H):
    """H = 8: one 16-byte piece of a 16-bit row, most lanes idle; 264: an fp32 row of 1056 B, one full lane sweep plus a tail."""
    from slime_amd import ops
    tokens, table32, extra32 = data(H)
    mid, out = DT[mid_dt], DT[out_dt]
    table = table32.to(DT[table_dt])
    rows = plan_rows()
    assert len(rows) % 4 == 1 and len(rows) > 8
    src_d = encode(rows).to(dev)
    tokens_d, table_d = tokens.to(dev), table.to(dev)
    other = {"f32": "bf16", "bf16": "f16", "f16": "f32"}[out_dt]
    for extra_dt in (out_dt, other):                                     # a bit copy and a cast
        extra = extra32.to(DT[extra_dt])
        want = expected(rows, tokens, table, extra, mid, out)
        zero = [r for r, row in enumerate(rows) if row == ("e", EXTRA_ROWS) or row == ("t", TABLE_ROWS) or row == ("z",)]
        assert len(zero) >= 4 and all(bool((bits(want[r]) == 0).all()) for r in zero)
        got = launch(dev, table_d, tokens_d, extra.to(dev), src_d, mid, out)
        assert_same_bits(got, want, f"extra {extra_dt}")
    # the wrapper makes the same call on tensors of exactly the told sizes
    extra = extra32[:EXTRA_ROWS].to(out)
    got = ops.splice_merged(table_d[:TABLE_ROWS], tokens_d[:TOKEN_ROWS], extra.to(dev), src_d, mid, out)
    assert_same_bits(got.cpu(), expected(rows, tokens, table, extra, mid, out), "ops.splice_merged")


def test_wrapper_without_tokens_and_without_extra(dev):
    from slime_amd import ops
    tokens, table32, extra32 = data(264)
    table = table32[:TABLE_ROWS].to(torch.bfloat16)
    rows = [("t", 1), ("z",), ("k", 0), ("e", 0), ("t", 2)]              # the feature rows resolve outside: zeros
    got = ops.splice_merged(table.to(dev), None, None, encode(rows).to(dev), torch.bfloat16, torch.bfloat16).cpu()
    assert_same_bits(got[0], table[1])
    assert_same_bits(got[4], table[2])
    assert bool((bits(got[1:4]) == 0).all())
    with pytest.raises(Exception, match="GPU"):
        ops.splice_merged(table.to(dev), tokens, None, encode(rows).to(dev), torch.bfloat16, torch.bfloat16)


def test_every_refusal_names_its_limit(dev):
    from slime_amd import _lib
    lib = _lib.load()
    H = 64
    t = {k: torch.zeros(n, H, dtype=d, device=dev) for k, n, d in (("table", 100, torch.bfloat16), ("tokens", 50, torch.float32),
                                                                   ("extra", 1, torch.float32), ("out", 12, torch.bfloat16))}
    src = torch.full((12,), -1, dtype=torch.int64, device=dev)

    def call(**over):
        a = dict(table=t["table"].data_ptr(), table_dtype=_lib.BF16, table_rows=100, tokens=t["tokens"].data_ptr(), token_rows=50,
                 mid_dtype=_lib.BF16, extra=t["extra"].data_ptr(), extra_dtype=_lib.F32, extra_rows=1, src=src.data_ptr(),
                 out=t["out"].data_ptr(), out_dtype=_lib.BF16, rows=12, H=H, stream=torch.cuda.current_stream().cuda_stream)
        a.update(over)
        return lib.slime_splice_merged(*a.values()), lib.slime_last_error().decode()

    EINVAL = -1
    assert call()[0] == 0
    for name in ("src", "out", "table"):
        rc, msg = call(**{name: None})
        assert rc == EINVAL and "null" in msg and name in msg, (name, msg)
    for name in ("rows", "H"):
        for v in (0, -1):
            rc, msg = call(**{name: v})
            assert rc == EINVAL and f"{name}={v}" in msg and "positive" in msg, (name, msg)
    for name in ("table_rows", "token_rows", "extra_rows"):
        rc, msg = call(**{name: -1})
        assert rc == EINVAL and f"{name}=-1" in msg and "negative" in msg, (name, msg)
    for ptr, n in (("tokens", "token_rows"), ("extra", "extra_rows")):
        for over in ({ptr: None}, {n: 0}):
            rc, msg = call(**over)
            assert rc == EINVAL and ptr in msg and n in msg, msg
        assert call(**{ptr: None, n: 0})[0] == 0                         # NULL iff no rows
    for name in ("table_dtype", "mid_dtype", "extra_dtype", "out_dtype"):
        for v in (_lib.U8, -1, 17):
            rc, msg = call(**{name: v})
            assert rc == EINVAL and "dtype" in msg and f"{name.split('_')[0]} {v}" in msg, (name, msg)
    for Hbad, dt in ((4, _lib.BF16), (12, _lib.F16), (6, _lib.F32), (2, _lib.F32), (63, _lib.BF16)):
        rc, msg = call(H=Hbad, out_dtype=dt)
        assert rc == EINVAL and "16 bytes" in msg and f"H={Hbad}" in msg
    for name in ("out", "table", "tokens", "extra"):
        rc, msg = call(**{name: t[name].data_ptr() + 8})
        assert rc == EINVAL and "16-byte aligned" in msg and name in msg
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end
SIZES = [(640, 480), (300, 300), (900, 700), (1000, 333)]              # the one-crop image's size is never read
SPLITS = [5, 1, 7, 4]                                                    # 17 crops
MASKS = [[1, 1, 1, 0, 1, 1, 0], [1], [1, 1, 1, 1, 1, 1, 1], [1, 0, 1, 1, 0, 1]]       # exactly the grids' crops are marked
GRIDS = [(2, 2), None, (3, 2), (3, 1)]
VOCAB = 64


def _encoder(dev, dtype, embed, hidden=256, **cfg_over):
    """SlimeVisualEncoder at the tiny fixture geometry (tower 128 wide / 3 layers, 576 patches per crop), no sampler."""
    from slime_amd import weights as W
    from slime_amd.model.llava_arch import SlimeVisualEncoder, default_slime_config
    from slime_amd.model.multimodal_encoder.clip_encoder import HipCLIPVisionModel
    from slime_amd.image_processor import ClipImageProcessor
    from slime_amd.model.multimodal_projector.builder import GatedBlock, HipMlp
    cfg = default_slime_config("synthetic:1", hidden_size=hidden, mm_hidden_size=128, mm_resampler_type=None, **cfg_over)
    enc = SlimeVisualEncoder(cfg, embed_tokens=embed)
    vt = enc.get_vision_tower()
    vt.vision_tower = HipCLIPVisionModel(W.TINY)
    vt.image_processor = ClipImageProcessor()
    vt.is_loaded = True
    enc.load_visual_state(W.make_tower_state_dict(W.TINY, seed=11), None)
    asd = W.sub_state(W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12), "mm_projector.")
    proj = enc.get_model().mm_projector
    if isinstance(proj, GatedBlock):
        proj.load_state_dict(asd)
    elif isinstance(proj, HipMlp):
        proj.load_state_dict({k[len("projection."):]: v for k, v in asd.items() if k.startswith("projection.")})
    if hasattr(enc.get_model(), "image_newline"):
        with torch.no_grad():
            enc.get_model().image_newline.copy_(torch.randn(hidden, generator=torch.Generator().manual_seed(21)) + 2.0 ** -10)
    enc.to(dev)
    vt.vision_tower.to(dtype)
    return enc


def _embedding(table_dt, hidden=256):
    embed = nn.Embedding(VOCAB, hidden)
    embed.weight.data.copy_(torch.randn(VOCAB, hidden, generator=torch.Generator().manual_seed(3)) * 0.5)
    return embed.to(table_dt)


def _pixels(splits, dev, dtype):
    from slime_amd import weights as W
    return [W.synthetic_pixels(c, seed=60 + i).to(dev).to(dtype) for i, c in enumerate(splits)]


def _text(dev, n_seq=4, where=((3,), (5,), (4,), (9,))):
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    ids = torch.randint(3, VOCAB, (n_seq, 12), generator=torch.Generator().manual_seed(5))
    for b, cols in enumerate(where):
        for c in cols:
            ids[b, c] = IMAGE_TOKEN_INDEX
    am = torch.ones_like(ids)
    am[0, -2:] = 0
    if n_seq > 2:
        am[2, :1] = 0                                                    # a masked token in front
    lab = torch.where(ids == IMAGE_TOKEN_INDEX, torch.full_like(ids, -100), ids + 1000)
    pos = torch.arange(12).expand_as(ids).contiguous()
    return ids.to(dev), am.to(dev), lab.to(dev), pos.to(dev)


def _window(size, cur_h, cur_w):
    """The rows and columns 'spatial_unpad' keeps: Python float division and int(), padding = (cur - new) // 2 from both ends."""
    w, h = size
    if w / h > cur_w / cur_h:
        pad = (cur_h - int(h * (cur_w / w))) // 2
        return pad, cur_h - pad, 0, cur_w
    pad = (cur_w - int(w * (cur_h / h))) // 2
    return 0, cur_h, pad, cur_w - pad


def _merge(f, size, grid, mask, merge_type, newline):
    """One image's feature rows from its [crops, 576, H] features: a torch transcription of the merge rules."""
    H = f.shape[-1]
    if f.shape[0] == 1:
        return torch.cat([f[0], newline[None].to(f.device)], 0) if "unpad" in merge_type else f[0]     # cat promotes; values unchanged
    base, loc = f[0], f[1:]
    if mask is not None:
        loc = loc[torch.nonzero(torch.tensor(mask[1:])).squeeze(1).to(f.device)]
    nw, nh = grid
    assert loc.shape[0] == nw * nh
    x = loc.view(nh, nw, 24, 24, H).permute(0, 2, 1, 3, 4).reshape(nh * 24, nw * 24, H)
    if "unpad" in merge_type:
        r0, r1, c0, c1 = _window(size, nh * 24, nw * 24)
        x = x[r0:r1, c0:c1]
        x = torch.cat([x, torch.zeros_like(x[:, :1])], 1)
    return torch.cat([base, x.reshape(-1, H)], 0)


def _yardstick(table, feats, ids, am, lab, max_len, side):
    """Per-sequence embed, cat, cut, pad (llava_arch.py:362-459) on the device with plain torch; every piece is cast to the table's
    dtype on its own (casts are element-wise: the same values as one cast of the concatenation)."""
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    out_dt, H = table.dtype, table.shape[1]
    seqs, labs, img = [], [], 0
    for b in range(ids.shape[0]):
        keep = am[b].bool()
        t, y = ids[b][keep], lab[b][keep]
        where = torch.nonzero(t == IMAGE_TOKEN_INDEX).squeeze(1).tolist()
        if not where:
            seqs.append(table[t]); labs.append(y); img += 1
            continue
        pe, pl, prev = [], [], 0
        for w in where:
            pe += [table[t[prev:w]], feats[img].to(out_dt)]
            pl += [y[prev:w], torch.full((feats[img].shape[0],), -100, dtype=y.dtype, device=y.device)]
            img, prev = img + 1, w + 1
        pe.append(table[t[prev:]]); pl.append(y[prev:])
        seqs.append(torch.cat(pe, 0)); labs.append(torch.cat(pl, 0))
    if max_len is not None:
        seqs, labs = [s[:max_len] for s in seqs], [l[:max_len] for l in labs]
    T = max(s.shape[0] for s in seqs)
    emb = torch.zeros((len(seqs), T, H), dtype=out_dt, device=table.device)
    nl = torch.full((len(seqs), T), -100, dtype=lab.dtype, device=lab.device)
    nm, npos = torch.zeros_like(nl).to(am.dtype), torch.zeros_like(nl)
    for b, (s, l) in enumerate(zip(seqs, labs)):
        n = s.shape[0]
        sl = slice(T - n, T) if side == "left" else slice(0, n)
        emb[b, sl], nl[b, sl], nm[b, sl], npos[b, sl] = s, l, 1, torch.arange(n, device=nl.device)
    return emb, nl, nm, npos


def _check(enc, dev, px, ids, am, lab, pos, sizes, grids, masks, what):
    cfg, model = enc.config, enc.get_model()
    splits = [p.shape[0] for p in px]
    imask = None if masks is None else [torch.tensor(m, device=dev) for m in masks]
    feats, _ = enc.encode_images(torch.cat(px, 0), ids, splits, am, imask, sizes, labels=lab)
    assert [tuple(f.shape[:2]) for f in feats] == [(s, 576) for s in splits]                  # encode_images is unchanged: [1 + n, P, H]
    newline = getattr(model, "image_newline", None)
    merged = [_merge(f, sizes[i], grids[i], None if masks is None else masks[i], cfg.mm_patch_merge_type, newline)
              for i, f in enumerate(feats)]
    want = _yardstick(model.embed_tokens.weight.detach(), merged, ids, am, lab, getattr(cfg, "tokenizer_model_max_length", None),
                      getattr(cfg, "tokenizer_padding_side", "right"))
    got = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=sizes, images_mask=imask)
    assert got[0] is None and got[3] is None
    assert_same_bits(got[4].cpu(), want[0].cpu(), what)
    for g, w in ((got[5], want[1]), (got[2], want[2]), (got[1], want[3])):
        assert g.dtype == w.dtype and torch.equal(g, w), what
    return merged, got


@pytest.mark.parametrize("merge_type", ["spatial", "spatial_unpad"])
@pytest.mark.parametrize("table_dt", ["bf16", "f32"])
@pytest.mark.parametrize("img_dt", ["f16", "bf16"])
@pytest.mark.parametrize("projector", ["mlp2x_gelu", "gated"])
def test_prepare_inputs_equals_the_materialising_yardstick(dev, monkeypatch, projector, img_dt, table_dt, merge_type):
    from slime_amd import ops
    dtype = DT[img_dt]
    enc = _encoder(dev, dtype, _embedding(DT[table_dt]), mm_projector_type=projector, mm_patch_merge_type=merge_type)
    calls = []
    real = ops.splice_merged
    monkeypatch.setattr(ops, "splice_merged", lambda *a, **k: (calls.append(a[4]), real(*a, **k))[1])
    monkeypatch.setattr(ops, "splice_rows", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the materialising splice ran")))
    px = _pixels(SPLITS, dev, dtype)
    ids, am, lab, pos = _text(dev)
    merged, got = _check(enc, dev, px, ids, am, lab, pos, SIZES, GRIDS, None, "right")
    unpad = merge_type == "spatial_unpad"
    assert [m.shape[0] for m in merged] == ([2340, 577, 3600, 2328] if unpad else [2880, 576, 4032, 2304])
    assert calls == [dtype] and got[4].dtype == DT[table_dt]                     # one launch; the middle rounding is the images' dtype
    if (projector, img_dt, table_dt) == ("mlp2x_gelu", "bf16", "bf16"):          # the glue's branches, once per merge type
        enc.config.tokenizer_padding_side = "left"
        _check(enc, dev, px, ids, am, lab, pos, SIZES, GRIDS, None, "left")
        enc.config.tokenizer_padding_side = "right"
        # sequence 1: 5 text rows, then its image; the cut leaves 300 of the second image's rows
        enc.config.tokenizer_model_max_length = 305
        _, cut = _check(enc, dev, px, ids, am, lab, pos, SIZES, GRIDS, None, "cut inside the second image")
        assert cut[4].shape[1] == 305
        enc.config.tokenizer_model_max_length = None
        pxm = _pixels([len(m) for m in MASKS], dev, dtype)
        _check(enc, dev, pxm, ids, am, lab, pos, SIZES, GRIDS, MASKS, "images_mask")
        assert len(calls) == 4


# ------------------------------------------------------------------------------------------------ the reference's order
@pytest.mark.parametrize("name", [n for n in F.case_names() if "single" not in n])
def test_row_order_equals_the_reference_record(dev, name):
    """mm_projector_type='identity', hidden_size = mm_hidden_size: the recorded position codes, applied to encode_images' features,
    the table and image_newline, give new_input_embeds bit for bit."""
    c = F.case(name)
    D = 128
    enc = _encoder(dev, torch.bfloat16, _embedding(torch.float32, D), hidden=D, mm_projector_type="identity", mm_patch_merge_type=c.merge_type)
    enc.config.tokenizer_padding_side, enc.config.tokenizer_model_max_length = c.side, c.max_length
    px = _pixels(c.splits, dev, torch.bfloat16)
    ids, am, lab = (torch.from_numpy(x).to(dev) for x in (c.ids, c.am, c.lab))
    pos = torch.arange(ids.shape[1], device=dev).expand_as(ids).contiguous()
    imask = None if c.masks is None else [torch.tensor(m, device=dev) for m in c.masks]
    feats, _ = enc.encode_images(torch.cat(px, 0), ids, c.splits, am, imask, c.sizes, labels=lab)
    assert all(f.dtype == torch.float32 for f in feats)                      # IdentityMap hands the tower's fp32 features through
    flat = torch.cat([f.reshape(-1, D) for f in feats], 0).cpu()
    table = enc.get_model().embed_tokens.weight.detach().cpu()
    codes = torch.from_numpy(c.codes)
    marker, a, b = codes >> 40, (codes >> 20) & 0xfffff, codes & 0xfffff
    want = torch.zeros(codes.shape + (D,), dtype=table.dtype)
    want[marker == F.M_FEATURE] = flat[(a * F.P + b)[marker == F.M_FEATURE]]
    want[marker == F.M_TABLE] = table[a[marker == F.M_TABLE]]
    if bool((marker == F.M_NEWLINE).any()):
        want[marker == F.M_NEWLINE] = enc.get_model().image_newline.detach().cpu().to(table.dtype)
    got = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=c.sizes, images_mask=imask)
    assert_same_bits(got[4].cpu(), want, name)
    assert np.array_equal(got[5].cpu().numpy(), c.new_lab) and np.array_equal(got[2].cpu().numpy(), c.new_mask)
    assert np.array_equal(got[1].cpu().numpy(), c.new_pos)


# ------------------------------------------------------------------------------------------------ what the feature leaves alone
def test_flat_unsampled_branch_is_unchanged(dev, monkeypatch):
    from slime_amd import ops
    enc = _encoder(dev, torch.bfloat16, _embedding(torch.bfloat16), mm_projector_type="mlp2x_gelu", mm_patch_merge_type="flat")
    monkeypatch.setattr(ops, "splice_merged", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the merged splice ran")))
    px = _pixels([3, 1, 2], dev, torch.bfloat16)
    ids, am, lab, pos = _text(dev, 3, ((3,), (5,), (4,)))
    feats, _ = enc.encode_images(torch.cat(px, 0), ids, [3, 1, 2], am, None, None, labels=lab)
    want = _yardstick(enc.get_model().embed_tokens.weight.detach(), [f.flatten(0, 1) for f in feats], ids, am, lab, None, "right")
    got = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px)
    assert_same_bits(got[4].cpu(), want[0].cpu(), "flat")
    assert torch.equal(got[5], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[1], want[3])


@pytest.mark.parametrize("fused_splice", [False, True])
def test_sampler_branch_is_unchanged(dev, monkeypatch, fused_splice):
    from slime_amd import ops
    from test_gpu_modules import _tiny_encoder
    embed = nn.Embedding(2048, 256)
    embed.weight.data.copy_(torch.randn(2048, 256, generator=torch.Generator().manual_seed(3)) * 0.5)
    enc, _, _ = _tiny_encoder(dev, torch.bfloat16, embed=embed.to(torch.bfloat16), mm_patch_merge_type="spatial", fused_splice=fused_splice)
    monkeypatch.setattr(ops, "splice_merged", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the merged splice ran")))
    px = _pixels([3, 3], dev, torch.bfloat16)
    sizes = [(672, 336), (672, 336)]
    ids, am, lab, pos = _text(dev, 2, ((3,), (5,)))
    feats, _ = enc.encode_images(torch.cat(px, 0), ids, [3, 3], am, None, sizes, labels=lab)
    assert all(f.dim() == 3 and f.shape[0] == 1 and f.shape[1] > 577 for f in feats)
    want = _yardstick(enc.get_model().embed_tokens.weight.detach(), [f[0] for f in feats], ids, am, lab, None, "right")
    got = enc.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=sizes)
    assert_same_bits(got[4].cpu(), want[0].cpu(), f"sampler, fused_splice={fused_splice}")
    assert torch.equal(got[5], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[1], want[3])
