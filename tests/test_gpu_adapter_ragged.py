"""GPU tests of the ragged fused adapter (slime_adapter_forward_ragged): a batch whose images have different crop counts and grids
through ONE launch sequence.  Tolerances are the project's own: rel-L2 < 1e-6 against the uniform fused call on each image alone (same
kernels on the same rows, only the GEMMs' M differs -- test_fused_adapter_equals_module_sequence's bound) and test_gpu_path.py's
per-stage bounds against the fp32 oracle (fp16 1.2e-3, bf16 8e-3; 1.5x at the end of the tower -> adapter chain)."""
import pytest
import torch
import torch.nn as nn

from conftest import rel_l2
from test_gpu_modules import _tiny_encoder

pytestmark = pytest.mark.gpu
TOL = {torch.float16: 1.2e-3, torch.bfloat16: 8e-3}
GRIDS = [(2, 1), (1, 3), (0, 0), (3, 2)]                                  # 2, 3, 0 and 6 local crops: 15 crops with the global views
SIZES = [(672, 336), (336, 1008), (336, 336), (1008, 700)]                # image sizes the slicer maps onto those grids (image 2: 1 crop)
P, Q, G = 576, 144, 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from slime_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _per_image_uniform(ops, pg, post, feats, grids, merge, gated):
    """slime_adapter_forward on every image alone (B = 1, its own grid; post = None for an image without local crops): fp32 [rows_i, H]."""
    outs, c = [], 0
    for nw, nh in grids:
        n = nw * nh
        f = feats[c:c + 1 + n]
        c += 1 + n
        if n == 0:
            outs.append(ops.adapter_forward(pg, None, f, 1, 0, 1, 1, False, gated, torch.float32)[0])
        elif merge:
            outs.append(ops.adapter_forward(pg, post, f, 1, n, nw, nh, True, gated, torch.float32)[0])
        else:
            outs.append(ops.adapter_forward(pg, post, f, 1, n, n, 1, False, gated, torch.float32)[0])
    return outs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("gated", [-1, 0, 1])
def test_ragged_fused_equals_per_image_uniform_fused(dev, dtype, gated):
    """Four images with grids 2x1, 1x3, none, 3x2 in one ragged call against the uniform call on each image alone: spatial and flat
    order in fp32, and T-typed output into a wider buffer whose images sit in another order with gaps (gap rows keep their value)."""
    from slime_amd import ops
    enc, _, _ = _tiny_encoder(dev, dtype, mm_learnable_gated=gated)
    model = enc.get_model()
    pg = model.mm_projector.packed(dtype)
    post = model.sampler.post_qformer.packed(P, dtype)
    feats = torch.randn(15, P, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(7)).to(dtype)
    own = [P + nw * nh * Q for nw, nh in GRIDS]
    ref = _per_image_uniform(ops, pg, post, feats, GRIDS, True, gated)
    out, row0 = ops.adapter_forward_ragged(pg, post, feats, GRIDS, True, gated, torch.float32)
    assert out.shape == (sum(own), 256) and out.dtype == torch.float32 and row0 == [sum(own[:i]) for i in range(4)]
    for i in range(4):
        err = rel_l2(out[row0[i]:row0[i] + own[i]].cpu(), ref[i].cpu())
        print(f"ragged vs uniform, {dtype}, gated {gated}, image {i} grid {GRIDS[i]}: rel-L2 {err:.3e}")
        assert ref[i].shape == (own[i], 256) and err < 1e-6, (i, err)
    # flat order: (n_i, 1)
    flat_grids = [(nw * nh, 1) if nw else (0, 0) for nw, nh in GRIDS]
    ref_flat = _per_image_uniform(ops, pg, post, feats, flat_grids, False, gated)
    flat, row0f = ops.adapter_forward_ragged(pg, post, feats, flat_grids, False, gated, torch.float32)
    assert row0f == row0
    for i in range(4):
        assert rel_l2(flat[row0[i]:row0[i] + own[i]].cpu(), ref_flat[i].cpu()) < 1e-6, i
    # T-typed output, images 3, 0, 2, 1 from the top of a wider buffer with 5 + i untouched rows in front of each
    order, r0, o = (3, 0, 2, 1), [0] * 4, 0
    for i in order:
        o += 5 + i
        r0[i] = o
        o += own[i]
    wide = torch.full((o + 9, 256), 3.0, dtype=dtype, device=dev)
    got, r0_back = ops.adapter_forward_ragged(pg, post, feats, GRIDS, True, gated, out=wide, out_row0=r0)
    assert got is wide and r0_back == r0
    owned = torch.zeros(wide.shape[0], dtype=torch.bool, device=dev)
    for i in range(4):
        rows = wide[r0[i]:r0[i] + own[i]]
        want = out[row0[i]:row0[i] + own[i]]
        assert torch.equal(rows, want.to(dtype)) or rel_l2(rows.float().cpu(), want.cpu()) < 2e-3, i
        owned[r0[i]:r0[i] + own[i]] = True
    assert int((~owned).sum()) == 5 * 4 + 6 + 9 and bool((wide[~owned] == 3.0).all())


@pytest.fixture(scope="module")
def ragged_oracle():
    """The fp32 oracle's global and merged rows of the four images (tiny geometry), computed once for both operand types."""
    from slime_amd import weights as W
    from oracle import slime_oracle as O
    tsd = W.strip_tower_prefix(W.make_tower_state_dict(W.TINY, seed=11))
    asd = W.make_adapter_state_dict(W.ADAPTER_TINY, seed=12)
    assert [tuple(O.anyres_grid_shape(s)) for s in SIZES[:2] + SIZES[3:]] == GRIDS[:2] + GRIDS[3:]
    px, ref = [], []
    for i, (nw, nh) in enumerate(GRIDS):
        px.append(W.synthetic_pixels(1 + nw * nh, seed=90 + i))
        if nw:
            r = O.encode_image(tsd, asd, W.TINY, W.ADAPTER_TINY, px[i], SIZES[i])
            ref.append((r["global"], r["merged"]))
        else:       # one crop: encode_image's global stage alone (llava_arch.py:222-224), there is nothing to compress or merge
            f = O.tower_forward(tsd, W.TINY, px[i])
            ref.append((O.gated_block_forward(W.sub_state(asd, "mm_projector."), f[0], W.ADAPTER_TINY.num_heads), None))
    return px, ref


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ragged_encode_visual_vs_oracle(dev, dtype, ragged_oracle):
    """SlimeVisualEncoder.encode_visual on the four-image ragged batch (pixels -> tower -> ragged fused adapter): the global and the
    merged local rows of every image against the oracle, at the end-of-chain bound of test_encode_images_vs_oracle."""
    px, ref = ragged_oracle
    enc, _, _ = _tiny_encoder(dev, dtype)
    counts = [1 + nw * nh for nw, nh in GRIDS]
    pairs = enc.encode_visual(torch.cat(px, 0).to(dev).to(dtype), counts, SIZES, merge="spatial")
    assert len(pairs) == 4
    for i, (glob, merged) in enumerate(pairs):
        assert glob.shape == (P, 256) and merged.shape == ((counts[i] - 1) * Q, 256) and glob.dtype == merged.dtype == torch.float32
        eg = rel_l2(glob.cpu(), ref[i][0])
        el = rel_l2(merged.cpu(), ref[i][1]) if ref[i][1] is not None else 0.0
        print(f"ragged encode_visual vs oracle, {dtype}, image {i}: global {eg:.3e}, merged {el:.3e}")
        assert eg < TOL[dtype] * 1.5 and el < TOL[dtype] * 1.5, (i, eg, el)


def test_encode_images_takes_the_ragged_fused_path(dev, monkeypatch):
    """encode_images (router and separator) on images with 2, 4 and 6 local crops: ONE ragged fused call and no merge_rows launch; each
    output is [1, 576 + 1 + k, H] in the input dtype, row 576 the separator, and the k routed rows are rows of encode_visual's merged
    tokens cast to that dtype, bit for bit and in ascending order."""
    from slime_amd import ops, weights as W
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    from oracle import slime_oracle as O
    dtype = torch.bfloat16
    torch.manual_seed(0)
    embed = nn.Embedding(2000, 256).to(dev)
    enc, _, _ = _tiny_encoder(dev, dtype, embed=embed)
    sizes = [(336, 336), (672, 672), (1344, 1344)]
    counts = [1 + O.anyres_grid_shape(s)[0] * O.anyres_grid_shape(s)[1] for s in sizes]
    assert counts == [3, 5, 7]
    images = torch.cat([W.synthetic_pixels(c, seed=50 + i) for i, c in enumerate(counts)], 0).to(dev).to(dtype)
    ids = torch.randint(3, 1900, (3, 12), device=dev)
    ids[:, 4] = IMAGE_TOKEN_INDEX
    am = torch.ones_like(ids)
    am[:, -2:] = 0
    calls = {"ragged": 0, "merge_rows": 0}
    real_ragged, real_merge = ops.adapter_forward_ragged, ops.merge_rows

    def spy_ragged(*a, **kw):
        calls["ragged"] += 1
        return real_ragged(*a, **kw)

    def spy_merge(*a, **kw):
        calls["merge_rows"] += 1
        return real_merge(*a, **kw)
    monkeypatch.setattr(ops, "adapter_forward_ragged", spy_ragged)
    monkeypatch.setattr(ops, "merge_rows", spy_merge)
    feats, ss = enc.encode_images(images, input_ids=ids, split_sizes=counts, attention_mask=am, image_sizes=sizes)
    assert calls == {"ragged": 1, "merge_rows": 0} and ss == counts and len(feats) == 3
    pairs = enc.encode_visual(images, counts, sizes, merge="spatial")
    assert calls == {"ragged": 2, "merge_rows": 0}
    sep = embed(torch.tensor(enc.config.seperator, device=dev)).to(dtype)
    for i, out in enumerate(feats):
        assert out.dim() == 3 and out.shape[0] == 1 and out.shape[2] == 256 and out.dtype == dtype
        out = out[0]
        k = out.shape[0] - 577
        assert 0 < k <= (counts[i] - 1) * Q
        assert torch.equal(out[:576], pairs[i][0].to(dtype)) and torch.equal(out[576], sep)
        cand = pairs[i][1].to(dtype)
        idx = torch.cdist(out[577:].float(), cand.float()).argmin(1)              # cdist only identifies the rows
        assert torch.equal(out[577:], cand[idx]) and bool((idx[1:] > idx[:-1]).all())


def test_ragged_fused_full_dims_vs_uniform_and_oracle(dev):
    """SliME-8B adapter dims (1024 -> 4096, 8 heads), bf16, two images with grids 2x1 and 2x2 (8 crops of tower-like features: unit-
    variance tokens with a per-crop offset): ragged == uniform per image at 1e-6, every image against the fp32 oracle at
    test_fused_adapter_bench_shape_vs_oracle's bound (bf16 8e-3); a grid that does not match the crops in feats raises."""
    from slime_amd import ops, weights as W
    from slime_amd._lib import SlimeHipError
    from oracle import slime_oracle as O
    dtype, A = torch.bfloat16, W.ADAPTER_8B
    asd = W.make_adapter_state_dict(A, seed=4321)
    proj_sd, post_sd = W.sub_state(asd, "mm_projector."), W.sub_state(asd, "sampler.post_qformer.")
    pg = ops.pack_gated(proj_sd, A, dtype, dev)
    post = ops.pack_resampler(post_sd, 1024, 8, 576, dtype, dev, A.ln_eps)
    grids = [(2, 1), (2, 2)]
    g = torch.Generator().manual_seed(31)
    feats = (torch.randn(8, 576, 1024, generator=g) + 0.3 * torch.randn(8, 1, 1024, generator=g)).to(dtype)
    fd = feats.to(dev)
    out, row0 = ops.adapter_forward_ragged(pg, post, fd, grids, True, -1, torch.float32)
    ref = _per_image_uniform(ops, pg, post, fd, grids, True, -1)
    assert out.shape == (2 * 576 + 6 * 144, 4096) and row0 == [0, 576 + 2 * 144]
    c = 0
    for i, (nw, nh) in enumerate(grids):
        n = nw * nh
        mine = out[row0[i]:row0[i] + 576 + n * 144]
        eu = rel_l2(mine.cpu(), ref[i].cpu())
        f = feats[c:c + 1 + n].float()                                       # the oracle sees the same (rounded) features
        c += 1 + n
        glob = O.gated_block_forward(proj_sd, f[0], A.num_heads)
        merged = O.spatial_merge(O.mlp_projector(proj_sd, O.resampler_forward(post_sd, f[1:], A.num_heads, A.ln_eps)), nw, nh, 12)
        eg, el = rel_l2(mine[:576].cpu(), glob), rel_l2(mine[576:].cpu(), merged)
        print(f"ragged adapter, 8B dims, image {i} grid {nw}x{nh}: vs uniform {eu:.3e}, vs oracle global {eg:.3e} merged {el:.3e}")
        assert eu < 1e-6 and eg < 8e-3 and el < 8e-3, (i, eu, eg, el)
    with pytest.raises(SlimeHipError, match="crops"):
        ops.adapter_forward_ragged(pg, post, fd, [(2, 1), (3, 2)], True, -1, torch.float32)


def test_uniform_batch_keeps_the_uniform_call(dev, monkeypatch):
    """Dispatch order: a uniform batch (3 x (1 + 4), 2 x 2) still goes through slime_adapter_forward -- encode_visual is bit-equal to
    ops.adapter_forward on the same tower features -- and never reaches the ragged entry point."""
    from slime_amd import ops, weights as W
    dtype = torch.bfloat16
    enc, _, _ = _tiny_encoder(dev, dtype)
    model = enc.get_model()
    images = W.synthetic_pixels(15, seed=61).to(dev).to(dtype)

    def no_ragged(*a, **kw):
        raise AssertionError("a uniform batch took the ragged call")
    monkeypatch.setattr(ops, "adapter_forward_ragged", no_ragged)
    pairs = enc.encode_visual(images, [5, 5, 5], [(672, 672)] * 3, merge="spatial")
    feats = enc.get_vision_tower()(images, out_dtype=dtype)
    tokens = ops.adapter_forward(model.mm_projector.packed(dtype), model.sampler.post_qformer.packed(576, dtype), feats, 3, 4, 2, 2, True, -1,
                                 torch.float32)
    for i in range(3):
        assert torch.equal(pairs[i][0], tokens[i, :576]) and torch.equal(pairs[i][1], tokens[i, 576:])
