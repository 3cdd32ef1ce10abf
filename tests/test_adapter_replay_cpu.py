"""CPU companion of tests/test_gpu_adapter_conformance.py: the replay is the right mathematics and the chosen layouts discriminate.

  * every ``replay_*`` of tests/adapter_conformance.py, run on the torch backend with unrounded fp32 operands, equals the oracle
    (oracle/slime_oracle.py) within the 2e-5 rel-L2 DESIGN.md section 2 states for the oracle itself, at every layout of the GPU module;
  * the row maps agree with the code that exists already (ops.adapter_ragged_plan) and with oracle.spatial_merge;
  * every deliberately broken glue variant changes the torch-backend replay at every layout where it can show at all
    (``adapter_conformance.applies``, reasoned from the layout alone), and every variant shows at one layout at least: a GPU run
    that is bit-equal to the replay at these layouts cannot hide one of them.
"""
import math

import pytest
import torch

import adapter_conformance as AC
from conftest import rel_l2

ORACLE_TOL = 2e-5
LAYOUT_IDS = sorted(AC.LAYOUTS)
UNIFORM_BROKEN = [b for b in AC.BROKEN if not b.startswith("ragged_")]
RAGGED_BROKEN = [b for b in AC.BROKEN if b.startswith("ragged_")]
_cache = {}


def tiny(name):
    if name not in _cache:
        _cache[name] = AC.make_tiny(AC.LAYOUTS[name], torch.float32, "cpu")
    return _cache[name]


def _oracle_image(t, f, nw, nh, merge, gated):
    """Oracle tokens of one image: f fp32 [1 + n, P, D] -> [P + n q, H]."""
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    L = t.layout
    proj, post = W.sub_state(t.sd, "mm_projector."), W.sub_state(t.sd, "sampler.post_qformer.")
    parts = [O.gated_block_forward(proj, f[:1], L.heads, gated, target_len=L.P)[0]]
    if f.shape[0] > 1:
        loc = O.mlp_projector(proj, O.resampler_forward(post, f[1:], L.heads, t.cfg.ln_eps))
        parts.append(O.spatial_merge(loc, nw, nh, L.g) if merge else loc.flatten(0, 1))
    return torch.cat(parts)


def _uniform(t, feats, gated, merge, stride, broken=None):
    L = t.layout
    be = AC.TorchBackend(None)
    out = torch.full((L.n_images * stride, L.H), -7.0, dtype=torch.float64)
    nw, nh = (L.nw, L.nh) if merge else (L.n_local, 1 if L.n_local else 0)
    AC.replay_adapter(be, t, feats, L.n_images, L.n_local, nw, nh, merge, gated, out, stride, broken)
    return out.view(L.n_images, stride, L.H)


@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_replay_parts_vs_oracle(name):
    """replay_resampler, replay_mlp (fp32 and T input) and replay_gated (-1 / 0 / 1) against the oracle's functions."""
    from oracle import slime_oracle as O
    from slime_amd import weights as W
    t, L, be = tiny(name), AC.LAYOUTS[name], AC.TorchBackend(None)
    proj, post = W.sub_state(t.sd, "mm_projector."), W.sub_state(t.sd, "sampler.post_qformer.")
    x = AC.make_feats(3, L.P, L.D, None, seed=11)
    got = AC.replay_resampler(be, t.post, x.reshape(-1, L.D), 3)[0]
    assert rel_l2(got, O.resampler_forward(post, x, L.heads, t.cfg.ln_eps).reshape(-1, L.D)) < ORACLE_TOL
    rows = x.reshape(-1, L.D)[:5]
    for is_t in (False, True):
        assert rel_l2(AC.replay_mlp(be, t.pg.mlp, rows, is_t), O.mlp_projector(proj, rows)) < ORACLE_TOL
    for gated in (-1, 0, 1):
        got = AC.replay_gated(be, t.pg, x.reshape(-1, L.D), 3, gated)
        assert rel_l2(got, O.gated_block_forward(proj, x, L.heads, gated, target_len=L.P).reshape(-1, L.H)) < ORACLE_TOL, gated


@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_replay_adapter_vs_oracle(name):
    t, L = tiny(name), AC.LAYOUTS[name]
    feats = AC.make_feats(L.n_crops, L.P, L.D, None)
    stride = L.rows_per_image + 5
    for gated in (-1, 0, 1):
        for merge in (0, 1):
            out = _uniform(t, feats, gated, merge, stride)
            for i in range(L.n_images):
                ref = _oracle_image(t, feats[i * (1 + L.n_local):(i + 1) * (1 + L.n_local)], L.nw, L.nh, merge, gated)
                assert rel_l2(out[i, :L.rows_per_image], ref) < ORACLE_TOL, (gated, merge, i)
            assert bool((out[:, L.rows_per_image:] == -7.0).all())


@pytest.mark.parametrize("grids", AC.RAGGED_GRIDS, ids=str)
def test_replay_ragged_vs_oracle(grids):
    t, L = tiny("a"), AC.LAYOUTS["a"]
    n_crops = sum(1 + nw * nh for nw, nh in grids)
    feats = AC.make_feats(n_crops, L.P, L.D, None, seed=8)
    rows = [L.P + nw * nh * L.q for nw, nh in grids]
    gaps, r = [], 2
    for x in rows:
        gaps.append(r)
        r += x + 3
    for row0, total in ((None, sum(rows)), (gaps, r + 4)):
        for merge in (0, 1):
            for gated in (-1, 1):
                out = torch.full((total, L.H), -7.0, dtype=torch.float64)
                g_ = grids if merge else [(nw * nh, 1 if nw * nh else 0) for nw, nh in grids]
                AC.replay_adapter_ragged(AC.TorchBackend(None), t, feats, g_, merge, gated, out, row0)
                owned, c, o = torch.zeros(total, dtype=torch.bool), 0, 0
                for i, (nw, nh) in enumerate(grids):
                    start = o if row0 is None else row0[i]
                    ref = _oracle_image(t, feats[c:c + 1 + nw * nh], nw, nh, merge, gated)
                    assert rel_l2(out[start:start + rows[i]], ref) < ORACLE_TOL, (merge, gated, i)
                    owned[start:start + rows[i]] = True
                    c, o = c + 1 + nw * nh, o + rows[i]
                assert bool((out[~owned] == -7.0).all())


@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_row_maps_agree(name):
    """row_map_uniform == ops.adapter_ragged_plan on equal grids == the row order of oracle.spatial_merge."""
    from oracle import slime_oracle as O
    L = AC.LAYOUTS[name]
    stride = L.rows_per_image + 5
    for merge in (0, 1):
        nw, nh = (L.nw, L.nh) if merge else (L.n_local, 1 if L.n_local else 0)
        rm = AC.row_map_uniform(L.n_images, L.P, L.n_local, L.q, nw, merge, stride, nh)
        row0 = [i * stride for i in range(L.n_images)]
        _, _, rr = AC.ragged_row_map([(nw, nh)] * L.n_images, L.P, L.q if L.n_local else 1, merge, row0)
        assert rm == rr
        assert len(set(rm)) == len(rm)
        if L.n_local:
            own = torch.arange(L.n_local * L.q, dtype=torch.float32).reshape(L.n_local, L.q, 1)
            merged = (O.spatial_merge(own, L.nw, L.nh, L.g) if merge else own.flatten(0, 1)).reshape(-1).long().tolist()
            for i in range(L.n_images):
                loc = rm[L.n_images * L.P + i * L.n_local * L.q:][:L.n_local * L.q]
                assert [merged[d - i * stride - L.P] for d in loc] == list(range(L.n_local * L.q))
        assert rm[:L.n_images * L.P] == [i * stride + p for i in range(L.n_images) for p in range(L.P)]


def test_every_broken_variant_shows_at_the_layouts():
    """Each wrong glue changes the torch-backend replay wherever ``applies`` says it can, and somewhere."""
    seen = {b: 0 for b in AC.BROKEN}
    for name in LAYOUT_IDS:
        t, L = tiny(name), AC.LAYOUTS[name]
        feats = AC.make_feats(L.n_crops, L.P, L.D, None)
        stride = L.rows_per_image + 5
        for gated in (-1, 1):
            for merge in (0, 1):
                good = _uniform(t, feats, gated, merge, stride)
                grids = [((L.nw, L.nh) if merge else (L.n_local, 1 if L.n_local else 0))] * L.n_images
                for b in UNIFORM_BROKEN:
                    if not AC.applies(b, n_images=L.n_images, grids=grids, g=L.g, merge=bool(merge), learnable_gated=gated, padded_stride=True):
                        continue
                    bad = _uniform(t, feats, gated, merge, stride, b)
                    assert not torch.equal(bad, good), (name, gated, merge, b)
                    seen[b] += 1
    t, L = tiny("a"), AC.LAYOUTS["a"]
    for grids in AC.RAGGED_GRIDS:
        feats = AC.make_feats(sum(1 + nw * nh for nw, nh in grids), L.P, L.D, None, seed=8)
        total = sum(L.P + nw * nh * L.q for nw, nh in grids)
        for merge in (0, 1):
            g_ = grids if merge else [(nw * nh, 1 if nw * nh else 0) for nw, nh in grids]
            run = lambda b: AC.replay_adapter_ragged(AC.TorchBackend(None), t, feats, g_, merge, -1,
                                                     torch.full((total, L.H), -7.0, dtype=torch.float64), None, b)
            good = run(None)
            for b in RAGGED_BROKEN:
                if AC.applies(b, n_images=len(grids), grids=g_, g=L.g, merge=bool(merge), learnable_gated=-1, padded_stride=False):
                    assert not torch.equal(run(b), good), (grids, merge, b)
                    seen[b] += 1
    assert all(seen.values()), seen
    # layout a alone discriminates every uniform variant, the first ragged grid list both ragged ones
    La = AC.LAYOUTS["a"]
    for b in UNIFORM_BROKEN:
        assert AC.applies(b, n_images=La.n_images, grids=[(La.nw, La.nh)] * La.n_images, g=La.g, merge=True, learnable_gated=-1, padded_stride=True)
    for b in RAGGED_BROKEN:
        assert AC.applies(b, n_images=4, grids=AC.RAGGED_GRIDS[0], g=La.g, merge=True, learnable_gated=-1, padded_stride=False)


def test_rounding_backend_and_guards():
    """TorchBackend(T) rounds where the kernels round (a replay in T stays within the bf16 scale of the unrounded one), and the
    guarded workspace reports a write on either side of its exactly sized window."""
    t, L = tiny("a"), AC.LAYOUTS["a"]
    feats = AC.make_feats(L.n_crops, L.P, L.D, torch.bfloat16)
    out = torch.zeros(L.n_images * L.rows_per_image, L.H, dtype=torch.float32)
    t16 = AC.Tiny(L, t.cfg, t.sd, t.pg, t.post, torch.bfloat16)
    AC.replay_adapter(AC.TorchBackend(torch.bfloat16), t16, feats, L.n_images, L.n_local, L.nw, L.nh, 1, -1, out, L.rows_per_image)
    ref = _uniform(t, feats.float(), -1, 1, L.rows_per_image).reshape(-1, L.H)
    assert 1e-4 < rel_l2(out, ref) < 2e-2
    ws = AC.GuardedWorkspace(1000, "cpu")
    assert ws.ptr() % 256 == 0 and ws.intact() and bool((ws.window == 0xFF).all())
    ws.window.fill_(0)
    assert ws.intact()
    for off in (ws.off - 1, ws.off + ws.nbytes):
        snap = ws.snapshot()
        ws.buf[off] = 0
        assert not ws.intact() and not ws.unchanged(snap)
        ws.buf[off] = AC.SENTINEL_BYTE
    assert AC.GuardedWorkspace(1000, "cpu", misalign=128).ptr() % 256 == 128
    o = AC.guarded_output(3, 8, torch.float32, "cpu")
    assert bool(AC.sentinel_rows(o.win).all())
    o.win[1, 2] = 0.0
    assert AC.sentinel_rows(o.win).tolist() == [True, False, True]
    assert math.isqrt(L.q) == L.g
