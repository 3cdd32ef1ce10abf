"""CPU tests of the ragged fused adapter's host side: the plan's row map against the oracle's spatial merge, the per-image grids the
glue derives from the image sizes, and the argument checks of slime_adapter_forward_ragged (all of which run before any launch).
No GPU."""
import ctypes as C

import pytest
import torch

PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"
LAYOUT = [(2, 1), (1, 3), (0, 0), (3, 2), (2, 2)]
P, G = 576, 12


@pytest.mark.parametrize("merge", [True, False])
@pytest.mark.parametrize("explicit", [False, True])
def test_ragged_row_map_restates_the_spatial_merge(merge, explicit):
    """rowwise.hip: adapter_ragged_plan_kernel, restated by ops.adapter_ragged_plan: GEMM row r of projection[2]'s output [global rows
    of every image | local rows of every image] -> row of the flat token buffer.  Scattering row ids through the map must reproduce,
    per image, cat(global rows, oracle.spatial_merge(local rows, nw_i, nh_i, g)) (flat order for merge=False), without collisions
    and without touching a row no image owns -- packed, and with explicit first rows in another order with gaps between them."""
    from oracle import slime_oracle as O
    from slime_amd import ops
    q = G * G
    grids = LAYOUT if merge else [(nw * nh, 1) if nw else (0, 0) for nw, nh in LAYOUT]
    n = [nw * nh for nw, nh in grids]
    own = [P + n_i * q for n_i in n]
    row0_in = None
    if explicit:                                                      # images 4, 0, 3, 1, 2 from the top, 3 + i spare rows around each
        row0_in, o = [0] * len(n), 7
        for i in (4, 0, 3, 1, 2):
            row0_in[i] = o
            o += own[i] + 3 + i
    row0, rows, row_map = ops.adapter_ragged_plan(grids, P, q, merge, row0_in)
    if explicit:
        assert row0 == row0_in and rows == max(r + w for r, w in zip(row0, own))
    else:
        assert row0 == [sum(own[:i]) for i in range(len(n))] and rows == sum(own)
    B, rows_l = len(n), sum(n) * q
    dst = [row_map(r) for r in range(B * P + rows_l)]
    assert len(set(dst)) == len(dst) and min(dst) >= 0 and max(dst) < rows          # a scatter without collisions, inside the buffer
    buf = torch.full((rows + 11,), -1.0)
    buf[torch.tensor(dst)] = torch.arange(len(dst), dtype=torch.float32)
    owned = torch.zeros(rows + 11, dtype=torch.bool)
    lrow = B * P
    for i, (nw, nh) in enumerate(grids):
        glob = torch.arange(i * P, (i + 1) * P, dtype=torch.float32)
        loc = torch.arange(lrow, lrow + n[i] * q, dtype=torch.float32).view(n[i], q, 1)
        lrow += n[i] * q
        want = loc.view(-1)
        if merge and n[i]:
            want = O.spatial_merge(loc, nw, nh, G).view(-1)
        assert torch.equal(buf[row0[i]:row0[i] + P], glob), i
        assert torch.equal(buf[row0[i] + P:row0[i] + own[i]], want), i
        owned[row0[i]:row0[i] + own[i]] = True
    assert int(owned.sum()) == len(dst) and bool((buf[~owned] == -1).all())          # unowned rows untouched


def test_ragged_layout_follows_the_slicer_grids():
    """llava_arch._ragged_layout: the per-image grids are mm_utils.get_anyres_image_grid_shape's; None where the fused call cannot
    take the batch (a crop count that does not match its grid, 'spatial' without sizes, more than 64 images)."""
    from slime_amd import mm_utils as M
    from slime_amd.model.llava_arch import _ragged_layout, default_slime_config
    cfg = default_slime_config()
    sizes = [(336, 336), (672, 672), (1344, 1344), (300, 2352)]
    want = [tuple(M.get_anyres_image_grid_shape(s, PIN, 336)) for s in sizes]
    assert len(set(want)) > 1                                          # a ragged batch indeed
    split = [1 + nw * nh for nw, nh in want]
    assert _ragged_layout(split, sizes, cfg, 336, "spatial") == want
    assert _ragged_layout([split[0], 1] + split[2:], sizes, cfg, 336, "spatial") == [want[0], (0, 0)] + want[2:]     # a global-only image
    assert _ragged_layout(split, None, cfg, 336, "flat") == [(s - 1, 1) for s in split]
    assert _ragged_layout([split[0] + 1] + split[1:], sizes, cfg, 336, "spatial") is None                              # mismatching crop count
    assert _ragged_layout(split, None, cfg, 336, "spatial") is None
    assert _ragged_layout([3] * 65, [(336, 336)] * 65, cfg, 336, "spatial") is None
    assert _ragged_layout([3] * 64, [(336, 336)] * 64, cfg, 336, "spatial") == [(1, 2)] * 64


def _descs():
    """Adapter descriptors at the tiny geometry with dummy non-null weight addresses: the checks under test never dereference them."""
    from slime_amd import _lib
    mlp = _lib.MlpDesc()
    mlp.in_dim, mlp.hidden, mlp.dtype = 128, 256, _lib.BF16
    res = []
    for nq in (576, 144):
        r = _lib.ResamplerDesc()
        r.dim, r.heads, r.n_query, r.n_kv, r.dtype, r.eps = 128, 1, nq, 576, _lib.BF16, 1e-6
        res.append(r)
    for d in [mlp] + res:
        for name, typ in d._fields_:
            if typ is C.c_void_p:
                setattr(d, name, 0x1000)
    return mlp, res[0], res[1]


def test_ragged_entry_points_check_their_arguments_on_the_host():
    """slime_adapter_ragged_workspace_bytes grows with the batch's local crops; slime_adapter_forward_ragged returns SLIME_EINVAL and
    names the limit for more than 64 images, a grid with one factor 0, first rows that overlap or leave the buffer, a buffer beyond
    the 32-bit row map and a 16-bit output type that is not the operand type -- before anything is launched (dummy pointers)."""
    from slime_amd import _lib
    lib = _lib.load()
    mlp, attn, post = _descs()

    def arr(v, t=C.c_int):
        return (t * len(v))(*v)

    def ws_bytes(grids):
        return lib.slime_adapter_ragged_workspace_bytes(C.byref(mlp), C.byref(attn), C.byref(post), len(grids), arr([g[0] for g in grids]),
                                                        arr([g[1] for g in grids]))

    sizes = [ws_bytes([(0, 0), (0, 0)]), ws_bytes([(1, 2), (0, 0)]), ws_bytes([(1, 2), (2, 1)]), ws_bytes([(2, 3), (2, 1)]),
             ws_bytes([(2, 3), (3, 2)])]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert ws_bytes([(2, 1), (3, 2)]) == ws_bytes([(3, 2), (1, 2)])             # a function of sum n_i, not of who has them
    assert ws_bytes([(1, 1)] * 65) == 0 and ws_bytes([(0, 2)]) == 0

    def forward(grids, out_row0=None, out_rows=1 << 20, out_dtype=_lib.F32):
        r0 = None if out_row0 is None else arr(out_row0, C.c_longlong)
        return lib.slime_adapter_forward_ragged(C.byref(mlp), C.byref(attn), 0x1000, -1, C.byref(post), 0x1000, len(grids),
                                                arr([g[0] for g in grids]), arr([g[1] for g in grids]), 1, 0x1000, out_dtype, r0, out_rows,
                                                0x1000, 0, None)

    cases = [
        (dict(grids=[(1, 1)] * 65), "SLIME_ADAPTER_RAGGED_MAX_IMAGES = 64"),
        (dict(grids=[(2, 1), (0, 2)]), "grid 0x2"),
        (dict(grids=[(2, 1), (1, 3)], out_row0=[0, 576 + 2 * 144 - 1]), "overlap"),
        (dict(grids=[(2, 1), (1, 3)], out_row0=[576 + 3 * 144, 0], out_rows=2 * 576 + 5 * 144 - 1), "outside the token buffer"),
        (dict(grids=[(2, 1), (1, 3)], out_rows=2 * 576 + 5 * 144 - 1), "too small"),
        (dict(grids=[(2, 1)], out_rows=1 << 31), "32-bit row map"),
        (dict(grids=[(2, 1)], out_dtype=_lib.F16), "operand type"),
    ]
    for kw, word in cases:
        assert forward(**kw) == -1, kw                                           # SLIME_EINVAL
        assert word in lib.slime_last_error().decode(), (word, lib.slime_last_error())
    # a valid layout passes every argument check and stops at the workspace (0 bytes given): nothing was launched
    assert forward([(2, 1), (1, 3), (0, 0)], out_row0=[0, 2000, 1000]) == -2
    assert "workspace" in lib.slime_last_error().decode()
