"""Host side of the routed splice (slime_splice_routed, cfg.fused_splice): the (image, position) form of the splice plan decoded as
the kernel decodes it, the index plan of get_pure_text_embedding, and every refusal that returns before a launch.  No GPU: the
refusals are reached with made-up (aligned, never dereferenced) pointer values."""
import numpy as np
import pytest

from slime_amd import _lib
from slime_amd.constants import IMAGE_TOKEN_INDEX as IMG

FAKE = 0x10000          # a 256-byte aligned address that no refusal path reads


# ------------------------------------------------------------------------------------------------ routed_src
def decode(src, P, sep_id, off, n_rows, keep, cnt, table_rows, token_rows):
    """The kernel's rule for one src entry, restated from include/slime_hip.h: ('table', id) | ('sep', id) | ('tok', row) | ('zero',)."""
    B, T_max = keep.shape
    s = int(src)
    if s == -1:
        return ("zero",)
    if s >= 0:
        return ("table", s) if s < table_rows else ("zero",)
    q = -2 - s
    b, p = q >> 32, q & 0xffffffff
    if b >= B:
        return ("zero",)
    if p < P:
        row = int(off[b]) - P + p
    elif p == P:
        return ("sep", sep_id)
    else:
        j = p - P - 1
        if j >= T_max or j >= cnt[b]:
            return ("zero",)
        k = int(keep[b, j])
        if k < 0 or k >= n_rows[b]:
            return ("zero",)
        row = int(off[b]) + k
    return ("tok", row) if 0 <= row < token_rows else ("zero",)


def router_arrays(counts, P, seed):
    """An arbitrary router state for images with the given kept counts: every image has more local rows than it keeps (except one
    that keeps all), the kept indices are ascending and not the identity, the images are packed back to back after P global rows."""
    rng = np.random.default_rng(seed)
    B = len(counts)
    n_rows = np.array([c + (0 if i == 0 else int(rng.integers(1, 5))) for i, c in enumerate(counts)], dtype=np.int64)
    T_max = max(1, int(n_rows.max()))
    keep = np.full((B, T_max), -7, dtype=np.int64)                 # entries past the count are garbage the decode must not use
    off, o = [], 0
    for b, c in enumerate(counts):
        if c:
            keep[b, :c] = np.sort(rng.choice(int(n_rows[b]), size=c, replace=False))
        off.append(o + P)
        o += P + int(n_rows[b])
    return np.array(off, dtype=np.int64), n_rows, keep, np.array(counts, dtype=np.int64), o


def cat_based(src, P, sep_id, off, keep, cnt, table_rows):
    """Today's path: per image cat([glob, sep, routed]), all images concatenated, then splice_rows' rule on the -2 - k plan."""
    allf = []
    for b in range(len(cnt)):
        allf += [("tok", int(off[b]) - P + p) for p in range(P)] + [("sep", sep_id)] + [("tok", int(off[b] + keep[b, j])) for j in range(cnt[b])]
    out = []
    for s in np.asarray(src).reshape(-1):
        s = int(s)
        out.append(("zero",) if s == -1 else ("table", s) if s >= 0 else allf[-2 - s])
    return out


def _fixture_cases():
    import prefill_fixture as F
    g = F.load()
    for name in ("A", "B", "C"):
        c = F.splice_case(g, name)
        yield (f"fixture {name}", c["input_ids"].numpy(), None if c["attention_mask"] is None else c["attention_mask"].numpy(),
               [f.shape[0] for f in c["feats"]], c["max_length"], c["padding_side"])


def _own_cases():
    t = lambda n, base=10: list(range(base, base + n))
    # (name, ids, mask, feature lengths, max_length, side); P = 2, so a feature of length 3 has 0 kept rows
    yield ("left padding", np.array([[0, 0, 0] + t(2) + [IMG] + t(3), t(4) + [IMG] + t(4)]),
           np.array([[0, 0, 0] + [1] * 6, [1] * 9]), [6, 4], None, "left")
    yield ("max_length inside an image", np.array([t(3) + [IMG] + t(2), t(1) + [IMG] + t(4)]), None, [9, 5], 7, "right")
    yield ("max_length inside an image, left", np.array([t(3) + [IMG] + t(2), t(1) + [IMG] + t(4)]), None, [9, 5], 7, "left")
    yield ("two image tokens in one sequence", np.array([t(1) + [IMG] + t(2) + [IMG] + t(2), [IMG] + t(6)]), None, [4, 7, 5], None, "right")
    yield ("sequence without an image token", np.array([t(6), t(2) + [IMG] + t(3), t(6)]), None, [8, 5, 6], None, "right")
    yield ("image with 0 kept rows", np.array([t(2) + [IMG] + t(1), [IMG] + t(3), t(1) + [IMG] + t(2)]), None, [3, 6, 3], None, "right")


@pytest.mark.parametrize("case", list(_fixture_cases()) + list(_own_cases()), ids=lambda c: c[0])
def test_routed_src_decodes_to_the_rows_of_the_cat_based_plan(case):
    from slime_amd.model.llava_arch import splice_plan, routed_src
    _, ids, am, lens, max_len, side = case
    P, sep_id, table_rows = 2, 31, 1000
    counts = [n - P - 1 for n in lens]
    assert min(counts) >= 0
    off, n_rows, keep, cnt, token_rows = router_arrays(counts, P, seed=len(lens))
    src, _, _, _ = splice_plan(ids, am, None, lens, max_len, side)
    assert (src <= -2).any()
    rs = routed_src(src, lens)
    assert rs.shape == src.shape and rs.dtype == np.int64
    assert np.array_equal(rs[src >= -1], src[src >= -1])                      # token ids and padding are untouched
    got = [decode(s, P, sep_id, off, n_rows, keep, cnt, table_rows, token_rows) for s in rs.reshape(-1)]
    want = cat_based(src, P, sep_id, off, keep, cnt, table_rows)
    assert got == want
    assert ("zero",) not in [g for g, s in zip(got, src.reshape(-1)) if s <= -2]   # a plan entry never needs the kernel's backstop
    if 0 in counts:
        assert any(g[0] == "sep" for g in got)
    with pytest.raises(ValueError, match="past the last image"):
        routed_src(np.array([[-2 - sum(lens)]]), lens)


def test_routed_src_names_image_and_position():
    from slime_amd.model.llava_arch import routed_src
    lens = [3, 0, 4]                                     # the middle image feeds a sequence without an image token: zero rows
    src = np.array([[5, -2, -3, -4, -1], [-5, -6, -7, -8, 9]])
    rs = routed_src(src, lens)
    q = -2 - rs
    assert rs[0, 0] == 5 and rs[0, 4] == -1 and rs[1, 4] == 9
    assert (q[0, 1:4] >> 32).tolist() == [0, 0, 0] and (q[0, 1:4] & 0xffffffff).tolist() == [0, 1, 2]
    assert (q[1, :4] >> 32).tolist() == [2, 2, 2, 2] and (q[1, :4] & 0xffffffff).tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------ pure_text_plan
def pure_text_reference(ids, side, max_len):
    """The reference's get_pure_text_embedding as index logic (llava_arch.py:162-210): the text between the image tokens, in order,
    then one zero row per image token after it (before it for left padding); cut to max_len; -1 stands for a zero row."""
    rows = []
    for seq in np.asarray(ids).tolist():
        text, n_img = [], 0
        for tok in seq:
            if tok == IMG:
                n_img += 1
            else:
                text.append(tok)
        row = [-1] * n_img + text if side == "left" else text + [-1] * n_img
        rows.append(row[:max_len] if max_len is not None else row)
    return np.array(rows, dtype=np.int64)


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("max_len", [None, 5, 9, 40])
def test_pure_text_plan_matches_the_reference_index_logic(side, max_len):
    from slime_amd.model.llava_arch import pure_text_plan, _pure_text_order
    ids = np.array([[4, 9, IMG, 7, 0, 0, 3, 8, 1], [IMG, 3, IMG, 6, 8, IMG, 2, 2, 5], [1, 2, 3, 4, 5, 6, 7, 8, 9],
                    [0, 0, 0, 0, 11, IMG, 12, 13, IMG]])
    got = pure_text_plan(ids, side, max_len)
    want = pure_text_reference(ids, side, max_len)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert got.shape == (4, 9 if max_len is None else min(9, max_len))
    # the mask rides on the same order: a placeholder row has mask 0, a text row its own mask bit
    order = _pure_text_order(ids, side, max_len)
    assert np.array_equal(order >= 0, want >= 0)
    assert np.array_equal(np.take_along_axis(ids, np.maximum(order, 0), 1)[order >= 0], want[want >= 0])


def test_pure_text_plan_is_the_default_right_padded_uncut():
    from slime_amd.model.llava_arch import pure_text_plan
    assert pure_text_plan(np.array([[IMG, 5, 6]])).tolist() == [[5, 6, -1]]


# ------------------------------------------------------------------------------------------------ C ABI
def test_signature_is_bound():
    res, args = _lib._SIGNATURES["slime_splice_routed"]
    assert len(args) == 20 and "slime_splice_routed" in _lib.header_symbols()
    assert _lib.load().slime_abi_version() == 7


def _call(lib, **over):
    a = dict(table=FAKE, table_dtype=_lib.BF16, table_rows=100, sep_id=7, tokens=FAKE, token_rows=50, local_row_off=FAKE, n_rows=FAKE,
             B=3, P=5, T_max=7, keep_idx=FAKE, keep_count=FAKE, mid_dtype=_lib.BF16, src=FAKE, out=FAKE, out_dtype=_lib.BF16, rows=12,
             H=64, stream=None)
    a.update(over)
    rc = lib.slime_splice_routed(*a.values())
    return rc, lib.slime_last_error().decode()


def test_splice_routed_refusals():
    lib = _lib.load()
    EINVAL = -1
    for name in ("src", "out", "tokens", "table", "local_row_off", "n_rows", "keep_idx", "keep_count"):
        rc, msg = _call(lib, **{name: None})
        assert rc == EINVAL and "null" in msg and name in msg, (name, msg)
    for name in ("rows", "H", "B", "T_max"):
        for v in (0, -1):
            rc, msg = _call(lib, **{name: v})
            assert rc == EINVAL and f"{name}={v}" in msg and "positive" in msg, (name, msg)
    rc, msg = _call(lib, P=-1)
    assert rc == EINVAL and "P=-1" in msg
    for sep in (-1, 100, 1 << 40):
        rc, msg = _call(lib, sep_id=sep)
        assert rc == EINVAL and f"sep_id={sep}" in msg and "100 rows" in msg
    for name in ("table_dtype", "mid_dtype", "out_dtype"):
        for v in (_lib.U8, -1, 17):
            rc, msg = _call(lib, **{name: v})
            assert rc == EINVAL and "dtype" in msg and f"{name.split('_')[0]} {v}" in msg, (name, msg)
    for H, dt in ((4, _lib.BF16), (12, _lib.F16), (6, _lib.F32), (2, _lib.F32), (63, _lib.BF16)):
        rc, msg = _call(lib, H=H, out_dtype=dt)
        assert rc == EINVAL and "16 bytes" in msg and f"H={H}" in msg
    for name in ("out", "table", "tokens"):
        rc, msg = _call(lib, **{name: FAKE + 8})
        assert rc == EINVAL and "16-byte aligned" in msg and name in msg
