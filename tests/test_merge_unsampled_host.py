"""Host side of the un-sampled LLaVA-NeXT merge (mm_patch_merge_type 'spatial' / 'spatial_unpad' without a sampler): the unpad window
and the composed splice plan against what the reference recorded (tests/golden/merge_unsampled.npz), the plan lengths, every
refusal that is raised before the device is touched, ``image_newline``, the C signature -- and, where the reference is present, its
unmodified glue against this repository's ``prepare_inputs_labels_for_multimodal`` with CPU stand-ins for the ``ops`` calls."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import merge_unsampled_fixture as F

PIN = "[(336, 672), (672, 336), (672, 672), (1008, 336), (336, 1008)]"


def _cfg(merge_type="spatial_unpad", **over):
    from slime_amd.model.llava_arch import default_slime_config
    kw = dict(hidden_size=128, mm_hidden_size=128, mm_resampler_type=None, mm_projector_type="identity", mm_patch_merge_type=merge_type)
    kw.update(over)
    return default_slime_config("synthetic:1", **kw)


# ------------------------------------------------------------------------------------------------ unpad_window
def test_unpad_window_equals_the_reference_on_every_recorded_case():
    from slime_amd.model.llava_arch import unpad_window
    g = F.load()
    canvas, size, window = g["unpad_canvas"], g["unpad_size"], g["unpad_window"]
    # the factor pairs of 2 .. 7 slices: every canvas the uhd rule chooses from
    assert window.shape[0] > 5000 and len({tuple(c) for c in canvas.tolist()}) == 15
    cut_rows = cut_cols = 0
    for (ch, cw), (w, h), want in zip(canvas.tolist(), size.tolist(), window.tolist()):
        got = unpad_window((w, h), ch, cw)
        assert list(got) == want, ((w, h), (ch, cw), got, want)
        cut_rows += got[1] - got[0] < ch
        cut_cols += got[3] - got[2] < cw
    assert cut_rows > 100 and cut_cols > 100                               # the sweep trims in both directions


# size, grid (nw, nh), kept window (r0, r1, c0, c1), length with 'spatial_unpad'; side 24
TABLE = [((640, 480), (2, 2), (6, 42, 0, 48), 576 + 36 * 49),
         ((480, 640), (2, 2), (0, 48, 6, 42), 576 + 48 * 37),
         ((1000, 333), (3, 1), (0, 24, 0, 72), 576 + 24 * 73),
         ((900, 700), (3, 2), (0, 48, 5, 67), 576 + 48 * 63),
         ((700, 300), (3, 1), (0, 24, 8, 64), 576 + 24 * 57),
         ((336, 336), (1, 2), (12, 36, 0, 24), 576 + 24 * 25),
         ((500, 500), (2, 2), (0, 48, 0, 48), 576 + 48 * 49)]


@pytest.mark.parametrize("size,grid,window,length", TABLE, ids=lambda v: str(v))
def test_plan_lengths_and_windows_of_the_issue_table(size, grid, window, length):
    from slime_amd.mm_utils import get_anyres_image_grid_shape
    from slime_amd.model.llava_arch import unpad_window, unsampled_merge_plans, MERGE_ZERO
    nw, nh = get_anyres_image_grid_shape(size, PIN, 336)
    assert (nw, nh) == grid
    assert unpad_window(size, nh * 24, nw * 24) == window
    n = 1 + nw * nh
    (plan,) = unsampled_merge_plans([n], [size], None, _cfg("spatial_unpad"), F.stand_in_tower(), True)
    assert plan.dtype == np.int64 and plan.shape[0] == length
    r0, r1, c0, c1 = window
    assert int((plan == MERGE_ZERO).sum()) == r1 - r0                     # one zero row behind every kept raster row
    assert plan[:576].tolist() == list(range(576))                        # the base crop first
    assert plan[576] == (1 + (r0 // 24) * nw + c0 // 24) * 576 + (r0 % 24) * 24 + c0 % 24
    (flat,) = unsampled_merge_plans([n], [size], None, _cfg("spatial"), F.stand_in_tower(), False)
    assert flat.shape[0] == n * 576 and sorted(flat.tolist()) == list(range(n * 576))


def test_plan_of_a_single_crop_image():
    from slime_amd.model.llava_arch import unsampled_merge_plans, MERGE_NEWLINE
    (p,) = unsampled_merge_plans([1], None, None, _cfg("spatial_unpad"), F.stand_in_tower(), True)
    assert p.shape[0] == 577 and p[:576].tolist() == list(range(576)) and p[576] == MERGE_NEWLINE
    (p,) = unsampled_merge_plans([1], None, None, _cfg("spatial"), F.stand_in_tower(), False)
    assert p.tolist() == list(range(576))


# ------------------------------------------------------------------------------------------------ the composed plan
@pytest.mark.parametrize("name", F.case_names())
def test_composed_src_equals_the_reference_record(name):
    c = F.case(name)
    src, lab, mask, pos, lens, token_rows = F.plan_src(c, _cfg(), F.stand_in_tower())
    assert src.dtype == np.int64 and src.shape == c.codes.shape, (src.shape, c.codes.shape)
    got = F.decode_src(src, token_rows)
    assert np.array_equal(got, c.codes), np.argwhere(got != c.codes)[:5]
    assert np.array_equal(lab, c.new_lab) and np.array_equal(mask, c.new_mask) and np.array_equal(pos, c.new_pos)
    if c.max_length is not None:
        assert src.shape[1] == c.max_length and max(lens) > c.max_length          # the cut lies inside an image


def test_the_record_covers_what_it_should():
    names = F.case_names()
    for merge in ("spatial", "spatial_unpad"):
        for tag in ("right", "mask", "left", "cut", "two_tokens"):
            assert f"{merge}_{tag}" in names
    c = F.case("spatial_unpad_right")
    assert c.splits == [5, 1, 7, 4] and c.sizes[0] == (640, 480) and c.sizes[2:] == [(900, 700), (1000, 333)]
    kinds = set((c.codes >> 40).reshape(-1).tolist())
    assert kinds == {0, F.M_FEATURE, F.M_TABLE, F.M_NEWLINE}
    assert F.M_NEWLINE not in set((F.case("spatial_right").codes >> 40).reshape(-1).tolist())
    m = F.case("spatial_unpad_mask")
    assert m.masks is not None and [len(x) for x in m.masks] == m.splits and sum(m.splits) == 21


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture()
def host_encoder(monkeypatch):
    """A SlimeVisualEncoder on the host (tower not loaded: its config is enough for the plan) whose device entry points fail the test
    when they are reached."""
    from slime_amd import ops
    from slime_amd.model.llava_arch import SlimeVisualEncoder

    def make(merge_type="spatial_unpad", **over):
        enc = SlimeVisualEncoder(_cfg(merge_type, **over), embed_tokens=nn.Embedding(64, 128))

        def device(*a, **k):
            raise AssertionError("device work was reached")
        monkeypatch.setattr(enc, "_project_crops", device)
        for name in ("splice_merged", "splice_rows", "tower_forward"):
            monkeypatch.setattr(ops, name, device)
        return enc
    return make


def _call(enc, splits, sizes, masks=None):
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    ids = torch.full((len(splits), 4), 5, dtype=torch.long)
    ids[:, 1] = IMAGE_TOKEN_INDEX
    images = [torch.zeros(s, 3, 336, 336) for s in splits]
    return enc.prepare_inputs_labels_for_multimodal(ids, None, torch.ones_like(ids), None, None, images, image_sizes=sizes, images_mask=masks)


def test_refusals_are_raised_before_any_device_work(host_encoder):
    with pytest.raises(AssertionError, match="device work"):                      # the probe itself: a legal call reaches the device
        _call(host_encoder(), [5], [(640, 480)])
    with pytest.raises(NotImplementedError, match="anyres"):
        _call(host_encoder(image_aspect_ratio="pad"), [5], [(640, 480)])
    with pytest.raises(ValueError, match="grid 2x2 does not match 3 local crops"):
        _call(host_encoder(), [4], [(640, 480)])
    with pytest.raises(ValueError, match="grid 2x2 does not match 3 local crops"):
        _call(host_encoder(), [5], [(640, 480)], [torch.tensor([1, 1, 0, 1, 1])])
    with pytest.raises(ValueError, match="no image_sizes"):
        _call(host_encoder(), [5], None)
    with pytest.raises(ValueError, match="2 images, 1 image_sizes"):
        _call(host_encoder(), [5, 1], [(640, 480)])
    with pytest.raises(ValueError, match="576 tower rows per crop.*577"):
        _call(host_encoder(mm_vision_select_feature="cls_patch"), [5], [(640, 480)])
    enc = host_encoder()
    del enc.get_model().image_newline
    with pytest.raises(ValueError, match="image_newline"):
        _call(enc, [5, 1], [(640, 480), (300, 300)])
    with pytest.raises(AssertionError, match="device work"):                      # without a single-crop image nothing needs the row
        _call(enc, [5], [(640, 480)])


def test_sampler_and_other_merge_types_do_not_take_the_branch(host_encoder, monkeypatch):
    from slime_amd.model import llava_arch as A
    seen = []
    monkeypatch.setattr(A, "unsampled_merge_plans", lambda *a, **k: seen.append(1))
    enc = host_encoder("flat")
    monkeypatch.setattr(enc, "encode_images", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("encode_images")))
    with pytest.raises(RuntimeError, match="encode_images"):
        _call(enc, [5], [(640, 480)])
    assert not seen


# ------------------------------------------------------------------------------------------------ image_newline
def test_image_newline_exists_exactly_with_unpad_and_round_trips():
    from slime_amd.model.llava_arch import SlimeVisualEncoder
    for merge, has in (("spatial_unpad", True), ("spatial", False), ("flat", False)):
        enc = SlimeVisualEncoder(_cfg(merge))
        assert hasattr(enc.get_model(), "image_newline") == has
        assert ("model.image_newline" in enc.state_dict()) == has and ("image_newline" in enc.get_model().state_dict()) == has
    enc = SlimeVisualEncoder(_cfg("spatial_unpad"))
    nl = enc.get_model().image_newline
    assert isinstance(nl, nn.Parameter) and nl.shape == (128,) and nl.dtype == torch.float32 and not bool(nl.any())
    v = torch.randn(128, generator=torch.Generator().manual_seed(1))
    sd = enc.state_dict()
    sd["model.image_newline"] = v.clone()
    other = SlimeVisualEncoder(_cfg("spatial_unpad"))
    other.load_state_dict(sd)
    assert torch.equal(other.get_model().image_newline.detach(), v)
    assert torch.equal(other.state_dict()["model.image_newline"], v)


@pytest.mark.parametrize("key", ["image_newline", "model.image_newline", None])
def test_load_visual_state_loads_image_newline_under_both_spellings(key):
    from slime_amd.model.llava_arch import SlimeVisualEncoder
    v = torch.randn(128, generator=torch.Generator().manual_seed(2))
    sd = {} if key is None else {key: v.clone()}
    enc = SlimeVisualEncoder(_cfg("spatial_unpad", mm_vision_tower="synthetic:1"))
    enc.get_vision_tower().is_loaded = True                                # the tower's own weights are not the subject
    enc.load_visual_state(None, sd)                                        # IdentityMap projector: no other adapter keys
    want = torch.zeros(128) if key is None else v                          # the key is optional
    assert torch.equal(enc.get_model().image_newline.detach(), want)
    plain = SlimeVisualEncoder(_cfg("spatial"))
    plain.get_vision_tower().is_loaded = True
    plain.load_visual_state(None, {"model.image_newline": v})              # no parameter: the key is ignored
    assert not hasattr(plain.get_model(), "image_newline")
    with pytest.raises(ValueError, match="shape"):
        enc.load_visual_state(None, {"image_newline": torch.zeros(7)})


# ------------------------------------------------------------------------------------------------ C ABI
def test_argtypes_match_the_header_declaration():
    from slime_amd import _lib
    import ctypes as C
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+slime_splice_merged\s*\(([^)]*)\)\s*;", text)
    assert m, "slime_splice_merged is not declared in the header"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [p.split(" ")[-1].lstrip("*") for p in params]
    assert names == ["table", "table_dtype", "table_rows", "tokens", "token_rows", "mid_dtype", "extra", "extra_dtype", "extra_rows", "src",
                     "out", "out_dtype", "rows", "H", "stream"]

    def ctype(p):
        t = p.rsplit(" ", 1)[0].replace("const ", "")
        return C.c_void_p if "*" in p else {"int": C.c_int, "long": C.c_long}[t]
    res, args = _lib._SIGNATURES["slime_splice_merged"]
    assert res is C.c_int and list(args) == [ctype(p) for p in params]
    assert "slime_splice_merged" in _lib.header_symbols()
    lib = _lib.load()
    assert hasattr(lib, "slime_splice_merged") and lib.slime_abi_version() == 7


FAKE = 0x10000          # an aligned address that no refusal path reads


def _abi(lib, **over):
    from slime_amd import _lib
    a = dict(table=FAKE, table_dtype=_lib.BF16, table_rows=100, tokens=FAKE, token_rows=50, mid_dtype=_lib.BF16, extra=FAKE,
             extra_dtype=_lib.F32, extra_rows=1, src=FAKE, out=FAKE, out_dtype=_lib.BF16, rows=12, H=64, stream=None)
    a.update(over)
    return lib.slime_splice_merged(*a.values()), lib.slime_last_error().decode()


def test_splice_merged_refusals_return_before_a_launch():
    from slime_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    for name in ("src", "out", "table"):
        rc, msg = _abi(lib, **{name: None})
        assert rc == EINVAL and "null" in msg and name in msg, (name, msg)
    for name in ("rows", "H"):
        for v in (0, -1):
            rc, msg = _abi(lib, **{name: v})
            assert rc == EINVAL and f"{name}={v}" in msg and "positive" in msg, (name, msg)
    for name in ("table_rows", "token_rows", "extra_rows"):
        rc, msg = _abi(lib, **{name: -1})
        assert rc == EINVAL and f"{name}=-1" in msg and "negative" in msg, (name, msg)
    for ptr, n in (("tokens", "token_rows"), ("extra", "extra_rows")):
        rc, msg = _abi(lib, **{ptr: None})                                 # null with rows: refused
        assert rc == EINVAL and ptr in msg and n in msg, msg
        rc, msg = _abi(lib, **{n: 0})                                      # rows 0 with a pointer: refused
        assert rc == EINVAL and ptr in msg and f"{n}=0" in msg, msg
    for name in ("table_dtype", "mid_dtype", "extra_dtype", "out_dtype"):
        for v in (_lib.U8, -1, 17):
            rc, msg = _abi(lib, **{name: v})
            assert rc == EINVAL and "dtype" in msg and f"{name.split('_')[0]} {v}" in msg, (name, msg)
    for H, dt in ((4, _lib.BF16), (12, _lib.F16), (6, _lib.F32), (2, _lib.F32), (63, _lib.BF16)):
        rc, msg = _abi(lib, H=H, out_dtype=dt)
        assert rc == EINVAL and "16 bytes" in msg and f"H={H}" in msg
    for name in ("out", "table", "tokens", "extra"):
        rc, msg = _abi(lib, **{name: FAKE + 8})
        assert rc == EINVAL and "16-byte aligned" in msg and name in msg


# ------------------------------------------------------------------------------------------------ the reference's glue
from oracle.make_golden import REF                    # where the reference lives in the build container


def _splice_merged_cpu(table, tokens, extra, src, mid_dtype, out_dtype):
    """ops.splice_merged restated with torch on the host (include/slime_hip.h)."""
    rows, H = src.numel(), table.shape[-1]
    out = torch.zeros((rows, H), dtype=out_dtype)
    n_tok = 0 if tokens is None else tokens.shape[0]
    n_extra = 0 if extra is None else extra.shape[0]
    for r, s in enumerate(src.reshape(-1).tolist()):
        k = -2 - s
        if 0 <= s < table.shape[0]:
            out[r] = table[s].to(out_dtype)
        elif s <= -2 and k < n_tok:
            out[r] = tokens[k].to(mid_dtype).to(out_dtype)
        elif s <= -2 and k < n_tok + n_extra:
            out[r] = extra[k - n_tok].to(out_dtype)
    return out


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "llava")), reason="the reference is only present in the build container")
@pytest.mark.parametrize("merge_type", ["spatial", "spatial_unpad"])
def test_reference_glue_equals_this_repository(merge_type, monkeypatch, tmp_path):
    """The reference's unmodified LlavaMetaModel.__init__ / encode_images / prepare_inputs_labels_for_multimodal over the swapped-in
    builders against SlimeVisualEncoder.prepare_inputs_labels_for_multimodal, identity projector, no
    sampler; the tower behind both is the CPU oracle."""
    import sys
    import test_reference_glue as G
    from slime_amd import ops, weights as W
    from slime_amd.constants import IMAGE_TOKEN_INDEX
    from slime_amd.model.llava_arch import SlimeVisualEncoder
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle.make_golden import import_reference
    import_reference()
    import llava.model.llava_arch as A
    from slime_amd.model.multimodal_encoder.builder import build_vision_tower
    from slime_amd.model.multimodal_projector.builder import build_vision_projector
    from slime_amd.model.multimodal_resampler.builder import build_vision_sampler
    from slime_amd.mm_utils import get_anyres_image_grid_shape
    for name, fn in (("build_vision_tower", build_vision_tower), ("build_vision_projector", build_vision_projector),
                     ("build_vision_sampler", build_vision_sampler), ("get_anyres_image_grid_shape", get_anyres_image_grid_shape)):
        monkeypatch.setattr(A, name, fn)
    oo = G._OracleOps()
    for name in ("pack_tower", "tower_forward"):
        monkeypatch.setattr(ops, name, getattr(oo, name))
    monkeypatch.setattr(ops, "splice_merged", _splice_merged_cpu)
    D, VOCAB = W.TINY.hidden_size, 64
    tdir = G._tower_dir(tmp_path)

    def config():
        c = G._config(tdir, W.ADAPTER_TINY)
        c.mm_resampler_type, c.mm_projector_type, c.mm_patch_merge_type = None, "identity", merge_type
        c.hidden_size = c.mm_hidden_size = D
        return c

    class _Base(nn.Module):
        dtype = torch.float32                                 # PreTrainedModel.dtype in the reference (llava_arch.py:43)

        def __init__(self, cfg):
            super().__init__()
            self.config = cfg
            self.embed_tokens = nn.Embedding(VOCAB, D)

    class Model(A.LlavaMetaModel, _Base):
        pass

    class Wrapper(A.LlavaMetaForCausalLM):
        def __init__(self, cfg):
            self.model, self.config = Model(cfg), cfg

        def get_model(self):
            return self.model

        device = torch.device("cpu")

    ref = Wrapper(config())
    ref.get_vision_tower().load_model()
    assert hasattr(ref.model, "image_newline") == ("unpad" in merge_type) and not ref.model.has_sampler
    g = torch.Generator().manual_seed(7)
    table = torch.randn(VOCAB, D, generator=g)
    newline = torch.randn(D, generator=g)
    embed = nn.Embedding(VOCAB, D)
    with torch.no_grad():
        ref.model.embed_tokens.weight.copy_(table)
        embed.weight.copy_(table)
        if "unpad" in merge_type:
            ref.model.image_newline.copy_(newline)
    ours = SlimeVisualEncoder(config(), embed_tokens=embed)
    ours.get_vision_tower().load_model()
    ours.get_vision_tower().vision_tower.two_streams = False          # 9 crops in one call: no HIP streams on the host
    if "unpad" in merge_type:
        ours.load_visual_state(None, {"model.image_newline": newline})

    splits, sizes = [5, 1, 3], [(640, 480), (300, 300), (336, 336)]
    px = [W.synthetic_pixels(s, seed=40 + i) for i, s in enumerate(splits)]
    ids = torch.randint(3, VOCAB, (3, 9), generator=g)
    ids[0, 2] = ids[1, 0] = ids[2, 8] = IMAGE_TOKEN_INDEX
    am = torch.ones_like(ids)
    am[1, -3:] = 0
    lab = ids + 100
    pos = torch.arange(9).expand(3, 9).contiguous()
    for side, max_len in (("right", None), ("left", 700)):
        for m in (ref, ours):
            m.config.tokenizer_padding_side, m.config.tokenizer_model_max_length = side, max_len
        want = ref.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=sizes)
        got = ours.prepare_inputs_labels_for_multimodal(ids, pos, am, None, lab, px, image_sizes=sizes)
        assert want[0] is None and got[0] is None and want[3] is None and got[3] is None
        for i in (1, 2, 4, 5):
            assert got[i].dtype == want[i].dtype and torch.equal(got[i], want[i]), (side, max_len, i)
        assert got[4].shape[1] == (max_len or got[4].shape[1])
