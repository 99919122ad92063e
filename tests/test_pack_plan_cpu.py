"""The site-to-format decision of the pack (mmsa.pack.PackPlan) as a literal table: which operand format every GEMM site gets and
which LayerNorm folds apply, per architecture and per state of the model.  No device: the plan is plain Python.  The expectations are written out by hand
from the rules (h8 where the site is selected and the contraction is a multiple of 64, h8c from 512 on, the pair format where a block or an interaction
has moved, bf16 pairs everywhere in the wide-range state, W8 where fp8 weights are on and the blocks qualify), not computed from the plan."""
import pytest
import torch

from tests.configs import CONFIGS

B3, H8, HC, F3, W8 = 0, 1, 2, 3, 4   # include/mmsa.h MMSA_FMT_*: bf16 hi/lo, h8 lines, h8c, fp16 hi/lo, fp8 weights
SHORT = "mmsa: fp8_weights needs the ViT-block GEMMs on h8c planes, but a contraction is shorter than 512 "

# contraction lengths of the interaction GEMMs: value / offsets projections and fc1 read the embed width, the output projection the MSDA
# width (embed x deform_ratio), fc2 the ConvFFN hidden width (embed x cffn_ratio); the up-conv reads the embed width
K = {"tiny256": dict(embed=64, msda=32, cffn=16), "hd80_256": dict(embed=320, msda=160, cffn=80), "vitb512": dict(embed=768, msda=384, cffn=192),
     "vitl1024": dict(embed=1024, msda=512, cffn=256), "vith1024": dict(embed=1280, msda=640, cffn=320)}

# per configuration and state: (block, pair, value, offsets, output, fc1, fc2, up, ConvNeXt (pw1, pw2) of every stage, fold_ln, padded head width);
# "pairs1" lists interaction 1 (interaction 0 is the default row's); "fp8" gives the block format or the refusal
TABLE = {
    # every contraction below 512: h8 lines; the MSDA width 32 and the ConvFFN width 16 (padded to 32) are no multiples of 64: bf16 pairs
    "tiny256": dict(default=(H8, F3, H8, H8, B3, H8, B3, H8, F3, False, 32), no_h8=(F3, F3, B3, B3, B3, B3, B3, B3, F3, False, 32),
                    no_h8c=(H8, F3, H8, H8, B3, H8, B3, H8, F3, False, 32), wide=(B3, B3, B3, B3, B3, B3, B3, B3, B3, False, 32),
                    pairs1=(H8, F3, F3, F3, F3, F3, F3, H8, F3, False, 32),
                    fp8=SHORT + "(embed 64, attention width 64, MLP hidden 256)"),
    # head width 80 runs as 96: attention width 384; MSDA width 160 and ConvFFN width 80 (-> 96) are no multiples of 64
    "hd80_256": dict(default=(H8, F3, H8, H8, B3, H8, B3, H8, F3, True, 96), no_h8=(F3, F3, B3, B3, B3, B3, B3, B3, F3, True, 96),
                     no_h8c=(H8, F3, H8, H8, B3, H8, B3, H8, F3, True, 96), wide=(B3, B3, B3, B3, B3, B3, B3, B3, B3, True, 96),
                     pairs1=(H8, F3, F3, F3, F3, F3, F3, H8, F3, True, 96),
                     fp8=SHORT + "(embed 320, attention width 384, MLP hidden 1280)"),
    # ViT-B: embed 768 -> h8c; the output projection (K = 384) and fc2 (K = 192) stay on h8 lines
    "vitb512": dict(default=(HC, F3, HC, HC, H8, HC, H8, HC, F3, True, 64), no_h8=(F3, F3, B3, B3, B3, B3, B3, B3, F3, True, 64),
                    no_h8c=(H8, F3, H8, H8, H8, H8, H8, H8, F3, True, 64), wide=(B3, B3, B3, B3, B3, B3, B3, B3, B3, True, 64),
                    pairs1=(HC, F3, F3, F3, F3, F3, F3, HC, F3, True, 64), fp8=W8),
    # ViT-L: the output projection reaches 512 -> h8c; fc2 (K = 256) on h8 lines
    "vitl1024": dict(default=(HC, F3, HC, HC, HC, HC, H8, HC, F3, True, 64), no_h8=(F3, F3, B3, B3, B3, B3, B3, B3, F3, True, 64),
                     no_h8c=(H8, F3, H8, H8, H8, H8, H8, H8, F3, True, 64), wide=(B3, B3, B3, B3, B3, B3, B3, B3, B3, True, 64),
                     pairs1=(HC, F3, F3, F3, F3, F3, F3, HC, F3, True, 64), fp8=W8),
    # ViT-H: head width 80 -> 96 (attention width 1536); fc2 (K = 320) on h8 lines
    "vith1024": dict(default=(HC, F3, HC, HC, HC, HC, H8, HC, F3, True, 96), no_h8=(F3, F3, B3, B3, B3, B3, B3, B3, F3, True, 96),
                     no_h8c=(H8, F3, H8, H8, H8, H8, H8, H8, F3, True, 96), wide=(B3, B3, B3, B3, B3, B3, B3, B3, B3, True, 96),
                     pairs1=(HC, F3, F3, F3, F3, F3, F3, HC, F3, True, 96), fp8=W8),
}
STATES = dict(default={}, no_h8=dict(h8_sites=()), no_h8c=dict(h8c=False), wide=dict(_wide_range=True), pairs1=dict(_inter_pairs={1}))


_BUILT = {}


def _model(kwargs, **attrs):
    """The (cached) model of `kwargs` with exactly `attrs` set on it."""
    import mmsa
    m = _BUILT.get(repr(kwargs))
    if m is None:
        with torch.device("meta"):   # the plan reads the architecture and the attributes only: no weights needed
            m = _BUILT[repr(kwargs)] = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **kwargs))
        m._clean = set(m.__dict__)
    for k in set(m.__dict__) - m._clean - {"_clean"}:
        delattr(m, k)
    m.invalidate()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _answers(p, k, inter):
    return (p.block_fmt(), p.pair_fmt, p.inter_fmt(k["embed"], inter), p.inter_fmt(k["embed"], inter), p.inter_fmt(k["msda"], inter),
            p.inter_fmt(k["embed"], inter), p.inter_fmt(k["cffn"], inter, h8c_ok=False), p.inter_fmt(k["embed"], site="up"))


@pytest.mark.parametrize("name", list(TABLE))
def test_plan_table(name):
    from mmsa.pack import PackPlan
    for state, attrs in STATES.items():
        m = _model(CONFIGS[name]["kwargs"], **attrs)
        p = PackPlan.of(m)
        want = TABLE[name][state]
        assert _answers(p, K[name], 1 if state == "pairs1" else 0) == want[:8], (name, state)
        assert [(p.cnx_fmt(c, 1), p.cnx_fmt(c, 2)) for c in p.channels] == [(want[8], want[8])] * 4, (name, state)
        assert p.cnx_fmt(p.channels[0]) == want[8]      # stem and downsample convs
        # the four folds: the ViT blocks' by the tile rule (3 x attention width and the MLP hidden whole 128-column tiles), the ConvNeXt and adapter folds
        # opt-in (off), the shared c-norm on
        assert (p.fold_ln, [p.fold_cnx(c) for c in p.channels], p.fold_adapter_ln, p.share_c_norm) == (want[9], [False] * 4, False, True), (name, state)
        assert (p.hd_pad, m._hd_pad, m._hd_true) == (want[10], want[10], CONFIGS[name]["kwargs"]["embed_dim"] // CONFIGS[name]["kwargs"]["num_heads"])
        if state == "pairs1":    # interaction 0 has not moved
            assert _answers(p, K[name], 0) == TABLE[name]["default"][:8], name
    p = PackPlan.of(_model(CONFIGS[name]["kwargs"], fp8_weights=True))
    if isinstance(TABLE[name]["fp8"], str):
        with pytest.raises(ValueError) as e:
            p.block_fmt()
        assert str(e.value) == TABLE[name]["fp8"]
    else:
        assert p.block_fmt() == TABLE[name]["fp8"] and p.settings()["fp8_weights"] is True
        # in the wide-range state the fp8 values travel on bf16 pairs
        assert PackPlan.of(_model(CONFIGS[name]["kwargs"], fp8_weights=True, _wide_range=True)).block_fmt() == B3


def test_opt_in_folds_and_sites():
    from mmsa.pack import PackPlan
    kw = CONFIGS["vitl1024"]["kwargs"]
    # a ConvFFN hidden width of 512 (cffn_ratio 0.5 at embed 1024): fc2's A operand is written by the depthwise conv, which cannot write h8c -> h8 lines;
    # the same contraction anywhere else is h8c
    p = PackPlan.of(_model(dict(kw, cffn_ratio=0.5)))
    assert p.hid_c == 512 and p.inter_fmt(512, 0, h8c_ok=False) == H8 and p.inter_fmt(512, 0) == HC
    # adapter fold: opt-in, needs the shared c-norm, the "inter" site and no interaction on pairs
    assert PackPlan.of(_model(kw, fold_adapter_ln=True)).fold_adapter_ln is True
    for off in (dict(share_c_norm=False), dict(h8_sites=("vit",)), dict(_inter_pairs={2}), dict(_wide_range=True)):
        assert PackPlan.of(_model(kw, fold_adapter_ln=True, **off)).fold_adapter_ln is False, off
    assert PackPlan.of(_model(CONFIGS["tiny256"]["kwargs"], fold_adapter_ln=True)).fold_adapter_ln is False    # MSDA width 32: no whole 128-column tile
    # ConvNeXt fold: opt-in, the stages that run pointwise_conv1 as a GEMM (not the fused 96-wide stage 0); it puts the chain on bf16 pairs
    p = PackPlan.of(_model(kw, fold_convnext_ln=True))
    assert [p.fold_cnx(c) for c in p.channels] == [False, True, True, True] and p.cnx_fmt(192, 1) == B3 and p.settings()["cnx_f16"] is False
    assert PackPlan.of(_model(kw, fold_ln=False)).fold_ln is False
    # the opt-in ConvNeXt sites: "cnx" = h8 lines for every pointwise conv but the fused stage 0, "cnx2p2" = stage 2's pointwise_conv2 alone on h8c
    p = PackPlan.of(_model(kw, h8_sites=("vit", "inter", "up", "attnv", "cnx")))
    assert [(p.cnx_fmt(c, 1), p.cnx_fmt(c, 2)) for c in p.channels] == [(F3, F3), (H8, H8), (H8, H8), (H8, H8)] and p.cnx_fmt(192) == F3
    p = PackPlan.of(_model(kw, h8_sites=("vit", "inter", "up", "attnv", "cnx2p2")))
    assert [(p.cnx_fmt(c, 1), p.cnx_fmt(c, 2)) for c in p.channels] == [(F3, F3), (F3, F3), (F3, HC), (F3, F3)]


def test_settings_of_vitl_are_the_files():
    """PackPlan.settings() = what a format-12 packed file of the default ViT-L carries under "settings": keys, values and their types."""
    from mmsa.pack import PackPlan, packed_settings
    s = PackPlan.of(_model(CONFIGS["vitl1024"]["kwargs"])).settings()
    want = {"h8_sites": ["vit", "inter", "up", "attnv"], "h8c": True, "share_c_norm": True, "fold_ln": True, "fold_cnx_ln": False, "cnx_f16": True,
            "fold_adapter_ln": False, "wide": False, "inter_pairs": []}
    assert s == want and {k: type(v) for k, v in s.items()} == {k: type(v) for k, v in want.items()}
    m = _model(CONFIGS["vitl1024"]["kwargs"], _wide_range=True, _inter_pairs={3, 1}, fp8_weights=True)
    s = PackPlan.of(m).settings()
    assert s == dict(want, h8_sites=["attnv"], cnx_f16=False, wide=True, inter_pairs=[1, 3], fp8_weights=True)
    assert m._h8_sites() == ("attnv",) and m._wide() and m._fold_ln_wanted()
    # what a pack stores under the same names reads back as the same dict (tuples and lists as a decoded file holds them)
    pk = dict(s, h8_sites=("attnv",), fp8_weights=True, blocks=[])
    assert packed_settings(pk) == s and packed_settings(dict(pk, fp8_weights=False)) == {k: v for k, v in s.items() if k != "fp8_weights"}
