"""The pack (mmsa/pack.py) on the device: every GEMM weight of the packed tree carries the operand format the plan gives for its site, and a pack-time
setting that changes after a forward is noticed by the next one."""
import pytest
import torch

from tests.configs import CONFIGS, make_input
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the smallest width at which h8c and W8 are selected at all (every contraction of the blocks >= 512)
KW512 = dict(CONFIGS["tiny256"]["kwargs"], embed_dim=512, num_heads=8, deform_num_heads=8)
NOT_GEMM_WEIGHTS = ("qkv_bp", "qkv_bp16", "qkv_bp_b3", "relp", "relp16")   # the attention kernels' own operands: bias rows and rel-pos tables


def _model(kwargs, seed, **attrs):
    import mmsa
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **kwargs))
    m.load_state_dict(seeded_state_dict(m, seed=seed), strict=True)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def _planes_of(o, path=()):
    from mmsa import ops
    if isinstance(o, ops.Planes):
        yield path, o
    elif isinstance(o, dict):
        for k, v in o.items():
            yield from _planes_of(v, path + (k,))
    elif isinstance(o, (list, tuple)):
        for i, v in enumerate(o):
            yield from _planes_of(v, path + (i,))


def _expected(m, p):
    """path in the packed tree -> the format the plan gives for that site, for every GEMM weight of the model"""
    from mmsa import ops
    cfg, D = m.cfg, m.cfg["embed_dim"]
    dv, hid = int(D * cfg["deform_ratio"]), int(D * cfg["cffn_ratio"])
    want = {("pe_w",): ops.FMT_B3, ("up",): p.inter_fmt(D, site="up")}
    for i in range(cfg["depth"]):
        for k in ("qkv", "proj", "lin1", "lin2"):
            want[("blocks", i, k)] = p.block_fmt()
    n_int = len(cfg["interaction_indexes"])
    for i in range(n_int):
        attns = [("inter", i, "inj", "attn")]
        for j in range(3 if i == n_int - 1 else 1):     # (the last interaction has the two extra extractors)
            e = ("inter", i, "ext", j)
            attns.append(e + ("attn",))
            want[e + ("fc1",)], want[e + ("fc2",)] = p.inter_fmt(D, i), p.inter_fmt(hid, i, h8c_ok=False)
        for a in attns:
            want[a + ("oa",)], want[a + ("val",)], want[a + ("out",)] = p.inter_fmt(D, i), p.inter_fmt(D, i), p.inter_fmt(dv, i)
    ch = m.channels
    want[("twin2", "stem")] = p.cnx_fmt(ch[0])
    for s in range(4):
        if s:
            want[("twin2", "ds", s - 1, "w")] = p.cnx_fmt(ch[s])
        for j in range(m.depths[s]):
            want[("twin2", "stages", s, j, "pw1")], want[("twin2", "stages", s, j, "pw2")] = p.cnx_fmt(ch[s], 1), p.cnx_fmt(ch[s], 2)
        for k in ("mlp_in", "mlp_out", "ca1", "cah", "caw", "fc"):      # the neck stays on bf16 hi/lo
            want[("neck", s, k)] = ops.FMT_B3
        for e in range(2):
            want[("neck", s, "loc", e, "w1")] = want[("neck", s, "loc", e, "w3")] = ops.FMT_B3
    return want


@pytest.mark.parametrize("kwargs,seed,attrs", [
    (CONFIGS["tiny256"]["kwargs"], 2, {}), (CONFIGS["tiny256"]["kwargs"], 2, dict(_wide_range=True)), (CONFIGS["tiny256"]["kwargs"], 2, dict(_inter_pairs={1})),
    (KW512, 61, {}), (KW512, 61, dict(_wide_range=True)), (KW512, 61, dict(_inter_pairs={1})), (KW512, 61, dict(fp8_weights=True))],
    ids=["tiny", "tiny-wide", "tiny-pairs1", "w512", "w512-wide", "w512-pairs1", "w512-fp8"])
def test_packed_formats_are_the_plans(kwargs, seed, attrs):
    from mmsa.pack import PackPlan
    m = _model(kwargs, seed, **attrs)
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        pk = m._pack(dev)     # pack only, no forward
    have = {path: pl.fmt for path, pl in _planes_of(pk) if path[-1] not in NOT_GEMM_WEIGHTS}
    want = _expected(m, PackPlan.of(m))
    assert set(have) == set(want), (sorted(set(have) ^ set(want), key=str))     # no site skipped, none unknown
    wrong = {k: (have[k], want[k]) for k in want if have[k] != want[k]}
    assert not wrong, wrong
    assert pk["vit_fmt"] == PackPlan.of(m).block_fmt()


def test_changed_pack_setting_repacks_without_invalidate():
    """A pack-time attribute changed after a forward, no invalidate(): the next forward packs again and computes what a model built with that setting computes."""
    cfg = CONFIGS["tiny256"]
    x = make_input(cfg, batch=2).to(DEV)
    m = _model(cfg["kwargs"], cfg["seed"])
    m(x)
    stale = m._packed
    assert stale["share_c_norm"] is True
    m.share_c_norm = False
    outs, _ = m(x)
    fresh, _ = _model(cfg["kwargs"], cfg["seed"], share_c_norm=False)(x)
    torch.cuda.synchronize()
    assert m._packed is not stale and m._packed["share_c_norm"] is False     # not the stale pack's route
    for a, b in zip(outs, fresh):
        assert torch.equal(a, b)
