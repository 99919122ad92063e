"""The diagnostic pictures of mmsa.Renderer on the GPU against the numpy restatement (tests/render_diag_ref.py): bit for bit, no tolerance; and the five
identities that hold the pictures to the counts (mmsa.confusion, mmsa.boundary_counts, mmsa.abstain, __call__, the calibration bins)."""
import functools

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import calibration_ref as CR
from tests import eval_ref as ER
from tests import render_diag_ref as DR
from tests import render_ref as RR
from tests.test_render_gpu import LIDAR, _guard_intact, _guarded, _pp
from tests.test_topk_gpu import NUM_CLASSES, models  # noqa: F401  (the tiny model of the entry tests, a module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 25
SIZES = [(1, 1), (5, 3), (37, 53), (64, 64), (130, 67), (33, 257), (3, 1029)]      # both sides of the 4-pixel vector path, the 64-pixel tiles, 1024 pixels
RADII = (1, 2, 3, 7, 16, 32)
PAL = np.array([((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256) for i in range(C)])
CM15 = np.array([(17 * k, 255 - 9 * k, (k * k) % 256) for k in range(15)])
OP = 0.3


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(H, W, B=2):
    """(wide pred [B, H + 3, W + 7], label [B, H, W], conf [B, H, W], raw source [B, H + 2, W + 5, 3]); pred = wide[:, :H, :W] holds 255 and bytes >= C."""
    g = np.random.default_rng(7000 * H + W)
    pred, label = ER.make_case(1000 * H + W, H, W, C, B=B, special=True)
    wide = g.integers(0, 256, (B, H + 3, W + 7), dtype=np.uint8)
    wide[:, :H, :W] = pred
    wide[0, 0, 0] = 200
    conf = g.random((B, H, W), dtype=np.float32)
    edges = (g.integers(0, 16, (B, H, W)).astype(np.float64) / 15).astype(np.float32)
    conf = np.where(g.random((B, H, W)) < 0.2, edges, conf).astype(np.float32)
    flat = conf.reshape(B, -1)
    n = min(flat.shape[1], len(CR.SPECIALS))
    flat[:, :n] = CR.SPECIALS[:n]
    src = g.integers(0, 256, (B, H + 2, W + 5, 3), dtype=np.uint8)
    for a in (wide, label, conf, src):
        a.setflags(write=False)
    return wide, label, conf, src


def _renderer(bgr=True, opacity=OP, pp=None, pal=PAL):
    from mmsa.render import Renderer
    return Renderer(pal, opacity=opacity, preprocess=pp, bgr=bgr)


def _check(call, want, shape):
    out, buf = _guarded(shape)
    assert call(out) is out
    got = out.cpu().numpy()
    assert _guard_intact(buf), "bytes outside the picture were written"
    assert np.array_equal(got, want), f"{int((got != want).any(-1).sum())} pixels differ"


def _all_methods(r, d_pred, d_lab, d_conf, lp, pred, label, conf, lut, d_src, src_pic, rev=False, bgr=True, radius=2, tabs=(None, None)):
    """Every method once on the same maps against the restatement; src_pic = the source as the picture sees it (numpy, channel order of the picture)."""
    B, H, W = pred.shape
    shape = (B, H, W, 3)
    kw = dict(source=d_src, source_reverse=rev)
    ref = dict(source=src_pic, bgr=bgr)
    ym, xm = tabs
    _check(lambda o: r.labels(d_lab, lp, ignored=(1, 2, 3), out=o, **kw), DR.labels_ref(label, lut, C, PAL, OP, H, W, ignored=(1, 2, 3), ymap=ym, xmap=xm, **ref), shape)
    _check(lambda o: r.errors(d_pred, d_lab, lp, wrong="label", correct="pred", ignored=(9, 8, 7), mark_opacity=0.8, out=o, **kw),
           DR.errors_ref(pred, label, lut, C, PAL, OP, wrong="label", correct="pred", ignored=(9, 8, 7), mark_opacity=0.8, ymap=ym, xmap=xm, **ref), shape)
    _check(lambda o: r.errors(d_pred, d_lab, lp, wrong="pred", out=o, **kw), DR.errors_ref(pred, label, lut, C, PAL, OP, wrong="pred", ymap=ym, xmap=xm, **ref), shape)
    _check(lambda o: r.heat(d_conf, CM15, out=o, **kw), DR.heat_ref(conf, CM15, OP, **ref), shape)
    _check(lambda o: r.abstained(d_pred, d_conf, 15, min_bin=6, colour=(5, 6, 7), mark_opacity=0.9, out=o, **kw),
           DR.abstained_ref(pred, conf, 15, 6, PAL, OP, colour=(5, 6, 7), mark_opacity=0.9, **ref), shape)
    _check(lambda o: r.abstained(d_pred, d_conf, 15, threshold=0.2, colour=CM15, out=o, **kw), DR.abstained_ref(pred, conf, 15, 3, PAL, OP, colour=CM15, **ref), shape)
    _check(lambda o: r.band(d_pred, d_lab, lp, radius=radius, colour="label", inside="pred", where="both", mark_opacity=0.7, out=o, **kw),
           DR.band_ref(pred, label, lut, C, PAL, OP, radius, colour="label", inside="pred", where="both", mark_opacity=0.7, ymap=ym, xmap=xm, **ref), shape)
    _check(lambda o: r.band(d_pred, radius=radius, border=True, num_classes=C, out=o, **kw), DR.band_ref(pred, None, None, C, PAL, OP, radius, True, **ref), shape)
    _check(lambda o: r.band(labels=d_lab, prep=lp, radius=radius, colour=(250, 1, 2), inside=None, where="label", out=o, **kw),
           DR.band_ref(None, label, lut, C, PAL, OP, radius, colour=(250, 1, 2), inside=None, where="label", ymap=ym, xmap=xm, **ref), shape)


# ---- 1. sizes: every method, pred a strided view of a wider map, the source larger than the map, `out` inside a guarded buffer

@pytest.mark.parametrize("H,W", SIZES)
def test_sizes(H, W):
    from mmsa.evaluate import LabelPrep
    wide, label, conf, src = _case(H, W)
    d_wide = _dev(wide)
    d_pred, pred = d_wide[:, :H, :W], wide[:, :H, :W]
    assert d_pred.stride(1) == W + 7 and d_pred.stride(0) == (H + 3) * (W + 7)
    _all_methods(_renderer(), d_pred, _dev(label), _dev(conf), LabelPrep(C), pred, label, conf, ER.lut(C), _dev(src), src)


# ---- 2. each method x each source form x bgr

@pytest.mark.parametrize("bgr", (True, False))
@pytest.mark.parametrize("H,W", ((37, 53), (64, 128)))
def test_source_forms(H, W, bgr):
    from mmsa.evaluate import LabelPrep
    wide, label, conf, src = _case(H, W)
    d_wide = _dev(wide)
    d_pred, pred = d_wide[:, :H, :W], wide[:, :H, :W]
    lp, lut = LabelPrep(C), ER.lut(C)
    d_lab, d_conf = _dev(label), _dev(conf)
    r = _renderer(bgr)
    _all_methods(r, d_pred, d_lab, d_conf, lp, pred, label, conf, lut, None, None, bgr=bgr)
    for rev in (False, True):
        _all_methods(r, d_pred, d_lab, d_conf, lp, pred, label, conf, lut, _dev(src), src[..., ::-1] if rev else src, rev=rev, bgr=bgr)
    pp = _pp("muses")
    g = np.random.default_rng(H + W)
    rgb, aux = g.integers(0, 256, (2, H + 3, W + 4, 3), dtype=np.uint8), g.integers(0, 256, (2, H + 3, W + 4, 3), dtype=np.uint8)
    x = pp(_dev(rgb), _dev(aux))
    pic = RR.tensor2imgs_ref(x.cpu().numpy(), LIDAR["mean"], LIDAR["std"], pp.to_rgb[0], pp.div255[0])
    _all_methods(_renderer(bgr, pp=pp), d_pred, d_lab, d_conf, lp, pred, label, conf, lut, x, pic, bgr=bgr)


# ---- 3. the label side: tables, reduce_zero_label, a label_map, bytes that map to 255 and out of range

def test_the_label_side():
    from mmsa.evaluate import LabelPrep
    H, W = 37, 53
    wide, _, conf, src = _case(H, W)
    d_wide = _dev(wide)
    d_pred, pred = d_wide[:, :H, :W], wide[:, :H, :W]
    for Hl, Wl in ((19, 23), (90, 120)):                                # up and down through the tables
        label = _case(Hl, Wl)[1]
        lp = LabelPrep(C, resize=dict(seg_scale=(W, H), keep_ratio=False))
        tabs = (ER.nearest_index(Hl, H), ER.nearest_index(Wl, W))
        _all_methods(_renderer(), d_pred, _dev(label), _dev(conf), lp, pred, label, conf, ER.lut(C), _dev(src), src, radius=3, tabs=tabs)
    label = _case(H, W)[1]
    assert (label == 255).any() and (label == C + 5).any() and (label == 0).any() and (pred == 255).any()
    for kw in (dict(reduce_zero_label=True), dict(label_map={0: 2, 10: 1, 3: 255}), dict(ignore_index=2)):
        _all_methods(_renderer(), d_pred, _dev(label), _dev(conf), LabelPrep(C, **kw), pred, label, conf, ER.lut(C, **kw), _dev(src), src)


# ---- 4. heat: every bin edge and its float32 neighbours, NaN, infinities, -0.0, denormals, values above 1 -- one ramp image per N

@pytest.mark.parametrize("N", (1, 15, 256))
def test_heat_edge_values(N):
    from mmsa.render import colormap
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 1.0, 2.0, 1e30, -1.0]
    for k in range(N + 1):
        e = np.float32(k / N)
        vals += [e, np.nextafter(e, np.float32(-1)), np.nextafter(e, np.float32(2))]
    h, w = 13, 67
    v = np.resize(np.array(vals, dtype=np.float32), (1, h, w))
    assert len(vals) <= h * w
    cm = colormap([(3, 0, 250), (250, 3, 0), (9, 250, 9)], N)
    bins = CR.bin_index(v, N)
    assert bins.min() == 0 and bins.max() == N - 1 and len(np.unique(bins)) == N
    r = _renderer(bgr=False, opacity=1.0)
    got = r.heat(_dev(v), cm).cpu().numpy()
    assert np.array_equal(got, DR.heat_ref(v, cm, 1.0, bgr=False)) and np.array_equal(got, cm[bins])


# ---- 5. band: radii, borders, sizes; the reach of the radius

@pytest.mark.parametrize("H,W", SIZES)
def test_band_radii_and_borders(H, W):
    from mmsa.evaluate import LabelPrep
    wide, label, _, src = _case(H, W)
    d_wide, d_lab, d_src = _dev(wide), _dev(label), _dev(src)
    d_pred, pred = d_wide[:, :H, :W], wide[:, :H, :W]
    lp, lut, r = LabelPrep(C), ER.lut(C), _renderer()
    near = {}
    for b in range(2):
        L, P = BR.codes(pred[b], label[b], lut, C)
        for d in RADII:
            for border in (False, True):
                near[b, d, border] = (BR.near(L, d, border), BR.near(P, d, border), L, P)
    for d in RADII:
        for border in (False, True):
            _check(lambda o: r.band(d_pred, d_lab, lp, radius=d, border=border, colour="pred", inside="label", where="both", mark_opacity=0.6, source=d_src, out=o),
                   DR.band_ref(pred, label, lut, C, PAL, OP, d, border, colour="pred", inside="label", where="both", mark_opacity=0.6, source=src), (2, H, W, 3))
            # the marked set is the evaluation's near sets (restated above), read back from an opaque picture
            pic = _renderer(opacity=1.0).band(d_pred, d_lab, lp, radius=d, border=border, colour=(255, 255, 255), inside=None, where="both").cpu().numpy()
            for b in range(2):
                nl, npd, L, _ = near[b, d, border]
                assert np.array_equal(pic[b, ..., 0] == 255, (nl | npd) & (L != 255)), (d, border, b)


DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


@pytest.mark.parametrize("side", ["label", "pred"])
@pytest.mark.parametrize("d", [1, 3, 32])
def test_the_band_reaches_exactly_d_in_all_eight_directions(d, side):
    """A uniform map with one differing pixel: the marked set is exactly its (2 d + 1)^2 window -- distance d is in, d + 1 is out, in all eight directions."""
    from mmsa.evaluate import LabelPrep
    H, W, cy, cx = 75, 71, 36, 35
    one = np.zeros((1, H, W), dtype=np.uint8)
    one[0, cy, cx] = 1
    r = _renderer(opacity=1.0)
    kw = dict(radius=d, colour=(255, 255, 255), inside=None)
    pic = (r.band(labels=_dev(one), prep=LabelPrep(C), where="label", **kw) if side == "label" else r.band(_dev(one), where="pred", **kw)).cpu().numpy()
    marked = pic[0, ..., 0] == 255
    for dy, dx in DIRS:
        assert marked[cy + d * dy, cx + d * dx] and not marked[cy + (d + 1) * dy, cx + (d + 1) * dx], (dy, dx)
    want = np.zeros((H, W), dtype=bool)
    want[cy - d:cy + d + 1, cx - d:cx + d + 1] = True
    assert np.array_equal(marked, want) and int(marked.sum()) == (2 * d + 1) ** 2


# ---- 6. the identities on device results

def _count(pic, colour):
    return int((pic == np.array(colour, dtype=np.uint8)).all(-1).sum())


def test_identity_labels_is_call_on_the_label_map():
    from mmsa.evaluate import LabelPrep
    H, W = 37, 53
    _, label, _, src = _case(H, W)
    assert (label == 255).any() and (label == C + 5).any()
    r = _renderer()
    d_lab, d_src = _dev(label), _dev(src)
    for kw in (dict(), dict(source=d_src), dict(source=d_src, source_reverse=True)):
        assert torch.equal(r.labels(d_lab, LabelPrep(C), **kw), r(d_lab, **kw))


@pytest.mark.parametrize("k", (0, 7, 15))
def test_identity_abstained_is_call_on_the_abstain_map(k):
    import mmsa
    H, W = 37, 53
    wide, _, conf, src = _case(H, W)
    pred = np.ascontiguousarray(wide[:, :H, :W])
    pal256 = np.zeros((256, 3), dtype=np.int64)
    pal256[:C] = PAL
    pal256[255] = c = (9, 200, 77)
    r = _renderer(pal=pal256)
    d_pred, d_conf, d_src = _dev(pred), _dev(conf), _dev(src)
    amap = mmsa.abstain(d_pred, d_conf, 15, k)
    assert np.array_equal(amap.cpu().numpy(), DR.abstain_ref(pred, conf, 15, k))
    for kw in (dict(), dict(source=d_src)):
        assert torch.equal(r.abstained(d_pred, d_conf, 15, k, colour=c, mark_opacity=OP, **kw), r(amap, **kw))


def test_identity_errors_picture_counts_are_the_confusion_counts():
    import mmsa
    from mmsa.evaluate import LabelPrep
    H, W = 130, 67
    wide, label, _, _ = _case(H, W)
    pred = np.ascontiguousarray(wide[:, :H, :W])
    lp = LabelPrep(C)
    red, green, blue = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    pic = _renderer(bgr=False, opacity=1.0).errors(_dev(pred), _dev(label), lp, wrong=red, correct=green, ignored=blue, mark_opacity=1.0).cpu().numpy()
    conf = mmsa.confusion(_dev(pred), _dev(label), lp).cpu().numpy()
    for b in range(2):
        trace = int(np.trace(conf[b][:C, :C]))
        assert _count(pic[b], green) == trace and _count(pic[b], red) == int(conf[b].sum()) - trace and _count(pic[b], blue) == H * W - int(conf[b].sum())


@pytest.mark.parametrize("d,border", ((1, False), (3, True), (16, False)))
def test_identity_band_picture_counts_are_the_boundary_zones(d, border):
    import mmsa
    from mmsa.evaluate import LabelPrep
    H, W = 130, 67
    wide, label, _, _ = _case(H, W)
    pred = np.ascontiguousarray(wide[:, :H, :W])
    lp, r = LabelPrep(C), _renderer(opacity=1.0)
    d_pred, d_lab = _dev(pred), _dev(label)
    counts = mmsa.boundary_counts(d_pred, d_lab, lp, d, border=border).cpu().numpy()
    for where, zones in (("label", (2, 3)), ("pred", (1, 3))):
        pic = r.band(d_pred, d_lab, lp, radius=d, border=border, colour=(255, 255, 255), inside=None, where=where).cpu().numpy()
        for b in range(2):
            assert _count(pic[b], (255, 255, 255)) == int(counts[b, zones[0]].sum() + counts[b, zones[1]].sum()), (where, b)
            assert _count(pic[b], (255, 255, 255)) + _count(pic[b], (0, 0, 0)) == H * W


def test_identity_heat_colour_counts_are_the_bin_histogram():
    H, W = 130, 67
    _, _, conf, _ = _case(H, W)
    cm = np.array([(k + 1, 2 * k + 1, 255 - k) for k in range(15)])
    pic = _renderer(bgr=False, opacity=1.0).heat(_dev(conf), cm).cpu().numpy()
    hist = np.bincount(CR.bin_index(conf, 15).reshape(-1), minlength=15)
    assert [_count(pic, cm[k]) for k in range(15)] == hist.tolist() and int(hist.sum()) == conf.size


# ---- 7. end to end on the tiny model

def test_pictures_of_a_slide_class_map(models):  # noqa: F811
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    from mmsa.render import HEAT
    cfg, m, h, frame, x = models
    cm, _, conf = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, confidence=True)
    B, H, W = cm.shape
    g = np.random.default_rng(3)
    coarse = g.integers(0, NUM_CLASSES, (B, (H + 15) // 16, (W + 15) // 16))
    label = np.repeat(np.repeat(coarse, 16, 1), 16, 2)[:, :H, :W].astype(np.uint8)
    label[g.random((B, H, W)) < 0.03] = 255
    pal = PAL[:NUM_CLASSES]
    lp, lut = LabelPrep(NUM_CLASSES), ER.lut(NUM_CLASSES)
    r = _renderer(pal=pal)
    pred, cf, d_lab = cm.cpu().numpy(), conf.cpu().numpy(), _dev(label)
    assert np.array_equal(r.errors(cm, d_lab, lp, wrong="label", correct="pred").cpu().numpy(),
                          DR.errors_ref(pred, label, lut, NUM_CLASSES, pal, OP, wrong="label", correct="pred"))
    assert np.array_equal(r.heat(conf, HEAT).cpu().numpy(), DR.heat_ref(cf, HEAT, OP))
    assert np.array_equal(r.band(cm, d_lab, lp, radius=3, where="both").cpu().numpy(), DR.band_ref(pred, label, lut, NUM_CLASSES, pal, OP, 3, where="both"))


# ---- 8. out= and the cached table

def test_out_and_the_cached_tables():
    from mmsa.evaluate import LabelPrep
    H, W = 37, 53
    wide, label, conf, _ = _case(H, W)
    d_pred, d_lab, d_conf = _dev(np.ascontiguousarray(wide[:, :H, :W])), _dev(label), _dev(conf)
    lp, r = LabelPrep(C), _renderer()
    out = torch.empty(2, H, W, 3, dtype=torch.uint8, device=DEV)
    calls = (lambda: r.labels(d_lab, lp, out=out), lambda: r.errors(d_pred, d_lab, lp, out=out), lambda: r.heat(d_conf, CM15, out=out),
             lambda: r.abstained(d_pred, d_conf, 15, min_bin=4, out=out), lambda: r.band(d_pred, d_lab, lp, radius=2, out=out))
    for n, call in enumerate(calls):
        assert call() is out
        first = dict(r._tab_dev)
        assert len(first) == n + 1
        want = out.clone()
        assert call() is out and torch.equal(out, want)
        assert r._tab_dev.keys() == first.keys() and all(r._tab_dev[k] is first[k] for k in first), "the second call uploaded a table"
    r.band(d_pred, d_lab, lp, radius=2, colour=(1, 2, 3), out=out)
    assert len(r._tab_dev) == len(calls) + 1                            # other options: another table
    with pytest.raises(RuntimeError, match="`out` must be a contiguous uint8"):
        r.heat(d_conf, CM15, out=out[:, :, :-1])
