"""The diagnostic pictures without a GPU: the restatement (tests/render_diag_ref.py) against independent facts, `mmsa.render.colormap` against rational
arithmetic, the packing of the paint tables, header / ctypes table / version, the C entries' argument checks on the host and the Python refusals."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import calibration_ref as CR
from tests import eval_ref as ER
from tests import render_diag_ref as DR
from tests import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_render_labels_u8", "mmsa_render_values_f32", "mmsa_render_band_u8")
PAL25 = np.array([((37 * i + 11) % 256, (91 * i + 5) % 256, (53 * i + 200) % 256) for i in range(25)])


# ---- 1. the restatement against independent facts

@pytest.mark.parametrize("bgr", (True, False))
def test_labels_with_the_identity_lut_is_show_result(bgr):
    """A label map read through the identity LUT of 25 classes whose bytes are all classes: the ground-truth picture is show_result of that map."""
    g = np.random.default_rng(1)
    label = g.integers(0, 25, (2, 19, 23), dtype=np.uint8)
    src = g.integers(0, 256, (2, 21, 25, 3), dtype=np.uint8)
    for source in (None, src):
        assert np.array_equal(DR.labels_ref(label, ER.lut(25), 25, PAL25, 0.3, 19, 23, source, bgr=bgr), RR.render_ref(label, PAL25, 0.3, source, bgr=bgr))
    # 255 and an out-of-range byte get `ignored`: colour 0 by default, which is what show_result gives a value without a palette entry
    label[0, 3, 4], label[1, 0, 0] = 255, 30
    assert np.array_equal(DR.labels_ref(label, ER.lut(25), 25, PAL25, 0.3, 19, 23, src, bgr=bgr), RR.render_ref(label, PAL25, 0.3, src, bgr=bgr))
    pic = DR.labels_ref(label, ER.lut(25), 25, PAL25, 1.0, 19, 23, None, ignored=(1, 2, 3), bgr=bgr)
    assert pic[0, 3, 4].tolist() == pic[1, 0, 0].tolist() == ([3, 2, 1] if bgr else [1, 2, 3])
    assert np.array_equal(DR.labels_ref(label, ER.lut(25), 25, PAL25, 0.3, 19, 23, src, ignored=None)[0, 3, 4], src[0, 3, 4])


@pytest.mark.parametrize("kw", (dict(), dict(reduce_zero_label=True), dict(label_map={3: 7, 7: 255, 2: 40})))
def test_the_wrong_pixel_mask_sums_to_the_confusion_matrix(kw):
    C = 9
    pred, label = ER.make_case(5, 37, 53, C, B=2, special=True)
    lut = ER.lut(C, **kw)
    for b in range(2):
        L = DR.label_codes(label[b], lut, C, 37, 53)
        st = DR.error_states(pred[b], L, C)
        conf = ER.confusion(pred[b], label[b], C, **kw)
        assert int((st == 2).sum()) == int(conf.sum() - np.trace(conf[:C, :C]))
        assert int((st == 1).sum()) == int(np.trace(conf[:C, :C])) and int((st == 0).sum()) == pred[b].size - int(conf.sum())
        # distinct opaque colours on a black source: the picture's colour counts are those numbers
        pic = DR.errors_ref(pred[b:b + 1], label[b:b + 1], lut, C, PAL25, 0.4, wrong=(255, 0, 0), correct=(0, 255, 0), ignored=(0, 0, 255), bgr=False)[0]
        assert int((pic[..., 0] == 255).sum()) == int((st == 2).sum())          # MARKED, mark_opacity 1
        assert int((pic[..., 1] == int(255 * 0.4)).sum()) == int((st == 1).sum()) and int((pic[..., 2] == int(255 * 0.4)).sum()) == int((st == 0).sum())


@pytest.mark.parametrize("d,border", ((1, False), (2, True), (3, False)))
def test_the_band_mask_is_near(d, border):
    C = 5
    pred, label = ER.make_case(9, 17, 21, C, B=1, special=True)
    lut = ER.lut(C)
    L, P = BR.codes(pred[0], label[0], lut, C)
    m_pred = DR.band_masks(pred[0], None, lut, C, d, border, "pred")[0]
    assert np.array_equal(m_pred, BR.near(P, d, border)) and np.array_equal(m_pred, BR.near_loops(P, d, border))
    m_lab = DR.band_masks(pred[0], label[0], lut, C, d, border, "label")[0]
    assert np.array_equal(m_lab, BR.near_loops(L, d, border) & (L != 255))
    m_both = DR.band_masks(pred[0], label[0], lut, C, d, border, "both")[0]
    assert np.array_equal(m_both, (BR.near(L, d, border) | BR.near(P, d, border)) & (L != 255))
    # the marked pixels over non-ignored labels are zones 2 + 3 (label) / 1 + 3 (pred) of the counts
    counts = BR.boundary_counts(pred, label, lut, C, d, border)[0]
    assert int(m_lab.sum()) == int(counts[2].sum() + counts[3].sum())
    assert int((m_pred & (L != 255)).sum()) == int(counts[1].sum() + counts[3].sum())
    pic = DR.band_ref(pred, label, lut, C, PAL25, 0.5, d, border, colour=(255, 255, 255), inside=None, where="label")
    assert np.array_equal(pic[0, ..., 0] == 255, m_lab) and int(pic[0][~m_lab].max(initial=0)) == 0


@pytest.mark.parametrize("k", (0, 7, 15))
def test_abstained_is_show_result_of_the_abstain_map(k):
    pred, conf, _ = CR.make_case(3, 19, 23, 25, 15, B=2)
    pal256 = np.zeros((256, 3), dtype=np.int64)
    pal256[:25] = PAL25
    pal256[255] = (9, 200, 77)
    src = np.random.default_rng(2).integers(0, 256, (2, 19, 23, 3), dtype=np.uint8)
    amap = DR.abstain_ref(pred, conf, 15, k)
    assert ((amap == 255) == ((CR.bin_index(conf, 15) < k) | (pred == 255))).all()
    for source in (None, src):
        got = DR.abstained_ref(pred, conf, 15, k, pal256, 0.6, colour=(9, 200, 77), mark_opacity=0.6, source=source)
        assert np.array_equal(got, RR.render_ref(amap, pal256, 0.6, source))
    # a [bins, 3] colormap is indexed by the pixel's bin
    cm = np.arange(45).reshape(15, 3)
    got = DR.abstained_ref(pred, conf, 15, 15, PAL25, 1.0, colour=cm, bgr=False)
    assert np.array_equal(got, cm[CR.bin_index(conf, 15)].astype(np.uint8))


def test_heat_paints_the_calibration_bins():
    _, conf, _ = CR.make_case(4, 19, 23, 25, 15, B=1)
    cm = np.array([(10 * k, 255 - k, k) for k in range(15)])
    pic = DR.heat_ref(conf, cm, 1.0, bgr=False)
    k = CR.bin_index(conf, 15)
    assert np.array_equal(pic, cm[k].astype(np.uint8))
    assert k.reshape(-1)[:10].tolist() == [0, 0, 14, 0, 14, 0, 14, 14, 0, 0]      # CR.SPECIALS: NaN, -1, 2, 0, 1, 1e-40, 1 - ulp, inf, -inf, -0.0


# ---- 2. colormap

def test_colormap_is_exact_integer_arithmetic():
    from mmsa.render import HEAT, colormap
    stops = [(0, 0, 0), (255, 0, 0), (255, 255, 0), (255, 255, 255)]
    assert HEAT.dtype == np.uint8 and HEAT.shape == (256, 3) and np.array_equal(HEAT, colormap(stops, 256))
    assert HEAT[0].tolist() == [0, 0, 0] and HEAT[255].tolist() == [255, 255, 255] and HEAT[85].tolist() == [255, 0, 0] and HEAT[170].tolist() == [255, 255, 0]
    assert (np.diff(HEAT.astype(int), axis=0) >= 0).all()
    assert colormap(stops, 1).tolist() == [[0, 0, 0]] and colormap([(7, 8, 9)], 5).tolist() == [[7, 8, 9]] * 5
    for st, n in ((stops, 256), (stops, 15), ([(200, 10, 0), (3, 250, 0), (90, 90, 255)], 37), ([(0, 0, 0), (255, 255, 255)], 2), (stops, 4), (stops, 7)):
        got = colormap(st, n)
        assert got[0].tolist() == list(st[0]) and got[-1].tolist() == list(st[-1])
        S = len(st)
        for i in range(n):
            t = Fraction(i * (S - 1), n - 1)
            seg = min(int(t), S - 2)
            for c in range(3):
                exact = st[seg][c] + (st[seg + 1][c] - st[seg][c]) * (t - seg)
                assert int(got[i, c]) == (exact + Fraction(1, 2)).__floor__(), (n, i, c)
        # every stop that falls on an entry is hit exactly, and every channel is monotone between two stops
        for s in range(S - 1):
            lo, hi = -(-s * (n - 1) // (S - 1)), (s + 1) * (n - 1) // (S - 1)
            seg = got[lo:hi + 1].astype(int)
            for c in range(3):
                d = np.diff(seg[:, c])
                assert (d >= 0).all() if st[s + 1][c] >= st[s][c] else (d <= 0).all()
    for bad in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="colormap"):
            colormap(stops, bad)
    with pytest.raises(ValueError, match="RGB triple"):
        colormap([(0, 0, 256), (1, 1, 1)], 4)


# ---- 3. the packing of the tables

def test_table_packing():
    from mmsa.render import MARK, PAINT, Renderer, pack_paint
    assert (PAINT, MARK) == (1 << 24, 1 << 25)
    assert pack_paint((1, 2, 3), bgr=False) == 1 | 2 << 8 | 3 << 16 | PAINT and pack_paint((1, 2, 3), bgr=True, mark=True) == 3 | 2 << 8 | 1 << 16 | PAINT | MARK
    for bgr in (True, False):
        r = Renderer(PAL25, opacity=0.5, bgr=bgr)

        def col(e):
            c = [int(e) & 255, (int(e) >> 8) & 255, (int(e) >> 16) & 255]
            return c[::-1] if bgr else c
        t = r.labels_table(9, ignored=(4, 5, 6))
        assert t.dtype == np.uint32 and t.shape == (10,) and all(int(e) >> 24 == 1 for e in t)
        assert [col(e) for e in t[:9]] == PAL25[:9].tolist() and col(t[9]) == [4, 5, 6]
        assert int(r.labels_table(9, ignored=None)[9]) == 0                           # paint None: the entry has no PAINT bit
        t = r.errors_table(wrong="label", correct="pred", ignored=None)
        assert t.shape == (513,) and int(t[0]) == 0
        assert all(int(e) >> 24 == 1 for e in t[1:257]) and all(int(e) >> 24 == 3 for e in t[257:])      # correct: PAINT; wrong: PAINT | MARK
        assert [col(e) for e in t[1:26]] == PAL25.tolist() and [col(e) for e in t[257:282]] == PAL25.tolist()
        assert all(col(e) == [0, 0, 0] for e in t[26:257]) and all(col(e) == [0, 0, 0] for e in t[282:])   # a code without a palette entry: colour 0
        t = r.errors_table()
        assert all(int(e) == 0 for e in t[:257]) and all(int(e) >> 24 == 3 and col(e) == [255, 0, 0] for e in t[257:])
        t = r.heat_table([(1, 2, 3), (4, 5, 6)])
        assert t.shape == (2,) and [col(e) for e in t] == [[1, 2, 3], [4, 5, 6]] and all(int(e) >> 24 == 1 for e in t)
        t = r.abstained_table(15, (7, 8, 9))
        assert t.shape == (271,) and [col(e) for e in t[:25]] == PAL25.tolist() and all(int(e) >> 24 == 1 for e in t[:256])
        assert all(int(e) >> 24 == 3 and col(e) == [7, 8, 9] for e in t[256:])
        cm = np.arange(45).reshape(15, 3)
        assert [col(e) for e in r.abstained_table(15, cm)[256:]] == cm.tolist()
        t = r.band_table(colour=(255, 255, 255), inside="label")
        assert t.shape == (512,) and all(int(e) >> 24 == 3 and col(e) == [255] * 3 for e in t[:256])
        assert [col(e) for e in t[256:281]] == PAL25.tolist() and all(int(e) >> 24 == 1 for e in t[256:])
        assert all(int(e) == 0 for e in r.band_table(colour="pred", inside=None)[256:])


# ---- 4. header, ctypes table, version; the C entries' argument checks on the host

def test_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    vh = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\(", hdr) and e in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, e) and e in vh, e
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == int(re.search(r"#define MMSA_ABI_VERSION (\d+)", vh).group(1)) == 114
    for m in ("labels", "errors", "heat", "abstained", "band"):
        assert callable(getattr(mmsa.Renderer, m))
    assert mmsa.render.HEAT.shape == (256, 3)


def test_the_library_refuses_bad_arguments_on_the_host():
    """Called with fake pointers: every refusal comes before any launch (no GPU needed)."""
    import mmsa
    fake = ctypes.c_void_p(256)
    tail = dict(table=fake, ntab=512, src=None, form=0, Cs=0, Hs=0, Ws=0, rev=0, mean=None, std=None, to_rgb=0, mul255=0, op=0.5, om=0.5, mop=1.0, mom=0.0, out=fake)

    def refused(entry, head, **kw):
        t = dict(tail, **kw)
        rc = getattr(mmsa.lib.raw, entry)(*head, *(t[k] for k in tail), None)
        return rc != 0 and mmsa.lib.last_error()

    def band(radius=1, C=25, pred=fake, label=fake, where=3, Hl=8, **kw):
        return refused("mmsa_render_band_u8", (pred, 64, 8, label, 1, 8, 8, Hl, 8, fake, C, None, None, radius, 0, where, 0, 0), **kw)

    def values(bins=15, min_bin=3, pred=fake, **kw):
        return refused("mmsa_render_values_f32", (fake, pred, 64, 8, 1, 8, 8, bins, min_bin), **dict(dict(ntab=(256 if pred else 0) + bins), **kw))

    def labels(mode=1, C=25, Hl=8, **kw):
        return refused("mmsa_render_labels_u8", (fake, 64, 8, fake, 1, 8, 8, Hl, 8, fake, C, None, None, mode, 0), **dict(dict(ntab=513 if mode else C + 1), **kw))

    for r in (0, 33):
        assert "1..32" in band(radius=r)
    assert "1..253" in band(C=254) and "1..253" in band(C=0)
    assert "pred or label is required" in band(pred=None, label=None)
    assert "needs label" in band(label=None) and "needs pred" in band(pred=None)
    assert "size mismatch" in band(Hl=9)
    for b in (0, 257):
        assert "1..256" in values(bins=b)
    assert "0..15 for 15 bins" in values(min_bin=16) and "0..15 for 15 bins" in values(min_bin=-1)
    assert "paint table has 15 entries, this picture needs 271" in values(ntab=15)
    assert "1..254" in labels(C=255) and "mode = 2" in labels(mode=2) and "size mismatch" in labels(Hl=9)
    for fn in (band, values, labels):
        assert "table and out are required" in fn(out=None) and "table and out are required" in fn(table=None)
        assert "source is smaller than the 8 x 8 map" in fn(src=fake, form=1, Hs=8, Ws=7)
        assert "source is smaller than the 8 x 8 map" in fn(src=fake, form=2, Cs=3, Hs=7, Ws=8, mean=fake, std=fake)
        assert "needs src" in fn(form=1, Hs=8, Ws=8) and "src_form = 3" in fn(src=fake, form=3)
        assert "first 3" in fn(src=fake, form=2, Cs=2, Hs=8, Ws=8, mean=fake, std=fake) and "mean and std" in fn(src=fake, form=2, Cs=3, Hs=8, Ws=8)
        assert "mark_opacity" in fn(mop=0.0, mom=1.0) and "opacity" in fn(op=1.5)
        assert "overlap" in refused(*{band: ("mmsa_render_band_u8", (fake, 64, 7, fake, 1, 8, 8, 8, 8, fake, 25, None, None, 1, 0, 3, 0, 0)),
                                      values: ("mmsa_render_values_f32", (fake, fake, 64, 7, 1, 8, 8, 15, 3)),
                                      labels: ("mmsa_render_labels_u8", (fake, 64, 7, fake, 1, 8, 8, 8, 8, fake, 25, None, None, 1, 0))}[fn],
                                    **({"ntab": 271} if fn is values else {"ntab": 513} if fn is labels else {}))


# ---- 5. the Python refusals (every one before anything is looked at on a device)

class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on a GPU: the argument checks of the methods run, no launch is ever reached."""
    @property
    def is_cuda(self):
        return True


def _fake(t):
    return t.as_subclass(_FakeCuda)


def test_python_refusals():
    from mmsa.evaluate import LabelPrep
    from mmsa.render import Renderer
    r = Renderer(PAL25, opacity=0.5)
    prep = LabelPrep(25)
    pred = _fake(torch.zeros(1, 8, 8, dtype=torch.uint8))
    lab = _fake(torch.zeros(1, 8, 8, dtype=torch.uint8))
    conf = _fake(torch.zeros(1, 8, 8))
    with pytest.raises(ValueError, match="band needs pred=, labels= or both"):
        r.band()
    with pytest.raises(ValueError, match="band colour='label' needs labels="):
        r.band(pred, colour="label")
    with pytest.raises(ValueError, match="band inside='label' needs labels="):
        r.band(pred, inside="label")
    with pytest.raises(ValueError, match="band where='both' needs labels="):
        r.band(pred, where="both")
    with pytest.raises(ValueError, match="band where='pred' needs pred="):
        r.band(labels=lab, prep=prep)
    with pytest.raises(ValueError, match="labels need prep="):
        r.band(pred, labels=lab, where="label")
    with pytest.raises(ValueError, match="where = 'edge'"):
        r.band(pred, where="edge")
    for rad in (0, 33, 1.0):
        with pytest.raises(ValueError, match=r"mmsa.Renderer: radius = .*1\.\.32"):
            r.band(pred, radius=rad)
    with pytest.raises(ValueError, match=r"band with 254 classes; 1\.\.253"):
        r.band(pred, num_classes=254)
    with pytest.raises(ValueError, match=r"band with 256 classes; 1\.\.253"):
        Renderer(np.zeros((256, 3), dtype=np.int64)).band(pred)
    with pytest.raises(ValueError, match="not a bin edge of 15 bins"):
        r.abstained(pred, conf, 15, threshold=0.5)
    with pytest.raises(ValueError, match="min_bin= or threshold=, one of them"):
        r.abstained(pred, conf, 15)
    with pytest.raises(ValueError, match="min_bin = 16; 0..15 for 15 bins"):
        r.abstained(pred, conf, 15, min_bin=16)
    with pytest.raises(ValueError, match="colormap of the abstained pixels has 3 rows for 15 bins"):
        r.abstained(pred, conf, 15, min_bin=3, colour=np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError, match=r"colormap has 257 rows; 1\.\.256"):
        r.heat(conf, np.zeros((257, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="colormap must be an"):
        r.heat(conf, np.zeros((4, 3)))
    with pytest.raises(RuntimeError, match="values must be a contiguous float32"):
        r.heat(pred, np.zeros((4, 3), dtype=np.int64))
    with pytest.raises(RuntimeError, match="size mismatch: the label maps are 9 x 8"):
        r.errors(pred, _fake(torch.zeros(1, 9, 8, dtype=torch.uint8)), prep)
    with pytest.raises(ValueError, match="wrong = None; a colour is required"):
        r.errors_table(wrong=None)
    with pytest.raises(ValueError, match="correct = 'label'; 'pred' or an RGB triple or None is expected"):
        r.errors_table(correct="label")
    with pytest.raises(ValueError, match="ignored = 'pred'"):
        r.labels_table(25, ignored="pred")
    with pytest.raises(ValueError, match="ignored = .*RGB triple of integers in 0..255"):
        r.labels_table(25, ignored=(0, 0, 300))
    with pytest.raises(ValueError, match=r"mark_opacity 0.0 must be in \(0, 1\]"):
        r._picture("mmsa_render_band_u8", (), None, 1, 8, 8, pred.device, None, False, 0.0, None)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        r.errors(torch.zeros(1, 8, 8, dtype=torch.uint8), lab, prep)
