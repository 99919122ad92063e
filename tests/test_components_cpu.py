"""Segment-level evaluation without a GPU: the restatement (tests/components_ref.py) against scipy.ndimage.label, the host functions on hand-made counts, every
argument refusal that needs no device, the C entries' checks on the host, and header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import components_ref as CR
from tests import eval_ref as ER

import mmsa.evaluate as E  # noqa: E402  (what this file is about: a tree without the segment passes fails every test of it here)

assert CR.SIZE_BUCKETS == E.SIZE_BUCKETS == 24

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mmsa_components_u8", "mmsa_component_area", "mmsa_suppress_small_u8", "mmsa_eval_segments")


def _checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) % 2 + 3).astype(np.uint8)


def _maps():
    rng = np.random.default_rng(21)
    return [("noise", rng.integers(0, 25, size=(37, 53)).astype(np.uint8)), ("noise3", rng.integers(0, 3, size=(40, 29)).astype(np.uint8)),
            ("blocky", CR.blocky(rng, 67, 131, 25)), ("blocky5", CR.blocky(rng, 50, 90, 5, 3, 9)), ("checkerboard", _checkerboard(11, 14)),
            ("serpentine", CR.serpentine(67, 131)), ("spiral", CR.spiral(67, 131)), ("comb", CR.comb(33, 70)), ("staircase", CR.staircase(40, 40)),
            ("one code", np.full((6, 9), 7, dtype=np.uint8)), ("one pixel", np.full((1, 1), 255, dtype=np.uint8))]


def _scipy_roots(code, connectivity):
    """Per code and with the structuring element of the connectivity: scipy's labels, relabelled to the smallest linear index of each component."""
    ndi = pytest.importorskip("scipy.ndimage")
    H, W = code.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    out = np.full((H, W), -1, dtype=np.int64)
    st = ndi.generate_binary_structure(2, 2 if connectivity == 8 else 1)
    for c in np.unique(code):
        lab, n = ndi.label(code == c, structure=st)
        low = np.asarray(ndi.minimum(idx, lab, index=np.arange(1, n + 1))).astype(np.int64)
        out[lab > 0] = low[lab[lab > 0] - 1]
    return out


# ---- 1. the restatement

@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_restated_roots_equal_scipy_label(connectivity):
    for name, m in _maps():
        got = CR.roots(m, connectivity)
        assert got.dtype == np.int32 and np.array_equal(got, _scipy_roots(m, connectivity)), name
        flat = got.ravel()
        assert np.array_equal(flat[flat], flat) and (flat <= np.arange(flat.size)).all(), name      # a root is its own root, and the smallest of its component


def test_checkerboard_serpentine_and_staircase_by_hand():
    cb = _checkerboard(11, 14)
    assert np.array_equal(CR.roots(cb, 4).ravel(), np.arange(cb.size))                  # every pixel is its own component
    r8 = CR.roots(cb, 8)
    assert np.array_equal(np.unique(r8), [0, 1]) and np.array_equal(r8 == 0, cb == cb[0, 0])      # one component per code
    s = CR.serpentine(9, 7)
    for conn in (4, 8):
        r = CR.roots(s, conn)
        assert (r[s == 1] == 0).all() and CR.areas(r)[0, 0] == (s == 1).sum()            # the path is ONE component, rooted at the corner
    st = CR.staircase(8, 8)
    assert len(np.unique(CR.roots(st, 4)[st == 1])) == 8 and len(np.unique(CR.roots(st, 8)[st == 1])) == 1
    sp = CR.spiral(20, 31)
    assert len(np.unique(CR.roots(sp, 4))) == 2 and len(np.unique(CR.roots(sp, 8))) == 2


def test_restated_areas_suppression_and_counts_by_hand():
    pred = np.array([[[0, 0, 1, 1, 9], [0, 2, 1, 1, 9], [0, 0, 0, 1, 9]]], dtype=np.uint8)      # C = 3: 9 reads as the code 3
    r = CR.roots(np.minimum(pred[0], 3), 4)
    assert r.tolist() == [[0, 0, 2, 2, 4], [0, 6, 2, 2, 4], [0, 0, 0, 2, 4]]
    a = CR.areas(r)
    assert a.sum() == 15 and a.ravel()[[0, 2, 4, 6]].tolist() == [6, 5, 3, 1] and np.array_equal(a != 0, r == np.arange(15).reshape(3, 5))
    assert np.array_equal(CR.suppress(pred, 3, 1, 4), pred)
    assert CR.suppress(pred, 3, 4, 4, fill=7)[0].tolist() == [[0, 0, 1, 1, 7], [0, 7, 1, 1, 7], [0, 0, 0, 1, 7]]      # the byte 9 stays a 9 where it is kept
    assert (CR.suppress(pred, 3, 16, 4) == 255).all()
    label = np.array([[[0, 0, 1, 1, 255], [0, 0, 1, 1, 255], [0, 0, 1, 1, 2]]], dtype=np.uint8)
    counts, planes, rp, rl = CR.segment_counts(pred, label, ER.lut(3), 3, 10, 4)
    assert counts.shape == (1, 2, 3, 24, 11) and planes.shape == (4, 1, 3, 5)
    # label segments: class 0 (6 pixels, 5 hit: bin 8), class 1 (6 pixels, 5 hit: bin 8), class 2 (1 pixel, none: bin 0); the ignored segment is counted nowhere
    assert counts[0, 0].sum() == 3 and counts[0, 0, 0, 2, 8] == 1 and counts[0, 0, 1, 2, 8] == 1 and counts[0, 0, 2, 0, 0] == 1
    # prediction segments: class 0 (6: 5 hit), class 2 (1: 0), class 1 (5: 5 -> the last bin); the code-3 blob (area 1 behind the ignored pixels) is no class
    assert counts[0, 1].sum() == 3 and counts[0, 1, 0, 2, 8] == 1 and counts[0, 1, 2, 0, 0] == 1 and counts[0, 1, 1, 2, 10] == 1
    assert planes[0].sum() == planes[2].sum() == 13 and planes[1].sum() == planes[3].sum() == 10


# ---- 2. the host functions

def _hand():
    c = np.zeros((2, 3, 24, 11), dtype=np.int64)
    c[0, 0, 0, 10] = 4          # four one-pixel objects of class 0, all found
    c[0, 0, 5, 3] = 2           # two of 32..63 pixels, covered to [0.3, 0.4)
    c[0, 0, 5, 5] = 1
    c[0, 1, 23, 10] = 1         # one huge object of class 1
    c[1, 0, 0, 0] = 6           # six one-pixel blobs of class 0, none real
    c[1, 0, 6, 9] = 2
    return c                    # class 2 has no segment on either side


def test_bucket_folding_and_its_refusals():
    c = _hand()
    t = E.segment_totals_of(c)
    assert t.shape == (2, 3, 11) and t.dtype == np.int64 and t.sum() == c.sum() and t[0, 0, 10] == 4 and t[0, 0, 3] == 2
    assert E.segment_totals_of(c, 2).sum() == 6 and E.segment_totals_of(c, 32, 64).sum() == 3 and E.segment_totals_of(c, 1, 2).sum() == 10
    assert E.segment_totals_of(c, 1 << 23).sum() == 1 and E.segment_totals_of(np.stack([c, c]), 64).shape == (2, 2, 3, 11)
    with pytest.raises(ValueError, match="min_area = 48 is not the edge of a size bucket.*nearest edges are 32 and 64"):
        E.segment_totals_of(c, 48)
    with pytest.raises(ValueError, match="max_area = 100 is not the edge.*64 and 128"):
        E.segment_totals_of(c, 1, 100)
    with pytest.raises(ValueError, match=r"min_area = 16777216 is not the edge.*8388608"):
        E.segment_totals_of(c, 1 << 24)
    for bad in (0, -4, 2.0, True, "8"):
        with pytest.raises(ValueError, match="min_area"):
            E.segment_totals_of(c, bad)
    with pytest.raises(ValueError, match="max_area = 8 must be above min_area = 8"):
        E.segment_totals_of(c, 8, 8)
    for bad in (np.zeros((2, 3, 23, 11), dtype=np.int64), np.zeros((3, 3, 24, 11), dtype=np.int64), np.zeros((2, 3, 24, 11)), np.zeros((24, 11), dtype=np.int64)):
        with pytest.raises(ValueError, match="segment counts are an integer"):
            E.segment_totals_of(bad)


def test_rates_thresholds_and_nan():
    c = _hand()
    r = E.segment_rate_of(c, 0)
    assert r.dtype == np.float64 and r[0] == 5 / 7 and r[1] == 1.0 and np.isnan(r[2])                      # 0 / 0 is NaN
    assert E.segment_rate_of(c, 0, 0.3)[0] == 1.0 and E.segment_rate_of(c, 0, 0.4)[0] == 5 / 7 and E.segment_rate_of(c, 0, 1.0)[0] == 4 / 7
    assert E.segment_rate_of(c, 0, 0)[0] == 1.0 and E.segment_rate_of(c, 0, 0.5, 32)[0] == 1 / 3 and np.isnan(E.segment_rate_of(c, 0, 0.5, 64)[0])
    p = E.segment_rate_of(c, 1)
    assert p[0] == 2 / 8 and np.isnan(p[1]) and np.isnan(p[2])
    f = E.segment_f_of(c)
    assert f[0] == 2 * (5 / 7) * (2 / 8) / (5 / 7 + 2 / 8) and np.isnan(f[1]) and np.isnan(f[2])
    zero = np.zeros_like(c)
    zero[0, 0, 0, 0] = zero[1, 0, 0, 0] = 1
    assert np.isnan(E.segment_f_of(zero)[0])                                                              # both rates 0: 0 / 0
    with pytest.raises(ValueError, match="threshold 0.25 is not a bin edge of 10 coverage bins.*nearest edges are 0.2 and 0.3"):
        E.segment_rate_of(c, 0, 0.25)
    for bad in (-0.1, 1.5, "0.5", None, True):
        with pytest.raises(ValueError, match="threshold"):
            E.segment_rate_of(c, 0, bad)
    for bad in (2, -1, None, True):
        with pytest.raises(ValueError, match="side = "):
            E.segment_rate_of(c, bad)


def test_recall_is_one_when_the_prediction_is_the_labels():
    rng = np.random.default_rng(5)
    label = np.stack([CR.blocky(rng, 40, 70, 6, 3, 9), rng.integers(0, 6, size=(40, 70)).astype(np.uint8)])
    label[0, 5:9, 10:30] = 255
    pred = np.where(label == 255, 3, label).astype(np.uint8)          # the ignored pixels join whatever blob: their area does not count
    counts = CR.segment_counts(pred, label, ER.lut(6), 6, 10)[0]
    assert counts[:, 0, :, :, :10].sum() == 0 and counts[:, 0].sum() > 100
    r = E.segment_rate_of(counts.sum(0), 0, 1.0)
    assert (r == 1.0).all() and (E.segment_rate_of(counts.sum(0), 1, 1.0) == 1.0).all() and (E.segment_f_of(counts, 1.0) == 1.0).all()


def test_evaluator_on_hand_made_counts():
    from mmsa.evaluate import LabelPrep, SegmentEvaluator
    from mmsa.dist import allreduce_counts
    lp = LabelPrep(3)
    se = SegmentEvaluator(lp, cases=["fog", "night"])
    assert se.n_bins == 10 and se.connectivity == 8 and se.counts is None and se._trailing() == (2, 3, 24, 11) and se.host_counts().shape == (2, 2, 3, 24, 11)
    assert SegmentEvaluator(lp, bins=64, connectivity=4, images=5).host_counts().shape == (0, 2, 3, 24, 65)
    c = _hand()
    se.host_counts = lambda: np.stack([c, np.zeros_like(c)])
    assert np.array_equal(se.recall(slot="fog"), E.segment_rate_of(c, 0), equal_nan=True) and np.array_equal(se.recall(), se.recall(slot=0), equal_nan=True)
    assert se.precision(0.5, 64)[0] == 1.0 and se.f1(slot="fog")[0] == E.segment_f_of(c)[0] and np.isnan(se.recall(slot="night")).all()
    b = se.by_size(slot="fog")
    assert list(b) == ["min_area", "label_segments", "pred_segments", "recall", "precision"] and b["min_area"].tolist() == [1 << s for s in range(24)]
    assert b["label_segments"].shape == (24, 3) and b["label_segments"][5, 0] == 3 and b["recall"][5, 0] == 1 / 3 and b["recall"][0, 0] == 1.0
    assert b["precision"][0, 0] == 0.0 and np.isnan(b["precision"][1, 0]) and b["pred_segments"][6, 0] == 2
    s = se.summary(slot="fog")
    assert list(s) == ["label_segments", "pred_segments", "mSR", "mSP", "mSF", "threshold", "connectivity"]
    assert s["label_segments"] == 8 and s["pred_segments"] == 8 and s["mSR"] == np.round((5 / 7 + 1) / 2 * 100, 2) / 100.0 and s["mSP"] == 0.25
    assert s["threshold"] == 0.5 and s["connectivity"] == 8
    assert np.isnan(se.summary(slot="night")["mSR"]) and se.summary(slot="night")["label_segments"] == 0
    assert SegmentEvaluator(lp, bins=5).summary()["threshold"] == 0.6      # an odd bin count: the next edge above one half
    t = torch.from_numpy(np.stack([c, c]))
    assert allreduce_counts(t) is t and torch.equal(t[0], torch.from_numpy(c))      # one rank: the one collective hands the buffer back


# ---- 3. refusals that need no device

def test_python_refusals_of_maps_and_arguments():
    import mmsa
    from mmsa.evaluate import LabelPrep, SegmentEvaluator
    lp = LabelPrep(5)
    m = torch.zeros(1, 6, 8, dtype=torch.uint8)
    r = torch.zeros(1, 6, 8, dtype=torch.int32)
    # components
    for conn in (0, 6, "8", None, True, 8.0):
        with pytest.raises(ValueError, match="connectivity = .*4 .* or 8"):
            mmsa.components(m, num_classes=5, connectivity=conn)
    with pytest.raises(ValueError, match="components takes num_classes= .* or labels_prep="):
        mmsa.components(m)
    with pytest.raises(ValueError, match="components takes num_classes= .* or labels_prep="):
        mmsa.components(m, num_classes=5, labels_prep=lp)
    with pytest.raises(ValueError, match="num_classes 300"):
        mmsa.components(m, num_classes=300)
    with pytest.raises(RuntimeError, match="map is torch.float32"):
        mmsa.components(m.float(), num_classes=5)
    with pytest.raises(RuntimeError, match=r"map must be a contiguous \[B, H, W\] tensor"):
        mmsa.components(m[0], num_classes=5)
    with pytest.raises(RuntimeError, match="map must be a tensor"):
        mmsa.components(m.numpy(), num_classes=5)
    with pytest.raises(RuntimeError, match="only labels are resized"):
        mmsa.components(m, num_classes=5, size=(3, 4))
    with pytest.raises(RuntimeError, match="size mismatch: the label maps are 6 x 8"):
        mmsa.components(m, labels_prep=lp, size=(12, 16))
    with pytest.raises(RuntimeError, match="an empty map"):
        mmsa.components(torch.zeros(1, 0, 8, dtype=torch.uint8), num_classes=5)
    with pytest.raises(RuntimeError, match="map must be a GPU tensor"):
        mmsa.components(m, num_classes=5)
    with pytest.raises(TypeError):
        mmsa.components(m, 5)                                        # the keywords are keywords
    # component_areas
    with pytest.raises(RuntimeError, match="root is torch.int64; an int32 root map"):
        mmsa.component_areas(r.long())
    with pytest.raises(RuntimeError, match="an empty map"):
        mmsa.component_areas(r[:, :0].contiguous())
    with pytest.raises(RuntimeError, match=r"out must be a contiguous int32 \(1, 6, 8\) tensor"):
        mmsa.component_areas(r, out=torch.zeros(1, 6, 9, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="root must be a GPU tensor"):
        mmsa.component_areas(r)
    # suppress_small
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="min_area = "):
            mmsa.suppress_small(m, bad, num_classes=5)
    for bad in (-1, 256, 1.0):
        with pytest.raises(ValueError, match="fill = "):
            mmsa.suppress_small(m, 4, num_classes=5, fill=bad)
    with pytest.raises(ValueError, match="connectivity = 5"):
        mmsa.suppress_small(m, 4, num_classes=5, connectivity=5)
    with pytest.raises(TypeError):
        mmsa.suppress_small(m, 4)                                    # num_classes= is required
    with pytest.raises(RuntimeError, match="pred is torch.int32"):
        mmsa.suppress_small(r, 4, num_classes=5)
    with pytest.raises(RuntimeError, match=r"out has shape \(1, 6, 9\)"):
        mmsa.suppress_small(m, 4, num_classes=5, out=torch.zeros(1, 6, 9, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"area must be a contiguous int32 \(1, 6, 8\) tensor"):
        mmsa.suppress_small(m, 4, num_classes=5, area=r.long())
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        mmsa.suppress_small(m, 4, num_classes=5, root=r, area=r.clone())
    # segment_counts
    for bins in (0, 65, 2.0, None, True):
        with pytest.raises(ValueError, match="bins = .*1..64 coverage bins"):
            mmsa.segment_counts(m, m, lp, r, r, bins=bins)
    with pytest.raises(RuntimeError, match="root_pred is torch.uint8; an int32 root map"):
        mmsa.segment_counts(m, m, lp, m, r)
    with pytest.raises(RuntimeError, match=r"root_label has shape \(1, 6, 9\)"):
        mmsa.segment_counts(m, m, lp, r, torch.zeros(1, 6, 9, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        mmsa.segment_counts(m, m, lp, r, r)
    # the evaluator
    with pytest.raises(ValueError, match="mmsa.SegmentEvaluator: bins = 0"):
        SegmentEvaluator(lp, bins=0)
    with pytest.raises(ValueError, match="mmsa.SegmentEvaluator: connectivity = 6"):
        SegmentEvaluator(lp, connectivity=6)
    with pytest.raises(ValueError, match="at least one slot"):
        SegmentEvaluator(lp, cases=[])
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        SegmentEvaluator(lp).add(m, m)
    se = SegmentEvaluator(lp, cases=["a"])
    with pytest.raises(KeyError, match="case 'b' is not one of"):
        se.slots_for(1, case="b")


def test_python_refusals_of_the_entries():
    """segments= on every class-map entry: refused before the frame is looked at, under the entry's name (the form of boundary=)."""
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import BoundaryEvaluator, Evaluator, LabelPrep, SegmentEvaluator
    lp = LabelPrep(5)
    se = SegmentEvaluator(lp, images=2)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    out = torch.zeros(1, 8, 8, dtype=torch.uint8)
    plan = inf.MapPlan.whole(1, 8, 8)

    def entries(**kw):
        return [("slide_class_map", lambda: inf.slide_class_map(None, None, None, (8, 8), (8, 8), **kw)), ("whole_class_map", lambda: inf.whole_class_map(None, None, None, **kw)),
                ("class_map", lambda: inf.class_map(None, None, None, dict(mode="whole"), **{k: v for k, v in kw.items() if k != "return_map"})),
                ("aug_class_map", lambda: inf.aug_class_map(None, None, None, dict(mode="whole"), **{k: v for k, v in kw.items() if k != "return_map"})),
                ("inference", lambda: plan.class_map(None, out, None, **kw))]

    for name, call in entries(segments=se):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: segments= needs labels="):
            call()
    for other in (Evaluator(lp), BoundaryEvaluator(lp, 2), 3, lp):
        for name, call in entries(segments=other, labels=lab):
            with pytest.raises(RuntimeError, match=f"mmsa.{name}: segments= takes an mmsa.evaluate.SegmentEvaluator, got {type(other).__name__}"):
                call()
    for name, call in entries(segments=se, labels=lab, evaluator=Evaluator(lp), return_map=False):
        if name in ("class_map", "aug_class_map"):      # these take no return_map=
            continue
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: segments= with return_map=False: .*stores none"):
            call()
    o = inf.MapOptions.of("SlideRunner")
    for kw, why in ((dict(segments=se), "segments= needs labels="), (dict(segments=Evaluator(lp), labels=lab), "segments= takes an mmsa.evaluate.SegmentEvaluator, got Evaluator"),
                    (dict(segments=se, labels=lab, evaluator=Evaluator(lp), return_map=False), "segments= with return_map=False")):
        with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: " + why):
            o.with_call("SlideRunner.run", **kw)
    ok = inf.MapOptions.of("whole_class_map", labels=lab, segments=se).at((1, 8, 8), None, "whole_class_map")      # labels= + segments= is a complete call
    assert ok.segments is se and ok.evaluator is None and ok.boundary is None and ok.labels is lab
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.SlideRunner.run, inf.MapOptions.with_call):
        assert inspect.signature(fn).parameters["segments"].default is None, fn
    assert inf.MapOptions().segments is None
    for name in ("SegmentEvaluator", "components", "component_areas", "suppress_small", "segment_counts", "segment_totals_of", "segment_rate_of", "segment_f_of"):
        assert name in mmsa.__all__ and getattr(mmsa, name) is getattr(E, name), name


def test_the_entries_refuse_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but the slot table, which the entry reads on the host."""
    import mmsa
    raw = mmsa.lib.raw
    fake, other = ctypes.c_void_p(256), ctypes.c_void_p(512)
    ERR_ARG = -1

    def comp(src=fake, B=1, Hs=4, Ws=4, lut=None, ymap=None, xmap=None, H=4, W=4, conn=8, root=other):
        rc = raw.mmsa_components_u8(src, B, Hs, Ws, lut, ymap, xmap, H, W, conn, root, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for conn in (0, 6, -8, 16):
        rc, msg = comp(conn=conn)
        assert rc == ERR_ARG and f"components_u8: connectivity = {conn}; 4 or 8 is expected" in msg, msg
    for kw in (dict(src=None), dict(root=None)):
        rc, msg = comp(**kw)
        assert rc == ERR_ARG and "components_u8: src and root are required" in msg, msg
    rc, msg = comp(xmap=fake)
    assert rc == ERR_ARG and "components_u8: ymap and xmap come together" in msg
    rc, msg = comp(Ws=5)
    assert rc == ERR_ARG and "components_u8: size mismatch: the source is 4 x 5, the grid 4 x 4" in msg
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(B=2, H=1 << 15, W=1 << 15, Hs=1 << 15, Ws=1 << 15), dict(B=70000, H=1, W=1, Hs=1, Ws=1)):
        rc, msg = comp(**kw)
        assert rc == ERR_ARG and "components_u8: bad map size" in msg, msg

    def call(entry, *args):
        rc = getattr(raw, entry)(*args, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    for args in ((None, 1, 4, 4, other), (fake, 1, 4, 4, None), (fake, 1, 4, 4, fake)):
        rc, msg = call("mmsa_component_area", *args)
        assert rc == ERR_ARG and "component_area: root and area are required, and two planes" in msg, msg
    rc, msg = call("mmsa_component_area", fake, 1, 0, 4, other)
    assert rc == ERR_ARG and "component_area: bad map size" in msg
    for k in range(4):
        args = [fake, fake, fake, 1, 4, 4, 2, 255, fake]
        args[k if k < 3 else 8] = None
        rc, msg = call("mmsa_suppress_small_u8", *args)
        assert rc == ERR_ARG and "suppress_small_u8: pred, root, area and out are required" in msg, msg
    for min_area in (0, -1):
        rc, msg = call("mmsa_suppress_small_u8", fake, fake, fake, 1, 4, 4, min_area, 255, fake)
        assert rc == ERR_ARG and f"suppress_small_u8: min_area = {min_area}; at least 1" in msg, msg
    for fill in (-1, 256):
        rc, msg = call("mmsa_suppress_small_u8", fake, fake, fake, 1, 4, 4, 2, fill, fake)
        assert rc == ERR_ARG and f"suppress_small_u8: fill = {fill}; a byte" in msg, msg

    slots = (ctypes.c_int * 1)(0)

    def seg(pred=fake, label=fake, Hl=4, lut=fake, C=5, tab=slots, rp=fake, rl=fake, bins=10, scratch=fake, buf=fake):
        return call("mmsa_eval_segments", pred, label, 1, 4, 4, Hl, 4, lut, C, None, None, tab, 1, rp, rl, bins, scratch, buf)

    for kw in (dict(pred=None), dict(rp=None), dict(rl=None), dict(scratch=None)):
        rc, msg = seg(**kw)
        assert rc == ERR_ARG and "eval_segments: pred, root_pred, root_label and scratch are required" in msg, msg
    for kw in (dict(label=None), dict(lut=None), dict(buf=None), dict(tab=None)):
        rc, msg = seg(**kw)
        assert rc == ERR_ARG and "eval_segments: label, lut, slots and counts are required" in msg, msg
    rc, msg = seg(Hl=5)
    assert rc == ERR_ARG and "eval_segments: size mismatch" in msg
    rc, msg = seg(tab=(ctypes.c_int * 1)(3))
    assert rc == ERR_ARG and "eval_segments: slots[0] = 3 outside the 1 count slots" in msg
    for bins in (0, 65, -2):
        rc, msg = seg(bins=bins)
        assert rc == ERR_ARG and f"eval_segments: bins = {bins}; 1..64 coverage bins" in msg, msg
    for C in (1, 255):
        rc, msg = seg(C=C)
        assert rc == ERR_ARG and f"eval_segments: {C} classes; 2..254 are supported" in msg, msg


def test_the_entries_are_declared_bound_and_versioned():
    import mmsa
    from tests.test_host_cpu import _header_prototypes
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == int(re.search(r"#define MMSA_ABI_VERSION (\d+)", ver).group(1)) == 114
    protos = _header_prototypes()
    kinds = {ctypes.c_void_p: "P", ctypes.c_int: "I"}
    sig = mmsa.lib.SIGNATURES
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\(", hdr) and e in sig and hasattr(mmsa.lib.raw, e) and e in ver, e
        assert protos[e] == ("I", [kinds[t] for t in sig[e]]), e
    # the distance entry's arguments without cap, border and scratch, with the connectivity
    assert len(sig["mmsa_components_u8"]) == len(sig["mmsa_boundary_distance_u8"]) - 3 + 1
    assert len(sig["mmsa_eval_segments"]) == len(sig["mmsa_eval_confusion_u8"]) + 4      # the two root maps, bins and the scratch
