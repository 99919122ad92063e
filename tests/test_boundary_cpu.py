"""Boundary evaluation without a GPU: the fixed example of DESIGN.md section 2 through the restatement (tests/boundary_ref.py) and the `_of` functions, the
restatement's identities on random maps, the metrics on hand-made counts, every refusal of `boundary=` before anything is launched, the C entry's argument
checks on the host, and header / ctypes table / version."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import boundary_ref as BR
from tests import eval_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mmsa_eval_boundary_u8"


# ---- 1. the fixed example: an 8 x 8 map, C = 2, label class 1 on rows 2..5 x cols 2..5, prediction class 1 on rows 2..5 x cols 3..6

def _example():
    label = np.zeros((1, 8, 8), dtype=np.uint8)
    pred = np.zeros((1, 8, 8), dtype=np.uint8)
    label[0, 2:6, 2:6] = 1
    pred[0, 2:6, 3:7] = 1
    return pred, label


EXAMPLE = [  # d, border, zone[0..3] as [l0p0, l0p1, l1p0, l1p1], BIoU class 0 / 1, band pixels, trimap aAcc
    (1, False, ([22, 0, 0, 2], [6, 0, 0, 2], [6, 0, 0, 2], [10, 4, 4, 6]), 1 / 3, 1 / 3, 32, 0.75),
    (1, True, ([0, 0, 0, 2], [0, 0, 0, 2], [6, 0, 0, 2], [38, 4, 4, 6]), 38 / 52, 1 / 3, 60, 52 / 60),
    (2, False, ([0, 0, 0, 0], [0, 0, 0, 0], [8, 0, 0, 0], [36, 4, 4, 12]), 36 / 52, 0.6, 64, 0.875),
]


@pytest.mark.parametrize("d,border,zone,biou0,biou1,band,aacc", EXAMPLE)
def test_the_fixed_example(d, border, zone, biou0, biou1, band, aacc):
    from mmsa.evaluate import area_metrics, areas_of, boundary_iou_of, boundary_zone_sum_of, trimap_counts_of
    pred, label = _example()
    c = BR.boundary_counts(pred, label, ER.lut(2), 2, d, border)[0]
    assert c.shape == (4, 3, 3) and c.dtype == np.int64
    for z in range(4):
        assert c[z, :2, :2].ravel().tolist() == zone[z], (z, c[z])
    assert int(c[:, 2, :].sum()) == 0 and int(c[:, :, 2].sum()) == 0 and int(c.sum()) == 64
    biou = boundary_iou_of(c)
    assert biou.dtype == np.float64 and biou.shape == (2,)
    assert abs(biou[0] - biou0) <= 1e-15 and abs(biou[1] - biou1) <= 1e-15
    assert np.array_equal(biou, BR.boundary_iou(c))
    tri = trimap_counts_of(c)
    assert int(tri.sum()) == band and int(trimap_counts_of(c, interior=True).sum()) == 64 - band
    assert abs(area_metrics(*areas_of(tri))["aAcc"] - aacc) <= 1e-15
    assert np.array_equal(boundary_zone_sum_of(c), ER.confusion(pred[0], label[0], 2))
    assert np.array_equal(BR.near(BR.codes(pred[0], label[0], ER.lut(2), 2)[0], d, border), BR.near_loops(BR.codes(pred[0], label[0], ER.lut(2), 2)[0], d, border))


# ---- 2. the restatement on random maps

@pytest.mark.parametrize("H,W,C,d", [(1, 1, 5, 1), (5, 3, 5, 2), (23, 31, 5, 1), (23, 31, 5, 3), (37, 53, 25, 7), (19, 40, 25, 32)])
def test_the_restatement_on_random_maps(H, W, C, d):
    pred, label = ER.make_case(100 * H + W + d, H, W, C, B=2, special=True)
    lut = ER.lut(C)
    got = BR.boundary_counts(pred, label, lut, C, d)
    bord = BR.boundary_counts(pred, label, lut, C, d, border=True)
    mask = BR.border_mask(H, W, d)
    for b in range(2):
        # the zone sum is the confusion matrix, with and without the border rule
        want = ER.confusion(pred[b], label[b], C)
        assert np.array_equal(got[b].sum(0), want) and np.array_equal(bord[b].sum(0), want)
        L, P = BR.codes(pred[b], label[b], lut, C)
        assert set(np.unique(L)) <= set(range(C + 1)) | {255} and int(P.max()) <= C
        for code in (L, P):
            free = BR.near(code, d)
            # clamp-to-edge addressing is border=False
            assert np.array_equal(BR.near_clamped(code, d), free)
            # border=True differs exactly on the pixels within d of the border: all near there, unchanged elsewhere
            with_border = BR.near(code, d, border=True)
            assert bool(with_border[mask].all()) and np.array_equal(with_border[~mask], free[~mask])
            assert np.array_equal(with_border != free, mask & ~free)
        if H * W <= 23 * 31:
            assert np.array_equal(BR.near(L, d), BR.near_loops(L, d)) and np.array_equal(BR.near(P, d, True), BR.near_loops(P, d, True))
        # an ignored pixel is counted nowhere, but is a neighbour: the kept pixels next to it are in the label band
        z, L, P = BR.zones(pred[b], label[b], lut, C, d)
        assert int(got[b].sum()) == int((L != 255).sum())
        ign = L == 255
        if ign.any() and (~ign).any() and H > 2 and W > 2:
            ys, xs = np.nonzero(ign)
            for y, x in list(zip(ys, xs))[:20]:
                for qy, qx in ((y, x + 1), (y + 1, x), (y, x - 1), (y - 1, x)):
                    if 0 <= qy < H and 0 <= qx < W and not ign[qy, qx]:
                        assert z[qy, qx] >= 2
    # the label side through the tables, and slots
    Hl, Wl = max(1, H // 2), W + 3
    _, small = ER.make_case(7, Hl, Wl, C, B=2, special=True)
    ym, xm = ER.nearest_index(Hl, H), ER.nearest_index(Wl, W)
    tab = BR.boundary_counts(pred, small, lut, C, d, ymap=ym, xmap=xm, slots=[1, 1], n_slots=3)
    assert tab.shape == (3, 4, C + 1, C + 1) and int(tab[0].sum()) == 0 and int(tab[2].sum()) == 0
    resized = ER.resize_nearest(small, H, W)
    assert np.array_equal(tab[1], BR.boundary_counts(pred, resized, lut, C, d).sum(0))


# ---- 3. the metrics on hand-made counts

def test_the_of_functions_on_hand_made_counts():
    from mmsa.evaluate import boundary_iou_of, boundary_zone_sum_of, trimap_counts_of
    rng = np.random.default_rng(3)
    c = rng.integers(0, 50, size=(4, 4, 4)).astype(np.int64)      # C = 3
    c[:, 2, :] = 0
    c[:, :, 2] = 0                                                 # class 2 appears nowhere: 0 / 0
    biou = boundary_iou_of(c)
    assert biou.shape == (3,) and np.isnan(biou[2]) and not np.isnan(biou[:2]).any()
    assert np.array_equal(biou, BR.boundary_iou(c), equal_nan=True)
    for k in range(2):
        G, Pd, I = c[2, k].sum() + c[3, k].sum(), c[1, :, k].sum() + c[3, :, k].sum(), c[3, k, k]
        assert biou[k] == np.float64(I) / np.float64(G + Pd - I)
    assert np.array_equal(trimap_counts_of(c), c[2] + c[3]) and np.array_equal(trimap_counts_of(c, interior=True), c[0] + c[1])
    assert np.array_equal(boundary_zone_sum_of(c), c.sum(0))
    assert np.isnan(boundary_iou_of(np.zeros((4, 3, 3), dtype=np.int64))).all()
    # leading batch axes
    batch = np.stack([c, 2 * c, np.zeros_like(c)])
    assert np.array_equal(boundary_iou_of(batch)[0], biou, equal_nan=True) and np.array_equal(boundary_iou_of(batch)[1], biou, equal_nan=True)
    assert np.isnan(boundary_iou_of(batch)[2]).all() and boundary_iou_of(batch[None]).shape == (1, 3, 3)
    assert np.array_equal(trimap_counts_of(batch)[1], 2 * (c[2] + c[3])) and trimap_counts_of(batch).shape == (3, 4, 4)
    assert np.array_equal(boundary_zone_sum_of(batch[None])[0, 1], 2 * c.sum(0))
    for bad in (np.zeros((3, 3, 3), dtype=np.int64), np.zeros((4, 3, 4), dtype=np.int64), np.zeros((4, 3, 3)), np.zeros((3, 3), dtype=np.int64)):
        for fn in (boundary_iou_of, trimap_counts_of, boundary_zone_sum_of):
            with pytest.raises(ValueError, match="boundary counts are an integer \\[..., 4, C \\+ 1, C \\+ 1\\] array"):
                fn(bad)


def test_boundary_evaluator_on_hand_made_counts():
    import mmsa
    from mmsa.evaluate import (MAX_BOUNDARY_CLASSES, MAX_BOUNDARY_RADIUS, BoundaryEvaluator, Evaluator, LabelPrep, area_metrics, areas_of,
                               boundary_launch_shape, summary_of)
    assert MAX_BOUNDARY_RADIUS == 32 and MAX_BOUNDARY_CLASSES >= 64
    src = open(os.path.join(ROOT, "multimodal-sam-adapter_amd", "csrc", "boundary.hip")).read()
    assert int(re.search(r"#define BOUNDARY_MAX_RADIUS (\d+)", src).group(1)) == MAX_BOUNDARY_RADIUS
    assert int(re.search(r"#define BOUNDARY_MAX_CLASSES (\d+)", src).group(1)) == MAX_BOUNDARY_CLASSES
    pred, label = _example()
    c1 = BR.boundary_counts(pred, label, ER.lut(2), 2, 1)[0]
    c2 = BR.boundary_counts(pred, label, ER.lut(2), 2, 2)[0]
    be = BoundaryEvaluator(LabelPrep(2), 1, cases=["fog", "night"])
    assert be.radius == 1 and be.border is False and be._trailing() == (4, 3, 3) and be.counts is None
    assert be.host_counts().shape == (2, 4, 3, 3) and BoundaryEvaluator(LabelPrep(5), 3, border=True, images=4).host_counts().shape == (0, 4, 6, 6)
    host = np.stack([c1, c2])
    be.host_counts = lambda: host
    assert np.array_equal(be.evaluator_counts(), host.sum(1))
    assert be.boundary_iou(slot="fog").tolist() == [1 / 3, 1 / 3] and abs(be.boundary_iou(slot=1)[1] - 0.6) <= 1e-15
    assert np.array_equal(be.boundary_iou(), mmsa.boundary_iou_of(c1 + c2))
    assert be.trimap_metrics(slot="fog")["aAcc"] == 0.75 and list(be.trimap_metrics(slot="fog")) == ["aAcc", "IoU", "Acc"]
    assert be.interior_metrics(slot="fog")["aAcc"] == 1.0 and np.isnan(be.interior_metrics(slot="night")["aAcc"])
    assert list(be.trimap_metrics(metric="mDice")) == ["aAcc", "Dice", "Acc"]
    s = be.summary(slot="fog")
    assert list(s) == ["aAcc", "mIoU", "trimap_aAcc", "trimap_mIoU", "mBIoU", "band"]
    whole = summary_of(area_metrics(*areas_of(c1.sum(0))))
    assert s["aAcc"] == whole["aAcc"] == 0.875 and s["mIoU"] == whole["mIoU"] and s["trimap_aAcc"] == 0.75 and s["mBIoU"] == 0.3333 and s["band"] == 0.5
    assert s["trimap_mIoU"] == summary_of(area_metrics(*areas_of(c1[2] + c1[3])))["mIoU"]
    assert be.summary()["band"] == 0.75 and be.summary(slot="night")["band"] == 1.0
    for bad in (0, 33, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="mmsa.BoundaryEvaluator: radius = .*1..32 pixels"):
            BoundaryEvaluator(LabelPrep(5), bad)
    with pytest.raises(RuntimeError, match=f"mmsa.BoundaryEvaluator: {MAX_BOUNDARY_CLASSES + 1} classes; boundary evaluation supports 2..{MAX_BOUNDARY_CLASSES}"):
        BoundaryEvaluator(LabelPrep(MAX_BOUNDARY_CLASSES + 1), 3)
    assert isinstance(be, type(Evaluator(LabelPrep(2))).__mro__[1])        # a _SlotOwner
    with pytest.raises(KeyError):
        be.slots_for(1, case="rain")
    # the launch shape: limits, not measurements -- groups grow with C, the LDS stays inside 64 KiB, the tile does not pay the largest halo at a small radius
    for r in (1, 2, 3, 7, 16, 17, 32):
        last = 1
        for C in range(2, MAX_BOUNDARY_CLASSES + 1):
            groups, lds, th, tw = boundary_launch_shape(C, r)
            assert groups in (1, 2, 4) and groups >= last and lds <= 65536 and tw == 64 and th == (64 if r <= 16 else 32)
            assert lds == (4 // groups) * (C + 1) ** 2 * 4 + 2 * (th + 2 * r) * (33 + r // 2) * 4 + 256
            assert groups == 1 or (4 // (groups // 2)) * (C + 1) ** 2 * 4 + 2 * (th + 2 * r) * (33 + r // 2) * 4 + 256 > 65536
            last = groups
    assert boundary_launch_shape(25, 1)[1] < boundary_launch_shape(25, 8)[1] < boundary_launch_shape(25, 32)[1]
    assert boundary_launch_shape(MAX_BOUNDARY_CLASSES, 32)[0] == 4
    assert 83 * 83 * 4 + 37632 + 256 <= 65536 < 84 * 84 * 4 + 37632 + 256      # MAX_BOUNDARY_CLASSES, as csrc/boundary.hip derives it


# ---- 4. refusals, all before any launch

def test_python_refusals_of_boundary():
    import mmsa
    import mmsa.inference as inf
    from mmsa.evaluate import BoundaryEvaluator, Evaluator, LabelPrep
    x = torch.zeros(1, 6, 8, 8)
    lab = torch.zeros(1, 8, 8, dtype=torch.uint8)
    plan = inf.MapPlan.whole(1, 8, 8)
    out = torch.zeros(1, 8, 8, dtype=torch.uint8)
    lp = LabelPrep(5)
    be = BoundaryEvaluator(lp, 2)

    def entries(**kw):
        """Every entry with `kw`, under its name: (name, call)."""
        return [("whole_class_map", lambda: inf.whole_class_map(None, None, x, **kw)),
                ("slide_class_map", lambda: inf.slide_class_map(None, None, x, (4, 4), (4, 4), **kw)),
                ("class_map", lambda: inf.class_map(None, None, x, dict(mode="whole"), **kw)),
                ("aug_class_map", lambda: inf.aug_class_map(None, None, [x], dict(mode="whole"), **kw)),
                ("inference", lambda: plan.class_map(None, out, None, **kw))]

    for name, call in entries(boundary=be):
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: boundary= needs labels="):
            call()
    for other in (Evaluator(lp), 3, "be", lp):
        for name, call in entries(boundary=other, labels=lab):
            with pytest.raises(RuntimeError, match=f"mmsa.{name}: boundary= takes an mmsa.evaluate.BoundaryEvaluator, got {type(other).__name__}"):
                call()
    for name, call in entries(boundary=be, labels=lab, evaluator=Evaluator(lp), return_map=False):
        if name in ("class_map", "aug_class_map"):      # these take no return_map=
            with pytest.raises(TypeError):
                call()
            continue
        with pytest.raises(RuntimeError, match=f"mmsa.{name}: boundary= with return_map=False: .*stores none"):
            call()
    # a SlideRunner's run(): the same refusals under its name, from the options record the runner keeps
    o = inf.MapOptions.of("SlideRunner")
    for kw, why in ((dict(boundary=be), "boundary= needs labels="), (dict(boundary=Evaluator(lp), labels=lab), "boundary= takes an mmsa.evaluate.BoundaryEvaluator, got Evaluator"),
                    (dict(boundary=be, labels=lab, evaluator=Evaluator(lp), return_map=False), "boundary= with return_map=False")):
        with pytest.raises(RuntimeError, match="mmsa.SlideRunner.run: " + why):
            o.with_call("SlideRunner.run", **kw)
    # labels= + boundary= without evaluator= is a complete call: the options go through both steps
    ok = inf.MapOptions.of("whole_class_map", labels=lab, boundary=be).at((1, 8, 8), None, "whole_class_map")
    assert ok.boundary is be and ok.evaluator is None and ok.labels is lab
    # None is the default everywhere, appended last
    for fn in (inf.slide_class_map, inf.whole_class_map, inf.class_map, inf.aug_class_map, inf.MapPlan.class_map, inf.SlideRunner.run, inf.MapOptions.with_call):
        params = inspect.signature(fn).parameters
        assert params["boundary"].default is None and list(params)[-1] == "boundary", fn
    assert mmsa.aug_class_map is inf.aug_class_map
    assert inf.MapOptions().boundary is None and [f.name for f in inf.dataclasses.fields(inf.MapOptions)][-1] == "boundary"
    for name in ("BoundaryEvaluator", "boundary_counts", "boundary_zone_sum_of", "trimap_counts_of", "boundary_iou_of"):
        assert name in mmsa.__all__ and hasattr(mmsa, name)
    # the launch alone: no CPU path, and the radius is checked
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        mmsa.boundary_counts(out, lab, lp, 2)
    with pytest.raises(RuntimeError, match="pred must be a GPU tensor"):
        be.add(out, lab)
    assert list(inspect.signature(mmsa.boundary_counts).parameters) == ["pred", "labels", "prep", "radius", "border", "counts", "slots"]
    assert inspect.signature(mmsa.boundary_counts).parameters["border"].default is False
    assert list(inspect.signature(BoundaryEvaluator.__init__).parameters) == ["self", "prep", "radius", "border", "cases", "images", "device"]


# ---- 5. the C entry on the host

def test_the_entry_refuses_bad_arguments_on_the_host():
    """Before any launch, so no GPU is needed: every pointer is a fake but the slot table, which the entry reads on the host."""
    import mmsa
    from mmsa.evaluate import MAX_BOUNDARY_CLASSES
    fake = ctypes.c_void_p(256)
    slots = (ctypes.c_int * 1)(0)

    def call(radius=2, border=0, C=5, pred=fake, label=fake, lut=fake, buf=fake, tab=slots, ymap=None, xmap=None, Hl=4):
        rc = mmsa.lib.raw.mmsa_eval_boundary_u8(pred, label, 1, 4, 4, Hl, 4, lut, C, ymap, xmap, tab, 1, radius, border, buf, None)
        return (rc, mmsa.lib.last_error()) if rc else (0, "")

    ERR_ARG = -1     # MMSA_ERR_ARG (csrc/common.h)
    for radius in (0, 33, -1, 1000):
        rc, msg = call(radius=radius)
        assert rc == ERR_ARG and f"eval_boundary_u8: radius = {radius}; 1..32 are supported" in msg, msg
    for border in (2, -1):
        rc, msg = call(border=border)
        assert rc == ERR_ARG and f"eval_boundary_u8: border = {border}; 0 " in msg and "or 1" in msg, msg
    for C in (1, 0, MAX_BOUNDARY_CLASSES + 1, 126):
        rc, msg = call(C=C)
        assert rc == ERR_ARG and f"eval_boundary_u8: {C} classes; 2..{MAX_BOUNDARY_CLASSES} are supported" in msg and "LDS" in msg, msg
    rc, msg = call(pred=None)
    assert rc == ERR_ARG and "eval_boundary_u8: pred is required" in msg
    for kw in (dict(label=None), dict(lut=None), dict(buf=None), dict(tab=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "eval_boundary_u8: label, lut, slots and counts are required" in msg, msg
    rc, msg = call(ymap=fake)
    assert rc == ERR_ARG and "eval_boundary_u8: ymap and xmap come together" in msg
    rc, msg = call(Hl=5)
    assert rc == ERR_ARG and "eval_boundary_u8: size mismatch" in msg
    rc, msg = call(tab=(ctypes.c_int * 1)(3))
    assert rc == ERR_ARG and "eval_boundary_u8: slots[0] = 3 outside the 1 count slots" in msg


def test_the_entry_is_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(ROOT, "include", "mmsa.h")).read()
    ver = open(os.path.join(ROOT, "include", "mmsa_version.h")).read()
    header = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", ver).group(1))
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == header == 114
    assert re.search(r"\b" + ENTRY + r"\s*\(", hdr), f"{ENTRY} is not declared in include/mmsa.h"
    assert ENTRY in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, ENTRY) and ENTRY in ver
    assert len(mmsa.lib.SIGNATURES[ENTRY]) == len(mmsa.lib.SIGNATURES["mmsa_eval_confusion_u8"]) + 2      # radius, border
