"""Keeps tests/class_map_ref.py honest without a GPU: the float64 reference is pinned against F.interpolate in double, the oracle's slide_inference and
tests/rescale_ref.py / tests/aug_ref.py in double; the float32 emulation of the kernels' formula lies within the bound for every case and output; every
mutation of the emulation is caught by a case designed for it; the case table's windows are ones the one-pass kernels take."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_segmentor as RS
from tests import aug_ref as AR
from tests import class_map_ref as M
from tests import rescale_ref as RR


def _toy(lg64, geo):
    """A toy encode_decode: call k returns the k-th window's logits (all B images) resized to the crop it was given, in double."""
    B, calls = geo["B"], iter(range(len(geo["wins"])))

    def fn(crop):
        k = next(calls)
        return F.interpolate(lg64[k * B:(k + 1) * B], size=crop.shape[2:], mode="bilinear", align_corners=False)
    return fn


def _inputs(gk, C):
    geo = M.GEOS[gk]
    lg = M.logits_of(f"{gk}-c{C}", geo, C)
    return geo, lg, lg.double().numpy()


@pytest.mark.parametrize("gk,C", M.CASES, ids=M.CASE_IDS)
def test_reference_is_pytorch_bilinear_and_the_oracle_slide(gk, C):
    geo, lg, lg64 = _inputs(gk, C)
    img = torch.zeros(geo["B"], 1, geo["H"], geo["W"], dtype=torch.float64)
    crop = (geo["hc"], geo["wc"])
    v, _, cnt = M.canvas(lg64, geo)
    if len(geo["wins"]) == 1:
        want = F.interpolate(lg.double(), size=crop, mode="bilinear", align_corners=False).numpy()
        assert np.abs(v - want).max() <= 1e-12 and int(cnt.max()) == 1
    want = RS.slide_inference(_toy(lg.double(), geo), img, crop, geo["stride"], C).numpy()
    assert np.abs(v - want).max() <= 1e-12, "the canvas is not the oracle's slide_inference (window order, overlap, count)"
    for tgt in geo["targets"][1:]:
        want = RR.rescaled_logits(_toy(lg.double(), geo), img, tgt[:2], crop, geo["stride"], num_classes=C)[:, :, :tgt[2], :tgt[3]].numpy()
        got = M.frame(lg64, geo, tgt)[0]
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, f"target {tgt}"
    if gk == M.IDENT:
        assert np.array_equal(v, lg64) and np.array_equal(M.emu_frame(lg.numpy(), geo), lg.numpy()), "ratio 1 must reproduce the logits bit for bit"


@pytest.mark.parametrize("ak", sorted(M.AUGS))
def test_aug_reference_is_aug_ref_in_double(ak):
    C, ac = RR.NUM_CLASSES, M.AUGS[ak]
    lgs = M.aug_logits(ak, C)
    Hd, Wd, Ho, Wo = ac["target"]
    acc = None
    for lg, (gk, code) in zip(lgs, ac["views"]):
        geo = M.GEOS_AUG[gk]
        img = torch.zeros(geo["B"], 1, geo["H"], geo["W"], dtype=torch.float64)
        crop = (geo["hc"], geo["wc"])
        if (Ho, Wo) == (Hd, Wd):
            p = AR.probabilities(_toy(lg.double(), geo), img, (Hd, Wd), AR.FLIP_NAMES[code], crop, geo["stride"])
        else:       # the cut comes before the softmax and the flip (whole_dim_cut), which aug_ref does not state: stated here
            y = RR.rescaled_logits(_toy(lg.double(), geo), img, (Hd, Wd), crop, geo["stride"])[:, :, :Ho, :Wo]
            p = F.softmax(y, dim=1)
            p = p.flip(3) if code == 1 else p.flip(2) if code == 2 else p
        acc = p if acc is None else acc + p
    want = (acc / len(lgs)).numpy()
    got = M.aug([lg.double().numpy() for lg in lgs], ac)[0]
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def _verdict(gk, C, mut=()):
    """Run the emulation (with `mut`) through every check the GPU test applies to the device -> (None or what failed first, worst ratios, excused)."""
    geo, lg, lg64 = _inputs(gk, C)
    worst, excused = {}, 0
    try:
        for tgt in geo["targets"]:
            r, b = M.frame(lg64, geo, tgt)
            y = M.emu_frame(lg.numpy(), geo, tgt, mut)
            what = f"{gk}-c{C} -> {tgt}"
            worst["values"] = max(worst.get("values", 0.0), M.check_values(y, r, b, f"{what}: logits"))
            excused = max(excused, M.check_map(M.first_argmax(y), r, b, f"{what}: map"))
            cr, cb = M.confidence(r, b)
            worst["conf"] = max(worst.get("conf", 0.0), M.check_values(M.emu_confidence(y), cr, cb, f"{what}: confidence"))
    except AssertionError as e:
        return str(e), worst, excused
    return None, worst, excused


def _aug_verdict(ak, C, mut=()):
    ac = M.AUGS[ak]
    lgs = M.aug_logits(ak, C)
    r, b = M.aug([lg.double().numpy() for lg in lgs], ac)
    y = M.emu_aug([lg.numpy() for lg in lgs], ac, mut)
    worst, excused = {}, 0
    try:
        worst["prob"] = M.check_values(y, r, b, f"{ak}-c{C}: mean probabilities")
        excused = M.check_map(M.first_argmax(y), r, b, f"{ak}-c{C}: map")
        worst["conf"] = M.check_values(y.max(1), r.max(1), b.max(1), f"{ak}-c{C}: confidence")
    except AssertionError as e:
        return str(e), worst, excused
    return None, worst, excused


@pytest.mark.parametrize("gk,C", M.CASES, ids=M.CASE_IDS)
def test_emulation_lies_within_the_bound(gk, C):
    fail, worst, excused = _verdict(gk, C)
    print(f"{gk}-c{C}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; excused pixels {excused}")
    assert fail is None, fail


@pytest.mark.parametrize("ak,C", M.AUG_CASES, ids=M.AUG_IDS)
def test_aug_emulation_lies_within_the_bound(ak, C):
    fail, worst, excused = _aug_verdict(ak, C)
    print(f"{ak}-c{C}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; excused pixels {excused}")
    assert fail is None, fail


# mutation -> the cases designed for it (EVERY one of them must catch it)
AUG3 = "aug3-26x37-cut23x31-b2"
DESIGNED = dict(
    swap_l=[(M.NONSQ, 5), (M.WIDE, 5)],              # lh in lw's place: ratios differ per axis
    rh_from_w=[(M.NONSQ, 5), (M.DOWN, 5)],           # 7/20 in place of 5/12; 11/5 in place of 13/6
    no_clamp0=[(M.NONSQ, 5), (M.THIRD, 5)],          # the first rows and columns of any upscale extrapolate
    row_step_hs=[(M.NONSQ, 5), (M.DOWN, 5)],         # hs != ws: the row below is hs, not ws, elements away
    h0_clamp_ws=[(M.DOWN, 5), (M.THIN_W, 5)],        # ws < hs: rows beyond ws - 1 are never reached
    first_adds=[(M.NONSQ, 5), (M.IDENT, 5)],         # a first window added to what the canvas held
    wrong_count=[(M.NONSQ, 5), (M.OV8, 5)],          # second stage across a change of overlap
    hflip_Ho=[(AUG3, 5)])                            # Ho = 23 != Wo = 31


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_every_mutation_is_caught(mut):
    for key, C in DESIGNED[mut]:
        fail, _, _ = (_aug_verdict if key in M.AUGS else _verdict)(key, C, (mut,))
        print(f"mutation {mut}: case {key}-c{C}: {'CAUGHT -- ' + fail if fail else 'not caught'}")
        assert fail is not None, f"mutation {mut} passes every check of case {key}-c{C}, which was designed for it"


def test_the_table_names_every_mutation_and_its_windows_are_supported():
    from mmsa.inference import MapPlan
    assert set(DESIGNED) == set(M.MUTATIONS)
    deepest = {}
    for gk, geo in M.GEOS_AUG.items():
        plan = MapPlan.slide(geo["B"], geo["H"], geo["W"], (geo["hc"], geo["wc"]), geo["stride"])
        assert list(plan.jobs) == M.jobs_of(geo), f"{gk}: the table's windows are not MapPlan.slide's for stride {geo['stride']}"
        plan.check_windows(gk)
        cnt = M.canvas(np.zeros((plan.n, 1, geo["hs"], geo["ws"])), geo)[2]
        deepest[gk] = int(cnt.max())
        assert cnt.min() >= 1 and cnt.max() <= 8 and plan.n <= 64
        for tgt in geo["targets"][1:]:
            assert max(tgt) <= 300 and tgt[2] <= tgt[0] and tgt[3] <= tgt[1]
            assert all(a % b and b % a for a, b in ((tgt[0], geo["H"]), (tgt[1], geo["W"]))), f"{gk}: target {tgt} has an integer ratio"
    assert deepest[M.NONSQ] == 4 and deepest[M.OV8] == 8 and deepest[M.WIDE] == 2 and deepest[M.DOWN] == 2
    for ak, ac in M.AUGS.items():
        assert len({M.GEOS_AUG[gk]["B"] for gk, _ in ac["views"]}) == 1, f"{ak}: the views share B"
