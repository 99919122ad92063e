"""Temperature scaling on the device.  APPLY: the `_t` siblings of the confidence kernels (csrc/segment.hip, csrc/augment.hip) at it = 1.0f against their
siblings bit for bit, every path at one temperature against every other bit for bit, and against the float64 softmax of x * it.  FIT: the sweep kernel
(csrc/temperature.hip) against mmsa.calibration of the canvas path's map and tempered confidence, temperature by temperature and bit for bit, its NLL
against float64, a planted temperature found, determinism and accumulation; and the public entries on the tiny model.  The kernels are driven from synthetic
head-resolution logits through MapPlan, as tests/test_confidence_gpu.py does."""
import numpy as np
import pytest
import torch

from tests import confidence_ref as CR
from tests import eval_ref as ER
from tests import temperature_ref as TR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP, DOWN = (61, 101), (29, 53)
TEMPS = (0.5, 2.5, 3.0)


def _plan(tgt=None, stride=(24, 24), B=2):
    """B = 2 frames of 45 x 77 under 32 x 32 windows: stride 24 gives 2 x 3 windows per frame with up to 4 over a pixel (the slot form of the rescaled kernel);
    stride (12, 24) gives 3 x 3 with up to 6 (its scanning form)."""
    import mmsa.inference as inf
    return inf.MapPlan.slide(B, 45, 77, (32, 32), stride, tgt)


def _run(plan, lg, **kw):
    """plan.class_map with a confidence buffer -> (map, conf); both buffers are pre-filled with values no launch writes."""
    out = torch.full((plan.B, plan.Ho, plan.Wo), 77, dtype=torch.uint8, device=DEV)
    conf = torch.full((plan.B, plan.Ho, plan.Wo), -1.0, device=DEV)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lg, out, unc, conf=conf, **kw)
    assert int(unc.item()) == 0
    return out, conf


def _canvas(plan, lg):
    """The plan's logits canvas at its output size, the long way round: what mmsa.inference.inference returns."""
    import mmsa.inference as inf
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = inf._canvas_logits(plan, lg, unc)[:, :, :plan.Ho, :plan.Wo].contiguous()
    assert int(unc.item()) == 0
    return y


def _canvas_conf(y, T=None):
    """What `probabilities(..., temperature=T).max(1)` launches on a canvas -> (argmax_map of the LOGITS, the maximum over the classes of the softmax)."""
    import mmsa.inference as inf
    from mmsa.evaluate import inv_temperature
    p = torch.full_like(y, float("nan"))
    inf._softmax_accum(y, p, it=None if T is None else inv_temperature(T))
    return inf.argmax_map(y), p.max(1).values


# ---- 1. it = 1.0f is the sibling, bit for bit

@pytest.mark.parametrize("C", [25, 64, 65])
def test_unit_temperature_is_the_sibling_bit_for_bit(C):
    """25: the per-lane LDS column; 64 and 65: the two sides of its limit (65 takes the second pass).  Rescaled up and down, slot and scanning form, the
    canvas path, and the canvas softmax with every argument in play."""
    import mmsa.inference as inf
    for tgt, stride in ((None, (24, 24)), (UP, (24, 24)), (DOWN, (24, 24)), (UP, (12, 24))):
        plan = _plan(tgt, stride)
        lg = CR.planted_logits(plan.n, C, 3000 + C).to(DEV)
        for kw in ((dict(),) if tgt is None else (dict(one_pass=True), dict(one_pass=False))):
            m0, c0 = _run(plan, lg, **kw)
            m1, c1 = _run(plan, lg, temperature=1.0, **kw)
            assert torch.equal(m0, m1) and torch.equal(c0, c1), f"C={C} target {tgt} stride {stride} {kw}"
            assert bool((c0 > 0).all()) and bool((c0 <= 1).all())
    y = _canvas(_plan(UP), CR.planted_logits(12, C, 3100 + C).to(DEV))
    for flip, acc, div in ((0, False, 0), (1, False, 0), (2, True, 0), (1, True, 3)):
        a, b = torch.full_like(y, 0.25), torch.full_like(y, 0.25)
        inf._softmax_accum(y, a, flip, acc, div)
        inf._softmax_accum(y, b, flip, acc, div, it=1.0)
        assert torch.equal(a, b), f"canvas softmax C={C} flip {flip} accumulate {acc} finish_div {div}"


# ---- 2. one temperature, every path the same bits

def _toy(C):
    """A backbone / head pair without weights to load: 4 x 4 average pooling and a seeded 1 x 1 conv to C classes."""
    import torch.nn.functional as F
    w = torch.randn(C, 6, 1, 1, generator=torch.Generator().manual_seed(5)).to(DEV) * 4
    return (lambda im: ([F.avg_pool2d(im, 4)], None)), (lambda feats: F.conv2d(feats[0], w).contiguous())


@pytest.mark.parametrize("T", TEMPS)
def test_every_path_gives_the_same_bits_at_one_temperature(T):
    import mmsa.inference as inf
    for C in (25, 65):
        for tgt, stride in ((None, (24, 24)), (UP, (24, 24)), (DOWN, (24, 24)), (DOWN, (12, 24))):
            plan = _plan(tgt, stride)
            lg = CR.planted_logits(plan.n, C, 3200 + C).to(DEV)
            y = _canvas(plan, lg)
            want_map, want = _canvas_conf(y, T)
            plain_map, plain = _canvas_conf(y)
            assert torch.equal(want_map, plain_map) and not torch.equal(want, plain)
            for kw in ((dict(),) if tgt is None else (dict(one_pass=True), dict(one_pass=False))):
                got_map, got = _run(plan, lg, temperature=T, **kw)
                untempered_map, untempered = _run(plan, lg, **kw)
                diff = int((got != want).sum().item())
                print(f"T={T} C={C} target {tgt} stride {stride} {kw}: {diff} of {got.numel()} confidences differ from the canvas path")
                assert torch.equal(got, want), f"T={T} C={C} target {tgt} stride {stride} {kw}"
                assert torch.equal(got_map, want_map) and torch.equal(got_map, untempered_map) and torch.equal(untempered, plain)
    # the same through `probabilities` and the slide entry, on a toy model
    bb, hd = _toy(7)
    img = torch.randn(2, 6, 45, 77, generator=torch.Generator().manual_seed(6)).to(DEV)
    tc = dict(mode="slide", crop_size=(32, 32), stride=(24, 24))
    for ori in (None, UP, DOWN):
        want = inf.probabilities(bb, hd, img, tc, ori_shape=ori, temperature=T).max(1).values
        plain_map = inf.slide_class_map(bb, hd, img, (32, 32), (24, 24), ori_shape=ori)[0]
        for kw in ((dict(),) if ori is None else (dict(one_pass=True), dict(one_pass=False))):
            cm, unc, conf = inf.slide_class_map(bb, hd, img, (32, 32), (24, 24), ori_shape=ori, confidence=True, temperature=T, **kw)
            assert int(unc.item()) == 0 and torch.equal(conf, want) and torch.equal(cm, plain_map), f"T={T} ori_shape={ori} {kw}"


# ---- 3. the tempered confidence against float64

@pytest.mark.parametrize("T", (0.25,) + TEMPS)
def test_tempered_confidence_against_float64(T):
    """Relative error per pixel at most (4 D_T + C + 4) 2^-23, D_T = max_c |x_c - m| * it, with a pixel of spread D >= 30 planted."""
    from mmsa.evaluate import inv_temperature
    it = inv_temperature(T)
    for C in (25, 65):
        for tgt in (None, UP):
            plan = _plan(tgt)
            lg = CR.planted_logits(plan.n, C, 3300 + C).to(DEV)
            y = _canvas(plan, lg)
            _, conf = _run(plan, lg, temperature=T)
            worst, DT = TR.confidence_check(conf, y, it)
            print(f"T={T} C={C} target {tgt}: D_T up to {DT:.1f}, worst error / bound {worst:.3f}; conf in [{conf.min().item():.3e}, {conf.max().item():.3e}]")
            assert worst <= 1.0, f"T={T} C={C} target {tgt}: {worst} of the bound"
            assert (tgt is not None or DT >= 30 * it * (1 - 2.0 ** -20)) and bool((conf >= 1.0 / C - 1e-6).all()) and bool((conf <= 1).all())


# ---- 4. the sweep is Calibration, temperature by temperature

SWEEP_CASES = [      # C, bins, J, canvas, labels through the nearest tables, two images on one slot
    (2, 1, 1, (37, 83), False, False),
    (25, 15, 16, (37, 83), True, True),
    (130, 64, 16, (5, 259), False, False),
    (25, 64, 1, (5, 259), True, True),
    (130, 15, 1, (37, 83), False, True),
    (2, 64, 16, (5, 259), True, False),
    (25, 1, 16, (37, 83), False, False),
    (25, 15, 3, (5, 259), True, False),      # J = 3 and 7: the kernel's compile-time bounds of 4 and 8 temperatures (1 and 16 are above)
    (25, 15, 7, (37, 83), False, True),
]


def _sweep_inputs(C, hw, tables, seed):
    """-> (canvas logits [2, C, H, W] on the device, raw labels on the device and on the host AT THE CANVAS SIZE, the LabelPrep)."""
    import mmsa.inference as inf
    from mmsa.evaluate import LabelPrep
    H, W = hw
    y = _canvas(inf.MapPlan.whole(2, H, W), CR.planted_logits(2, C, seed).to(DEV))
    if tables:
        Hl, Wl = H + 13, W + 37
        prep = LabelPrep(C, resize=dict(seg_scale=(W, H), keep_ratio=False))
    else:
        Hl, Wl = H, W
        prep = LabelPrep(C)
    lab = TR.labels_for(2, Hl, Wl, C, seed + 1)
    at_canvas = ER.resize_nearest(lab.numpy(), H, W) if tables else lab.numpy()
    return y, lab.to(DEV), at_canvas, prep


@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: "C%d-K%d-J%d-%dx%d-%s-%s" % (c[0], c[1], c[2], c[3][0], c[3][1], "tables" if c[4] else "same", "oneslot" if c[5] else "perimage"))
def test_sweep_equals_calibration_at_every_temperature(case):
    import mmsa
    from mmsa.evaluate import geometric_grid
    C, K, J, hw, tables, one_slot = case
    y, lab, lab_host, prep = _sweep_inputs(C, hw, tables, 3400 + C + K)
    temps = geometric_grid(0.25, 8, J) if J > 1 else np.array([2.5])
    slots = [0, 0] if one_slot else None
    got = mmsa.temperature_sweep(y, lab, prep, temps, bins=K, slots=slots)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1 if one_slot else 2, J, 4, K)
    taking_part = prep.lut[lab_host] < C
    per_slot = np.array([taking_part.sum()]) if one_slot else taking_part.reshape(2, -1).sum(1)
    assert (prep.lut[lab_host] == 255).any() and (C >= 254 or ((prep.lut[lab_host] == C)).any()) and taking_part.any()
    for j, T in enumerate(temps):
        pred, conf = _canvas_conf(y, float(T))
        want = mmsa.calibration(pred, conf, lab, prep, bins=K, slots=slots)
        assert torch.equal(got[:, j, :3], want), f"temperature {j} (T = {T})"
        assert np.array_equal(got[:, j, 0].sum(1).cpu().numpy(), per_slot)
    assert bool((got[:, :, 3] >= 0).all()) and bool((got[:, :, 3].sum(2) > 0).all())
    if K > 1 and J > 1:
        assert len({tuple(r) for r in got[0, :, 0].cpu().numpy().tolist()}) > 1      # the temperatures do move pixels between bins


# ---- 5. the NLL against float64

@pytest.mark.parametrize("C", [5, 25])
def test_nll_against_float64(C):
    """|sum n / 2^20 - sum nll64| <= sum over the pixels of (4 D_T + C + 4 + nll64) 2^-23 + 2^-20, on a grid from 0.25 to 8; the cap of
    1024 is not reached."""
    import mmsa
    from mmsa.evaluate import geometric_grid, inv_temperature
    y, lab, lab_host, prep = _sweep_inputs(C, (37, 83), False, 3500 + C)
    temps = geometric_grid(0.25, 8, 16)
    got = mmsa.temperature_sweep(y, lab, prep, temps, bins=15, slots=[0, 0]).cpu().numpy()[0]
    cls = torch.from_numpy(prep.lut[lab_host].astype(np.int64))
    part = cls < C
    for j, T in enumerate(temps):
        want, bound, largest = TR.nll_sum_bound(y, inv_temperature(T), cls, part)
        have = float(sum(int(v) for v in got[j, 3])) / TR.NLL_ONE
        print(f"C={C} T={T:.3f}: sum nll {have:.6f}, float64 {want:.6f}, |difference| {abs(have - want):.3e}, bound {bound:.3e}, largest nll {largest:.1f}")
        assert largest < 1000, "the cap must stay out of reach here"
        assert abs(have - want) <= bound, f"C={C} T={T}: {abs(have - want)} against {bound}"
    mean = mmsa.evaluate.sweep_nll_of(got)
    assert mean.shape == (16,) and np.isfinite(mean).all()


# ---- 6. it finds a planted temperature

def test_the_fit_finds_a_planted_temperature():
    import mmsa
    x, lab, grid = TR.planted_temperature_case()
    sw = mmsa.TemperatureSweep(mmsa.LabelPrep(5), grid, bins=15).add(x.to(DEV), lab.to(DEV))
    nll, ece = sw.nll(), sw.ece()
    want_nll, want_ece = TR.planted_float64(x, lab, grid)
    print("mean NLL", np.round(nll, 4), "float64", np.round(want_nll, 4))
    print("ECE     ", np.round(ece, 4), "float64", np.round(want_ece, 4))
    assert sw.best("nll") == (2.5, 3) and sw.best("ece") == (2.5, 3) and sw.best() == (2.5, 3)
    assert ece[3] < ece[1] / 2
    assert np.abs(nll - want_nll).max() < 1e-4 and sw.summary()["best_nll"] == 2.5
    assert np.array_equal(sw.bins(3), sw.host().sum(0)[3, :3]) and mmsa.evaluate.ece_of(sw.bins(3)) == ece[3]


# ---- 7. determinism and accumulation

def test_determinism_accumulation_and_cases():
    import mmsa
    from mmsa.dist import allreduce_counts
    from mmsa.evaluate import geometric_grid
    y, lab, _, prep = _sweep_inputs(25, (37, 83), True, 3700)
    temps = geometric_grid(0.5, 4, 8)
    a = mmsa.temperature_sweep(y, lab, prep, temps)
    b = mmsa.temperature_sweep(y, lab, prep, temps, bins=15)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (2, 8, 4, 15) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()      # integer sums: the same bytes run after run
    assert mmsa.temperature_sweep(y, lab, prep, temps, out=b) is b and torch.equal(b, 2 * a)                # the call ADDS; bins= defaults to the buffer's
    routed = mmsa.temperature_sweep(y, lab, prep, temps, slots=[1, 1])
    assert tuple(routed.shape) == (2, 8, 4, 15) and not bool(routed[0].any()) and torch.equal(routed[1], a.sum(0))
    sw = mmsa.TemperatureSweep(prep, temps, cases=["fog", "night"], device=DEV)
    assert sw.counts is not None and not sw.host().any()
    sw.add(y, lab, case="night").add(y[:1], lab[:1], case="fog").add(y[1:], lab[1:], case="night")
    assert np.array_equal(sw.host(), torch.stack([a[0], a.sum(0) + a[1]]).cpu().numpy())
    assert np.array_equal(sw.bins(2, slot="fog"), a[0, 2, :3].cpu().numpy()) and np.array_equal(sw.nll(slot=1), sw.nll(slot="night"))
    assert allreduce_counts(sw.counts) is sw.counts
    per = mmsa.TemperatureSweep(prep, temps, images=3).add(y, lab)
    assert per.used == 2 and np.array_equal(per.host(), a.cpu().numpy())
    with pytest.raises(RuntimeError, match="per-image slots"):
        per.add(y, lab)
    with pytest.raises(RuntimeError, match="classes, the LabelPrep"):
        per.add(y[:1, :5].contiguous(), lab[:1])
    assert per.used == 2
    per.reset()
    assert per.used == 0 and not per.host().any()


# ---- 8. through the public entries, on the tiny model

@pytest.fixture(scope="module")
def models():
    import mmsa
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(seeded_state_dict(h, seed=hcfg["seed"]))
    h = h.to(DEV)
    g = torch.Generator().manual_seed(9)
    frame = torch.randn(1, 6, 320, 400, generator=g)
    frame[:, 3:] = (torch.rand(1, 3, 320, 400, generator=g) < 0.05).float() * torch.rand(1, 3, 320, 400, generator=g)
    return m, h, frame.to(DEV), make_input(cfg, batch=2, seed=17).to(DEV)


SLIDE_CFG = dict(mode="slide", crop_size=(256, 256), stride=(170, 170))
NUM_CLASSES = HEAD_CONFIGS["head_tiny"]["kwargs"]["num_classes"]


def test_public_entries_with_and_without_a_temperature(models):
    import mmsa.inference as inf
    m, h, frame, x = models
    T = 2.5
    dim_cfg = dict(mode="whole_dim", dim=(300, 280))
    calls = [("slide", SLIDE_CFG, frame, dict(max_batch=2), lambda **kw: inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, **kw)),
             ("slide rescaled", SLIDE_CFG, frame, dict(max_batch=2, ori_shape=(300, 380, 3)),
              lambda **kw: inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=(300, 380, 3), **kw)),
             ("whole", dict(mode="whole"), x, {}, lambda **kw: inf.whole_class_map(m, h, x, **kw)),
             ("class_map whole_dim", dim_cfg, x, {}, lambda **kw: inf.class_map(m, h, x, dim_cfg, **kw))]
    for name, tc, img, pkw, call in calls:
        want_T = inf.probabilities(m, h, img, tc, temperature=T, **pkw).max(1).values
        want_1 = inf.probabilities(m, h, img, tc, **pkw).max(1).values
        plain = call()
        plain_map = plain if isinstance(plain, torch.Tensor) else plain[0]
        r0, rN, rT = call(confidence=True), call(confidence=True, temperature=None), call(confidence=True, temperature=T)
        assert torch.equal(r0[-1], want_1) and torch.equal(rN[-1], want_1), f"{name}: temperature=None must give today's bytes"
        assert torch.equal(rT[-1], want_T) and not torch.equal(want_T, want_1), name
        assert torch.equal(r0[0], plain_map) and torch.equal(rN[0], plain_map) and torch.equal(rT[0], plain_map), f"{name}: the map does not depend on T"
        if "rescaled" in name or "whole_dim" in name:
            assert torch.equal(call(confidence=True, temperature=T, one_pass=False)[-1], want_T), f"{name}: the canvas path"
    with pytest.raises(RuntimeError, match="temperature= without confidence="):
        inf.whole_class_map(m, h, x, temperature=T)


def test_runner_and_binned_passes_see_the_tempered_confidence(models):
    import mmsa
    import mmsa.inference as inf
    m, h, frame, x = models
    T = 2.5
    cm, _, want = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, confidence=True, temperature=T)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, confidence=True, temperature=T)
    res = sr.run()
    conf = res.confidence()
    torch.cuda.synchronize()
    assert conf is sr.conf and torch.equal(conf, want) and torch.equal(res.outputs()[0], cm)
    with pytest.raises(RuntimeError, match="SlideRunner: temperature= without confidence="):
        inf.SlideRunner(m, h, frame, (256, 256), (170, 170), temperature=T)
    # calibration= / selective= next to temperature=: the bins of the tempered confidence
    lp = mmsa.LabelPrep(NUM_CLASSES)
    lab = torch.randint(0, NUM_CLASSES, (2, 256, 256), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    cal, sel = mmsa.Calibration(lp, images=2, device=DEV), mmsa.SelectiveEvaluator(lp, images=2, device=DEV)
    wm, wc = inf.whole_class_map(m, h, x, labels=lab, confidence=True, temperature=T, calibration=cal, selective=sel)
    _, untempered = inf.whole_class_map(m, h, x, confidence=True)
    assert torch.equal(cal.bins, mmsa.calibration(wm, wc, lab, lp)) and torch.equal(sel.counts, mmsa.selective(wm, wc, lab, lp))
    assert not torch.equal(cal.bins, mmsa.calibration(wm, untempered, lab, lp))
    # and the sweep of the logits canvas at that temperature gives the same bins: fit and apply agree through the entries too
    y = inf.inference(m, h, x, dict(mode="whole")).contiguous()
    sw = mmsa.temperature_sweep(y, lab, lp, [T])
    assert torch.equal(sw[:, 0, :3], cal.bins)
