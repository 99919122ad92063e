"""Calibration on device (mmsa.evaluate.calibration / Calibration, csrc/calibrate.hip) on the GPU.  Every comparison of bins is exact (np.array_equal on
int64) against the numpy restatement tests/calibration_ref.py, which tests/test_calibration_cpu.py pins against a brute-force loop."""
import numpy as np
import pytest
import torch

from tests import calibration_ref as CR
from tests import eval_ref as ER
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (1, 2, 15, 16, 64)
VARIANTS = (dict(), dict(reduce_zero_label=True), dict(label_map={2: 1, 1: 0}), dict(ignore_index=0))
OFFSETS = ((0, 0), (1, 1), (3, 2), (2, 0), (0, 3), (2, 2), (3, 3))       # base pointers of pred and label: aligned, equally and differently misaligned


def _unaligned(a, off):
    """The array on the device at a base pointer `off` BYTES past an aligned one (a multiple of 4 for float32)."""
    nbytes = a.size * a.itemsize
    buf = torch.zeros(nbytes + 32, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == off % 16 and t.is_contiguous()
    return t


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


@pytest.mark.parametrize("C", (2, 25, 126, 254))
def test_bins_equal_the_restatement(C):
    from mmsa.evaluate import LabelPrep, calibration
    seen = set()
    k = (2, 25, 126, 254).index(C)
    for B in (1, 2, 3):
        for W in (1, 255, 257, 1021, 1024):
            H = 37 if W > 1 else 300
            K = KS[(k + k // 5) % 5]
            kw = VARIANTS[(k // 2) % 4]
            po, lo = OFFSETS[k % 7]
            co = 4 * ((k + k // 4) % 4)                                   # conf: 0, 4, 8 or 12 bytes past a 16-byte boundary
            pred, conf, label = CR.make_case(2000 + 31 * C + k, H, W, C, K, B=B)
            lp = LabelPrep(C, **kw)
            got = calibration(_unaligned(pred, po), _unaligned(conf, co), _unaligned(label, lo), lp, bins=K).cpu().numpy()
            want = CR.bins_of_batch(pred, conf, label, C, K, **kw)
            assert got.dtype == np.int64 and got.shape == (B, 3, K)
            assert np.array_equal(got, want), f"C {C} B {B} W {W} K {K} offsets {po},{lo},{co} {kw}"
            if W > 1 and not kw:
                assert (want[:, 0] > 0).all()                             # every bin of every image is in play
            seen.add((K, po, lo, co))
            k += 1
    assert {s[0] for s in seen} == set(KS) and {s[3] for s in seen} == {0, 4, 8, 12} and len({s[1:3] for s in seen}) >= 5


@pytest.mark.parametrize("K", KS)
def test_specials_land_where_the_definitions_put_them(K):
    """NaN, -1, 0, 1e-40, -inf, -0.0 -> bin 0 with confidence 0; 2, 1, +inf -> the last bin with 2^24; the float below 1 -> the last bin with 2^24 - 1.
    Everything else in the image is ignored, so the bins hold the specials alone; at every float4 phase of the confidence pointer."""
    from mmsa.evaluate import LabelPrep, calibration
    n = len(CR.SPECIALS)
    pred = np.full((1, 3, 11), 3, dtype=np.uint8)
    label = np.full((1, 3, 11), 255, dtype=np.uint8)
    conf = np.full((1, 3, 11), 0.5, dtype=np.float32)
    pred.reshape(-1)[:n] = label.reshape(-1)[:n] = np.arange(n) % 5
    conf.reshape(-1)[:n] = CR.SPECIALS
    want = np.zeros((1, 3, K), dtype=np.int64)
    want[0, :2, 0] += 6
    want[0, :2, K - 1] += 4
    want[0, 2, K - 1] += 4 * 2 ** 24 - 1
    assert np.array_equal(CR.bins_of_batch(pred, conf, label, 5, K), want)
    for co in (0, 4, 8, 12):
        got = calibration(_dev(pred)[0], _unaligned(conf, co), _dev(label)[0], LabelPrep(5), bins=K).cpu().numpy()
        assert np.array_equal(got, want), (K, co)


@pytest.mark.parametrize("geom", ((1042, 1042, (1024, 1024), True), (300, 550, (512, 256), True), (120, 200, (77, 91), False)))
def test_label_tables(geom):
    """The nearest-neighbour label resize through the index tables: 1042^2 -> 1024^2 (DELIVER) for two images, and non-square cases; tables holding
    anything are clamped into the label map."""
    from mmsa.evaluate import LabelPrep, calibration
    Hl, Wl, scale, keep = geom
    C, K = 25, 15
    lp = LabelPrep(C, resize=dict(seg_scale=scale, keep_ratio=keep))
    H, W = ER.new_size(Hl, Wl, scale, keep)
    _, _, label = CR.make_case(11, Hl, Wl, C, K, B=2)
    pred, conf, _ = CR.make_case(12, H, W, C, K, B=2)
    p, c, l = _dev(pred, conf, label)
    got = calibration(p, c, l, lp, bins=K).cpu().numpy()
    assert np.array_equal(got, CR.bins_of_batch(pred, conf, ER.resize_nearest(label, H, W), C, K))
    key = next(iter(lp._tables))
    ymap, xmap = lp._tables[key]
    ymap.fill_(10 ** 6)
    xmap.fill_(-5)
    got = calibration(p, c, l, lp, bins=K).cpu().numpy()
    corner = np.broadcast_to(label[:, -1:, :1], (2, H, W))
    assert np.array_equal(got, CR.bins_of_batch(pred, conf, corner, C, K))


def test_accumulation_slots_and_determinism():
    from mmsa.evaluate import Calibration, LabelPrep, calibration
    C, K = 19, 15
    pred, conf, label = CR.make_case(21, 150, 257, C, K, B=3)
    label[1] = 255                                                            # an all-ignored image leaves its slot zero
    lp = LabelPrep(C)
    p, c, l = _dev(pred, conf, label)
    per = CR.bins_of_batch(pred, conf, label, C, K)
    a = calibration(p, c, l, lp, bins=K)
    b = calibration(p, c, l, lp)                                              # 15 bins by default
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), per) and not per[1].any() and per[0].any() and per[2].any()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()             # integer sums: the same bytes run after run
    routed = calibration(p, c, l, lp, bins=K, slots=[1, 0, 1]).cpu().numpy()
    assert routed.shape == (2, 3, K) and np.array_equal(routed[1], per[0] + per[2]) and np.array_equal(routed[0], per[1])
    buf = torch.zeros(2, 3, K, dtype=torch.int64, device=DEV)
    assert calibration(p, c, l, lp, cal=buf, slots=[1, 0, 1]) is buf          # bins= defaults to the buffer's
    calibration(p, c, l, lp, cal=buf, slots=[0, 0, 0])                        # two calls sum
    assert np.array_equal(buf.cpu().numpy(), routed + np.stack([per.sum(0), np.zeros_like(per[0])]))
    # the Calibration: per image, in order, refusing overflow without consuming a slot; and per case
    cal = Calibration(lp, bins=K, images=3).add(p[:2], c[:2], l[:2])
    assert cal.used == 2 and np.array_equal(cal.host_bins(), per[:2])
    with pytest.raises(RuntimeError, match="per-image slots"):
        cal.add(p[:2], c[:2], l[:2])
    with pytest.raises(RuntimeError, match="size mismatch"):
        cal.add(p[2:], c[2:], l[2:, :-1].contiguous())
    assert cal.used == 2
    cal.add(p[2:], c[2:], l[2:])
    assert cal.used == 3 and np.array_equal(cal.host_bins(), per) and tuple(cal.bins.shape) == (3, 3, K)
    cc = Calibration(lp, bins=K, cases=["fog", "night"], device=DEV)
    assert cc.bins is not None and not cc.host_bins().any()
    cc.add(p[:2], c[:2], l[:2], case="night").add(p[2:], c[2:], l[2:], case="fog").add(p[:1], c[:1], l[:1], case="night")
    assert np.array_equal(cc.host_bins(), np.stack([per[2], per[0] + per[1] + per[0]]))
    cc.add(p, c, l, slots=[0, 0, 1])                                          # slots named outright, as a captured call names them
    assert np.array_equal(cc.host_bins(), np.stack([per[2] + per[0] + per[1], 2 * per[0] + per[1] + per[2]]))
    from mmsa.evaluate import ece_of, risk_coverage_of
    assert cc.ece(slot="fog") == ece_of(cc.host_bins()[0]) and cc.ece() == ece_of(cc.host_bins().sum(0)) and cc.ece(slot=1) == cc.ece(slot="night")
    assert np.array_equal(cc.risk_coverage()[1], risk_coverage_of(cc.host_bins().sum(0))[1])
    assert abs(float(cc.ece(slot="fog")) - CR.ece_float64(pred[[2, 0, 1]], conf[[2, 0, 1]], label[[2, 0, 1]], C, K)) < 2.0 ** -24
    cc.reset()
    assert not cc.host_bins().any() and np.isnan(cc.ece())


def test_agreement_with_the_evaluator():
    """On the same maps: sum(total) = sum over l < C of counts[l, :], sum(correct) = trace(counts[:C, :C]), and the accuracy is the unrounded aAcc."""
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep, confusion
    C, K = 25, 15
    pred, conf, label = CR.make_case(33, 211, 300, C, K, B=2)
    p, c, l = _dev(pred, conf, label)
    for kw in VARIANTS:
        lp = LabelPrep(C, **kw)
        counts = confusion(p, l, lp).cpu().numpy()
        cal = Calibration(lp, bins=K).add(p, c, l)
        b = cal.host_bins()
        assert np.array_equal(b[:, 0].sum(-1), counts[:, :C, :].sum((1, 2)))
        assert np.array_equal(b[:, 1].sum(-1), np.trace(counts[:, :C, :C], axis1=1, axis2=2))
        ev = Evaluator(lp).add(p, l)
        assert cal.accuracy() == ev.metrics()["aAcc"] and cal.accuracy(slot=1) == ev.metrics(slot=1)["aAcc"]
        assert counts[:, C, :].any()                                          # out-of-range labels are in play, and take no part


def test_refusals_raise_and_launch_nothing():
    from mmsa.evaluate import Calibration, LabelPrep, calibration
    C, K = 25, 15
    pred, conf, label = CR.make_case(5, 40, 64, C, K, B=2)
    p, c, l = _dev(pred, conf, label)
    lp = LabelPrep(C)
    with pytest.raises(RuntimeError, match="conf is torch.float16"):
        calibration(p, c.half(), l, lp)
    with pytest.raises(RuntimeError, match="conf has shape"):
        calibration(p, c[:, :39].contiguous(), l, lp)
    with pytest.raises(RuntimeError, match="conf must be a GPU tensor"):
        calibration(p, c.cpu(), l, lp)
    with pytest.raises(RuntimeError, match="conf must be contiguous"):
        calibration(p, torch.zeros(2, 40, 128, device=DEV)[:, :, ::2], l, lp)
    with pytest.raises(RuntimeError, match="uint8"):
        calibration(p.to(torch.int32), c, l, lp)
    with pytest.raises(RuntimeError, match="size mismatch"):
        calibration(p, c, l[:, :39].contiguous(), lp)
    with pytest.raises(RuntimeError, match="count slots"):
        calibration(p, c, l, lp, cal=torch.zeros(1, 3, K, dtype=torch.int64, device=DEV), slots=[0, 1])
    with pytest.raises(RuntimeError, match=r"int64 \[n_slots, 3, 15\]"):
        calibration(p, c, l, lp, bins=15, cal=torch.zeros(2, 3, 10, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="1..64"):
        calibration(p, c, l, lp, bins=65)
    cal = Calibration(lp, device=DEV)
    with pytest.raises(RuntimeError, match="conf is torch.float64"):
        cal.add(p, c.double(), l)
    assert cal.used == 0 and not cal.host_bins().any()
    torch.cuda.synchronize()                                                  # the device is alive and well
    assert np.array_equal(calibration(p, c, l, lp).cpu().numpy(), CR.bins_of_batch(pred, conf, label, C, K))


# ---- the class-map entries on the tiny model

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
    return cfg, m, h, frame.to(DEV), make_input(cfg, batch=2, seed=17).to(DEV)


NUM_CLASSES = HEAD_CONFIGS["head_tiny"]["kwargs"]["num_classes"]


def _labels(seed, B, H, W):
    return _dev(ER.make_case(seed, H, W, NUM_CLASSES, B=B)[1])[0]


def test_class_map_entries_with_a_calibration(models):
    """Each entry gives the bins Calibration.add gives on the map and confidence it returned, byte for byte, and returns what it returns without
    calibration=; with an evaluator as well, the evaluator's counts are what they are without."""
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    slide = lambda **kw: inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, **kw)
    calls = ((slide, _labels(61, 1, 320, 400)),
             (lambda **kw: inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=2, ori_shape=(300, 380, 3), **kw), _labels(62, 1, 300, 380)),
             (lambda **kw: inf.whole_class_map(m, h, x, **kw), _labels(63, 2, 256, 256)),
             (lambda **kw: inf.whole_class_map(m, h, x, dim=(192, 240), **kw), _labels(64, 2, 192, 240)),              # the rescaled kernel
             (lambda **kw: inf.class_map(m, h, x, dict(mode="whole_dim_cut", dim=(200, 300), cut_dim=(260, 150)), **kw), _labels(65, 2, 150, 260)),
             (lambda **kw: inf.aug_class_map(m, h, [x, x.flip(3)], dict(mode="whole"), ori_shape=(200, 310), flips=[None, "horizontal"], **kw),
              _labels(66, 2, 200, 310)))
    for i, (call, lab) in enumerate(calls):
        B = lab.shape[0]
        plain = call(confidence=True)
        cal = Calibration(lp, images=B, device=DEV)
        got = call(confidence=True, labels=lab, calibration=cal)               # labels= with a calibration and no evaluator
        assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain)), i
        want = Calibration(lp, images=B).add(got[0], got[-1], lab)
        assert cal.used == B and cal.bins.cpu().numpy().tobytes() == want.bins.cpu().numpy().tobytes() and int(cal.bins[:, 0].sum()) > 0, i
        assert np.array_equal(cal.host_bins(), CR.bins_of_batch(got[0].cpu().numpy(), got[-1].cpu().numpy(), lab.cpu().numpy(), NUM_CLASSES, 15)), i
        ev0, ev1, cal1 = Evaluator(lp, images=B, device=DEV), Evaluator(lp, images=B, device=DEV), Calibration(lp, images=B, device=DEV)
        call(labels=lab, evaluator=ev0)
        got = call(confidence=True, labels=lab, evaluator=ev1, calibration=cal1)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)) and torch.equal(ev1.counts, ev0.counts) and torch.equal(cal1.bins, cal.bins), i
        assert cal1.accuracy() == ev1.metrics()["aAcc"]
    # per case, into a given confidence buffer
    cc = Calibration(lp, bins=10, cases=["fog", "night"], device=DEV)
    buf = torch.empty(1, 320, 400, device=DEV)
    lab = calls[0][1]
    cm, _, conf = slide(confidence=buf, labels=lab, calibration=cc, case="night")
    slide(confidence=buf, labels=lab, calibration=cc, case="night")
    one = CR.bins_of_batch(cm.cpu().numpy(), conf.cpu().numpy(), lab.cpu().numpy(), NUM_CLASSES, 10)[0]
    assert conf is buf and np.array_equal(cc.host_bins(), np.stack([np.zeros_like(one), 2 * one]))


def test_slide_runner_with_a_calibration(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    lab = _labels(71, 1, 320, 400)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, confidence=True)
    r = sr.run()
    want_map, want_conf = r.outputs()[0].clone(), r.confidence().clone()
    cal = Calibration(lp, cases=["clear"], device=DEV)
    r = sr.run(labels=lab, calibration=cal, case="clear")
    assert torch.equal(r.outputs()[0], want_map) and torch.equal(r.confidence(), want_conf) and int(r.outputs()[1].item()) == 0
    one = Calibration(lp, cases=["clear"]).add(want_map, want_conf, lab, case="clear")
    assert cal.bins.cpu().numpy().tobytes() == one.bins.cpu().numpy().tobytes() and int(cal.bins[0, 0].sum()) > 0
    ev = Evaluator(lp, cases=["clear"], device=DEV)
    sr.run(labels=lab, evaluator=ev, calibration=cal, case="clear").outputs()
    assert np.array_equal(cal.host_bins(), 2 * one.host_bins()) and cal.accuracy() == ev.metrics()["aAcc"]       # twice the bins of one frame, exactly
    # refusals: before anything is enqueued
    for kw, msg in ((dict(calibration=cal), "needs labels="), (dict(labels=lab, calibration=cal, fused=True), "fused=True / return_map=False"),
                    (dict(labels=lab, calibration=cal, return_map=False), "fused=True / return_map=False")):
        with pytest.raises(RuntimeError, match=msg):
            sr.run(case="clear", **kw)
    plain = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2)
    with pytest.raises(RuntimeError, match="SlideRunner.run: calibration= needs the confidence map"):
        plain.run(labels=lab, calibration=cal, case="clear")
    assert np.array_equal(cal.host_bins(), 2 * one.host_bins())


def test_entries_refuse_before_any_launch(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, LabelPrep
    cfg, m, h, frame, x = models
    lab_w, lab_s = _labels(81, 2, 256, 256), _labels(82, 1, 320, 400)
    cal = Calibration(LabelPrep(NUM_CLASSES), images=2, device=DEV)
    with pytest.raises(RuntimeError, match="whole_class_map: calibration= needs labels="):
        inf.whole_class_map(m, h, x, confidence=True, calibration=cal)
    with pytest.raises(RuntimeError, match="slide_class_map: calibration= needs the confidence map"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab_s, calibration=cal)
    with pytest.raises(RuntimeError, match="class_map: calibration= needs the confidence map"):
        inf.class_map(m, h, x, dict(mode="whole"), labels=lab_w, calibration=cal)
    with pytest.raises(RuntimeError, match="aug_class_map: calibration= needs labels="):
        inf.aug_class_map(m, h, [x], dict(mode="whole"), confidence=True, calibration=cal)
    for kw in (dict(fused=True), dict(return_map=False)):
        with pytest.raises(RuntimeError, match="whole_class_map: confidence with fused=True / return_map=False"):
            inf.whole_class_map(m, h, x, labels=lab_w, confidence=True, calibration=cal, **kw)
        with pytest.raises(RuntimeError, match="slide_class_map: confidence with fused=True / return_map=False"):
            inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab_s, confidence=True, calibration=cal, **kw)
    # a confidence buffer of the wrong dtype, shape or device, or non-contiguous
    with pytest.raises(RuntimeError, match="must be float32"):
        inf.whole_class_map(m, h, x, labels=lab_w, calibration=cal, confidence=torch.empty(2, 256, 256, device=DEV, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="has shape"):
        inf.whole_class_map(m, h, x, labels=lab_w, calibration=cal, confidence=torch.empty(2, 256, 255, device=DEV))
    with pytest.raises(RuntimeError, match="is on cpu"):
        inf.slide_class_map(m, h, frame, (256, 256), (170, 170), labels=lab_s, calibration=cal, confidence=torch.empty(1, 320, 400))
    with pytest.raises(RuntimeError, match="must be contiguous"):
        inf.whole_class_map(m, h, x, labels=lab_w, calibration=cal, confidence=torch.empty(2, 256, 512, device=DEV)[:, :, ::2])
    with pytest.raises(RuntimeError, match="come together"):                 # labels= with neither still raises as before
        inf.whole_class_map(m, h, x, labels=lab_w)
    torch.cuda.synchronize()
    assert cal.used == 0 and not cal.host_bins().any() and int(cal.bins.sum()) == 0
