"""Evaluation on device (mmsa.evaluate, csrc/evaluate.hip, the fused variant of csrc/segment.hip) on the GPU.  Every comparison of counts is exact
(np.array_equal on int64) against the numpy restatement tests/eval_ref.py, which tests/test_evaluate_cpu.py pins against the imported reference."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ref_counts(pred, label, C, slots=None, n_slots=None, **kw):
    B = pred.shape[0]
    slots = list(range(B)) if slots is None else slots
    out = np.zeros((max(slots) + 1 if n_slots is None else n_slots, C + 1, C + 1), dtype=np.int64)
    for b in range(B):
        out[slots[b]] += ER.confusion(pred[b], label[b], C, **kw)
    return out


def _unaligned(a, off):
    """The array on the device at a base pointer `off` bytes past an aligned one."""
    buf = torch.zeros(a.size + 8, dtype=torch.uint8, device=DEV)
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 4 == off % 4 and t.is_contiguous()
    return t


@pytest.mark.parametrize("C", (2, 14, 19, 25, 64, 126))          # 126 = the limit: 64772 bytes of dynamic LDS
def test_counts_equal_the_restatement(C):
    from mmsa.evaluate import LabelPrep, confusion
    k = 0
    for B in (1, 2, 3):
        for W in (1, 255, 257, 1021, 1024):
            H = 37 if W > 1 else 300
            pred, label = ER.make_case(1000 + 31 * C + k, H, W, C, B=B)
            kw = (dict(), dict(reduce_zero_label=True), dict(label_map={2: 1, 1: 0}))[k % 3]
            po, lo = ((0, 0), (1, 1), (3, 2), (2, 0), (0, 3))[k % 5]       # base pointers: aligned, equally and differently misaligned
            lp = LabelPrep(C, ignore_index=255, **kw)
            got = confusion(_unaligned(pred, po), _unaligned(label, lo), lp).cpu().numpy()
            want = _ref_counts(pred, label, C, **kw)
            assert got.dtype == np.int64 and np.array_equal(got, want), f"C {C} B {B} W {W} offsets {po},{lo} {kw}"
            if W > 1:
                assert want[:, C, :].any() and want[:, :, C].any()        # out-of-range labels and 255 predictions are in play
            k += 1


def test_all_ignored_image_and_determinism():
    from mmsa.evaluate import LabelPrep, confusion
    C = 25
    pred, label = ER.make_case(7, 200, 333, C, B=3)
    label[1] = 255
    lp = LabelPrep(C)
    p, l = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    a = confusion(p, l, lp)
    b = confusion(p, l, lp)
    torch.cuda.synchronize()
    assert not a[1].any() and a[0].any() and a[2].any()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()         # integer sums: the same bytes run after run
    assert np.array_equal(a.cpu().numpy(), _ref_counts(pred, label, C))
    # ignore_index other than 255: 255 is then an out-of-range label, counted under index C
    lp0 = LabelPrep(C, ignore_index=0)
    assert np.array_equal(confusion(p, l, lp0).cpu().numpy(), _ref_counts(pred, label, C, ignore_index=0))


@pytest.mark.parametrize("geom", ((1042, 1042, (1024, 1024), True), (300, 550, (512, 256), True), (120, 200, (77, 91), False)))
def test_label_tables(geom):
    """The nearest-neighbour label resize through the index tables: 1042^2 -> 1024^2 (DELIVER) and non-square cases."""
    from mmsa.evaluate import LabelPrep, confusion
    Hl, Wl, scale, keep = geom
    C = 25
    lp = LabelPrep(C, resize=dict(seg_scale=scale, keep_ratio=keep))
    H, W = ER.new_size(Hl, Wl, scale, keep)
    assert lp.resized(Hl, Wl) == (H, W)
    _, label = ER.make_case(11, Hl, Wl, C, B=2)
    pred, _ = ER.make_case(12, H, W, C, B=2)
    got = confusion(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), lp).cpu().numpy()
    assert np.array_equal(got, _ref_counts(pred, ER.resize_nearest(label, H, W), C))
    # the second call finds its tables on the device
    n = len(lp._tables)
    confusion(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), lp)
    assert len(lp._tables) == n == 1
    # tables holding anything are clamped into the label map (no out-of-bounds read): indices far outside give the border pixels
    key = next(iter(lp._tables))
    ymap, xmap = lp._tables[key]
    ymap.fill_(10 ** 6)
    xmap.fill_(-5)
    got = confusion(torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV), lp).cpu().numpy()
    corner = np.broadcast_to(label[:, -1:, :1], (2, H, W))
    assert np.array_equal(got, _ref_counts(pred, corner, C))


def test_slots_and_accumulation():
    from mmsa.evaluate import Evaluator, LabelPrep, confusion
    C = 19
    pred, label = ER.make_case(21, 150, 257, C, B=3)
    lp = LabelPrep(C)
    p, l = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    per = confusion(p, l, lp).cpu().numpy()
    routed = confusion(p, l, lp, slots=[1, 0, 1]).cpu().numpy()
    assert routed.shape[0] == 2 and np.array_equal(routed[1], per[0] + per[2]) and np.array_equal(routed[0], per[1])
    counts = torch.zeros(2, C + 1, C + 1, dtype=torch.int64, device=DEV)
    confusion(p, l, lp, counts=counts, slots=[1, 0, 1])
    confusion(p, l, lp, counts=counts, slots=[0, 0, 0])
    assert np.array_equal(counts.cpu().numpy(), routed + np.stack([per.sum(0), np.zeros_like(per[0])]))
    # the Evaluator: per image, and per case
    ev = Evaluator(lp).add(p[:2], l[:2]).add(p[2:], l[2:])
    assert np.array_equal(ev.host_counts(), per)
    for got, want in zip(ev.areas(), zip(*[ER.intersect_and_union(pred[b], label[b], C) for b in range(3)])):
        assert np.array_equal(got, np.stack(want))
    evc = Evaluator(lp, cases=["fog", "night"], device=DEV).add(p[:2], l[:2], case="night").add(p[2:], l[2:], case="fog").add(p[:1], l[:1], case="night")
    assert np.array_equal(evc.host_counts(), np.stack([per[2], per[0] + per[1] + per[0]]))
    m = evc.metrics(("mIoU", "mFscore"), slot="night")
    want = ER.total_area_to_metrics(*ER.areas_of(per[0] + per[1] + per[0]), metrics=("mIoU", "mFscore"))
    assert all(np.array_equal(m[k], want[k], equal_nan=True) for k in want)
    tot = evc.metrics()
    assert np.array_equal(tot["IoU"], ER.total_area_to_metrics(*ER.areas_of(per.sum(0) + per[0]))["IoU"], equal_nan=True)
    evc.reset()
    assert not evc.host_counts().any()


def test_refusals_raise_and_launch_nothing():
    from mmsa.evaluate import LabelPrep, confusion
    C = 25
    pred, label = ER.make_case(5, 40, 64, C, B=2)
    p, l = torch.from_numpy(pred).to(DEV), torch.from_numpy(label).to(DEV)
    lp = LabelPrep(C)
    with pytest.raises(RuntimeError, match=r"2\.\.126"):                      # the histogram of 200 classes does not fit the LDS: named limit
        confusion(p, l, LabelPrep(200))
    with pytest.raises(RuntimeError, match="size mismatch"):
        confusion(p, l[:, :39].contiguous(), lp)
    with pytest.raises(RuntimeError, match="size mismatch"):                 # ... also after the tables
        confusion(p, l, LabelPrep(C, resize=dict(seg_scale=(32, 32), keep_ratio=False)))
    with pytest.raises(RuntimeError, match="uint8"):
        confusion(p, l.to(torch.int64), lp)
    with pytest.raises(RuntimeError, match="uint8"):
        confusion(p.to(torch.int32), l, lp)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        confusion(p, l.cpu(), lp)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        confusion(p.cpu(), l, lp)
    with pytest.raises(RuntimeError, match="count slots"):
        confusion(p, l, lp, counts=torch.zeros(1, C + 1, C + 1, dtype=torch.int64, device=DEV), slots=[0, 1])
    with pytest.raises(RuntimeError, match="int64"):
        confusion(p, l, lp, counts=torch.zeros(2, C + 1, C + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="label maps for"):
        confusion(p, l[:1], lp)
    torch.cuda.synchronize()                                                  # the device is alive and well
    assert np.array_equal(confusion(p, l, lp).cpu().numpy(), _ref_counts(pred, label, C))


def _windows(jobs):
    return (ctypes.c_int * (3 * len(jobs)))(*[v for j in jobs for v in j])


@pytest.mark.parametrize("case", ("overlap", "whole", "uncovered"))
def test_fused_entry(case):
    """mmsa_slide_argmax_eval on seeded logits: the map is mmsa_slide_argmax's byte for byte, the counts are the standalone entry's on that map, and
    out == NULL gives the same counts and writes nothing."""
    from mmsa import lib, ops
    from mmsa.evaluate import LabelPrep, confusion, slide_argmax_eval
    C = 25
    g = torch.Generator().manual_seed(3)
    if case == "overlap":        # 2 images, 64 x 64 windows (16 x 16 logits) on a 90 x 150 frame, stride 40: pixels covered 1, 2 and 4 times
        B, H, W, hc, wc, hs, ws = 2, 90, 150, 64, 64, 16, 16
        ys, xs = (0, 26), (0, 40, 80, 86)
        jobs = [(b, y, x) for y in ys for x in xs for b in range(B)]
    elif case == "whole":
        B, H, W, hc, wc, hs, ws = 2, 101, 259, 101, 259, 26, 65
        jobs = [(b, 0, 0) for b in range(B)]
    else:                        # one window that leaves most of the frame uncovered: class 255 there, counted under pred index C
        B, H, W, hc, wc, hs, ws = 1, 80, 80, 64, 64, 16, 16
        jobs = [(0, 0, 0)]
    n = len(jobs)
    lg = torch.randn(n, C, hs, ws, generator=g).to(DEV)
    _, label = ER.make_case(17, H, W, C, B=B)
    lab = torch.from_numpy(label).to(DEV)
    lp = LabelPrep(C)
    tab = _windows(jobs)
    want = torch.empty(B, H, W, dtype=torch.uint8, device=DEV)
    unc0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.call("mmsa_slide_argmax", lg.data_ptr(), n, C, hs, ws, tab, want.data_ptr(), B, H, W, hc, wc, unc0.data_ptr(), ops._stream())
    want_counts = confusion(want, lab, lp)
    assert np.array_equal(want_counts.cpu().numpy(), _ref_counts(want.cpu().numpy(), label, C))

    got = torch.full((B, H, W), 77, dtype=torch.uint8, device=DEV)
    unc1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    counts = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=DEV)
    slide_argmax_eval(lg, n, tab, got, B, H, W, hc, wc, unc1, lab, lp, counts)
    assert torch.equal(got, want) and int(unc1.item()) == int(unc0.item())
    assert torch.equal(counts, want_counts)
    if case == "uncovered":
        assert int(unc1.item()) == 80 * 80 - 64 * 64 and int(counts[0, :, C].sum()) == int((label[0][want.cpu().numpy()[0] == 255] != 255).sum())
    else:
        assert int(unc1.item()) == 0

    # out == NULL: the same counts (no map pointer reaches the kernel; that a caller's map buffer stays as it was is shown on SlideRunner's below)
    counts2 = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=DEV)
    unc2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    slide_argmax_eval(lg, n, tab, None, B, H, W, hc, wc, unc2, lab, lp, counts2)
    torch.cuda.synchronize()
    assert torch.equal(counts2, want_counts) and int(unc2.item()) == int(unc0.item())
    # through label tables too (a label map of another size)
    lp2 = LabelPrep(C, resize=dict(seg_scale=(W, H), keep_ratio=False))
    _, big = ER.make_case(18, H + 13, W + 29, C, B=B)
    counts3 = torch.zeros(1, C + 1, C + 1, dtype=torch.int64, device=DEV)
    slide_argmax_eval(lg, n, tab, None, B, H, W, hc, wc, unc2, torch.from_numpy(big).to(DEV), lp2, counts3, slots=[0] * B)
    assert np.array_equal(counts3.cpu().numpy(), _ref_counts(want.cpu().numpy(), ER.resize_nearest(big, H, W), C, slots=[0] * B))
    # refusals of the fused entry
    with pytest.raises(RuntimeError, match="size mismatch"):
        slide_argmax_eval(lg, n, tab, None, B, H, W, hc, wc, unc2, lab[:, :-1].contiguous(), lp, counts2)
    with pytest.raises(RuntimeError, match="classes"):
        slide_argmax_eval(lg, n, tab, None, B, H, W, hc, wc, unc2, lab, LabelPrep(C + 1), counts2)


@pytest.fixture(scope="module")
def models():
    import mmsa
    from oracle import ref_encoder as R
    from oracle import ref_head as RH
    from tests.configs import CONFIGS, HEAD_CONFIGS
    from tests.weights import seeded_state_dict
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    sd = seeded_state_dict(R.OracleEncoder(**cfg["kwargs"]), seed=cfg["seed"])
    hsd = seeded_state_dict(RH.OracleSegformerHead(**hcfg["kwargs"]), seed=hcfg["seed"])
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(sd)
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(hsd)
    return cfg, hcfg["kwargs"]["num_classes"], m, h


@pytest.mark.parametrize("fused", (True, False))
def test_class_map_calls_with_labels(models, fused):
    """whole_class_map / slide_class_map with labels= return the map they return without it, and the evaluator's counts are the restatement's on that
    map -- with the fused launch and with two launches."""
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep
    from tests.configs import make_input
    cfg, C, m, h = models
    lp = LabelPrep(C)
    x = make_input(cfg, batch=2, seed=4).to(DEV)
    want = inf.whole_class_map(m, h, x)
    _, label = ER.make_case(41, 256, 256, C, B=2)
    ev = Evaluator(lp)
    got = inf.whole_class_map(m, h, x, labels=torch.from_numpy(label).to(DEV), evaluator=ev, fused=fused)
    assert torch.equal(got, want)
    assert np.array_equal(ev.host_counts(), _ref_counts(want.cpu().numpy(), label, C))
    if fused:
        ev2 = Evaluator(lp, cases=["all"])
        assert inf.whole_class_map(m, h, x, labels=torch.from_numpy(label).to(DEV), evaluator=ev2, case="all", return_map=False) is None
        assert np.array_equal(ev2.host_counts()[0], ev.host_counts().sum(0))
    with pytest.raises(RuntimeError, match="come together"):
        inf.whole_class_map(m, h, x, labels=torch.from_numpy(label).to(DEV))

    g = torch.Generator().manual_seed(9)
    frame = torch.randn(2, 6, 320, 400, generator=g).to(DEV)
    want, unc = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=3)
    _, label = ER.make_case(42, 320, 400, C, B=2)
    ev = Evaluator(lp)
    got, unc2 = inf.slide_class_map(m, h, frame, (256, 256), (170, 170), max_batch=3, labels=torch.from_numpy(label).to(DEV), evaluator=ev, fused=fused)
    assert torch.equal(got, want) and int(unc.item()) == int(unc2.item()) == 0
    assert np.array_equal(ev.host_counts(), _ref_counts(want.cpu().numpy(), label, C))


def test_slide_runner_with_labels_counts_every_frame(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep
    cfg, C, m, h = models
    g = torch.Generator().manual_seed(77)
    frame = torch.randn(1, 6, 300, 420, generator=g).to(DEV)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (160, 160), chains=2)
    want, _ = sr.run().outputs()
    want = want.clone()
    _, label = ER.make_case(43, 300, 420, C, B=1)
    lab = torch.from_numpy(label).to(DEV)
    ev = Evaluator(LabelPrep(C), cases=["clear"], device=DEV)
    one = _ref_counts(want.cpu().numpy(), label, C)
    cm, unc = sr.run(labels=lab, evaluator=ev, case="clear").outputs()
    assert torch.equal(cm, want) and int(unc.item()) == 0
    assert np.array_equal(ev.host_counts(), one)
    sr.run(labels=lab, evaluator=ev, case="clear").outputs()
    assert np.array_equal(ev.host_counts(), 2 * one)                        # twice the counts of one frame, exactly
    sr.run(labels=lab, evaluator=ev, case="clear", fused=False).outputs()
    assert np.array_equal(ev.host_counts(), 3 * one)

    # return_map=False: the counts of one more frame, the runner's map buffer (filled with a sentinel as guard) is not written, and the result has no map
    sr.out.fill_(77)
    cm, unc = sr.run(labels=lab, evaluator=ev, case="clear", return_map=False).outputs()
    torch.cuda.synchronize()
    assert cm is None and int(unc.item()) == 0
    assert bool((sr.out == 77).all())
    assert np.array_equal(ev.host_counts(), 4 * one)
    with pytest.raises(RuntimeError, match="fused launch"):
        sr.run(labels=lab, evaluator=ev, case="clear", return_map=False, fused=False)
    # ... and a refused call consumes no per-image slot: the next image still lands in slot 0
    per = Evaluator(LabelPrep(C), images=2)
    with pytest.raises(RuntimeError, match="size mismatch"):
        per.add(want, lab[:, :-1].contiguous())
    assert per.used == 0
    per.add(want, lab)
    assert per.used == 1 and np.array_equal(per.host_counts(), one)


def test_class_map_launch_without_a_map_writes_none():
    """whole_class_map(return_map=False) allocates its map buffer as ever and hands it to nobody: shown one level down, on the launch helper, with a
    sentinel-filled buffer in the map's place."""
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep
    C = 7
    g = torch.Generator().manual_seed(8)
    lg = torch.randn(2, C, 16, 16, generator=g).to(DEV)
    _, label = ER.make_case(44, 64, 64, C, B=2)
    lab = torch.from_numpy(label).to(DEV)
    plan = inf.MapPlan.whole(2, 64, 64)
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((2, 64, 64), 77, dtype=torch.uint8, device=DEV)
    ev = Evaluator(LabelPrep(C))
    plan.class_map(lg, out, unc, lab, ev, return_map=False)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    ev2 = Evaluator(LabelPrep(C))
    plan.class_map(lg, out, unc, lab, ev2, fused=True, return_map=True)
    assert not bool((out == 77).all()) and np.array_equal(ev.host_counts(), ev2.host_counts())
    assert np.array_equal(ev.host_counts(), _ref_counts(out.cpu().numpy(), label, C))
