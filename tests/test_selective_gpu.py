"""Selective evaluation on device (mmsa.evaluate.selective / abstain / SelectiveEvaluator, csrc/selective.hip) on the GPU.  Every comparison is exact
(np.array_equal on int64 or uint8) against the numpy restatement tests/selective_ref.py, which tests/test_selective_cpu.py pins against a brute-force
loop, or against what the existing device passes (mmsa.confusion, mmsa.calibration) give for the same maps."""
import numpy as np
import pytest
import torch

from tests import calibration_ref as CR
from tests import eval_ref as ER
from tests import selective_ref as SR
from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_BYTES = 65536 - 256                  # the histogram's share of the 64 KiB a launch asks for (csrc/selective.hip SEL_LDS_BYTES)


def _groups(C, K):
    """(bins resident per workgroup, bin groups, bins of the last group) as csrc/selective.hip forms them."""
    G = LDS_BYTES // ((C + 1) ** 2 * 4)
    n = -(-K // G)
    return G, n, K - (n - 1) * G


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


def test_the_pairs_cover_the_bin_group_arithmetic():
    """One group (2, 1), (2, 64), (25, 15); G = 24 -> 24 + 24 + 16 (25, 64); G = 3 -> five full groups (63, 15) and five and one bin (63, 16); G = 1 ->
    two and 64 groups (126, .).  A later change of the budget cannot silently stop covering a partial last group or several groups."""
    got = {p: _groups(*p) for p in SR.GPU_PAIRS}
    assert got == {(2, 1): (1813, 1, 1), (2, 64): (1813, 1, 64), (25, 15): (24, 1, 15), (25, 64): (24, 3, 16), (63, 15): (3, 5, 3), (63, 16): (3, 6, 1),
                   (126, 2): (1, 2, 1), (126, 64): (1, 64, 1)}
    assert {g[1] for g in got.values()} == {1, 2, 3, 5, 6, 64}
    partial = {p for p, (G, n, last) in got.items() if n > 1 and last < G}
    assert partial == {(25, 64), (63, 16)}


@pytest.mark.parametrize("C,K", SR.GPU_PAIRS)
def test_counts_equal_the_restatement(C, K):
    from mmsa.evaluate import LabelPrep, selective
    seen = set()
    for B, H, W, kw, po, lo, co, seed in SR.gpu_cases(C, K):
        pred, conf, label = CR.make_case(seed, H, W, C, K, B=B)
        got = selective(_unaligned(pred, po), _unaligned(conf, co), _unaligned(label, lo), LabelPrep(C, **kw), bins=K).cpu().numpy()
        want = SR.counts_of_batch(pred, conf, label, C, K, **kw)
        assert got.dtype == np.int64 and got.shape == (B, K, C + 1, C + 1)
        assert np.array_equal(got, want), f"C {C} K {K} B {B} W {W} offsets {po},{lo},{co} {kw}"
        if W > 1 and not kw:                                              # every bin of every image holds a correct, a wrong and a row-C pixel
            good = np.trace(want[:, :, :C, :C], axis1=2, axis2=3)
            assert (good > 0).all() and (want[:, :, :C, :].sum((2, 3)) - good > 0).all() and (want[:, :, C, :].sum(2) > 0).all()
        seen.add((tuple(sorted(kw)), po, lo, co, W))
    assert {s[0] for s in seen} == {tuple(sorted(v)) for v in SR.VARIANTS} and {s[3] for s in seen} == {0, 4, 8, 12} and len({s[1:3] for s in seen}) >= 5
    assert {s[4] for s in seen} == set(SR.GPU_WIDTHS)


@pytest.mark.parametrize("H,W,B", ((64, 1024, 4), (37, 257, 32)))
def test_patchy_data_exercises_the_merged_adds(H, W, B):
    """Patches of classes, one confidence per 16 x 16 block, 90 % of the blocks in the top bin: whole waves hold ONE cell, which uniform noise never does.
    Per image and with every image routed to one slot, where some cell passes 4096 (25 classes share an image: B images make up the weight)."""
    from mmsa.evaluate import LabelPrep, selective
    C, K = 25, 15
    pred, conf, label = SR.make_patchy_case(5 + W, H, W, C, K, B=B)
    want = SR.counts_of_batch(pred, conf, label, C, K)
    assert want.sum(0).max() > 4096                                        # the merged adds carry real weight
    assert want[:, K - 1].sum() > 0.8 * want.sum() and (want[:, :K - 1].sum((0, 2, 3)) > 0).sum() >= K // 2
    for po, lo, co in ((0, 0, 0), (1, 1, 4), (3, 2, 12)):
        p, c, l = _unaligned(pred, po), _unaligned(conf, co), _unaligned(label, lo)
        assert np.array_equal(selective(p, c, l, LabelPrep(C), bins=K).cpu().numpy(), want), (po, lo, co)
        one = selective(p, c, l, LabelPrep(C), bins=K, slots=[0] * B).cpu().numpy()
        assert one.shape == (1, K, C + 1, C + 1) and np.array_equal(one[0], want.sum(0)), (po, lo, co)


@pytest.mark.parametrize("K", (1, 2, 15, 64))
def test_specials_land_where_the_definitions_put_them(K):
    """NaN, -1, 0, 1e-40, -inf, -0.0 -> bin 0; 2, 1, the float below 1, +inf -> the last bin.  Everything else in the image is ignored, so the counts hold
    the specials alone; at every float4 phase of the confidence pointer; and `abstain` cuts them at the same place."""
    from mmsa.evaluate import LabelPrep, abstain, selective
    n = len(CR.SPECIALS)
    pred = np.full((1, 3, 11), 3, dtype=np.uint8)
    label = np.full((1, 3, 11), 255, dtype=np.uint8)
    conf = np.full((1, 3, 11), 0.5, dtype=np.float32)
    pred.reshape(-1)[:n] = label.reshape(-1)[:n] = np.arange(n) % 5
    conf.reshape(-1)[:n] = CR.SPECIALS
    want = np.zeros((1, K, 6, 6), dtype=np.int64)
    for i, k in enumerate((0, 0, K - 1, 0, K - 1, 0, K - 1, K - 1, 0, 0)):
        want[0, k, i % 5, i % 5] += 1
    assert np.array_equal(SR.counts_of_batch(pred, conf, label, 5, K), want)
    for co in (0, 4, 8, 12):
        c = _unaligned(conf, co)
        got = selective(_dev(pred)[0], c, _dev(label)[0], LabelPrep(5), bins=K).cpu().numpy()
        assert np.array_equal(got, want), (K, co)
        if K > 1:
            kept = abstain(_dev(pred)[0], c, K, K - 1).cpu().numpy().reshape(-1)[:n]
            assert np.array_equal(kept != 255, np.array([0, 0, 1, 0, 1, 0, 1, 1, 0, 0], dtype=bool)), (K, co)


@pytest.mark.parametrize("geom", ((1042, 1042, (1024, 1024), True), (120, 200, (77, 91), False)))
def test_label_tables(geom):
    """The nearest-neighbour label resize through the index tables: 1042^2 -> 1024^2 (DELIVER) for two images, and a non-square case; tables holding
    anything are clamped into the label map."""
    from mmsa.evaluate import LabelPrep, selective
    Hl, Wl, scale, keep = geom
    C, K = 25, 15
    lp = LabelPrep(C, resize=dict(seg_scale=scale, keep_ratio=keep))
    H, W = ER.new_size(Hl, Wl, scale, keep)
    _, _, label = CR.make_case(11, Hl, Wl, C, K, B=2)
    pred, conf, _ = CR.make_case(12, H, W, C, K, B=2)
    p, c, l = _dev(pred, conf, label)
    got = selective(p, c, l, lp, bins=K).cpu().numpy()
    assert np.array_equal(got, SR.counts_of_batch(pred, conf, ER.resize_nearest(label, H, W), C, K))
    ymap, xmap = lp._tables[next(iter(lp._tables))]
    ymap.fill_(10 ** 6)
    xmap.fill_(-5)
    got = selective(p, c, l, lp, bins=K).cpu().numpy()
    corner = np.broadcast_to(label[:, -1:, :1], (2, H, W))
    assert np.array_equal(got, SR.counts_of_batch(pred, conf, corner, C, K))


def test_accumulation_slots_and_determinism():
    from mmsa.evaluate import Evaluator, LabelPrep, SelectiveEvaluator, selective, selective_metrics_of
    C, K = 19, 15
    pred, conf, label = CR.make_case(21, 150, 257, C, K, B=3)
    label[1] = 255                                                            # an all-ignored image leaves its slot zero
    lp = LabelPrep(C)
    p, c, l = _dev(pred, conf, label)
    per = SR.counts_of_batch(pred, conf, label, C, K)
    a = selective(p, c, l, lp, bins=K)
    b = selective(p, c, l, lp)                                                # 15 bins by default
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), per) and not per[1].any() and per[0].any() and per[2].any()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()             # integer sums: the same bytes run after run
    routed = selective(p, c, l, lp, bins=K, slots=[1, 0, 1]).cpu().numpy()
    assert routed.shape == (2, K, C + 1, C + 1) and np.array_equal(routed[1], per[0] + per[2]) and np.array_equal(routed[0], per[1])
    buf = torch.zeros(2, K, C + 1, C + 1, dtype=torch.int64, device=DEV)
    assert selective(p, c, l, lp, counts=buf, slots=[1, 0, 1]) is buf         # bins= defaults to the buffer's
    selective(p, c, l, lp, counts=buf, slots=[0, 0, 0])                       # two calls sum
    assert np.array_equal(buf.cpu().numpy(), routed + np.stack([per.sum(0), np.zeros_like(per[0])]))
    # the SelectiveEvaluator: per image, in order, refusing overflow without consuming a slot; and per case
    se = SelectiveEvaluator(lp, bins=K, images=3).add(p[:2], c[:2], l[:2])
    assert se.used == 2 and np.array_equal(se.host_counts(), per[:2])
    with pytest.raises(RuntimeError, match="per-image slots"):
        se.add(p[:2], c[:2], l[:2])
    with pytest.raises(RuntimeError, match="size mismatch"):
        se.add(p[2:], c[2:], l[2:, :-1].contiguous())
    assert se.used == 2
    se.add(p[2:], c[2:], l[2:])
    assert se.used == 3 and np.array_equal(se.host_counts(), per) and tuple(se.counts.shape) == (3, K, C + 1, C + 1)
    ev = Evaluator(lp, images=3).add(p, l)
    assert np.array_equal(se.evaluator_counts(), ev.host_counts()) and all(np.array_equal(x, y) for x, y in zip(se.areas(), ev.areas()))
    for slot in (None, 0, 2):
        m0, m1 = se.metrics(slot=slot, metric=("mIoU", "mDice")), ev.metrics(metric=("mIoU", "mDice"), slot=slot)
        assert list(m0) == list(m1) and all(np.array_equal(m0[k], m1[k], equal_nan=True) for k in m0)
    assert se.summary() == ev.summary() and se.summary(slot=2) == ev.summary(slot=2)
    curve = se.coverage_curve()
    assert all(np.array_equal(v, selective_metrics_of(per.sum(0))[k], equal_nan=True) for k, v in curve.items()) and curve["coverage"][0] == 1
    assert se.metrics(min_bin=7)["aAcc"] == curve["aAcc"][7] and np.array_equal(se.metrics(min_bin=7)["IoU"], curve["IoU"][7], equal_nan=True)
    cc = SelectiveEvaluator(lp, bins=K, cases=["fog", "night"], device=DEV)
    assert cc.counts is not None and not cc.host_counts().any()
    cc.add(p[:2], c[:2], l[:2], case="night").add(p[2:], c[2:], l[2:], case="fog").add(p[:1], c[:1], l[:1], case="night")
    assert np.array_equal(cc.host_counts(), np.stack([per[2], per[0] + per[1] + per[0]]))
    cc.add(p, c, l, slots=[0, 0, 1])                                          # slots named outright, as a captured call names them
    assert np.array_equal(cc.host_counts(), np.stack([per[2] + per[0] + per[1], 2 * per[0] + per[1] + per[2]]))
    assert cc.metrics(slot="fog", min_bin=3)["aAcc"] == cc.metrics(slot=0, min_bin=3)["aAcc"]
    cc.reset()
    assert not cc.host_counts().any() and np.isnan(cc.metrics()["aAcc"])


def test_identities_on_the_device_results():
    """(1) the sum over the bins is mmsa.confusion's matrix; (2) the rows < C of bin k and the trace of its [:C, :C] block are rows 0 and 1 of
    mmsa.calibration's bins -- on the device results themselves, under every label variant and at several (C, K)."""
    from mmsa.evaluate import LabelPrep, calibration, confusion, reliability_counts_of, selective
    for C, K in ((25, 15), (25, 64), (63, 16), (126, 2)):
        pred, conf, label = CR.make_case(33 + K, 211, 300, C, K, B=2)
        p, c, l = _dev(pred, conf, label)
        for kw in SR.VARIANTS:
            lp = LabelPrep(C, **kw)
            counts = selective(p, c, l, lp, bins=K).cpu().numpy()
            assert np.array_equal(counts.sum(1), confusion(p, l, lp).cpu().numpy()), (C, K, kw)
            cal = calibration(p, c, l, lp, bins=K).cpu().numpy()
            assert np.array_equal(reliability_counts_of(counts), cal[:, :2]), (C, K, kw)
            assert np.array_equal(counts[:, :, :C, :].sum((2, 3)), cal[:, 0]) and np.array_equal(np.trace(counts[:, :, :C, :C], axis1=2, axis2=3), cal[:, 1])
        assert counts[:, :, C, :].any()                                       # out-of-range labels are in play: counted here, dropped there


@pytest.mark.parametrize("K", (1, 15, 64))
def test_abstain(K):
    """The thresholded map equals the numpy expression at every pointer offset, in place, and with threshold= on an edge; and (identity 3) its plain
    confusion counts are what the device's own per-bin counts say they are."""
    from mmsa.evaluate import LabelPrep, abstain, bin_edge, confusion, selective
    C = 25
    lp = LabelPrep(C)
    for n, (H, W) in enumerate(((37, 257), (1, 5), (1, 1), (3, 1021))):
        pred, conf, label = CR.make_case(40 + n, H, W, C, K, B=2) if H * W >= 10 else (np.full((2, H, W), 7, np.uint8), np.full((2, H, W), 0.5, np.float32), None)
        for i, k0 in enumerate(sorted({0, 1, K // 2, K - 1, K})):
            want = SR.abstain_of(pred, conf, K, k0)
            po, lo = SR.OFFSETS[(i + n) % 7]
            p, c = _unaligned(pred, po), _unaligned(conf, 4 * ((i + n) % 4))
            got = abstain(p, c, K, k0)
            assert got.dtype == torch.uint8 and got.shape == p.shape and np.array_equal(got.cpu().numpy(), want), (K, H, W, k0, po)
            assert np.array_equal(p.cpu().numpy(), pred)                       # the input is left alone
            out = _unaligned(np.zeros_like(pred), lo)                          # an output of another alignment
            assert abstain(p, c, K, k0, out=out) is out and np.array_equal(out.cpu().numpy(), want), (K, H, W, k0, po, lo)
            if k0 < K:
                assert np.array_equal(abstain(p, c, K, threshold=float(bin_edge(k0, K))).cpu().numpy(), want)
            assert abstain(p, c, K, k0, out=p) is p and np.array_equal(p.cpu().numpy(), want)          # in place
            if label is not None and n == 0:                                   # identity 3
                l = _dev(label)[0]
                counts = selective(_dev(pred)[0], c, l, lp, bins=K).cpu().numpy()
                assert np.array_equal(confusion(p, l, lp).cpu().numpy(), np.stack([SR.abstained_counts(one, k0) for one in counts])), (K, k0)
        if n == 0:
            assert (want == 255).all() and (SR.abstain_of(pred, conf, K, 0) == pred).all()      # min_bin == K abstains everywhere, 0 copies
    p, c = _dev(pred, conf)
    if K == 15:
        with pytest.raises(ValueError, match="not a bin edge of 15 bins"):
            abstain(p, c, K, threshold=0.5)
    for bad in (dict(min_bin=-1), dict(min_bin=K + 1), dict(), dict(min_bin=0, threshold=0.0)):
        with pytest.raises(ValueError, match="min_bin"):
            abstain(p, c, K, **bad)
    with pytest.raises(RuntimeError, match="out must be a contiguous uint8"):
        abstain(p, c, K, 0, out=torch.empty(2, 3, 1022, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="conf has shape"):
        abstain(p, c[:1], K, 0)
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy(), pred)


def test_refusals_raise_and_launch_nothing():
    from mmsa.evaluate import LabelPrep, SelectiveEvaluator, selective
    C, K = 25, 15
    pred, conf, label = CR.make_case(5, 40, 64, C, K, B=2)
    p, c, l = _dev(pred, conf, label)
    lp = LabelPrep(C)
    with pytest.raises(RuntimeError, match="conf is torch.float16"):
        selective(p, c.half(), l, lp)
    with pytest.raises(RuntimeError, match="conf has shape"):
        selective(p, c[:, :39].contiguous(), l, lp)
    with pytest.raises(RuntimeError, match="conf must be a GPU tensor"):
        selective(p, c.cpu(), l, lp)
    with pytest.raises(RuntimeError, match="uint8"):
        selective(p.to(torch.int32), c, l, lp)
    with pytest.raises(RuntimeError, match="size mismatch"):
        selective(p, c, l[:, :39].contiguous(), lp)
    with pytest.raises(RuntimeError, match="count slots"):
        selective(p, c, l, lp, counts=torch.zeros(1, K, C + 1, C + 1, dtype=torch.int64, device=DEV), slots=[0, 1])
    with pytest.raises(RuntimeError, match=r"int64 \[n_slots, 15, 26, 26\]"):
        selective(p, c, l, lp, bins=15, counts=torch.zeros(2, 10, C + 1, C + 1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="1..64"):
        selective(p, c, l, lp, bins=65)
    with pytest.raises(RuntimeError, match="selective evaluation supports 2..126"):
        selective(p, c, l, LabelPrep(127))
    se = SelectiveEvaluator(lp, device=DEV)
    with pytest.raises(RuntimeError, match="conf is torch.float64"):
        se.add(p, c.double(), l)
    assert se.used == 0 and not se.host_counts().any() and int(se.counts.sum()) == 0
    torch.cuda.synchronize()                                                  # the device is alive and well
    assert np.array_equal(selective(p, c, l, lp).cpu().numpy(), SR.counts_of_batch(pred, conf, label, C, K))


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


def test_class_map_entries_with_a_selective_evaluator(models):
    """Each entry, with an Evaluator and a Calibration next to the SelectiveEvaluator: it returns what it returns without selective=; the sum over the
    bins is the Evaluator's counts, the reliability counts are the Calibration's first two rows, and the counts are what `selective` gives on the
    returned map and confidence, byte for byte -- and what the restatement gives."""
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep, SelectiveEvaluator, selective
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
        se, ev, cal = SelectiveEvaluator(lp, images=B, device=DEV), Evaluator(lp, images=B, device=DEV), Calibration(lp, images=B, device=DEV)
        got = call(confidence=True, labels=lab, selective=se, evaluator=ev, calibration=cal)
        assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain)), i
        assert se.used == B and np.array_equal(se.evaluator_counts(), ev.host_counts()) and ev.host_counts().any(), i
        assert np.array_equal(se.reliability_counts(), cal.host_bins()[:, :2]), i
        want = selective(got[0], got[-1], lab, lp)
        assert se.counts.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), i
        assert np.array_equal(se.host_counts(), SR.counts_of_batch(got[0].cpu().numpy(), got[-1].cpu().numpy(), lab.cpu().numpy(), NUM_CLASSES, 15)), i
        alone = SelectiveEvaluator(lp, images=B, device=DEV)
        got = call(confidence=True, labels=lab, selective=alone)               # labels= with a selective evaluator and nothing else
        assert all(torch.equal(a, b) for a, b in zip(got, plain)) and torch.equal(alone.counts, se.counts), i
        assert se.metrics()["aAcc"] == ev.metrics()["aAcc"] == cal.accuracy()
    # per case, into a given confidence buffer
    cc = SelectiveEvaluator(lp, bins=10, cases=["fog", "night"], device=DEV)
    buf = torch.empty(1, 320, 400, device=DEV)
    lab = calls[0][1]
    cm, _, conf = slide(confidence=buf, labels=lab, selective=cc, case="night")
    slide(confidence=buf, labels=lab, selective=cc, case="night")
    one = SR.counts_of_batch(cm.cpu().numpy(), conf.cpu().numpy(), lab.cpu().numpy(), NUM_CLASSES, 10)[0]
    assert conf is buf and np.array_equal(cc.host_counts(), np.stack([np.zeros_like(one), 2 * one]))


def test_slide_runner_with_a_selective_evaluator(models):
    import mmsa.inference as inf
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep, SelectiveEvaluator
    cfg, m, h, frame, x = models
    lp = LabelPrep(NUM_CLASSES)
    lab = _labels(71, 1, 320, 400)
    sr = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2, confidence=True)
    r = sr.run()
    want_map, want_conf = r.outputs()[0].clone(), r.confidence().clone()
    se = SelectiveEvaluator(lp, cases=["clear"], device=DEV)
    r = sr.run(labels=lab, selective=se, case="clear")
    assert torch.equal(r.outputs()[0], want_map) and torch.equal(r.confidence(), want_conf) and int(r.outputs()[1].item()) == 0
    one = SelectiveEvaluator(lp, cases=["clear"]).add(want_map, want_conf, lab, case="clear")
    assert se.counts.cpu().numpy().tobytes() == one.counts.cpu().numpy().tobytes() and int(se.counts.sum()) > 0
    ev, cal = Evaluator(lp, cases=["clear"], device=DEV), Calibration(lp, cases=["clear"], device=DEV)
    sr.run(labels=lab, evaluator=ev, calibration=cal, selective=se, case="clear").outputs()
    assert np.array_equal(se.host_counts(), 2 * one.host_counts())            # twice the counts of one frame, exactly
    assert np.array_equal(se.evaluator_counts(), 2 * ev.host_counts()) and np.array_equal(se.reliability_counts(), 2 * cal.host_bins()[:, :2])
    # refusals: before anything is enqueued
    for kw, msg in ((dict(selective=se), "selective= needs labels="), (dict(labels=lab, selective=se, fused=True), "fused=True / return_map=False"),
                    (dict(labels=lab, selective=se, return_map=False), "fused=True / return_map=False")):
        with pytest.raises(RuntimeError, match=msg):
            sr.run(case="clear", **kw)
    plain = inf.SlideRunner(m, h, frame, (256, 256), (170, 170), chains=2)
    with pytest.raises(RuntimeError, match="SlideRunner.run: selective= needs the confidence map"):
        plain.run(labels=lab, selective=se, case="clear")
    assert np.array_equal(se.host_counts(), 2 * one.host_counts())
