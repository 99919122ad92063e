"""Host side of mmsa.evaluate (no GPU): the numpy restatement (tests/eval_ref.py) against the imported reference's recorded results
(tests/golden/eval_counts.npz, written by tools/oracle/make_golden.py gen_eval), the label LUT, the metrics, the nearest-neighbour tables,
from_pipeline on the reference's test-pipeline shapes, and the one collective of a multi-GPU evaluation on gloo."""
import os

import numpy as np
import pytest
import torch

from tests import eval_ref as ER
from tests import preprocess_ref as PR
from tests import preprocess_resize_ref as RR

VARIANTS = ("plain", "rzl", "map")


def _variant(g, tag):
    return dict(label_map={int(a): int(b) for a, b in g[f"{tag}_label_map"]}, reduce_zero_label=bool(g[f"{tag}_reduce_zero_label"]))


@pytest.mark.parametrize("tag", VARIANTS)
def test_restatement_equals_the_reference_histograms(tag):
    g = ER.load_golden()
    C, kw = int(g["num_classes"]), _variant(g, tag)
    ref = g[f"{tag}_areas"]                       # [3, 4, C] float32, exact integers
    assert np.array_equal(ref, np.round(ref)) and ref.sum() < 2 ** 24
    for b in range(3):
        ours = ER.intersect_and_union(g["pred"][b], g["label"][b], C, int(g["ignore_index"]), **kw)
        assert np.array_equal(np.stack(ours), ref[b].astype(np.int64))
        # ... and the [C + 1, C + 1] layout yields the same four histograms
        conf = ER.confusion(g["pred"][b], g["label"][b], C, int(g["ignore_index"]), **kw)
        assert np.array_equal(np.stack(ER.areas_of(conf)), ref[b].astype(np.int64))
    # the fixture exercises what it is meant to
    assert (g["label"] == 255).any() and (g["label"] == 30).any() and (g["label"] == 0).any() and (g["pred"] == 255).any()


@pytest.mark.parametrize("tag", VARIANTS)
def test_lut_equals_the_reference_bytes(tag):
    from mmsa.evaluate import IGNORE, LabelPrep, label_bytes
    g = ER.load_golden()
    C, kw = int(g["num_classes"]), _variant(g, tag)
    ref = g[f"{tag}_bytes"].astype(np.int64)      # transformed byte per input byte, -1 = ignored
    t, keep = label_bytes(255, **kw)
    assert np.array_equal(np.where(keep, t.astype(np.int64), -1), ref)
    t2, keep2 = ER.transform_bytes(255, **kw)
    assert np.array_equal(t2, t) and np.array_equal(keep2, keep)
    want = np.where(ref < 0, IGNORE, np.minimum(ref, C)).astype(np.uint8)
    assert np.array_equal(LabelPrep(C, ignore_index=255, **kw).lut, want)
    assert np.array_equal(ER.lut(C, 255, **kw), want)
    if tag == "map":                              # chained: 30 -> 3 -> 7 in dict order; 0 -> 255 is then ignored
        assert ref[30] == 7 and ref[3] == 7 and ref[0] == -1
    if tag == "rzl":
        assert ref[0] == -1 and ref[1] == 0 and ref[255] == -1 and ref[254] == 253


@pytest.mark.parametrize("tag", VARIANTS)
@pytest.mark.parametrize("nan", ("nan", "num"))
def test_metrics_against_the_reference(tag, nan):
    """The fixture's totals are below 2^24, so the reference's float32 operands are exact integers and each of its quotients (aAcc, IoU, Acc, Dice,
    Precision, Recall) is ONE float32 rounding of the exact ratio: |ours - ref| <= 2^-24 |ref|.  Its Fscore is formed from the ROUNDED float32
    Precision P and Recall R as fl(fl(2 fl(P R)) / fl(P + R)) (beta = 1; the doublings are exact): relative errors u = 2^-24 each from P, R, the
    product, the sum (which also carries at most u from its operands) and the quotient, (1 + u)^4 / (1 - u)^2 - 1 < 7u against the exact value; ours
    is the float64 evaluation of the exact value.  NaN positions are identical."""
    from mmsa.evaluate import area_metrics, areas_of
    g = ER.load_golden()
    C, kw = int(g["num_classes"]), _variant(g, tag)
    conf = sum(ER.confusion(g["pred"][b], g["label"][b], C, 255, **kw) for b in range(3))
    ours = area_metrics(*areas_of(conf), metric=("mIoU", "mDice", "mFscore"), nan_to_num=None if nan == "nan" else 0, beta=1)
    keys = [k[len(f"{tag}_metrics_{nan}_"):] for k in g.files if k.startswith(f"{tag}_metrics_{nan}_")]
    assert sorted(keys) == sorted(ours) == sorted(["aAcc", "IoU", "Acc", "Dice", "Fscore", "Precision", "Recall"])
    u = 2.0 ** -24
    seen_nan = False
    for k in keys:
        ref = np.asarray(g[f"{tag}_metrics_{nan}_{k}"])
        assert ref.dtype == np.float32
        ref = ref.astype(np.float64)
        got = np.asarray(ours[k], dtype=np.float64)
        assert got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref)), k
        seen_nan |= bool(np.isnan(ref).any())
        ok = ~np.isnan(ref)
        bound = (7 * u if k == "Fscore" else u) * np.abs(ref[ok])
        err = np.abs(got[ok] - ref[ok])
        print(tag, nan, k, "max err / |ref| in units of 2^-24:", float((err / np.maximum(np.abs(ref[ok]), 1e-300)).max() / u) if ok.any() else 0.0)
        assert (err <= bound).all(), k
    assert seen_nan == (nan == "nan")             # class 24 occurs nowhere: 0 / 0
    # the restatement in tests/eval_ref.py is the same function
    mine = ER.total_area_to_metrics(*ER.areas_of(conf), metrics=("mIoU", "mDice", "mFscore"), nan_to_num=None if nan == "nan" else 0)
    for k in keys:
        assert np.array_equal(np.asarray(mine[k]), np.asarray(ours[k]), equal_nan=True)


def test_evaluator_host_side_without_a_buffer():
    from mmsa.evaluate import Evaluator, LabelPrep, summary_of, area_metrics
    ev = Evaluator(LabelPrep(5), cases=["fog", "night"])
    a = ev.areas()
    assert all(x.shape == (2, 5) and x.dtype == np.int64 and not x.any() for x in a)
    assert Evaluator(LabelPrep(5)).areas()[0].shape == (0, 5)
    with pytest.raises(KeyError):
        ev.slots_for(2, case="rain")
    assert ev.slots_for(3, case="night") == [1, 1, 1]
    per = Evaluator(LabelPrep(5), images=3)
    assert per.slots_for(2) == [0, 1] == per.slots_for(2)           # nothing is taken before a launch has gone through
    per._taken(2, None, None)
    assert per.used == 2 and per.slots_for(1) == [2]
    with pytest.raises(RuntimeError, match="per-image slots"):
        per.slots_for(2)
    per._taken(1, None, [0])                                         # slots named outright (or a case) take no per-image slot
    assert per.used == 2
    with pytest.raises(KeyError):
        area_metrics(*[np.ones(3)] * 4, metric=("mAP",))
    # 'microIoU' (the reference's fourth allowed name, metrics_micro.py:484-488) forms the same per-class IoU / Acc as 'mIoU'
    a4 = (np.array([1, 0, 2]), np.array([2, 0, 3]), np.array([1, 0, 3]), np.array([2, 0, 2]))
    mi, mu = area_metrics(*a4, metric="microIoU"), area_metrics(*a4, metric="mIoU")
    assert list(mi) == list(mu) == ["aAcc", "IoU", "Acc"] and all(np.array_equal(mi[k], mu[k], equal_nan=True) for k in mu)
    s = summary_of(area_metrics(np.array([1, 0, 2]), np.array([2, 0, 3]), np.array([1, 0, 3]), np.array([2, 0, 2]), metric="mIoU"))
    assert list(s) == ["aAcc", "mIoU", "mAcc"] and s["aAcc"] == 0.75 and s["mIoU"] == np.round(np.nanmean([0.5, np.nan, 2 / 3]) * 100, 2) / 100


def test_nearest_tables():
    from mmsa.evaluate import nearest_axis_table
    for n_src, n_dst in ((1042, 1024), (1024, 1024), (7, 19), (19, 7), (600, 1080), (1, 5), (5, 1)):
        t = nearest_axis_table(n_src, n_dst)
        assert t.dtype == np.int32 and t.shape == (n_dst,)
        assert t.min() >= 0 and t.max() <= n_src - 1 and (np.diff(t) >= 0).all()
        assert np.array_equal(t, ER.nearest_index(n_src, n_dst))
    assert np.array_equal(nearest_axis_table(1024, 1024), np.arange(1024))
    assert np.array_equal(nearest_axis_table(2048, 1024), 2 * np.arange(1024))          # an exact 2 : 1 reduction keeps the even pixels
    assert np.array_equal(nearest_axis_table(1042, 1024), ER.nearest_index(1042, 1024))


def test_label_prep_geometry():
    from mmsa.evaluate import LabelPrep
    lp = LabelPrep(25, resize=dict(img_scale=(1024, 1024), keep_ratio=True))
    assert lp.resized(1042, 1042) == (1024, 1024) == ER.new_size(1042, 1042, (1024, 1024), True)
    # a non-square keep_ratio case: the largest size inside (long edge 1024, short edge 512)
    lp = LabelPrep(25, resize=dict(seg_scale=(1024, 512), img_scale=(2048, 1024), keep_ratio=True))
    assert lp.resize["scale"] == (1024, 512)                                             # seg_scale wins over the image scale (transform.py:1171-1188)
    assert lp.resized(600, 1100) == ER.new_size(600, 1100, (1024, 512), True) == RR.new_size(600, 1100, (1024, 512), True) == (512, 939)
    assert LabelPrep(25, resize=dict(img_scale=(640, 480), keep_ratio=False)).resized(600, 1100) == (480, 640)
    assert LabelPrep(25).resized(97, 131) == (97, 131)
    with pytest.raises(NotImplementedError):
        LabelPrep(25, resize=dict(img_scale=[(1024, 1024), (512, 512)]))
    with pytest.raises(ValueError):
        LabelPrep(300)


def test_from_pipeline_on_the_reference_pipeline_shapes():
    from mmsa.evaluate import LabelPrep
    cfgs = PR.load_cfgs()
    # DELIVER: Resize_multimodal(img_scale=(1024, 1024), seg_scale=(1024, 1024), keep_ratio=True) in front of MultiScaleFlipAug
    d = LabelPrep.from_pipeline(PR.pipeline_of(cfgs["deliver_rgb_lidar"]), 25)
    assert d.resize == dict(scale=(1024, 1024), keep_ratio=True) and d.resized(1042, 1042) == (1024, 1024)
    d2 = LabelPrep.from_pipeline(RR.pipeline_of(RR.load_cfgs()["deliver_rgb_lidar"]), 25, reduce_zero_label=True)
    assert d2.resize == d.resize and d2.reduce_zero_label and d2.lut[0] == 255
    # FMB: Pad_multimodal in front of it leaves the ground truth alone; MUSES: nothing in front of it
    f = LabelPrep.from_pipeline(PR.pipeline_of(cfgs["fmb_rgb_therm"]), 15)
    assert f.resize is None and f.resized(600, 800) == (600, 800)
    for name in ("muses_rgb_lidar", "muses_rgb_event"):
        m = LabelPrep.from_pipeline(PR.pipeline_of(cfgs[name]), 19)
        assert m.resize is None and m.num_classes == 19
    # refusals, by name
    base = PR.pipeline_of(cfgs["muses_rgb_lidar"])
    for extra in (dict(type="RandomFlip_multimodal", prob=0.5), dict(type="RandomCrop_multimodal", crop_size=(512, 512)), dict(type="Normalize_multimodal")):
        with pytest.raises(NotImplementedError, match=extra["type"]):
            LabelPrep.from_pipeline(base[:1] + [extra] + base[1:], 19)
    with pytest.raises(NotImplementedError, match="MultiScaleFlipAug"):
        LabelPrep.from_pipeline(base[:1], 19)
    rs = dict(type="Resize_multimodal", img_scale=(1920, 1080), keep_ratio=True)
    with pytest.raises(NotImplementedError, match="ratio range"):
        LabelPrep.from_pipeline(base[:1] + [dict(rs, ratio_range=(0.5, 2.0))] + base[1:], 19)
    with pytest.raises(NotImplementedError, match="second Resize_multimodal"):
        LabelPrep.from_pipeline(base[:1] + [rs, rs] + base[1:], 19)


def test_refusals_without_a_gpu():
    from mmsa.evaluate import LabelPrep, confusion
    lp = LabelPrep(25)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        confusion(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), lp)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        lp.check(torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_the_two_entries_are_declared_bound_and_versioned():
    import mmsa
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmsa.h")).read()
    for name in ("mmsa_eval_confusion_u8", "mmsa_slide_argmax_eval"):
        assert name in hdr and name in mmsa.lib.SIGNATURES and hasattr(mmsa.lib.raw, name)
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION >= 106
    assert mmsa.Evaluator is mmsa.evaluate.Evaluator and mmsa.LabelPrep is mmsa.evaluate.LabelPrep and mmsa.confusion is mmsa.evaluate.confusion
    # the library refuses bad arguments on the host, before any launch (no GPU needed): the class limit is named
    import ctypes
    one = (ctypes.c_int * 1)(0)
    fake = ctypes.c_void_p(256)
    rc = mmsa.lib.raw.mmsa_eval_confusion_u8(fake, fake, 1, 4, 4, 4, 4, fake, 127, None, None, one, 1, fake, None)
    assert rc != 0 and "2..126" in mmsa.lib.last_error()
    rc = mmsa.lib.raw.mmsa_eval_confusion_u8(fake, fake, 1, 4, 4, 5, 4, fake, 25, None, None, one, 1, fake, None)
    assert rc != 0 and "size mismatch" in mmsa.lib.last_error()
    one[0] = 3
    rc = mmsa.lib.raw.mmsa_eval_confusion_u8(fake, fake, 1, 4, 4, 4, 4, fake, 25, None, None, one, 2, fake, None)
    assert rc != 0 and "outside the 2 count slots" in mmsa.lib.last_error()


def _allreduce_worker(rk, ws, port, q):
    import torch.distributed as dist
    from mmsa.dist import allreduce_counts
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rk, world_size=ws)
    g = torch.Generator().manual_seed(100 + rk)
    counts = torch.randint(0, 2 ** 40, (3, 26, 26), generator=g, dtype=torch.int64)
    out = allreduce_counts(counts.clone())
    q.put((rk, counts.numpy(), out.numpy()))
    dist.destroy_process_group()


def test_allreduce_counts_gloo_world2():
    import torch.multiprocessing as mp
    from mmsa.dist import allreduce_counts
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29950 + os.getpid() % 300
    procs = [ctx.Process(target=_allreduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    total = res[0][1] + res[1][1]
    assert total.max() > 2 ** 32                  # beyond what a float32 or an int32 sum could hold exactly
    for _, _, out in res:
        assert out.dtype == np.int64 and np.array_equal(out, total)
    # world size 1 (no process group): handed back as it is; anything but int64 is refused
    c = torch.ones(1, 3, 3, dtype=torch.int64)
    assert allreduce_counts(c) is c
    with pytest.raises(ValueError):
        allreduce_counts(torch.ones(1, 3, 3))
