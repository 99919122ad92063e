"""The class-map family against float64 at non-square, non-dyadic windows (tests/class_map_ref.py has the reference, the bound and the case table;
tests/test_class_map_geometry_cpu.py keeps them honest).  Every launch runs twice into sentinel-filled outputs (NaN floats, 77 maps, a zeroed uncovered
word that must stay 0) and must give identical bits; values are held to the bound element by element, maps to the excused-pixel rule, and every one-pass
kernel must equal the canvas path bit for bit where the coordinates are inexact.

Entry point                      reached by (case -> kernel form)
  mmsa_bilinear_accum_nchw       every case: write mode into a NaN canvas, accumulate + count over the windows; second stage at every target
  mmsa_div_count_nchw            every case (overlap 1 / 2 / 4: nonsq; up to 8: ov8)
  mmsa_argmax_nchw, _argmax_max  every case, on the canvas and on the rescaled canvas; argmax_max also on the probabilities (confidence, aug)
  mmsa_slide_argmax              every case; ov8: all eight slots; wide: the second workgroup in x
  mmsa_slide_argmax_conf         C = 5, 33: the LDS-column form; nonsq C = 70: the second-pass form
  mmsa_slide_argmax_eval         every case, with and without a map
  mmsa_slide_argmax_resized      every case x three targets (up, down, mixed with a cut); overlap <= 4: the slot form; ov8: the scanning form
  mmsa_slide_argmax_resized_conf the same
  mmsa_aug_argmax, _conf         aug3 (views nonsq / down / third, flips none / horizontal / vertical) at C = 5: 256 lanes, C = 33: 128 lanes, C = 70: 64 lanes;
                                 aug-ov8: a view in the scanning form"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import class_map_ref as M
from tests import eval_ref as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tab(jobs):
    return (ctypes.c_int * (3 * len(jobs)))(*[v for j in jobs for v in j])


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _twice(launch):
    """launch() -> tuple of freshly sentinel-filled, then written tensors; run twice, identical bits -> the first run's."""
    a, b = launch(), launch()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_bits(x), _bits(y)), f"output {k} differs between two runs of the same launch"
    return a


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _map(*shape):
    return torch.full(shape, 77, dtype=torch.uint8, device=DEV)


def _unc():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _call(name, *args):
    from mmsa import lib, ops
    lib.call(name, *args, ops._stream())


def _accum(src, dst, y0, x0, hc, wc, count=None, accumulate=False):
    """mmsa_bilinear_accum_nchw: src [b, C, hs, ws] -> the window (y0, x0, hc, wc) of dst [b, C, Hd, Wd]."""
    b, C, hs, ws = src.shape
    assert src.is_contiguous() and dst.is_contiguous() and dst.shape[:2] == (b, C)
    _call("mmsa_bilinear_accum_nchw", src.data_ptr(), C * hs * ws, b, C, hs, ws, dst.data_ptr(), dst.shape[2], dst.shape[3], y0, x0, hc, wc,
          count.data_ptr() if count is not None else None, 1 if accumulate else 0)


def _canvas(lg, geo):
    """Accumulate + count over the case's windows, then div_count -> (canvas [B, C, H, W], count [B, H, W])."""
    B, H, W, C = geo["B"], geo["H"], geo["W"], lg.shape[1]

    def launch():
        cv, cnt = torch.zeros(B, C, H, W, device=DEV), torch.zeros(B, H, W, device=DEV)      # inputs of the accumulation, not outputs: no sentinel
        for k, (b, y0, x0) in enumerate(M.jobs_of(geo)):
            _accum(lg[k:k + 1], cv[b:b + 1], y0, x0, geo["hc"], geo["wc"], cnt[b:b + 1], True)
        _call("mmsa_div_count_nchw", cv.data_ptr(), cnt.data_ptr(), B, C, H * W)
        return cv, cnt
    return _twice(launch)


def _second(cv, target):
    """The second resize of the canvas path in write mode into NaN, cut -> contiguous [B, C, Ho, Wo]."""
    if target is None:
        return cv
    Hd, Wd, Ho, Wo = target

    def launch():
        out = _nan(cv.shape[0], cv.shape[1], Hd, Wd)
        _accum(cv, out, 0, 0, Hd, Wd)
        return (out,)
    return _twice(launch)[0][:, :, :Ho, :Wo].contiguous()


def _argmax(x):
    B, C, H, W = x.shape

    def launch():
        a, b, mx = _map(B, H, W), _map(B, H, W), _nan(B, H, W)
        _call("mmsa_argmax_nchw", x.data_ptr(), a.data_ptr(), B, C, H * W)
        _call("mmsa_argmax_max_nchw", x.data_ptr(), b.data_ptr(), mx.data_ptr(), B, C, H * W)
        return a, b, mx
    a, b, mx = _twice(launch)
    assert torch.equal(a, b), "argmax_nchw and argmax_max_nchw name different classes"
    assert torch.equal(_bits(mx), _bits(x.max(1).values)), "argmax_max_nchw: the maximum is not the canvas maximum bit for bit"
    return a, mx


def _softmax_accum(x, acc, flip=0, accumulate=False, finish_div=0):
    B, C, H, W = x.shape
    _call("mmsa_softmax_flip_accum_nchw", x.data_ptr(), acc.data_ptr(), B, C, H, W, flip, 1 if accumulate else 0, finish_div)


def _canvas_conf(y):
    """The canvas path's confidence: the softmax of the logits at the map's size, then argmax_max."""
    prob = _nan(*y.shape)
    _softmax_accum(y, prob)
    return _argmax(prob)[1]


def _one_pass(lg, geo, target, conf):
    """mmsa_slide_argmax[_conf] (target None) or mmsa_slide_argmax_resized[_conf] -> (map, confidence or None)."""
    B, H, W = geo["B"], geo["H"], geo["W"]
    jobs = M.jobs_of(geo)
    Ho, Wo = (H, W) if target is None else target[2:]
    name = ("mmsa_slide_argmax" if target is None else "mmsa_slide_argmax_resized") + ("_conf" if conf else "")

    def launch():
        out, cf, unc = _map(B, Ho, Wo), _nan(B, Ho, Wo), _unc()
        outs = (out.data_ptr(), cf.data_ptr()) if conf else (out.data_ptr(),)
        _call(name, lg.data_ptr(), len(jobs), lg.shape[1], geo["hs"], geo["ws"], _tab(jobs), *outs, B, H, W, geo["hc"], geo["wc"],
              *(() if target is None else target), unc.data_ptr())
        return (out, cf, unc) if conf else (out, unc)
    r = _twice(launch)
    assert int(r[-1].item()) == 0, f"{name}: uncovered pixels counted on a covered frame"
    return r[0], (r[1] if conf else None)


def _inputs(gk, C, ties=False):
    geo = M.GEOS_AUG[gk]
    lg = M.logits_of(f"{gk}-c{C}", geo, C, ties)
    return geo, lg.to(DEV), lg.double().numpy()


@pytest.mark.parametrize("gk,C", M.CASES, ids=M.CASE_IDS)
def test_canvas_kernels(gk, C):
    geo, lg, lg64 = _inputs(gk, C)
    B, H, W, hc, wc = geo["B"], geo["H"], geo["W"], geo["hc"], geo["wc"]

    def launch():      # the first window of every image, written into a window of a larger NaN canvas
        big = _nan(B, C, hc + 5, wc + 9)
        _accum(lg[:B].contiguous(), big, 2, 3, hc, wc)
        return (big,)
    big = _twice(launch)[0].cpu()
    inside = big[:, :, 2:2 + hc, 3:3 + wc]
    outside = big.clone()
    outside[:, :, 2:2 + hc, 3:3 + wc] = float("nan")
    assert bool(outside.isnan().all()), "bilinear_accum wrote outside its window"
    r, b = M.resize(lg64[:B], hc, wc)
    w_ratio = M.check_values(inside.numpy(), r, b, f"{gk}-c{C}: bilinear_accum, write mode")

    cv, cnt = _canvas(lg, geo)
    r, b, n = M.canvas(lg64, geo)
    assert np.array_equal(cnt.cpu().numpy(), n.astype(np.float32)), "the count is not the integer overlap"
    c_ratio = M.check_values(cv.cpu().numpy(), r, b, f"{gk}-c{C}: canvas")
    if gk == M.IDENT:
        assert torch.equal(_bits(cv), _bits(lg)), "ratio 1: the canvas must equal the logits bit for bit"
    m, _ = _argmax(cv)
    excused = M.check_map(m.cpu().numpy(), r, b, f"{gk}-c{C}: argmax_nchw")
    if gk == M.IDENT:
        assert excused == 0 and torch.equal(m.long(), lg.argmax(1))
    print(f"{gk}-c{C}: worst |err| / bound: bilinear_accum (write) {w_ratio:.3f}, canvas {c_ratio:.3f}; overlap up to {int(n.max())}; argmax excused {excused}")


@pytest.mark.parametrize("gk,C", M.CASES, ids=M.CASE_IDS)
def test_one_pass_maps(gk, C):
    from mmsa.evaluate import LabelPrep, slide_argmax_eval
    geo, lg, lg64 = _inputs(gk, C)
    B, H, W = geo["B"], geo["H"], geo["W"]
    cv, _ = _canvas(lg, geo)
    for tgt in geo["targets"]:
        what = f"{gk}-c{C} -> {tgt}"
        r, b = M.frame(lg64, geo, tgt)
        y = _second(cv, tgt)
        v_ratio = M.check_values(y.cpu().numpy(), r, b, f"{what}: canvas path")
        want_map, want_conf = _argmax(y)[0], _canvas_conf(y)
        got_map, _ = _one_pass(lg, geo, tgt, False)
        got_map2, got_conf = _one_pass(lg, geo, tgt, True)
        assert torch.equal(got_map, want_map), f"{what}: the one-pass map differs from the canvas path in {int((got_map != want_map).sum())} pixels"
        assert torch.equal(got_map2, want_map), f"{what}: the _conf kernel's map differs from the canvas path"
        assert torch.equal(_bits(got_conf), _bits(want_conf)), f"{what}: the one-pass confidence is not the canvas path's bit for bit"
        excused = M.check_map(got_map.cpu().numpy(), r, b, f"{what}: one-pass map")
        assert not bool((got_map == 255).any())
        cr, cb = M.confidence(r, b)
        c_ratio = M.check_values(got_conf.cpu().numpy(), cr, cb, f"{what}: confidence")
        if gk == M.IDENT and tgt is None:
            assert excused == 0 and torch.equal(got_map.long(), lg.argmax(1))
        print(f"{what}: worst |err| / bound: logits {v_ratio:.3f}, confidence {c_ratio:.3f}; excused {excused} of {got_map.numel()}")
        if tgt is not None:
            continue
        # mmsa_slide_argmax_eval: the same map, with and without `out`; the counts of tests/eval_ref.py on that map
        label = ER.make_case(7, H, W, C, B=B)[1]
        lab, lp, jobs = torch.from_numpy(label).to(DEV), LabelPrep(C), M.jobs_of(geo)
        want_counts = np.stack([ER.confusion(got_map[i].cpu().numpy(), label[i], C) for i in range(B)])

        def launch(with_map):
            out, unc, counts = _map(B, H, W), _unc(), torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=DEV)
            slide_argmax_eval(lg, len(jobs), _tab(jobs), out if with_map else None, B, H, W, geo["hc"], geo["wc"], unc, lab, lp, counts)
            return out, unc, counts
        out, unc, counts = _twice(lambda: launch(True))
        assert torch.equal(out, got_map) and int(unc.item()) == 0 and np.array_equal(counts.cpu().numpy(), want_counts), f"{what}: slide_argmax_eval"
        out, unc, counts = _twice(lambda: launch(False))
        assert bool((out == 77).all()) and int(unc.item()) == 0 and np.array_equal(counts.cpu().numpy(), want_counts), f"{what}: slide_argmax_eval, no map"


def _view_geo(k):
    """A view's geometry: a key of the case table, or the geometry itself."""
    return k if isinstance(k, dict) else M.GEOS_AUG[k]


def _aug_launch(lgs, ac, conf):
    """mmsa_aug_argmax[_conf] from explicit view rows (w0, n, hs, ws, H, W, hc, wc, Hd, Wd, flip)."""
    Hd, Wd, Ho, Wo = ac["target"]
    rows, table, w0 = [], [], 0
    for lg, (gk, code) in zip(lgs, ac["views"]):
        geo = _view_geo(gk)
        jobs = M.jobs_of(geo)
        rows.append((w0, len(jobs), geo["hs"], geo["ws"], geo["H"], geo["W"], geo["hc"], geo["wc"], Hd, Wd, code))
        table += jobs
        w0 += len(jobs)
    B, A, C = _view_geo(ac["views"][0][0])["B"], len(lgs), lgs[0].shape[1]
    ptrs = (ctypes.c_void_p * A)(*[lg.data_ptr() for lg in lgs])
    crow = (ctypes.c_int * (11 * A))(*[v for r in rows for v in r])
    tab_dev = torch.tensor(table, dtype=torch.int32).view(-1, 3).to(DEV)

    def launch():
        out, cf, unc = _map(B, Ho, Wo), _nan(B, Ho, Wo), _unc()
        outs = (out.data_ptr(), cf.data_ptr()) if conf else (out.data_ptr(),)
        _call("mmsa_aug_argmax" + ("_conf" if conf else ""), ptrs, crow, A, C, tab_dev.data_ptr(), _tab(table), len(table), *outs, B, Ho, Wo, unc.data_ptr())
        return (out, cf, unc) if conf else (out, unc)
    r = _twice(launch)
    assert int(r[-1].item()) == 0
    return r[0], (r[1] if conf else None)


def _aug_canvas(lgs, ac):
    """Per view: canvas, second resize, cut, softmax_flip_accum (the last one divides) -> mean probabilities [B, C, Ho, Wo]."""
    A = len(lgs)

    def launch():
        acc = None
        for a, (lg, (gk, code)) in enumerate(zip(lgs, ac["views"])):
            y = _second(_canvas(lg, _view_geo(gk))[0], ac["target"])
            acc = _nan(*y.shape) if acc is None else acc
            _softmax_accum(y, acc, code, a > 0, A if a == A - 1 else 0)
        return (acc,)
    return _twice(launch)[0]


@pytest.mark.parametrize("ak,C", M.AUG_CASES, ids=M.AUG_IDS)
def test_aug(ak, C):
    ac = M.AUGS[ak]
    lgs = M.aug_logits(ak, C)
    r, b = M.aug([lg.double().numpy() for lg in lgs], ac)
    lgs = [lg.to(DEV) for lg in lgs]
    prob = _aug_canvas(lgs, ac)
    p_ratio = M.check_values(prob.cpu().numpy(), r, b, f"{ak}-c{C}: mean probabilities, canvas path")
    want_map, want_conf = _argmax(prob)
    got_map, _ = _aug_launch(lgs, ac, False)
    got_map2, got_conf = _aug_launch(lgs, ac, True)
    assert torch.equal(got_map, want_map) and torch.equal(got_map2, want_map), f"{ak}-c{C}: aug_argmax differs from the canvas path"
    assert torch.equal(_bits(got_conf), _bits(want_conf)), f"{ak}-c{C}: aug_argmax_conf is not the canvas path's maximum bit for bit"
    excused = M.check_map(got_map.cpu().numpy(), r, b, f"{ak}-c{C}: aug_argmax")
    c_ratio = M.check_values(got_conf.cpu().numpy(), r.max(1), b.max(1), f"{ak}-c{C}: aug_argmax_conf")
    print(f"{ak}-c{C}: worst |err| / bound: mean probabilities {p_ratio:.3f}, confidence {c_ratio:.3f}; excused {excused} of {got_map.numel()}")


@pytest.mark.parametrize("gk", [M.NONSQ, M.OV8])
def test_exact_ties_at_inexact_coordinates(gk):
    """Class 3 is a copy of class 1 and both are the maximum everywhere: class 1 wins in every entry, and both stages of the canvas show the tie bit for bit."""
    from mmsa.evaluate import LabelPrep, slide_argmax_eval
    C = 5
    geo, lg, _ = _inputs(gk, C, ties=True)
    B, H, W = geo["B"], geo["H"], geo["W"]
    cv, _ = _canvas(lg, geo)
    for tgt in geo["targets"]:
        y = _second(cv, tgt)
        assert torch.equal(_bits(y[:, 1]), _bits(y[:, 3])), f"{gk} -> {tgt}: the canvas path does not see the tie"
        maps = [_argmax(y)[0], _one_pass(lg, geo, tgt, False)[0], _one_pass(lg, geo, tgt, True)[0]]
        if tgt is None:
            out, jobs = _map(B, H, W), M.jobs_of(geo)
            slide_argmax_eval(lg, len(jobs), _tab(jobs), out, B, H, W, geo["hc"], geo["wc"], _unc(), torch.zeros(B, H, W, dtype=torch.uint8, device=DEV),
                              LabelPrep(C), torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=DEV))
            maps.append(out)
        for k, m in enumerate(maps):
            assert bool((m == 1).all()), f"{gk} -> {tgt}: entry {k}: {int((m != 1).sum())} pixels do not name the first of the tied classes"
    ak = {M.NONSQ: "aug3-26x37-cut23x31-b2", M.OV8: "aug-ov8-25x41-b1"}[gk]       # the aug case whose first view is this geometry
    ac = M.AUGS[ak]
    lgs = [M.logits_of(f"{ak}-ties-view{a}", M.GEOS_AUG[k], C, ties=True).to(DEV) for a, (k, _) in enumerate(ac["views"])]
    prob = _aug_canvas(lgs, ac)
    assert torch.equal(_bits(prob[:, 1]), _bits(prob[:, 3]))
    for m in (_argmax(prob)[0], _aug_launch(lgs, ac, False)[0], _aug_launch(lgs, ac, True)[0]):
        assert bool((m == 1).all()), f"{ak}: a tied pixel does not name the first class"


# ---- the Python side: MapPlan.slide / MapPlan.whole and the aug view rows with non-square crops and frames, against raw launches with the sizes spelled out

POOL = (4, 2)      # the toy backbone's stride differs per axis, so the logits' (hs, ws) is no multiple of a swapped (ws, hs)


def _toy(C=5):
    w = torch.randn(C, 6, 1, 1, generator=torch.Generator().manual_seed(79)).to(DEV)
    return (lambda im: ([F.avg_pool2d(im, POOL)], None)), (lambda feats: F.conv2d(feats[0], w).contiguous())


def _frame(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 6, H, W, generator=g) + torch.randn(B, 6, 1, 1, generator=g)).to(DEV)


def _raw_geo(B, H, W, crop, wins, stride=None):
    return dict(hs=crop[0] // POOL[0], ws=crop[1] // POOL[1], hc=crop[0], wc=crop[1], H=H, W=W, B=B, wins=tuple(wins), stride=stride)


def _raw_logits(bb, hd, img, geo):
    crops = torch.cat([img[b:b + 1, :, y0:y0 + geo["hc"], x0:x0 + geo["wc"]] for b, y0, x0 in M.jobs_of(geo)], 0).contiguous()
    lg = hd(bb(crops)[0])
    assert lg.shape[2:] == (geo["hs"], geo["ws"])
    return lg


def test_python_entries_on_non_square_crops_and_frames():
    import mmsa.inference as inf
    bb, hd = _toy()
    # slide: 24 x 40 crops (logits 6 x 20) on 40 x 66 frames, stride (16, 26): 2 x 2 windows, overlap 1 / 2 / 4
    B, H, W, crop, stride = 2, 40, 66, (24, 40), (16, 26)
    img = _frame(B, H, W, 5)
    geo = _raw_geo(B, H, W, crop, [(0, 0), (0, 26), (16, 0), (16, 26)])
    assert [(y, x) for y, x, _, _ in inf.crop_boxes(H, W, crop, stride)] == list(geo["wins"])
    lg = _raw_logits(bb, hd, img, geo)
    tc = dict(mode="slide", crop_size=crop, stride=stride)
    for ori in (None, (57, 81), (29, 47), (51, 43)):
        tgt = None if ori is None else ori + ori
        want_map, want_conf = _one_pass(lg, geo, tgt, True)
        for one_pass in ((None,) if ori is None else (True, False)):
            got_map, got_conf = inf.class_map(bb, hd, img, tc, ori_shape=ori, confidence=True, one_pass=one_pass)
            assert torch.equal(got_map, want_map) and torch.equal(_bits(got_conf), _bits(want_conf)), f"slide, ori_shape {ori}, one_pass {one_pass}"
        assert torch.equal(inf.argmax_map(inf.inference(bb, hd, img, tc, ori_shape=ori)), want_map), f"slide logits, ori_shape {ori}"
    # whole / whole_dim / whole_dim_cut: a 28 x 44 frame (logits 7 x 22)
    B, H, W = 2, 28, 44
    img = _frame(B, H, W, 6)
    geo = _raw_geo(B, H, W, (H, W), [(0, 0)])
    lg = _raw_logits(bb, hd, img, geo)
    for tc, ori, tgt in ((dict(mode="whole"), None, None), (dict(mode="whole"), (33, 41, 3), (33, 41, 33, 41)),
                         (dict(mode="whole_dim", dim=(19, 57)), None, (19, 57, 19, 57)),
                         (dict(mode="whole_dim_cut", dim=(37, 30), cut_dim=(25, 31)), None, (37, 30, 31, 25))):
        want_map, want_conf = _one_pass(lg, geo, tgt, True)
        for one_pass in ((None,) if tgt is None else (True, False)):
            got_map, got_conf = inf.class_map(bb, hd, img, tc, ori_shape=ori, confidence=True, one_pass=one_pass)
            assert torch.equal(got_map, want_map) and torch.equal(_bits(got_conf), _bits(want_conf)), f"{tc}, ori_shape {ori}, one_pass {one_pass}"
        assert torch.equal(inf.argmax_map(inf.inference(bb, hd, img, tc, ori_shape=ori))[:, :want_map.shape[1], :want_map.shape[2]], want_map), f"{tc}: logits"
    # aug: three slide views of different sizes (the pipeline resized them), each with its own window grid, flips none / horizontal / vertical
    B, crop, stride, ori = 2, (24, 40), (16, 26), (45, 71)
    sizes, flips = ((40, 66), (32, 52), (24, 92)), (None, "horizontal", "vertical")
    imgs = [_frame(B, h, w, 10 + a) for a, (h, w) in enumerate(sizes)]
    tc = dict(mode="slide", crop_size=crop, stride=stride)
    geos = [_raw_geo(B, h, w, crop, [(y, x) for y, x, _, _ in inf.crop_boxes(h, w, crop, stride)]) for h, w in sizes]
    lgs = [_raw_logits(bb, hd, im, geo) for im, geo in zip(imgs, geos)]
    ac = dict(views=tuple((geo, inf.FLIPS[f]) for geo, f in zip(geos, flips)), target=ori + ori)
    want_map, want_conf = _aug_launch(lgs, ac, True)
    for one_pass in (True, False):
        got_map, unc, got_conf = inf.aug_class_map(bb, hd, imgs, tc, ori_shape=ori, flips=list(flips), one_pass=one_pass, confidence=True)
        assert int(unc.item()) == 0 and torch.equal(got_map, want_map) and torch.equal(_bits(got_conf), _bits(want_conf)), f"aug, one_pass {one_pass}"
