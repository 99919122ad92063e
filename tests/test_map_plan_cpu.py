"""The output geometry of a frame (mmsa.inference.MapPlan) as a literal table: the windows, the size after the second resize, the
size after the cut and the `rs` tuple that chooses the class-map kernel, per entry and mode.  No device: the plan is plain Python.  The expectations are
written out by hand from the reference's rules -- the window grid of encoder_decoder.py:198-212 (windows at the right / bottom border are shifted
inwards), `ori_shape` / `dim` as the size of the second resize (a same-size resize is none), `cut_dim` = (w, h) clamped to the map -- not computed from
the plan."""
import pytest

# slide geometries: (H, W), crop, stride, B -> n, first job, last job (b, y0, x0)
#   90 x 150 / 64 / 40: rows at 0 and 40 -> 26 (shifted to end at 90), columns at 0, 40, 80 and 120 -> 86; two images, the image index runs fastest
#   70 x 70 / 64 / 64: rows and columns at 0 and 64 -> 6
#   90 x 150 / 64 / (32, 24): rows at 0 and 32 -> 26, columns at 0, 24, 48, 72 and 96 -> 86; column 86 lies under 4 windows, times 2 rows = 8: accepted
#   1080 x 1920 / 1024 / 640, the benchmark's frame: rows at 0 and 640 -> 56, columns at 0, 640 and 1280 -> 896: six windows
SLIDE = [
    ((90, 150), (64, 64), (40, 40), 2, 16, (0, 0, 0), (1, 26, 86)),
    ((70, 70), (64, 64), (64, 64), 1, 4, (0, 0, 0), (0, 6, 6)),
    ((90, 150), (64, 64), (32, 24), 1, 10, (0, 0, 0), (0, 26, 86)),
    ((1080, 1920), (1024, 1024), (640, 640), 1, 6, (0, 0, 0), (0, 56, 896)),
]
OTHER = (77, 131, 3)     # an `ori_shape` that is no frame's own size


@pytest.mark.parametrize("hw,crop,stride,B,n,first,last", SLIDE)
def test_slide_geometries(hw, crop, stride, B, n, first, last):
    from mmsa.inference import MapPlan
    H, W = hw
    for ori, sizes, rs in ((None, (H, W, H, W), None), ((H, W, 3), (H, W, H, W), None), (OTHER, (77, 131, 77, 131), (77, 131, 77, 131))):
        p = MapPlan.slide(B, H, W, crop, stride, ori_shape=ori)
        p.check_windows("slide_class_map")
        assert (p.B, p.H, p.W, p.hc, p.wc) == (B, H, W) + crop
        assert (p.n, p.jobs[0], p.jobs[-1]) == (n, first, last) and len(p.jobs) == n
        assert (p.Hd, p.Wd, p.Ho, p.Wo) == sizes and p.rs == rs and p.rescaled == (rs is not None)
        assert list(p.tab) == [v for job in p.jobs for v in job] and p.tab is p.tab           # built once and kept
    if B == 2:      # the accumulation order of slide_inference: window by window, the images of a window one after the other
        assert p.jobs[:4] == ((0, 0, 0), (1, 0, 0), (0, 0, 40), (1, 0, 40))


def test_whole_geometries():
    from mmsa.inference import MapPlan
    H, W = 64, 88
    table = [   # keywords -> (Hd, Wd, Ho, Wo), rs
        (dict(), (64, 88, 64, 88), None),
        (dict(ori_shape=(96, 120, 3)), (96, 120, 96, 120), (96, 120, 96, 120)),                     # 'whole' with rescale
        (dict(ori_shape=(96, 120, 3), rescale=False), (64, 88, 64, 88), None),
        (dict(dim=(40, 50)), (40, 50, 40, 50), (40, 50, 40, 50)),                                   # 'whole_dim'
        (dict(dim=(40, 50), cut_dim=(30, 20)), (40, 50, 20, 30), (40, 50, 20, 30)),                 # 'whole_dim_cut': cut_dim is (w, h)
        (dict(dim=(40, 50), cut_dim=(30, 20), rescale=False), (64, 88, 20, 30), (64, 88, 20, 30)),  # ... the cut of the map at the input size
        (dict(dim=(40, 50), cut_dim=(400, 400)), (40, 50, 40, 50), (40, 50, 40, 50)),               # a cut larger than the map is clamped
        (dict(dim=(40, 50), cut_dim=(400, 400), rescale=False), (64, 88, 64, 88), None),            # ... and then cuts nothing
        (dict(dim=(64, 88)), (64, 88, 64, 88), None),                                               # dim equal to the input, no cut
        (dict(dim=(64, 88), cut_dim=(88, 60)), (64, 88, 60, 88), (64, 88, 60, 88)),
    ]
    for kw, sizes, rs in table:
        p = MapPlan.whole(2, H, W, **kw)
        assert (p.B, p.H, p.W, p.hc, p.wc) == (2, 64, 88, 64, 88), kw
        assert (p.n, p.jobs) == (2, ((0, 0, 0), (1, 0, 0))) and list(p.tab) == [0, 0, 0, 1, 0, 0], kw      # one full-size window per image
        assert (p.Hd, p.Wd, p.Ho, p.Wo) == sizes and p.rs == rs and p.rescaled == (rs is not None), kw


def test_refusals():
    from mmsa.inference import MapPlan, _check_overlap, crop_boxes
    with pytest.raises(RuntimeError, match="at least as large as the crop"):
        MapPlan.slide(1, 60, 150, (64, 64), (40, 40))
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner: the image must be at least as large as the crop"):
        MapPlan.slide(1, 90, 63, (64, 64), (40, 40), what="SlideRunner")
    # 512 x 576 in 64 x 64 windows side by side: 8 x 9 = 72 windows, none overlapping
    many = MapPlan.slide(1, 512, 576, (64, 64), (64, 64))
    assert many.n == 72
    with pytest.raises(RuntimeError, match="at most 64 windows per call"):
        many.check_windows("slide_class_map")
    with pytest.raises(RuntimeError, match="mmsa.SlideRunner: at most 64 windows per frame batch"):
        many.check_windows("SlideRunner", per="frame batch")
    # stride (32, 16): columns at 0, 16, 32, 48, 64, 80 and 96 -> 86; column 86 lies under the windows at 32, 48, 64, 80 and 86, times 2 rows = 10
    deep = MapPlan.slide(1, 90, 150, (64, 64), (32, 16))
    for check in (lambda: deep.check_windows("slide_class_map"), lambda: _check_overlap(crop_boxes(90, 150, (64, 64), (32, 16)), "slide_class_map")):
        with pytest.raises(RuntimeError, match="covers some pixels 10 times, the one-pass class-map kernel handles up to 8"):
            check()
    # ... which slide_inference's plan never asks
    assert deep.n == 14 and many.rs is None
    with pytest.raises(RuntimeError, match="comes with dim"):
        MapPlan.whole(2, 64, 88, cut_dim=(30, 20))
    with pytest.raises(RuntimeError, match="give one of them"):
        MapPlan.whole(2, 64, 88, dim=(40, 50), ori_shape=(40, 50))
    with pytest.raises(RuntimeError, match="no defined result"):
        MapPlan.whole(2, 64, 88, dim=(40, 50), rescale=False)
    for bad in (lambda: MapPlan.whole(2, 64, 88, ori_shape=(0, 50)), lambda: MapPlan.whole(2, 64, 88, dim=(40,)),
                lambda: MapPlan.slide(1, 90, 150, (64, 64), (40, 40), ori_shape=(77, 0, 3))):
        with pytest.raises(RuntimeError, match="the rescale target must be"):
            bad()
    with pytest.raises(RuntimeError, match="leaves nothing of the map"):
        MapPlan.whole(2, 64, 88, dim=(40, 50), cut_dim=(0, 20))


def test_plan_is_immutable():
    import dataclasses
    from mmsa.inference import MapPlan
    p = MapPlan.whole(1, 64, 88)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.H = 65


# ---- which library entry a plan's class_map calls, and with which arguments, as a literal table: mmsa.lib.call is recorded, nothing runs.  Logits
# [1, 5, 2, 2] of one full-size 8 x 8 window; the rescaled plan ends at 12 x 10.  `tail`: what stands between the uncovered-pixel word and the stream --
# nothing, the inverse temperature of the `_t` entries, or (kind, inverse temperature, 1 / log C) of the `_score` entries (1.0 where no temperature is given).
def _dispatch_options():
    from mmsa.evaluate import inv_log_classes, inv_temperature
    it, ilc = inv_temperature(2.0), inv_log_classes(5)
    return [    # keywords besides conf=, takes conf, suffix of the entry's name, tail
        (dict(), False, "", ()),
        (dict(), True, "_conf", ()),
        (dict(temperature=2.0), True, "_conf_t", (it,)),
        (dict(score="margin"), True, "_score", (1, 1.0, ilc)),
        (dict(score="entropy", temperature=2.0), True, "_score", (2, it, ilc)),
    ]


def _dispatched(monkeypatch, plan, kw, with_conf):
    """The (name, args) of every mmsa.lib.call that plan.class_map(...) makes on CPU tensors, and the tensors."""
    import torch
    from mmsa import lib, ops
    calls = []
    lg = torch.zeros(plan.n, 5, 2, 2)
    out = torch.zeros(plan.B, plan.Ho, plan.Wo, dtype=torch.uint8)
    unc = torch.zeros(1, dtype=torch.int32)
    conf = torch.zeros(plan.B, plan.Ho, plan.Wo) if with_conf else None
    with monkeypatch.context() as mp:
        mp.setattr(lib, "call", lambda name, *args: calls.append((name, args)))
        mp.setattr(ops, "_stream", lambda: None)
        plan.class_map(lg, out, unc, conf=conf, **kw)
    return calls, lg, out, unc, conf


def test_class_map_dispatch_at_frame_size(monkeypatch):
    from mmsa.inference import MapPlan
    plan = MapPlan.whole(1, 8, 8)
    for kw, with_conf, suffix, tail in _dispatch_options():
        calls, lg, out, unc, conf = _dispatched(monkeypatch, plan, kw, with_conf)
        assert len(calls) == 1, (kw, calls)
        name, args = calls[0]
        outs = (out.data_ptr(), conf.data_ptr()) if with_conf else (out.data_ptr(),)
        assert name == "mmsa_slide_argmax" + suffix, kw
        assert args == (lg.data_ptr(), 1, 5, 2, 2, plan.tab) + outs + (1, 8, 8, 8, 8, unc.data_ptr()) + tail + (None,), (kw, args)
        assert len(args) == 14 + with_conf + len(tail)       # no (Hd, Wd, Ho, Wo), and no scalar the entry does not take


def test_class_map_dispatch_at_a_rescaled_size(monkeypatch):
    from mmsa.inference import MapPlan
    plan = MapPlan.whole(1, 8, 8, ori_shape=(12, 10))
    for kw, with_conf, suffix, tail in _dispatch_options():
        for one_pass in (True,) if "score" in kw else (True, None):      # None follows ONE_PASS_RESCALE_DEFAULT: one pass; with a score the default is the canvas path (a device)
            calls, lg, out, unc, conf = _dispatched(monkeypatch, plan, dict(kw, one_pass=one_pass), with_conf)
            assert len(calls) == 1, (kw, one_pass, calls)
            name, args = calls[0]
            outs = (out.data_ptr(), conf.data_ptr()) if with_conf else (out.data_ptr(),)
            assert name == "mmsa_slide_argmax_resized" + suffix, (kw, one_pass)
            assert args == (lg.data_ptr(), 1, 5, 2, 2, plan.tab) + outs + (1, 8, 8, 8, 8, 12, 10, 12, 10, unc.data_ptr()) + tail + (None,), (kw, one_pass, args)
            assert len(args) == 18 + with_conf + len(tail)
