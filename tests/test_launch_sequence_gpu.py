"""The launches the class-map and logits entries of mmsa.inference make once the head has returned, as literal lists: the names of the library's entries
in call order, with the `torch.empty` / `torch.zeros` calls of the glue between them.  The lists are those of the commit before `MapPlan` (the glue then
spelled the frame geometry out in every entry): same kernels, same order, same count, same allocations is the evidence that moving the geometry into one
record changed no launch.  They were written down by reading that commit's mmsa/inference.py, evaluate.py and render.py call by call, NOT by running
this recorder there: no MI355X could be had while the change was made, and this test has not run on one yet.  Tiny backbone + head_tiny, the 320 x 400 frame with 256 x 256 windows at stride 170 (four
windows, one encoder batch, so the head returns once) and two 256 x 256 whole frames."""
import numpy as np
import pytest
import torch

from tests.configs import CONFIGS, HEAD_CONFIGS, make_input
from tests.weights import seeded_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CROP, STRIDE, ORI = (256, 256), (170, 170), (300, 380, 3)
MAP = ["torch.empty", "torch.zeros"]                                                  # the map buffer and the uncovered-pixel word of a class-map call
RESIZE = ["torch.empty", "mmsa_bilinear_accum_nchw"]                                  # a canvas and the resize that writes it
CANVAS = ["torch.zeros", "torch.zeros"] + 4 * ["mmsa_bilinear_accum_nchw"] + ["mmsa_div_count_nchw"]   # canvas and count, one accumulating resize per window, the division

EXPECTED = {
    "slide_plain": MAP + ["mmsa_slide_argmax"],
    "slide_ori": MAP + ["mmsa_slide_argmax_resized"],
    "slide_ori_canvas": MAP + CANVAS + RESIZE + ["torch.empty", "mmsa_argmax_nchw"],      # the canvas path: slide_inference's launches, then argmax_map's
    "slide_labels_fused": MAP + ["mmsa_slide_argmax_eval"],
    "slide_labels_two_launches": MAP + ["mmsa_slide_argmax", "mmsa_eval_confusion_u8"],
    "slide_render": MAP + ["mmsa_slide_argmax", "torch.empty", "mmsa_render_denorm_f32"],   # the picture buffer and the launch that paints it
    "whole_plain": MAP + ["mmsa_slide_argmax"],
    "whole_ori": MAP + ["mmsa_slide_argmax_resized"],
    "whole_dim": MAP + ["mmsa_slide_argmax_resized"],
    "whole_dim_cut": MAP + ["mmsa_slide_argmax_resized"],
    "whole_dim_cut_no_rescale": MAP + ["mmsa_slide_argmax_resized"],
    "slide_inference_ori": CANVAS + RESIZE,
    "whole_inference_dim_cut": RESIZE + RESIZE,                                          # encode_decode's resize to the input size, then the one to `dim`
}


def _models():
    import mmsa
    cfg, hcfg = CONFIGS["tiny256"], HEAD_CONFIGS["head_tiny"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]))
    h = mmsa.build_head(dict(type="SegformerHead", **hcfg["kwargs"]))
    h.load_state_dict(seeded_state_dict(h, seed=hcfg["seed"]))
    h = h.to(DEV)
    frame = torch.randn(1, 6, 320, 400, generator=torch.Generator().manual_seed(9)).to(DEV)
    x = make_input(cfg, batch=2, seed=17).to(DEV)
    return hcfg["kwargs"]["num_classes"], m, h, frame, x


@pytest.fixture(scope="module")
def models():
    return _models()


def _calls(models):
    """name -> the public call of that case, as a function of nothing."""
    import mmsa.inference as inf
    from mmsa.evaluate import Evaluator, LabelPrep
    from mmsa.preprocess import Preprocess
    from mmsa.render import Renderer
    C, m, h, frame, x = models
    lp = LabelPrep(C)
    lab = torch.randint(0, C, (1, 320, 400), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    lp.lut_on(torch.device(DEV))                                   # the one upload of a LabelPrep: made here, outside the recorded calls
    r = Renderer(np.arange(3 * C).reshape(C, 3) % 256, opacity=0.5,
                 preprocess=Preprocess(mean=[0.485, 0.456, 0.406, 0, 0, 0], std=[0.229, 0.224, 0.225, 1, 1, 1], to_rgb=[True, True],
                                       modalities_name=["rgb", "lidar"], modalities_ch=[3, 3], norm_by_max=True))
    r.palette_on(torch.device(DEV))
    ev = lambda: Evaluator(lp, images=1, device=DEV)
    slide = lambda **kw: inf.slide_class_map(m, h, frame, CROP, STRIDE, **kw)
    whole = lambda **kw: inf.whole_class_map(m, h, x, **kw)
    return dict(
        slide_plain=lambda: slide(),
        slide_ori=lambda: slide(ori_shape=ORI),
        slide_ori_canvas=lambda: slide(ori_shape=ORI, one_pass=False),
        slide_labels_fused=lambda: slide(labels=lab, evaluator=ev(), fused=True),
        slide_labels_two_launches=lambda: slide(labels=lab, evaluator=ev(), fused=False),
        slide_render=lambda: slide(render=r),
        whole_plain=lambda: whole(),
        whole_ori=lambda: whole(ori_shape=(200, 310)),
        whole_dim=lambda: whole(dim=(192, 240)),
        whole_dim_cut=lambda: whole(dim=(200, 300), cut_dim=(260, 150)),
        whole_dim_cut_no_rescale=lambda: whole(dim=(192, 256), cut_dim=(256, 192), rescale=False),
        slide_inference_ori=lambda: inf.slide_inference(m, h, frame, CROP, STRIDE, ori_shape=ORI),
        whole_inference_dim_cut=lambda: inf.whole_inference_dim_cut(m, h, x, (200, 300), (260, 150)),
    )


def _recorded(monkeypatch, head, fn):
    """The names of the library entries and allocations `fn` makes after its last head call; `head` None: a call at plan level, all it makes."""
    from mmsa import lib
    names = []
    real_call, real_forward = lib.call, getattr(head, "forward", None)

    def call(name, *args):
        names.append(name)
        return real_call(name, *args)

    def forward(*args, **kw):
        out = real_forward(*args, **kw)
        names.append("<head>")
        return out

    def allocator(name):
        real = getattr(torch, name)

        def alloc(*args, **kw):
            names.append(f"torch.{name}")
            return real(*args, **kw)
        return alloc

    with monkeypatch.context() as mp:
        mp.setattr(lib, "call", call)
        if head is not None:
            mp.setattr(head, "forward", forward)
        for name in ("empty", "zeros"):
            mp.setattr(torch, name, allocator(name))
        fn()
    torch.cuda.synchronize()
    if head is None:
        return names
    assert names.count("<head>") == 1, "one encoder batch per case"
    return names[names.index("<head>") + 1:]


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_launches_after_the_head(models, monkeypatch, case):
    got = _recorded(monkeypatch, models[2], _calls(models)[case])
    print(f"{case}: {got}")
    assert got == EXPECTED[case]


def test_every_case_has_a_list(models):
    assert sorted(_calls(models)) == sorted(EXPECTED)


# ---- the same recorder at plan level: MapPlan.class_map / AugPlan.class_map on random head-resolution logits, without backbone or head, so the record is
# the WHOLE call.  Which launch a plan takes for every combination of conf / temperature / score / labels / evaluator / calibration / selective / return_map /
# one_pass, written out by reading mmsa/inference.py and evaluate.py at the commit before the option record and the launch table, and confirmed by running
# this file on that commit (an MI355X: every case passed there before the code was touched).  The 40 x 56 frame in
# 32 x 32 windows at stride 24 (four windows), at its own size and rescaled to 30 x 50; five classes, logits [4, 5, 8, 8].
P_CANVAS = CANVAS                                                                      # canvas and count, four accumulating resizes, the division
P_CANVAS_MAP = CANVAS + RESIZE + ["torch.empty", "mmsa_argmax_nchw"]                   # ... the second resize, argmax_map
PLAN_EXPECTED = {
    "conf_canvas": P_CANVAS_MAP + ["mmsa_softmax_flip_accum_nchw", "mmsa_argmax_max_nchw"],
    "conf_t_canvas": P_CANVAS_MAP + ["mmsa_softmax_flip_accum_nchw_t", "mmsa_argmax_max_nchw"],
    "margin_rescaled_default": P_CANVAS_MAP + ["mmsa_softmax_flip_accum_nchw", "mmsa_argmax_score_nchw"],      # ONE_PASS_SCORE_RESCALE_DEFAULT: the canvas path
    "margin_rescaled_one_pass": ["mmsa_slide_argmax_resized_score"],
    "conf_rescaled_default": ["mmsa_slide_argmax_resized_conf"],                                               # ONE_PASS_RESCALE_DEFAULT: one pass
    "conf_t_rescaled_labels": ["mmsa_slide_argmax_resized_conf_t", "mmsa_eval_confusion_u8", "mmsa_eval_calibration", "mmsa_eval_selective"],
    "labels_evaluator_conf": ["mmsa_slide_argmax_conf", "mmsa_eval_confusion_u8"],                             # never the fused launch
    "labels_evaluator_conf_fused_none": ["mmsa_slide_argmax_conf", "mmsa_eval_confusion_u8"],
    "labels_binned_no_evaluator": ["mmsa_slide_argmax_conf", "mmsa_eval_calibration", "mmsa_eval_selective"],
    "labels_all_three_entropy_t": ["mmsa_slide_argmax_score", "mmsa_eval_confusion_u8", "mmsa_eval_calibration", "mmsa_eval_selective"],
    "labels_evaluator_no_map": ["mmsa_slide_argmax_eval"],                                                    # the fused launch alone
    "labels_evaluator_two_launches": ["mmsa_slide_argmax", "mmsa_eval_confusion_u8"],
    "labels_evaluator_rescaled": ["mmsa_slide_argmax_resized", "mmsa_eval_confusion_u8"],                      # a rescaled plan counts through the stored map
    "aug_conf": 2 * (P_CANVAS + ["mmsa_softmax_flip_accum_nchw"]) + ["mmsa_argmax_max_nchw"],
    "aug_entropy": 2 * (P_CANVAS + RESIZE + ["mmsa_softmax_flip_accum_nchw"]) + ["mmsa_argmax_score_nchw"],     # its views are rescaled to 30 x 50
    "aug_plain": 2 * (P_CANVAS + ["mmsa_softmax_flip_accum_nchw"]) + ["torch.empty", "mmsa_argmax_nchw"],
}


@pytest.fixture(scope="module")
def plan_calls():
    """name -> the plan-level call of that case; everything a first call uploads or allocates is on the device before any of them is recorded."""
    from mmsa.evaluate import Calibration, Evaluator, LabelPrep, SelectiveEvaluator
    from mmsa.inference import AugPlan, MapPlan
    g = torch.Generator().manual_seed(11)
    C, lp = 5, LabelPrep(5)
    lp.lut_on(torch.device(DEV))
    lg = torch.randn(4, C, 8, 8, generator=g).to(DEV)
    lg2 = torch.randn(4, C, 8, 8, generator=g).to(DEV)
    plans = {None: MapPlan.slide(1, 40, 56, (32, 32), (24, 24)), "ori": MapPlan.slide(1, 40, 56, (32, 32), (24, 24), ori_shape=(30, 50))}
    labs = {k: torch.randint(0, C, (1, p.Ho, p.Wo), generator=g, dtype=torch.uint8).to(DEV) for k, p in plans.items()}
    cfg = dict(mode="slide", crop_size=(32, 32), stride=(24, 24))
    augs = {k: AugPlan.make(cfg, [(1, 40, 56)] * 2, [None, "horizontal"], ori_shape=o) for k, o in ((None, None), ("ori", (30, 50)))}
    ev, cal, sel = (cls(lp, images=64, device=DEV) for cls in (Evaluator, Calibration, SelectiveEvaluator))

    def run(key=None, conf=True, aug=False, **kw):
        plan = (augs if aug else plans)[key]
        B, Ho, Wo = plan.size if aug else (plan.B, plan.Ho, plan.Wo)
        out = torch.empty(B, Ho, Wo, dtype=torch.uint8, device=DEV)
        unc = torch.zeros(1, dtype=torch.int32, device=DEV)
        cf = torch.empty(B, Ho, Wo, dtype=torch.float32, device=DEV) if conf else None
        if "labels" in kw:
            kw["labels"] = labs[key]

        return lambda: plan.class_map([lg, lg2] if aug else lg, out, unc, conf=cf, **kw)

    return dict(
        conf_canvas=run("ori", one_pass=False),
        conf_t_canvas=run("ori", one_pass=False, temperature=1.7),
        margin_rescaled_default=run("ori", score="margin"),
        margin_rescaled_one_pass=run("ori", score="margin", one_pass=True),
        conf_rescaled_default=run("ori"),
        conf_t_rescaled_labels=run("ori", temperature=1.7, labels=True, evaluator=ev, calibration=cal, selective=sel),
        labels_evaluator_conf=run(labels=True, evaluator=ev, fused=False),
        labels_evaluator_conf_fused_none=run(labels=True, evaluator=ev),
        labels_binned_no_evaluator=run(labels=True, calibration=cal, selective=sel),
        labels_all_three_entropy_t=run(score="entropy", temperature=1.7, labels=True, evaluator=ev, calibration=cal, selective=sel),
        labels_evaluator_no_map=run(conf=False, labels=True, evaluator=ev, return_map=False),
        labels_evaluator_two_launches=run(conf=False, labels=True, evaluator=ev, fused=False),
        labels_evaluator_rescaled=run("ori", conf=False, labels=True, evaluator=ev),
        aug_conf=run(aug=True),
        aug_entropy=run("ori", aug=True, score="entropy"),
        aug_plain=run(aug=True, conf=False),
    )


@pytest.mark.parametrize("case", sorted(PLAN_EXPECTED))
def test_launches_of_a_plan(plan_calls, monkeypatch, case):
    got = _recorded(monkeypatch, None, plan_calls[case])
    print(f"{case}: {got}")
    assert got == PLAN_EXPECTED[case]


def test_every_plan_case_has_a_list(plan_calls):
    assert sorted(plan_calls) == sorted(PLAN_EXPECTED)


# ---- the same recorder on the count passes of mmsa.evaluate, at entry and at owner level: every entry that adds into an int64 [n_slots, ...] buffer, and the
# add() of every owner of such a buffer.  The lists were written by reading mmsa/evaluate.py at the commit before the shared launch preamble and the shared
# add(), and confirmed by running this file on that commit (an MI355X: every case passed there before the code was touched).  Five classes, two 24 x 40 maps,
# the labels 12 x 20 and read through the resize tables; 4 bins, 3 temperatures, 3 rank planes, Chebyshev radius 2, Euclidean radius 2 at cap 4.
D = "mmsa_boundary_distance_u8"
EVAL_ENTRIES = {                                       # entry -> the library call it makes
    "confusion": "mmsa_eval_confusion_u8",
    "calibration": "mmsa_eval_calibration",
    "selective": "mmsa_eval_selective",
    "temperature_sweep": "mmsa_temperature_sweep_nchw",
    "topk_counts": "mmsa_eval_topk_u8",
    "boundary_counts": "mmsa_eval_boundary_u8",
    "boundary_counts_d2": "mmsa_eval_boundary_d2",
    "boundary_displacement": "mmsa_eval_boundary_displacement",
}
EVAL_EXPECTED = {
    "confusion": ["torch.zeros", "mmsa_eval_confusion_u8"],
    "confusion_buffer": ["mmsa_eval_confusion_u8"],
    "calibration": ["torch.zeros", "mmsa_eval_calibration"],
    "calibration_buffer": ["mmsa_eval_calibration"],
    "selective": ["torch.zeros", "mmsa_eval_selective"],
    "selective_buffer": ["mmsa_eval_selective"],
    "temperature_sweep": ["torch.zeros", "mmsa_temperature_sweep_nchw"],
    "temperature_sweep_buffer": ["mmsa_temperature_sweep_nchw"],
    "topk_counts": ["torch.zeros", "mmsa_eval_topk_u8"],
    "topk_counts_buffer": ["mmsa_eval_topk_u8"],
    "boundary_counts": ["torch.zeros", "mmsa_eval_boundary_u8"],
    "boundary_counts_buffer": ["mmsa_eval_boundary_u8"],
    "boundary_counts_d2": ["torch.zeros", "mmsa_eval_boundary_d2"],
    "boundary_counts_d2_buffer": ["mmsa_eval_boundary_d2"],
    "boundary_displacement": ["torch.zeros", "mmsa_eval_boundary_displacement"],
    "boundary_displacement_buffer": ["mmsa_eval_boundary_displacement"],
    "boundary_distance": ["torch.empty", D],                                            # the map; the scratch plane of the stream exists
    "boundary_distance_buffers": [D],
}
OWNER_EXPECTED = {                                     # owner -> what a warm add() records; the first add of an owner made without device= has "torch.zeros" in front
    "Evaluator": ["mmsa_eval_confusion_u8"],
    "Calibration": ["mmsa_eval_calibration"],
    "SelectiveEvaluator": ["mmsa_eval_selective"],
    "TemperatureSweep": ["mmsa_temperature_sweep_nchw"],
    "TopKEvaluator": ["mmsa_eval_topk_u8"],
    "BoundaryEvaluator": ["mmsa_eval_boundary_u8"],
}
EUCLIDEAN_EXPECTED = {
    "first": 3 * ["torch.empty"] + [D, D, "mmsa_eval_boundary_d2", "mmsa_eval_boundary_displacement"],      # the distance maps and the scratch of a shape
    "second": [D, D, "mmsa_eval_boundary_d2", "mmsa_eval_boundary_displacement"],
    "first_no_device": 2 * ["torch.zeros"] + 3 * ["torch.empty"] + [D, D, "mmsa_eval_boundary_d2", "mmsa_eval_boundary_displacement"],
    "first_no_displacement": 3 * ["torch.empty"] + [D, D, "mmsa_eval_boundary_d2"],
    "first_no_device_no_displacement": ["torch.zeros"] + 3 * ["torch.empty"] + [D, D, "mmsa_eval_boundary_d2"],
    "second_no_displacement": [D, D, "mmsa_eval_boundary_d2"],
}


@pytest.fixture(scope="module")
def count_inputs():
    """The maps of the count cases, with everything a first call uploads (the label LUT, the label tables, both code LUTs) and the scratch plane of the
    distance launch on the device before anything is recorded: one warm call per entry."""
    import mmsa.evaluate as E
    g = torch.Generator().manual_seed(23)
    C = 5
    lp = E.LabelPrep(C, resize=dict(seg_scale=(40, 24), keep_ratio=False))
    pred = torch.randint(0, C, (2, 24, 40), generator=g, dtype=torch.uint8).to(DEV)
    lab = torch.randint(0, C + 1, (2, 12, 20), generator=g, dtype=torch.uint8)
    lab[torch.rand(2, 12, 20, generator=g) < 0.1] = 255
    lab = lab.to(DEV)
    conf = torch.rand(2, 24, 40, generator=g).to(DEV)
    logits = torch.randn(2, C, 24, 40, generator=g).to(DEV)
    planes = torch.randint(0, C, (3, 2, 24, 40), generator=g, dtype=torch.uint8).to(DEV)
    d2p = E.boundary_distance(pred, 4, num_classes=C)
    d2l = E.boundary_distance(lab, 4, labels_prep=lp, size=(24, 40))
    calls = dict(
        confusion=lambda buf=None, slots=None: E.confusion(pred, lab, lp, counts=buf, slots=slots),
        calibration=lambda buf=None, slots=None: E.calibration(pred, conf, lab, lp, bins=4, cal=buf, slots=slots),
        selective=lambda buf=None, slots=None: E.selective(pred, conf, lab, lp, bins=4, counts=buf, slots=slots),
        temperature_sweep=lambda buf=None, slots=None: E.temperature_sweep(logits, lab, lp, (0.5, 1, 2), bins=4, out=buf, slots=slots),
        topk_counts=lambda buf=None, slots=None: E.topk_counts(planes, lab, lp, counts=buf, slots=slots),
        boundary_counts=lambda buf=None, slots=None: E.boundary_counts(pred, lab, lp, 2, counts=buf, slots=slots),
        boundary_counts_d2=lambda buf=None, slots=None: E.boundary_counts_d2(pred, lab, lp, d2p, d2l, 4, counts=buf, slots=slots),
        boundary_displacement=lambda buf=None, slots=None: E.boundary_displacement(pred, lab, lp, d2p, d2l, 4, hist=buf, slots=slots),
    )
    for fn in calls.values():
        fn()
    owners = dict(
        Evaluator=(lambda **kw: E.Evaluator(lp, **kw), (pred, lab)),
        Calibration=(lambda **kw: E.Calibration(lp, bins=4, **kw), (pred, conf, lab)),
        SelectiveEvaluator=(lambda **kw: E.SelectiveEvaluator(lp, bins=4, **kw), (pred, conf, lab)),
        TemperatureSweep=(lambda **kw: E.TemperatureSweep(lp, (0.5, 1, 2), bins=4, **kw), (logits, lab)),
        TopKEvaluator=(lambda **kw: E.TopKEvaluator(lp, 3, **kw), (planes, lab)),
        BoundaryEvaluator=(lambda **kw: E.BoundaryEvaluator(lp, 2, **kw), (pred, lab)),
        EuclideanBoundaryEvaluator=(lambda **kw: E.EuclideanBoundaryEvaluator(lp, 2, cap=4, **kw), (pred, lab)),
    )
    torch.cuda.synchronize()
    return dict(E=E, C=C, lp=lp, pred=pred, lab=lab, calls=calls, owners=owners)


@pytest.mark.parametrize("entry", sorted(EVAL_ENTRIES))
def test_launches_of_a_count_entry(count_inputs, monkeypatch, entry):
    """Without a buffer: the zeroed buffer, then the launch; with one: the launch alone, and a second launch into it doubles it."""
    call, got = count_inputs["calls"][entry], {}
    got[entry] = _recorded(monkeypatch, None, lambda: got.setdefault("one", call()))
    buf = torch.zeros_like(got["one"])
    got[entry + "_buffer"] = _recorded(monkeypatch, None, lambda: got.setdefault("same", call(buf)))
    for key in (entry, entry + "_buffer"):
        print(f"{key}: {got[key]}")
        assert got[key] == EVAL_EXPECTED[key]
    assert got["same"] is buf and torch.equal(buf, got["one"]) and int(buf.sum()) > 0
    call(buf)
    assert torch.equal(buf, 2 * got["one"])
    both = call(torch.zeros_like(buf[:1]), [0, 0])                     # both images into slot 0
    assert torch.equal(both[0], got["one"].sum(0))


def test_launches_of_a_distance_map(count_inputs, monkeypatch):
    E, pred = count_inputs["E"], count_inputs["pred"]
    got, keep = {}, {}
    got["boundary_distance"] = _recorded(monkeypatch, None, lambda: keep.setdefault("one", E.boundary_distance(pred, 4, num_classes=5)))
    out, scratch = torch.empty_like(keep["one"]), torch.empty_like(keep["one"])
    got["boundary_distance_buffers"] = _recorded(monkeypatch, None, lambda: E.boundary_distance(pred, 4, num_classes=5, out=out, scratch=scratch))
    for key, names in got.items():
        print(f"{key}: {names}")
        assert names == EVAL_EXPECTED[key]
    assert torch.equal(out, keep["one"])


def test_every_count_case_has_a_list(count_inputs):
    assert sorted(count_inputs["calls"]) == sorted(EVAL_ENTRIES)
    assert sorted(EVAL_EXPECTED) == sorted(list(EVAL_ENTRIES) + [e + "_buffer" for e in EVAL_ENTRIES] + ["boundary_distance", "boundary_distance_buffers"])
    assert all(EVAL_EXPECTED[e + "_buffer"] == [name] for e, name in EVAL_ENTRIES.items())
    assert sorted(count_inputs["owners"]) == sorted(list(OWNER_EXPECTED) + ["EuclideanBoundaryEvaluator"])


def _buffers(owner):
    """The device buffers of an owner: `.bins` of a Calibration, `.counts` of the others, and `.displacement` where there is one."""
    first = owner.bins if type(owner).__name__ == "Calibration" else owner.counts
    return [b for b in (first, getattr(owner, "displacement", None)) if b is not None]


def _owner_case(count_inputs, monkeypatch, name, warm, first_with_device, first_without, **kw):
    """An owner's add() four ways: made with device= (the first and a second add, then two adds into named slots), and made without."""
    make, args = count_inputs["owners"][name]
    rec = lambda o, **k: _recorded(monkeypatch, None, lambda: o.add(*args, **k))
    o = make(device=DEV, **kw)
    got = [rec(o)]
    assert o.used == 2
    got.append(rec(o))
    assert o.used == 4
    print(f"{name} {kw} device=: {got}")
    assert got == [first_with_device, warm]
    per_image = [b.clone() for b in _buffers(o)]
    for b in per_image:
        assert int(b[:2].sum()) > 0 and torch.equal(b[2:4], b[:2]) and int(b[4:].sum()) == 0      # the second batch went to the next two slots
    s = make(device=DEV, **kw)
    s.add(*args)                                                                                   # the distance maps of the shape
    s.reset()
    assert rec(s, slots=[0, 0]) == warm and s.used == 0
    one = [b.clone() for b in _buffers(s)]
    assert rec(s, slots=[0, 0]) == warm and s.used == 0
    for b, b1, p in zip(_buffers(s), one, per_image):
        assert torch.equal(b, 2 * b1) and torch.equal(b1[0], p[:2].sum(0)) and int(b1[1:].sum()) == 0
    n = make(**kw)
    got = [rec(n), rec(n)]
    print(f"{name} {kw} no device: {got}")
    assert got == [first_without, warm] and n.used == 4
    for b, p in zip(_buffers(n), per_image):
        assert torch.equal(b, p)


@pytest.mark.parametrize("name", sorted(OWNER_EXPECTED))
def test_launches_of_an_owner(count_inputs, monkeypatch, name):
    warm = OWNER_EXPECTED[name]
    _owner_case(count_inputs, monkeypatch, name, warm, warm, ["torch.zeros"] + warm)


@pytest.mark.parametrize("displacement", [True, False])
def test_launches_of_the_euclidean_owner(count_inputs, monkeypatch, displacement):
    x = EUCLIDEAN_EXPECTED
    if displacement:
        _owner_case(count_inputs, monkeypatch, "EuclideanBoundaryEvaluator", x["second"], x["first"], x["first_no_device"])
    else:
        _owner_case(count_inputs, monkeypatch, "EuclideanBoundaryEvaluator", x["second_no_displacement"], x["first_no_displacement"],
                    x["first_no_device_no_displacement"], displacement=False)
