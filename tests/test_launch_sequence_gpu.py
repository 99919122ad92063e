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
