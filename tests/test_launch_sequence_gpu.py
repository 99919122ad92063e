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
    """The names of the library entries and allocations `fn` makes after its last head call."""
    from mmsa import lib
    names = []
    real_call, real_forward = lib.call, head.forward

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
        mp.setattr(head, "forward", forward)
        for name in ("empty", "zeros"):
            mp.setattr(torch, name, allocator(name))
        fn()
    torch.cuda.synchronize()
    assert names.count("<head>") == 1, "one encoder batch per case"
    return names[names.index("<head>") + 1:]


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_launches_after_the_head(models, monkeypatch, case):
    got = _recorded(monkeypatch, models[2], _calls(models)[case])
    print(f"{case}: {got}")
    assert got == EXPECTED[case]


def test_every_case_has_a_list(models):
    assert sorted(_calls(models)) == sorted(EXPECTED)
