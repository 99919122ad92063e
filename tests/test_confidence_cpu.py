"""Host side of the confidence maps (no GPU): the float32 restatement of the rule (tests/confidence_ref.py) against the float64 softmax, the ABI number
of the new entries, and the refusals a plan makes before it launches anything."""
import os
import re

import pytest
import torch

from tests import confidence_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("C", [1, 5, 33])
def test_restatement_within_the_float64_bound(C):
    """The inputs of the GPU test (planted_logits) as a [n, C, 16, 16] canvas; torch's float32 exp stands in for the device's expf, both within 1 ulp."""
    x = CR.planted_logits(8, C, 1000 + C)
    conf = CR.confidence(x)
    worst, D = CR.float64_check(conf, x)
    print(f"C={C}: D up to {D:.1f}, worst error / bound {worst:.3f}")
    assert (D >= 30 or C == 1) and worst <= 1.0
    assert bool((conf <= 1).all()) and bool((conf >= torch.tensor(1.0) / torch.tensor(float(C))).all())
    if C == 1:
        assert bool((conf == 1).all())
    # all classes equal: exactly 1 / C; one class ahead by more than 104: the other exponentials are 0, exactly 1
    same = x[:, :1].expand(-1, C, -1, -1).contiguous()
    assert bool((CR.confidence(same) == torch.tensor(1.0) / torch.tensor(float(C))).all())
    ahead = x.clone()
    ahead[:, C // 2] += 300.0
    assert bool((CR.confidence(ahead) == 1).all())


def test_abi_number():
    import mmsa
    header = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "mmsa_version.h")).read()).group(1))
    assert mmsa.lib.version() == mmsa.lib.ABI_VERSION == header and header >= 111
    for name in ("mmsa_argmax_max_nchw", "mmsa_slide_argmax_conf", "mmsa_slide_argmax_resized_conf", "mmsa_aug_argmax_conf"):
        assert name in mmsa.lib.SIGNATURES and re.search(r"\b%s\(" % name, open(os.path.join(ROOT, "include", "mmsa.h")).read())
    # each _conf entry takes its sibling's arguments plus one pointer
    for name in ("mmsa_slide_argmax", "mmsa_slide_argmax_resized", "mmsa_aug_argmax"):
        assert len(mmsa.lib.SIGNATURES[name + "_conf"]) == len(mmsa.lib.SIGNATURES[name]) + 1
    assert len(mmsa.lib.SIGNATURES["mmsa_argmax_max_nchw"]) == len(mmsa.lib.SIGNATURES["mmsa_argmax_nchw"]) + 1


def test_plan_refusals_without_a_device():
    """Everything a plan refuses about a confidence buffer is refused on the host, before the first launch: CPU tensors never reach a kernel here."""
    import mmsa.inference as inf
    plan = inf.MapPlan.slide(2, 90, 150, (64, 64), (40, 40))
    resized = inf.MapPlan.slide(2, 90, 150, (64, 64), (40, 40), (77, 131))
    aug = inf.AugPlan((resized, resized), (0, 1))
    lg = torch.zeros(plan.n, 5, 16, 16)
    unc = torch.zeros(1, dtype=torch.int32)
    for p, size, call in ((plan, (2, 90, 150), lambda c, **kw: plan.class_map(lg, torch.empty(2, 90, 150, dtype=torch.uint8), unc, conf=c, **kw)),
                          (resized, (2, 77, 131), lambda c, **kw: resized.class_map(lg, torch.empty(2, 77, 131, dtype=torch.uint8), unc, conf=c, **kw)),
                          (aug, (2, 77, 131), lambda c, **kw: aug.class_map([lg, lg], torch.empty(2, 77, 131, dtype=torch.uint8), unc, conf=c, **kw))):
        with pytest.raises(RuntimeError, match="has shape"):
            call(torch.empty(size[0], size[1], size[2] + 1))
        with pytest.raises(RuntimeError, match="must be float32"):
            call(torch.empty(size, dtype=torch.float64))
        with pytest.raises(RuntimeError, match="is on meta"):
            call(torch.empty(size, device="meta"))
        with pytest.raises(RuntimeError, match="must be contiguous"):
            call(torch.empty(size[0], size[2], size[1]).transpose(1, 2))
        with pytest.raises(RuntimeError, match="must be a tensor"):
            call(True)
        if p is not aug:
            for kw in (dict(fused=True), dict(return_map=False)):
                with pytest.raises(RuntimeError, match="no confidence variant"):
                    call(torch.empty(size), labels=torch.zeros(size, dtype=torch.uint8), evaluator=object(), **kw)
    # the entries' `confidence=` refuses the same by the entry's name
    with pytest.raises(RuntimeError, match="slide_class_map: confidence with fused=True"):
        inf._confidence(True, (2, 90, 150), "cpu", "slide_class_map", fused=True)
    with pytest.raises(RuntimeError, match="whole_class_map: the confidence buffer has shape"):
        inf._confidence(torch.empty(1, 2, 3), (2, 90, 150), "cpu", "whole_class_map")
    assert inf._confidence(False, (2, 90, 150), "cpu", "x") is None and inf._confidence(None, (2, 90, 150), "cpu", "x") is None
    buf = torch.empty(2, 90, 150)
    assert inf._confidence(buf, (2, 90, 150), "cpu", "x") is buf and inf._confidence(True, (2, 9, 15), "cpu", "x").shape == (2, 9, 15)
    # a FrameResult of a runner made without confidence=True says so, before it looks at the pass
    import types
    with pytest.raises(RuntimeError, match="made without confidence=True"):
        inf.FrameResult(types.SimpleNamespace(conf=None), None).confidence()
