"""Test-time augmentation without a device: the AugPlan record (sizes, flips, the concatenated window table and its per-view offsets, every refusal), the
torch restatement tests/aug_ref.py against the reference's own aug_test (tests/golden/aug.npz), and the ABI number."""
import os
import re

import numpy as np
import pytest
import torch

from tests import aug_ref as AR
from tests.configs import toy_encode_decode
from tests.util import REL_TOL, assert_close

SLIDE = dict(mode="slide", crop_size=(64, 64), stride=(40, 40))


def test_aug_plan_table_sizes_flips_and_offsets():
    import mmsa.inference as inf
    shapes = [(2, 90, 150), (2, 100, 170), (2, 70, 70)]
    plan = inf.AugPlan.make(SLIDE, shapes, [None, "horizontal", "vertical"], ori_shape=(77, 131, 3))
    assert plan.A == 3 and plan.flips == (0, 1, 2) and plan.size == (2, 77, 131)
    singles = [inf.MapPlan.slide(B, H, W, (64, 64), (40, 40), (77, 131)) for B, H, W in shapes]
    assert list(plan.plans) == singles                                       # the same mode dispatch as class_map
    assert [p.n for p in plan.plans] == [16, 16, 8] and plan.offsets == (0, 16, 32) and plan.total == 40
    tab = np.array(list(plan.table)).reshape(-1, 3)
    assert tab.shape == (40, 3)
    for p, w0 in zip(plan.plans, plan.offsets):
        assert tab[w0:w0 + p.n].tolist() == [list(j) for j in p.jobs]       # view a's rows, in the accumulation order of slide_inference
    lgs = [torch.empty(p.n, 5, 16, 16) for p in plan.plans]
    assert plan.rows(lgs) == [(0, 16, 16, 16, 90, 150, 64, 64, 77, 131, 0), (16, 16, 16, 16, 100, 170, 64, 64, 77, 131, 1),
                              (32, 8, 16, 16, 70, 70, 64, 64, 77, 131, 2)]
    # the whole modes: one full-size window per image; whole_dim_cut cuts every view alike
    w = inf.AugPlan.make(dict(mode="whole"), [(1, 64, 64), (1, 80, 96)], ["vertical", None], ori_shape=(45, 75))
    assert w.size == (1, 45, 75) and w.offsets == (0, 1) and [p.jobs for p in w.plans] == [((0, 0, 0),), ((0, 0, 0),)] and w.flips == (2, 0)
    c = inf.AugPlan.make(dict(mode="whole_dim_cut", dim=(60, 80), cut_dim=(70, 50)), [(1, 64, 64), (1, 80, 96)])
    assert c.size == (1, 50, 70) and [(p.Hd, p.Wd) for p in c.plans] == [(60, 80)] * 2
    # remembered per geometry: the same views give the same record (whose device table is then already uploaded)
    a = inf.AugPlan.of(SLIDE, shapes, [None, "horizontal", "vertical"], ori_shape=(77, 131, 3))
    assert a is inf.AugPlan.of(dict(SLIDE), [tuple(s) for s in shapes], [None, "horizontal", "vertical"], ori_shape=(77, 131, 3)) and a == plan
    assert a is not inf.AugPlan.of(SLIDE, shapes, [None, "horizontal", None], ori_shape=(77, 131, 3))


def test_aug_plan_refusals():
    import mmsa.inference as inf
    one = [(1, 90, 150)]
    with pytest.raises(RuntimeError, match="only rescale=True"):
        inf.AugPlan.make(SLIDE, one, rescale=False)
    with pytest.raises(RuntimeError, match="0 views"):
        inf.AugPlan.make(SLIDE, [], ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="13 views"):
        inf.AugPlan.make(SLIDE, one * 13, ori_shape=(77, 131))
    assert inf.AugPlan.make(SLIDE, one * 12, ori_shape=(77, 131)).A == inf.MAX_AUGS == 12
    with pytest.raises(RuntimeError, match="'horizontal' or 'vertical'"):
        inf.AugPlan.make(SLIDE, one, ["diagonal"])
    with pytest.raises(RuntimeError, match="same length"):
        inf.AugPlan.make(SLIDE, one * 2, [None])
    with pytest.raises(RuntimeError, match="same length"):
        inf.AugPlan.views([0, 1, 2], [None, None])
    with pytest.raises(RuntimeError, match="same length"):
        inf.AugPlan.views([0, 1, 2], None, ["p", "q"])
    with pytest.raises(RuntimeError, match="LIST of views"):
        inf.AugPlan.views(torch.zeros(1, 6, 64, 64))
    assert inf.AugPlan.views([0, 1], None, "p") == ([0, 1], [None, None], ["p", "p"])
    with pytest.raises(RuntimeError, match="ori_shape="):                     # two scales without a common target
        inf.AugPlan.make(SLIDE, [(1, 90, 150), (1, 100, 170)])
    with pytest.raises(RuntimeError, match="ori_shape="):
        inf.AugPlan.make(SLIDE, [(1, 90, 150), (2, 90, 150)], ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="covers some pixels 9 times"):     # what MapPlan.check_windows refuses, per view: the 1.5 x view of `slide8`
        inf.AugPlan.make(dict(SLIDE, stride=(32, 24)), [(1, 90, 150), (1, 135, 225)], ori_shape=(135, 201))
    with pytest.raises(RuntimeError, match="covers some pixels 9 times"):     # ... and the 1.25 x view of `slide`: 113 x 188 under stride 40 has 3 x 3 windows on some pixels
        inf.AugPlan.make(SLIDE, [(1, 90, 150), (1, 113, 188)], ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="at most 64 windows per view"):
        inf.AugPlan.make(dict(SLIDE, stride=(40, 40)), [(1, 64 + 40 * 8, 64 + 40 * 8)], ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="at least as large as the crop"):
        inf.AugPlan.make(SLIDE, [(1, 60, 150)], ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="not one of"):
        inf.AugPlan.make(dict(mode="slide_mod_sel"), one, ori_shape=(77, 131))
    with pytest.raises(RuntimeError, match="'horizontal' or 'vertical'"):
        inf.probabilities(None, None, torch.zeros(1, 6, 64, 64), dict(mode="whole"), flip="h")


@pytest.mark.parametrize("tag", sorted(AR.CASES))
def test_restatement_against_the_reference_fixture(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "aug.npz"))
    case = AR.case_of(g[f"{tag}_cfg"])
    assert case == AR.CASES[tag]
    hw, crop, stride, ori, _ = case
    imgs, flips = AR.views_of(case)
    want, want_map = torch.from_numpy(g[f"{tag}_prob"]), torch.from_numpy(g[f"{tag}_map"]).long()
    assert torch.equal(want.argmax(1)[0], want_map)
    got = AR.aug_probabilities(toy_encode_decode(AR.RR.NUM_CLASSES, seed=AR.RR.TOY_SEED), imgs, flips, ori, crop, stride)
    r, mx = assert_close(got, want, what=f"averaged probabilities, case {tag}")
    skip = AR.near_ties(want, REL_TOL)
    share = skip.float().mean().item()
    wrong = int(((got.argmax(1) != want_map[None]) & ~skip).sum())
    print(f"aug {tag}: rel_l2 {r:.2e} max_rel {mx:.2e}; {share:.4%} near-tie pixels excluded; {wrong} other pixels differ")
    assert share <= 0.01 and wrong == 0
    assert_close(got.sum(1), torch.ones(1, *ori), tol=1e-6, what="the averaged probabilities sum to one")


def test_abi_number():
    import mmsa
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = int(re.search(r"#define MMSA_ABI_VERSION (\d+)", open(os.path.join(root, "include", "mmsa_version.h")).read()).group(1))
    assert n >= 110 and mmsa.lib.version() == n == mmsa.lib.ABI_VERSION
    for name in ("mmsa_softmax_flip_accum_nchw", "mmsa_aug_argmax"):
        assert name in mmsa.lib.SIGNATURES
    for name in ("probabilities", "aug_inference", "aug_class_map", "AugPlan"):
        assert getattr(mmsa, name) is getattr(mmsa.inference, name)
