"""The frame-size class-map pixel (csrc/slide_pixel.h) on the one frame where its early exits, its tail dispatch and the fused launch's histogram flush meet:
a ragged 35 x 290 frame (the second workgroup along x has 34 live lanes) with pixels under 0, 1, 2, 3, 8 and 9 windows (and every count between), at 5 classes (the per-lane LDS
column) and 65 (the recomputing form).  Every launch of the family -- plain, confidence, tempered confidence, margin, entropy, top-k, fused evaluation --
writes the same map and counts the same unsupported pixels, and the outputs keep the identities the project documents as bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, HC, WC = 2, 35, 290, 32, 32
JOBS = ((0, 0, 0), (0, 0, 16), (0, 3, 8), (0, 3, 258), (0, 0, 258), (1, 0, 0)) + tuple((1, 1, 100 + q) for q in range(9))
KS = (1, 3, 8)


def _cover():
    """Windows per pixel, int [B, H, W]."""
    n = np.zeros((B, H, W), dtype=np.int64)
    for b, y0, x0 in JOBS:
        n[b, y0:y0 + HC, x0:x0 + WC] += 1
    return n


def _launch(plan, lg, conf=False, **kw):
    """plan.class_map into buffers pre-filled with values no launch writes -> (map, confidence or score or None, what the launch added to `unc`)."""
    out = torch.full((B, H, W), 77, dtype=torch.uint8, device=DEV)
    cf = torch.full((B, H, W), -1.0, device=DEV) if conf else None
    unc = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan.class_map(lg, out, unc, conf=cf, **kw)
    return out, cf, int(unc.item())


@pytest.fixture(scope="module", params=[5, 65])
def runs(request):
    """Every launch of the family on the frame, once per class count."""
    import mmsa.evaluate as ev
    import mmsa.inference as inf
    C = request.param
    plan = inf.MapPlan(B, H, W, HC, WC, JOBS, H, W, H, W)
    g = torch.Generator().manual_seed(290 + C)
    lg = torch.randn(len(JOBS), C, 8, 8, generator=g, dtype=torch.float32).to(DEV)
    labels = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.int64).to(torch.uint8)
    labels[torch.rand(B, H, W, generator=g) < 0.1] = 255
    labels = labels.to(DEV)
    prep = ev.LabelPrep(C, ignore_index=255)
    r = dict(C=C, plain=_launch(plan, lg), conf=_launch(plan, lg, True), conf_t=_launch(plan, lg, True, temperature=1.0),
             margin=_launch(plan, lg, True, score="margin"), entropy=_launch(plan, lg, True, score="entropy"), topk={}, prep=prep, labels=labels)
    for K in KS:
        tk = inf.TopK(torch.full((K, B, H, W), 77, dtype=torch.uint8, device=DEV), torch.full((K, B, H, W), -1.0, device=DEV))
        unc = torch.zeros(1, dtype=torch.int32, device=DEV)
        plan.class_map(lg, tk.classes[0], unc, topk=tk)
        r["topk"][K] = (tk.classes, tk.probs, int(unc.item()))
    for name, return_map in (("fused", True), ("fused_no_map", False)):
        e = ev.Evaluator(prep, images=B)
        out, _, unc = _launch(plan, lg, labels=labels, evaluator=e, fused=True, return_map=return_map)
        r[name] = (out, e.host_counts(), unc)
    return r


def test_the_frame_has_every_window_count():
    n = _cover()
    assert {0, 1, 2, 3, 8, 9} <= set(np.unique(n).tolist())
    assert W - 256 == 34


def test_every_launch_writes_the_map_of_the_plain_launch(runs):
    plain = runs["plain"][0]
    bad = (_cover() == 0) | (_cover() > 8)
    assert np.array_equal(plain.cpu().numpy() == 255, bad), "255 exactly where no window or more than eight cover the pixel"
    assert bool((plain[torch.from_numpy(~bad).to(DEV)] < runs["C"]).all())
    for name in ("conf", "conf_t", "margin", "entropy", "fused"):
        assert torch.equal(runs[name][0], plain), name
    for K in KS:
        assert torch.equal(runs["topk"][K][0][0], plain), f"plane 0 of the classes, K = {K}"
    assert bool((runs["fused_no_map"][0] == 77).all()), "return_map=False writes no map"


def test_every_launch_counts_the_same_unsupported_pixels(runs):
    n = _cover()
    want = int(((n == 0) | (n > 8)).sum())
    got = {name: runs[name][2] for name in ("plain", "conf", "conf_t", "margin", "entropy", "fused", "fused_no_map")}
    got.update({f"topk{K}": runs["topk"][K][2] for K in KS})
    assert want > 0 and all(v == want for v in got.values()), (want, got)


def test_confidence_tempered_confidence_and_rank_zero_agree(runs):
    conf = runs["conf"][1]
    assert torch.equal(conf, runs["conf_t"][1]), "T = 1 is the untempered confidence, bit for bit"
    for K in KS:
        assert torch.equal(conf, runs["topk"][K][1][0]), f"plane 0 of the probabilities, K = {K}"


def test_margin_is_the_difference_of_the_first_two_ranks(runs):
    for K in (3, 8):
        probs = runs["topk"][K][1]
        assert torch.equal(runs["margin"][1], probs[0] - probs[1]), K


def test_pixels_without_a_class_get_zero_and_255_at_every_rank(runs):
    none = runs["plain"][0] == 255
    assert bool(none.any())
    for name in ("conf", "conf_t", "margin", "entropy"):
        assert bool((runs[name][1][none] == 0).all()), name
        assert bool((runs[name][1][~none] >= 0).all()) and bool((runs[name][1] <= 1).all()), name
    for K in KS:
        classes, probs, _ = runs["topk"][K]
        assert bool((classes[:, none] == 255).all()) and bool((probs[:, none] == 0).all()), K


def test_fused_counts_are_the_counts_of_the_stored_map(runs):
    import mmsa.evaluate as ev
    want = ev.confusion(runs["plain"][0], runs["labels"], runs["prep"]).cpu().numpy()
    assert want.sum() == int((runs["labels"] != 255).sum().item()) and want[:, :, runs["C"]].sum() > 0, "ignored labels are left out, class 255 is counted"
    assert np.array_equal(runs["fused"][1], want)
    assert np.array_equal(runs["fused_no_map"][1], want)
