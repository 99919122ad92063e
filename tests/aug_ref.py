"""Torch restatement of the reference's test-time augmentation (segmentors/encoder_decoder.py:448-469: softmax over the classes, flipped back when the
view was flipped; :509-546 `aug_test`: the views' probabilities added in view order, divided by their number, argmax) on top of tests/rescale_ref.py --
TEST INFRASTRUCTURE ONLY.  Pinned by tests/golden/aug.npz, which tools/oracle/make_golden.py::gen_aug produces by calling the reference's own, unmodified
`inference` and `aug_test`."""
import torch
import torch.nn.functional as F

from tests import rescale_ref as RR

FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2}
FLIP_NAMES = {v: k for k, v in FLIP_CODES.items()}

# tag -> (base frame (h, w), crop, stride, ori_shape, views (scale, flip)); crop None = test_cfg.mode 'whole'.  Both sizes of `slide8` give a window overlap
# of exactly 8 (a 1.5 x view would give 9, which the one-pass kernels refuse).
CASES = dict(
    slide=((90, 150), (64, 64), (40, 40), (77, 131), ((1.0, None), (1.0, "horizontal"), (1.25, None), (1.25, "horizontal"), (1.0, "vertical"))),
    slide8=((90, 150), (64, 64), (32, 24), (135, 201), ((1.0, None), (0.75, "horizontal"), (1.0, "vertical"), (0.75, None))),
    whole=((64, 64), None, None, (45, 75), ((1.0, None), (1.0, "horizontal"), (1.0, "vertical"))))


def view(frame, scale, flip):
    """One view of the test pipeline: the frame resized by `scale` (bilinear, to at least 64 x 64), then flipped."""
    if scale != 1.0:
        h, w = frame.shape[2:]
        frame = F.interpolate(frame, (max(int(h * scale + 0.5), 64), max(int(w * scale + 0.5), 64)), mode="bilinear", align_corners=False)
    return frame.flip(3) if flip == "horizontal" else frame.flip(2) if flip == "vertical" else frame


def views_of(case):
    """-> (list of view tensors, list of flip names) of one of CASES' rows (or a decoded fixture row)."""
    hw, _, _, _, vs = case
    base = RR.frame(hw)
    return [view(base, s, f) for s, f in vs], [f for _, f in vs]


def cfg_row(case):
    """A case as the fixture's integer `<tag>_cfg` row: frame, crop, stride (zeros: whole), ori_shape, number of views, then (scale x 100, flip code) each."""
    hw, crop, stride, ori, vs = case
    return list(hw) + (list(crop) + list(stride) if crop else [0, 0, 0, 0]) + list(ori) + [len(vs)] + [v for s, f in vs for v in (int(round(s * 100)), FLIP_CODES[f])]


def case_of(cfg):
    c = [int(v) for v in cfg]
    hw, crop, stride, ori = RR.case_of(c[:8])
    return hw, crop, stride, ori, tuple((c[9 + 2 * i] / 100.0, FLIP_NAMES[c[10 + 2 * i]]) for i in range(c[8]))


def probabilities(encode_decode_fn, img, ori_shape, flip=None, crop_size=None, stride=None):
    """ED:417-469 for one view: the rescaled logits, softmax over the classes, flipped back."""
    p = F.softmax(RR.rescaled_logits(encode_decode_fn, img, ori_shape, crop_size, stride), dim=1)
    return p.flip(3) if flip == "horizontal" else p.flip(2) if flip == "vertical" else p


def aug_probabilities(encode_decode_fn, imgs, flips, ori_shape, crop_size=None, stride=None):
    """ED:517, 538-541: the first view's probabilities, the others added in place in view order, divided by the number of views."""
    acc = probabilities(encode_decode_fn, imgs[0], ori_shape, flips[0], crop_size, stride)
    for img, f in zip(imgs[1:], flips[1:]):
        acc += probabilities(encode_decode_fn, img, ori_shape, f, crop_size, stride)
    acc /= len(imgs)
    return acc


def near_ties(p, tol):
    """Pixels whose top-two averaged-probability margin is within 2 * tol * max p: the ones a map within `tol` of p may decide differently."""
    top = p.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) <= 2 * tol * p.max()
