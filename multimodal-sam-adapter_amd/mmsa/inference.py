"""Inference glue of the reference's EncoderDecoder on device (segmentation/mmseg_custom/models/segmentors/encoder_decoder.py):
`encode_decode` (ED:85-95), `slide_inference` (ED:191-234), `whole_inference`, `whole_inference_dim` (ED:329-362),
`whole_inference_dim_cut` (ED:364-413), the mode dispatch of `inference` (ED:417-447) and the class map of `simple_test` (ED:449,477) -- with
`rescale=True` (test_bs.py:241-244) at the size the reference rescales to: `ori_shape` in the slide and whole modes (ED:227-233, 314-325), `dim` in the
`whole_dim*` modes, as logits (a second resize of the canvas) or as the class map of ONE launch that writes neither canvas (mmsa_slide_argmax_resized).

The crops of a sliding-window frame are batched through ONE backbone + head call (the reference runs them one by one,
ED:205-214), and the resize / pad / accumulate / count of every crop is one kernel launch on the logits canvas.

Test-time augmentation (`aug_test`, ED:509-546): `probabilities` (the softmax and un-flip of ED:448-469), `aug_inference` (the mean over the views, on
canvases), `aug_class_map` (its argmax, from the canvas path or from ONE launch after the head, mmsa_aug_argmax) and `AugPlan`, the MapPlan of several views.

Confidence maps (`confidence=` of the class-map entries, `conf=` of the plans, `argmax_max_map`): the probability of the predicted class, max over the
classes of what `probabilities` / `aug_inference` return (ED:449,460), float32 [B, Ho, Wo], written by the launch that writes the class map.
`calibration=` (mmsa.evaluate.Calibration) of the same entries bins that map against `labels=` on device: one more launch over the stored map and confidence.
`selective=` (mmsa.evaluate.SelectiveEvaluator) of the same entries keeps one confusion matrix per confidence bin, likewise by one more launch: mIoU at a coverage.
`temperature=` of the same entries (and of `probabilities`) writes the confidence of softmax(x / T) instead, by the `_t` sibling of whatever launch the plan takes; T
comes from mmsa.evaluate.TemperatureSweep.  The class map does not depend on it, and `temperature=None` takes exactly the launches it always took.
`score=` of the same entries ("max" | "margin" | "entropy") chooses what the confidence slot holds: the confidence, the top-2 margin P_(1) - P_(2) or the entropy
score 1 - H / log C (csrc/softmax_px.h), each in [0, 1] with higher = more certain, so `calibration=` / `selective=` / `abstain` take any of them; the two new
ones come from the `_score` sibling of the launch the plan takes (`argmax_score_map` on a probability canvas), and "max" takes exactly the launches it always took.

What a frame's output looks like -- its windows, the size after the second resize and after the cut, which class-map kernel that takes -- is decided once,
in `MapPlan`, a record without device state; the entries read the frame (`_intake`), make the plan, and launch from it.  What the keywords above ask of
that launch is decided once as well, in `MapOptions`: every entry validates the family under its own name, and the plan picks its launch from the record."""
import ctypes
import dataclasses
import functools
from collections import namedtuple

import torch

from . import lib
from . import ops
from .render import slide_source, whole_source


def _on_device(fn):
    """Run an entry point with its first tensor argument's device current (launches go to that device's current stream)."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        t = next((a for a in args if isinstance(a, torch.Tensor)), None)
        if t is None:                                           # raw frames (preprocess=): the first argument that is a pair of tensors
            t = next((a[0] for a in args if isinstance(a, (tuple, list)) and len(a) == 2 and isinstance(a[0], torch.Tensor)), None)
        if t is None or not t.is_cuda:
            return fn(*args, **kw)     # _check raises the "no CPU path" error
        with torch.cuda.device(t.device):
            return fn(*args, **kw)
    return wrapped


def _resize_into(logits, canvas, y0, x0, hc, wc, count=None, accumulate=False):
    b, c, hs, ws = logits.shape
    lib.call("mmsa_bilinear_accum_nchw", logits.data_ptr(), c * hs * ws, b, c, hs, ws, canvas.data_ptr(), canvas.shape[2], canvas.shape[3],
             y0, x0, hc, wc, count.data_ptr() if count is not None else None, 1 if accumulate else 0, ops._stream())


def _pair(backbone, head):
    """With this package's head behind this package's backbone, the backbone's tail also emits its maps as planes for the head."""
    from .head import SegformerHead
    if isinstance(head, SegformerHead) and hasattr(backbone, "_vit"):
        backbone.emit_planes = True


def _raw(preprocess, img, what):
    """With `preprocess=`: img is the pair (rgb, aux) of raw [B, Hs, Ws, 3] frames -> (rgb, aux, B, H, W) of the normalised canvas."""
    if not isinstance(img, (tuple, list)) or len(img) != 2:
        raise RuntimeError(f"mmsa.{what}: with preprocess=, the image is the pair (rgb, aux) of raw [B, H, W, 3] GPU tensors")
    rgb, aux = preprocess.check(*img)
    H, W = preprocess.canvas(rgb.shape[1], rgb.shape[2])
    return rgb, aux, rgb.shape[0], H, W


def _check(img):
    if not img.is_cuda or img.dtype != torch.float32 or img.dim() != 4:
        raise RuntimeError("mmsa.inference: img must be a float32 [B, C, H, W] GPU tensor (there is no CPU path)")


def _intake(img, preprocess, what, contiguous=True):
    """The frame of a slide entry -> (B, H, W, device, frame, cut): H x W is the canvas the windows cover; `frame` is the checked pair (rgb, aux) of raw frames
    (`preprocess=`) or the normalised tensor; `cut(windows, out=None, frame=frame)` is the one launch that cuts (and, from raw frames, normalises) the
    windows (image, (y1, x1, y2, x2)), all of the first one's size.  `contiguous=False` hands a strided tensor on as it came: what slide_inference does."""
    if preprocess is not None:
        rgb, aux, B, H, W = _raw(preprocess, img, what)
        frame, device = (rgb, aux), rgb.device
        crops = lambda f, windows, size, out: preprocess.crops(f[0], f[1], windows, size, out=out)
    else:
        _check(img)
        frame = img.contiguous() if contiguous else img
        (B, _, H, W), device = frame.shape, frame.device
        crops = _crops

    def cut(windows, out=None, frame=frame):
        y1, x1, y2, x2 = windows[0][1]
        return crops(frame, windows, (y2 - y1, x2 - x1), out)
    return B, H, W, device, frame, cut


@_on_device
@torch.no_grad()
def encode_decode(backbone, head, img):
    """ED:85-95: logits of the head resized (bilinear, align_corners=False) to the input size -> [B, classes, H, W]."""
    _check(img)
    _pair(backbone, head)
    feats, _ = backbone(img)
    lg = head(feats)
    out = torch.empty(img.shape[0], lg.shape[1], img.shape[2], img.shape[3], device=img.device)
    _resize_into(lg, out, 0, 0, img.shape[2], img.shape[3])
    return out


def crop_boxes(h_img, w_img, crop_size, stride):
    """The window grid of ED:198-212 (windows at the right / bottom border are shifted inwards)."""
    h_crop, w_crop = crop_size
    h_stride, w_stride = stride
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    boxes = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1, x1 = h_idx * h_stride, w_idx * w_stride
            y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
            y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
            boxes.append((y1, x1, y2, x2))
    return boxes


@_on_device
@torch.no_grad()
def slide_inference(backbone, head, img, crop_size, stride, max_batch=8, preprocess=None, rescale=True, ori_shape=None):
    """ED:191-234: averaged logits [B, classes, H, W] of overlapping windows; with `rescale` and an `ori_shape` (h, w[, 3]) other than the frame's they
    are resized once more (bilinear, align_corners=False) to [B, classes, h, w] (ED:227-233).  All windows have
    the crop size here (the backbone needs H = W = img_size), i.e. the image must be at least as large as the crop.
    `preprocess=` (mmsa.preprocess.Preprocess): img is the pair (rgb, aux) of raw frames; the windows are cut AND normalised by one launch."""
    B, H, W, device, _, cut = _intake(img, preprocess, "slide_inference", contiguous=False)
    plan = MapPlan.slide(B, H, W, crop_size, stride, ori_shape if rescale else None, what="slide_inference")     # any overlap, any number of windows
    _pair(backbone, head)
    preds = count = None
    for s in range(0, plan.n, max_batch):
        chunk = plan.windows[s:s + max_batch]
        crops = cut(chunk)
        feats, _ = backbone(crops)
        lg = head(feats)                                   # [n, classes, hc/4, wc/4]
        if preds is None:
            preds = torch.zeros(B, lg.shape[1], H, W, device=device)
            count = torch.zeros(B, H, W, device=device)
        for k, (b, (y1, x1, y2, x2)) in enumerate(chunk):   # preds[b] += pad(resize(logits_k)); count[b, window] += 1
            _resize_into(lg[k:k + 1], preds[b:b + 1], y1, x1, y2 - y1, x2 - x1, count=count[b:b + 1], accumulate=True)
    if bool((count == 0).any()):
        raise RuntimeError("mmsa.slide_inference: windows do not cover the image")   # ED:220
    lib.call("mmsa_div_count_nchw", preds.data_ptr(), count.data_ptr(), B, preds.shape[1], H * W, ops._stream())
    return _rescaled_logits(preds, (plan.Hd, plan.Wd) if plan.rescaled else None)


def _target(shape, H, W, what):
    """The size a prediction of an H x W frame is rescaled to: (h, w) of `ori_shape` / `dim`, or None where that is the frame's own size (a same-size
    align_corners=False resize is the identity) or no shape is given."""
    if shape is None:
        return None
    if len(shape) < 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise RuntimeError(f"mmsa.{what}: the rescale target must be (h, w[, channels]) with h, w >= 1, got {tuple(shape)}")
    t = (int(shape[0]), int(shape[1]))
    return None if t == (H, W) else t


def _rescaled_logits(y, target):
    """The second resize of ED:227-233 / 314-325 / 349-360 on the logits canvas."""
    if target is None:
        return y
    out = torch.empty(y.shape[0], y.shape[1], target[0], target[1], device=y.device)
    _resize_into(y, out, 0, 0, target[0], target[1])
    return out


def _crops(img, chunk, crop_size, out=None):
    """ED:205-212 for a batch of windows: one HIP launch (mmsa_crop_batch_nchw), no ATen slicing / stacking."""
    n = len(chunk)
    if out is None:
        out = torch.empty(n, img.shape[1], crop_size[0], crop_size[1], device=img.device)
    tab = (ctypes.c_int * (3 * n))(*[v for b, (y1, x1, _, _) in chunk for v in (b, y1, x1)])
    lib.call("mmsa_crop_batch_nchw", img.data_ptr(), img.shape[0], img.shape[1], img.shape[2], img.shape[3], tab, n, out.data_ptr(),
             crop_size[0], crop_size[1], ops._stream())
    return out


MAX_OVERLAP = 8   # windows per pixel mmsa_slide_argmax keeps in registers (csrc/segment.hip)


def _check_overlap(boxes, what):
    """The window grid is a product of row intervals and column intervals, so the largest per-pixel overlap is the product of the
    largest per-row and per-column overlaps: checked on the host BEFORE launching, because the one-pass kernel classifies only pixels
    covered by 1..MAX_OVERLAP windows (others get class 255 and are counted in its `uncovered` word)."""
    def deepest(iv):
        ev = sorted([(a, 1) for a, _ in iv] + [(b, -1) for _, b in iv], key=lambda t: (t[0], t[1]))   # half-open: close before open
        cur = best = 0
        for _, d in ev:
            cur += d
            best = max(best, cur)
        return best
    rows = sorted({(y1, y2) for y1, _, y2, _ in boxes})
    cols = sorted({(x1, x2) for _, x1, _, x2 in boxes})
    ov = deepest(rows) * deepest(cols)
    if ov > MAX_OVERLAP:
        raise RuntimeError(f"mmsa.{what}: the window grid covers some pixels {ov} times, the one-pass class-map kernel handles up to {MAX_OVERLAP} "
                           "(use slide_inference + argmax_map, or a larger stride)")


# Which launch makes a RESCALED class map by default: True = the one-pass kernel (mmsa_slide_argmax_resized), False = the canvas path
# (_rescaled_map_canvas: the launches of slide_inference + the second resize + argmax_map, from the same head-resolution logits; the same map bit for bit).
# Per direction of the second resize ("up": the target has more pixels than the frame).  `one_pass=` of the class-map calls overrides it.
ONE_PASS_RESCALE_DEFAULT = dict(up=True, down=True)   # not measured yet (tools/exp/rescale_class_map_bench.py)


# The same choice where the launch also writes an uncertainty score (`score=` "margin" / "entropy"): the one-pass kernel (mmsa_slide_argmax_resized_score)
# recomputes the pixel's values in three passes, and the canvas path (_rescaled_map_canvas + mmsa_argmax_score_nchw; the same map and score bit for bit) wins
# far outside the spread of the yardstick, the `confidence=True` launch on the same inputs (profiles/uncertainty.txt, 25 classes): 0.98 / 0.99 ms against
# 1.95 / 1.96 ms for two 1024 x 1024 maps to 1200 x 1200 (margin / entropy), 0.88 / 0.90 ms against 3.53 / 3.52 ms for the six-window 1080 x 1920 frame to
# 720 x 1280; the yardstick's p10 .. p90 spans 9 / 37 us.  One pass remains the choice where memory is: it allocates nothing, the canvas path three
# [B, C, h, w] float32 arrays.  At the frame's own size there is no such choice: the one-pass launch (+ 4 .. 32 us over the confidence launch) is the only one.
ONE_PASS_SCORE_RESCALE_DEFAULT = dict(up=False, down=False)


_NO_CONF_FUSED = ("confidence with fused=True / return_map=False: the fused class-map + evaluation launch (mmsa_slide_argmax_eval) has no confidence variant; "
                  "with labels= the counts of a map with confidence go through the stored map (drop fused= / return_map=)")


def _check_conf(conf, size, device, what="inference"):
    """A confidence buffer must be what the kernels write: a contiguous float32 [B, Ho, Wo] tensor on the map's device."""
    if not isinstance(conf, torch.Tensor):
        raise RuntimeError(f"mmsa.{what}: the confidence buffer must be a tensor, got {type(conf).__name__}")
    if tuple(conf.shape) != tuple(size):
        raise RuntimeError(f"mmsa.{what}: the confidence buffer has shape {tuple(conf.shape)}, the class map is [B, Ho, Wo] = {tuple(size)}")
    if conf.dtype != torch.float32:
        raise RuntimeError(f"mmsa.{what}: the confidence buffer must be float32, got {conf.dtype}")
    if conf.device != torch.device(device):
        raise RuntimeError(f"mmsa.{what}: the confidence buffer is on {conf.device}, the class map on {torch.device(device)}")
    if not conf.is_contiguous():
        raise RuntimeError(f"mmsa.{what}: the confidence buffer must be contiguous (its layout is the class map's)")
    return conf


def _confidence(confidence, size, device, what, fused=None, return_map=True):
    """`confidence=` of an entry -> the buffer the launch writes, or None: False / None = no confidence map; True = a new float32 [B, Ho, Wo]; a tensor = the
    output buffer itself (checked; nothing is allocated).  Refuses, before anything is launched, what has no confidence variant."""
    if confidence is None or confidence is False:
        return None
    if fused or not return_map:
        raise RuntimeError(f"mmsa.{what}: {_NO_CONF_FUSED}")
    if confidence is True:
        return torch.empty(size, dtype=torch.float32, device=device)
    return _check_conf(confidence, size, device, what)


def _inv_temperature(temperature, confidence, what):
    """`temperature=` of an entry -> the float32 inverse temperature of the `_t` launches (mmsa.evaluate.inv_temperature; ValueError for a T that is not
    finite and positive), or None.  Refused without a confidence map (`confidence`: the entry's `confidence=`, or the buffer)."""
    if temperature is None:
        return None
    if confidence is None or confidence is False:
        raise RuntimeError(f"mmsa.{what}: temperature= without confidence=: the class map does not depend on the temperature (the argmax of x / T is the argmax "
                           "of x for every T > 0), only the confidence map does; pass confidence=True or an output tensor as well")
    from .evaluate import inv_temperature
    return inv_temperature(temperature)


_NO_SCORE_AUG_ONE_PASS = ("with one_pass=True: the one-pass augmented launch (mmsa_aug_argmax_conf) has no score sibling; the margin and the entropy score of "
                          "augmented views come from the canvas path (drop one_pass=, or pass one_pass=False)")


def _score_kind(score, confidence, what):
    """`score=` of an entry -> the `kind` of the score launches: 0 for "max" (the confidence launches, exactly as without `score=`), 1 for "margin" (top-2
    margin), 2 for "entropy" (1 - H / log C); csrc/softmax_px.h.  Refused when unknown, and other than "max" without a confidence map (`confidence`: the
    entry's `confidence=`, or the buffer), in whose place the score is written."""
    from .evaluate import SCORES
    if not isinstance(score, str) or score not in SCORES:
        raise RuntimeError(f"mmsa.{what}: score= must be one of {tuple(SCORES)}, got {score!r}")
    if SCORES[score] and (confidence is None or confidence is False):
        raise RuntimeError(f"mmsa.{what}: score={score!r} without confidence=: the score is written in the confidence map's place and the class map does not "
                           "depend on it; pass confidence=True or an output tensor as well")
    return SCORES[score]


def _inv_log_c(C):
    from .evaluate import inv_log_classes
    return inv_log_classes(int(C))


def _check_binned(kw, cls, owner, labels, confidence, what, fused=None, return_map=True):
    """`calibration=` / `selective=` of an entry (`kw`: the keyword's name, `cls`: the mmsa.evaluate class it takes), refused by name before anything is
    launched: both reduce the confidence map against the labels, so they need both, and the stored map (the fused class-map + evaluation launch writes
    no confidence).  `confidence`: the entry's `confidence=`, or a runner's buffer."""
    if owner is None:
        return
    from . import evaluate
    if not isinstance(owner, getattr(evaluate, cls)):
        raise RuntimeError(f"mmsa.{what}: {kw}= takes an mmsa.evaluate.{cls}, got {type(owner).__name__}")
    if labels is None:
        raise RuntimeError(f"mmsa.{what}: {kw}= needs labels= (the raw uint8 label maps the confidence is checked against)")
    if confidence is None or confidence is False:
        raise RuntimeError(f"mmsa.{what}: {kw}= needs the confidence map: pass confidence=True or an output tensor (a SlideRunner: make it with "
                           "confidence=True)")
    if fused or not return_map:
        raise RuntimeError(f"mmsa.{what}: {_NO_CONF_FUSED}")


TopK = namedtuple("TopK", "classes probs")      # the top-k map of a call: uint8 / float32 [K, B, Ho, Wo], rank-major (csrc/softmax_px.h); classes[0] IS the class map

_NO_TOPK_ONE_PASS = ("with one_pass=True: there is no one-pass top-k launch at a rescaled or cut size or over augmented views; both are served by the canvas "
                     "path (mmsa_argmax_topk_nchw on the probabilities; drop one_pass=, or pass one_pass=False)")


def _check_topk_buffers(topk, size, device, what):
    """A TopK of caller buffers must be what the kernels write: contiguous uint8 / float32 [K, B, Ho, Wo] tensors on the map's device, 1 <= K <= MAX_TOPK."""
    from .evaluate import MAX_TOPK
    for name, buf, dtype in (("classes", topk.classes, torch.uint8), ("probs", topk.probs, torch.float32)):
        if not isinstance(buf, torch.Tensor):
            raise RuntimeError(f"mmsa.{what}: the top-k {name} buffer must be a tensor, got {type(buf).__name__}")
        if buf.dim() != 4 or tuple(buf.shape[1:]) != tuple(size) or not 1 <= buf.shape[0] <= MAX_TOPK:
            raise RuntimeError(f"mmsa.{what}: the top-k {name} buffer has shape {tuple(buf.shape)}, the class map is [B, Ho, Wo] = {tuple(size)}: "
                               f"[K, B, Ho, Wo] with 1 <= K <= {MAX_TOPK} is expected (rank-major)")
        if buf.dtype != dtype:
            raise RuntimeError(f"mmsa.{what}: the top-k {name} buffer must be {str(dtype).replace('torch.', '')}, got {buf.dtype}")
        if device is not None and buf.device != torch.device(device):
            raise RuntimeError(f"mmsa.{what}: the top-k {name} buffer is on {buf.device}, the class map on {torch.device(device)}")
        if not buf.is_contiguous():
            raise RuntimeError(f"mmsa.{what}: the top-k {name} buffer must be contiguous (every rank plane has the class map's layout)")
    if topk.classes.shape[0] != topk.probs.shape[0] or topk.classes.device != topk.probs.device:
        raise RuntimeError(f"mmsa.{what}: the top-k buffers disagree: classes {tuple(topk.classes.shape)} on {topk.classes.device}, probs "
                           f"{tuple(topk.probs.shape)} on {topk.probs.device}")
    return topk


def _topk_option(topk, what, confidence=False, score="max", one_pass=None, aug=False):
    """`topk=` of an entry, checked before the frame is looked at -> None, the int K, or the TopK of caller buffers (checked against the map by
    MapOptions.at).  Refuses by name what a top-k map replaces: `confidence=` and `score=`, whose maps are planes of it."""
    if topk is None:
        return None
    if not isinstance(topk, TopK):
        from .evaluate import check_topk
        topk = check_topk(topk, f"mmsa.{what}")
    if not (confidence is None or confidence is False):
        raise RuntimeError(f"mmsa.{what}: topk= with confidence=: the confidence map is plane 0 of the top-k probabilities; take topk.probs[0]")
    if score != "max":
        raise RuntimeError(f"mmsa.{what}: topk= with score={score!r}: the score is written in the confidence map's place, which a top-k map has none of; the "
                           "top-2 margin is topk.probs[0] - topk.probs[1], the confidence topk.probs[0]; make a second call without topk= for another score")
    if aug and one_pass:
        raise RuntimeError(f"mmsa.{what}: topk= {_NO_TOPK_ONE_PASS}")
    return topk


def _check_topk_call(topk, topk_evaluator, labels, calibration, selective, fused, return_map, what):
    """The per-call half of `topk=`: what has no top-k variant is refused by name, and `topk_evaluator=` needs `labels=` and `topk=`."""
    if topk_evaluator is not None:
        from .evaluate import TopKEvaluator
        if not isinstance(topk_evaluator, TopKEvaluator):
            raise RuntimeError(f"mmsa.{what}: topk_evaluator= takes an mmsa.evaluate.TopKEvaluator, got {type(topk_evaluator).__name__}")
        if labels is None:
            raise RuntimeError(f"mmsa.{what}: topk_evaluator= needs labels= (the raw uint8 label maps the ranks are checked against)")
        if topk is None:
            raise RuntimeError(f"mmsa.{what}: topk_evaluator= needs the top-k map: pass topk=K or a TopK of buffers (a SlideRunner: make it with topk=)")
        K = topk.classes.shape[0] if isinstance(topk, TopK) else topk
        if K != topk_evaluator.k:
            raise RuntimeError(f"mmsa.{what}: topk_evaluator= counts {topk_evaluator.k} ranks, topk= gives {K}")
    if topk is None:
        return
    for kw, owner, fn in (("calibration", calibration, "mmsa.calibration"), ("selective", selective, "mmsa.selective")):
        if owner is not None:
            raise RuntimeError(f"mmsa.{what}: topk= with {kw}=: the pass reads a confidence map, which a top-k call returns as planes; run "
                               f"{fn}(topk.classes[r], topk.probs[r], labels, prep) on the planes (rank 0: the map and its confidence)")
    if fused or not return_map:
        raise RuntimeError(f"mmsa.{what}: topk= with fused=True / return_map=False: the fused class-map + evaluation launch (mmsa_slide_argmax_eval) has no top-k "
                           "variant, and the map is plane 0 of the top-k classes; with labels= the counts go through the stored map (drop fused= / return_map=)")


def _check_boundary_call(boundary, labels, return_map, what):
    """`boundary=` of an entry: a BoundaryEvaluator, fed by `labels=` from the STORED map -- so there must be one."""
    if boundary is None:
        return
    from .evaluate import BoundaryEvaluator
    if not isinstance(boundary, BoundaryEvaluator):
        raise RuntimeError(f"mmsa.{what}: boundary= takes an mmsa.evaluate.BoundaryEvaluator, got {type(boundary).__name__}")
    if labels is None:
        raise RuntimeError(f"mmsa.{what}: boundary= needs labels= (the raw uint8 label maps whose boundaries the band is drawn around)")
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: boundary= with return_map=False: the boundary counts are one more launch over the stored map, and return_map=False "
                           "stores none (drop return_map=)")


def _check_segments_call(segments, labels, return_map, what):
    """`segments=` of an entry: a SegmentEvaluator, fed by `labels=` from the STORED map -- so there must be one."""
    if segments is None:
        return
    from .evaluate import SegmentEvaluator
    if not isinstance(segments, SegmentEvaluator):
        raise RuntimeError(f"mmsa.{what}: segments= takes an mmsa.evaluate.SegmentEvaluator, got {type(segments).__name__}")
    if labels is None:
        raise RuntimeError(f"mmsa.{what}: segments= needs labels= (the raw uint8 label maps whose segments the prediction's are counted against)")
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: segments= with return_map=False: the segment counts are further launches over the stored map, and return_map=False "
                           "stores none (drop return_map=)")


def _check_panoptic_call(panoptic, labels, return_map, what):
    """`panoptic=` of an entry: a PanopticEvaluator, fed by `labels=` from the STORED map -- so there must be one."""
    if panoptic is None:
        return
    from .evaluate import PanopticEvaluator
    if not isinstance(panoptic, PanopticEvaluator):
        raise RuntimeError(f"mmsa.{what}: panoptic= takes an mmsa.evaluate.PanopticEvaluator, got {type(panoptic).__name__}")
    if labels is None:
        raise RuntimeError(f"mmsa.{what}: panoptic= needs labels= (the raw uint8 label maps whose segments the prediction's are matched with)")
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: panoptic= with return_map=False: the panoptic counts are further launches over the stored map, and return_map=False "
                           "stores none (drop return_map=)")


def _check_segment_table_call(segment_table, return_map, what):
    """`segment_table=` of an entry: a SegmentTable made with num_classes=, filled from the STORED map -- so there must be one.  It needs no `labels=`."""
    if segment_table is None:
        return
    from .evaluate import SegmentTable
    if not isinstance(segment_table, SegmentTable):
        raise RuntimeError(f"mmsa.{what}: segment_table= takes an mmsa.evaluate.SegmentTable, got {type(segment_table).__name__}")
    if segment_table.labels_prep is not None:
        raise RuntimeError(f"mmsa.{what}: segment_table= takes a SegmentTable made with num_classes= (the stored map is a class map), this one reads raw labels "
                           "(labels_prep=)")
    if not return_map:
        raise RuntimeError(f"mmsa.{what}: segment_table= with return_map=False: the table is filled by further launches over the stored map, and return_map=False "
                           "stores none (drop return_map=)")


def _check_tracker_call(tracker, segment_table, what):
    """`tracker=` of SlideRunner.run: a SegmentTracker, together with `segment_table=` -- the tracker's own table, which the frame fills first."""
    if tracker is None:
        return
    from .evaluate import SegmentTracker
    if not isinstance(tracker, SegmentTracker):
        raise RuntimeError(f"mmsa.{what}: tracker= takes an mmsa.evaluate.SegmentTracker, got {type(tracker).__name__}")
    if segment_table is None:
        raise RuntimeError(f"mmsa.{what}: tracker= needs segment_table= (the tracker's own SegmentTable: the frame fills it, then the tracker follows it)")
    if tracker.table is not segment_table:
        raise RuntimeError(f"mmsa.{what}: tracker= is bound to another SegmentTable than segment_table= (pass tracker.table)")


def _check_labels(labels, evaluator, *binned):
    """`labels=` feed an evaluator, a calibration, a selective evaluator or several of them; an evaluator needs them."""
    if (labels is None) != (evaluator is None) and not (labels is not None and any(b is not None for b in binned)):
        raise RuntimeError("mmsa.inference: labels= and evaluator= come together")


@dataclasses.dataclass(frozen=True)
class MapOptions:
    """The option family of the class-map entries, validated: what a plan's launch needs, and nothing a callee has to check or derive again.  Built once per
    call, under the calling entry's name `what` (the `mmsa.<what>:` of every refusal), in two steps that own every refusal of the family, in this order:
    `of` -- `score=`, `temperature=`, `calibration=`, `selective=`, all before the frame is looked at; `at` -- once the map's size and device are known and
    before the backbone runs: `confidence=` with fused=True / return_map=False, the confidence buffer (made, or checked), `labels=`.
    `topk=` / `topk_evaluator=` follow the same two steps: `of` and `with_call` refuse by name what a top-k map replaces or has no variant of, `at` checks or
    makes the TopK buffers; with `topk=None` neither step does anything it did not do before.
    `boundary=` (a BoundaryEvaluator) is per call: `with_call` refuses it without `labels=`, of another type, or with `return_map=False`; `count` launches it.
    `segments=` (a SegmentEvaluator) goes exactly the same way, and so does `panoptic=` (a PanopticEvaluator).
    `segment_table=` (a SegmentTable made with num_classes=) is per call too and needs no `labels=`: `with_call` refuses another type, a table of raw labels and
    `return_map=False`; `count_segments` fills it from the stored map, with the confidence or score map (`confidence=`) or probs[0] (`topk=`) as its values.
    What depends on the plan (`one_pass=` at frame size, `fused=` / `return_map=` at a rescaled size or without an evaluator) is refused by MapPlan.class_map."""
    conf: object = None          # the float32 [B, Ho, Wo] buffer the launch writes the confidence (or score) map into, or None; before `at`: the entry's `confidence=`
    it: object = None            # the float32 inverse temperature of the `_t` / `_score` launches (mmsa.evaluate.inv_temperature), or None
    kind: int = 0                # 0: the confidence; 1 / 2: the top-2 margin / the entropy score (mmsa.evaluate.SCORES)
    labels: object = None
    evaluator: object = None
    case: object = None
    calibration: object = None
    selective: object = None
    fused: object = None
    return_map: bool = True
    one_pass: object = None
    topk: object = None          # the TopK of uint8 / float32 [K, B, Ho, Wo] buffers the launch writes, or None; before `at`: the entry's `topk=` (None, K or a TopK)
    topk_evaluator: object = None
    segments: object = None      # the mmsa.evaluate.SegmentEvaluator the stored map is counted into, or None
    panoptic: object = None      # the mmsa.evaluate.PanopticEvaluator the stored map is counted into, or None
    segment_table: object = None # the mmsa.evaluate.SegmentTable filled from the stored map (and the confidence / score / probs[0] next to it), or None
    tracker: object = None       # the mmsa.evaluate.SegmentTracker of `segment_table` (SlideRunner.run alone: a stream has frames), or None
    boundary: object = None      # the mmsa.evaluate.BoundaryEvaluator the stored map is counted into, or None

    @classmethod
    def of(cls, what, confidence=False, temperature=None, score="max", one_pass=None, aug=False, topk=None, **per_call):
        """`aug`: the entries of augmented views, whose one-pass launch has no score sibling.  A SlideRunner makes its record without `per_call` and adds
        them per frame (`with_call`).  `topk=` comes first: its refusals name what a top-k map replaces, and without it nothing here changes."""
        topk = _topk_option(topk, what, confidence, score, one_pass, aug)
        kind = _score_kind(score, confidence, what)
        if aug and kind and one_pass:
            raise RuntimeError(f"mmsa.{what}: score={score!r} {_NO_SCORE_AUG_ONE_PASS}")
        it = _inv_temperature(temperature, confidence if topk is None else True, what)      # the probabilities of a top-k map depend on T as the confidence does
        return cls(conf=confidence, it=it, kind=kind, one_pass=one_pass, topk=topk).with_call(what, **per_call)

    def with_call(self, what, labels=None, evaluator=None, case=None, calibration=None, selective=None, fused=None, return_map=True, topk_evaluator=None,
                  segments=None, panoptic=None, segment_table=None, tracker=None, boundary=None):
        _check_topk_call(self.topk, topk_evaluator, labels, calibration, selective, fused, return_map, what)
        _check_boundary_call(boundary, labels, return_map, what)
        _check_segments_call(segments, labels, return_map, what)
        _check_panoptic_call(panoptic, labels, return_map, what)
        _check_segment_table_call(segment_table, return_map, what)
        _check_tracker_call(tracker, segment_table, what)
        for kw, name, owner in (("calibration", "Calibration", calibration), ("selective", "SelectiveEvaluator", selective)):
            _check_binned(kw, name, owner, labels, self.conf, what, fused, return_map)
        return dataclasses.replace(self, labels=labels, evaluator=evaluator, case=case, calibration=calibration, selective=selective, fused=fused,
                                   return_map=return_map, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table,
                                   tracker=tracker)

    def at(self, size, device, what, make=True):
        """`make=False`: a plan's `conf=` / `topk=`, which are the buffers themselves -- True / K make none there."""
        conf = _confidence(self.conf, size, device, what, self.fused, self.return_map) if make or self.conf is not True else _check_conf(True, size, device, what)
        topk = self.topk
        if isinstance(topk, TopK):
            topk = _check_topk_buffers(topk, size, device, what)
        elif topk is not None:
            if not make:
                raise RuntimeError(f"mmsa.{what}: a plan's topk= is the TopK of buffers itself (classes uint8, probs float32, both [K, B, Ho, Wo]); `out` is its "
                                   "classes[0]")
            topk = TopK(torch.empty((topk,) + tuple(size), dtype=torch.uint8, device=device), torch.empty((topk,) + tuple(size), dtype=torch.float32, device=device))
        _check_labels(self.labels, self.evaluator, self.calibration, self.selective, self.topk_evaluator, self.boundary, self.segments, self.panoptic)
        return dataclasses.replace(self, conf=conf, topk=topk)

    def map_buffer(self, size, device):
        """The uint8 [B, Ho, Wo] buffer the map is written into: plane 0 of the top-k classes where there are any (the same storage, no second store)."""
        return self.topk.classes[0] if self.topk is not None else torch.empty(tuple(size), dtype=torch.uint8, device=device)

    def count(self, out):
        """What `labels=` feed, from the stored map `out` (and the confidence next to it): one more launch each -- the confusion counts
        (mmsa_eval_confusion_u8), the reliability bins (mmsa_eval_calibration), the per-bin confusion counts (mmsa_eval_selective)."""
        if self.evaluator is not None:
            self.evaluator.add(out, self.labels, case=self.case)
        if self.calibration is not None:
            self.calibration.add(out, self.conf, self.labels, case=self.case)
        if self.selective is not None:
            self.selective.add(out, self.conf, self.labels, case=self.case)
        if self.topk_evaluator is not None:      # the rank counts (mmsa_eval_topk_u8), from the stored planes
            self.topk_evaluator.add(self.topk.classes, self.labels, case=self.case)
        self.count_boundary(out)
        self.count_segments(out)

    def count_boundary(self, out):
        """The boundary counts (mmsa_eval_boundary_u8) of the stored map `out`: one more launch, whatever launch wrote the map."""
        if self.boundary is not None:
            self.boundary.add(out, self.labels, case=self.case)

    def count_segments(self, out):
        """The segment counts (mmsa_components_u8 on both sides, mmsa_eval_segments) of the stored map `out`, whatever launch wrote the map; then the panoptic
        counts (a PanopticEvaluator.add: the same launches, mmsa_segment_pairs and mmsa_eval_panoptic) where `panoptic=` is given."""
        if self.segments is not None:
            self.segments.add(out, self.labels, case=self.case)
        if self.panoptic is not None:
            self.panoptic.add(out, self.labels, case=self.case)
        if self.segment_table is not None:      # needs no labels: the components of the stored map, then mmsa_segment_table
            self.segment_table.update(out, values=self.topk.probs[0] if self.topk is not None else self.conf)
        if self.tracker is not None:            # behind its table: the frame's segments against the previous frame's (mmsa_track_pairs, mmsa_track_update)
            self.tracker.update()


@dataclasses.dataclass(frozen=True)
class MapPlan:
    """The output geometry of one frame batch, decided on the host before anything is launched: B x (H x W) is the canvas the windows cover, hc x wc the
    window size, `jobs` the windows (image, y0, x0) in the accumulation order of slide_inference, Hd x Wd the size after the second resize of
    `rescale=True` (H x W when there is none) and Ho x Wo the size after the cut of 'whole_dim_cut' (Hd x Wd without one): the class map is
    uint8 [B, Ho, Wo].  Made by `slide` (a window grid; target `ori_shape`) or `whole` (one full-size window per image; target `ori_shape` or `dim`, cut
    `cut_dim`), which own the refusals of a geometry; `class_map` is the launch."""
    B: int
    H: int
    W: int
    hc: int
    wc: int
    jobs: tuple
    Hd: int
    Wd: int
    Ho: int
    Wo: int

    @classmethod
    def slide(cls, B, H, W, crop_size, stride, ori_shape=None, what="slide_class_map"):
        """The window grid of ED:198-212 on a B x H x W frame batch; `ori_shape` (h, w[, 3]): the target of ED:227-233 (None: no second resize)."""
        hc, wc = crop_size
        if H < hc or W < wc:
            raise RuntimeError(f"mmsa.{what}: the image must be at least as large as the crop")
        Hd, Wd = _target(ori_shape, H, W, what) or (H, W)
        jobs = tuple((b, y1, x1) for y1, x1, _, _ in crop_boxes(H, W, crop_size, stride) for b in range(B))
        return cls(B, H, W, hc, wc, jobs, Hd, Wd, Hd, Wd)

    @classmethod
    def whole(cls, B, H, W, ori_shape=None, dim=None, cut_dim=None, rescale=True, what="whole_class_map"):
        """One window per image, the image itself.  `ori_shape`: 'whole' (ED:314-325); `dim` (h, w): 'whole_dim' (ED:349-360); `dim` + `cut_dim` (w, h):
        'whole_dim_cut' (ED:393-414), the top-left [:cut_dim[1], :cut_dim[0]] of the map at `dim` (`rescale`) or at the input size, clamped to it."""
        if cut_dim is not None and dim is None:
            raise RuntimeError(f"mmsa.{what}: cut_dim= comes with dim= (test_cfg of 'whole_dim_cut')")
        if dim is not None and ori_shape is not None:
            raise RuntimeError(f"mmsa.{what}: the whole_dim modes rescale to dim=, not to ori_shape=; give one of them")
        if dim is not None and cut_dim is None and not rescale:
            raise RuntimeError(f"mmsa.{what}: 'whole_dim' with rescale=False has no defined result in the reference (encoder_decoder.py:334-346 "
                               "returns None); use ori_shape= / no target, or dim= with cut_dim=")
        Hd, Wd = _target((dim if dim is not None else ori_shape) if rescale else None, H, W, what) or (H, W)
        Ho, Wo = (min(int(cut_dim[1]), Hd), min(int(cut_dim[0]), Wd)) if cut_dim is not None else (Hd, Wd)
        if Ho < 1 or Wo < 1:
            raise RuntimeError(f"mmsa.{what}: cut_dim {tuple(cut_dim)} leaves nothing of the map")
        return cls(B, H, W, H, W, tuple((b, 0, 0) for b in range(B)), Hd, Wd, Ho, Wo)

    def check_windows(self, what, per="call"):
        """What the one-pass class-map kernels ask of the windows (slide_inference asks neither): overlap up to MAX_OVERLAP, at most 64 windows."""
        _check_overlap({(y0, x0, y0 + self.hc, x0 + self.wc) for _, y0, x0 in self.jobs}, what)
        if self.n > 64:
            raise RuntimeError(f"mmsa.{what}: at most 64 windows per {per}")

    @property
    def n(self):
        return len(self.jobs)

    @property
    def resized(self):
        """A second resize applies (_target gave a size: one other than the canvas's own)."""
        return (self.Hd, self.Wd) != (self.H, self.W)

    @property
    def rescaled(self):
        """A second resize or a cut applies: the map comes from mmsa_slide_argmax_resized (or the canvas path), not from mmsa_slide_argmax."""
        return self.resized or (self.Ho, self.Wo) != (self.H, self.W)

    @property
    def rs(self):
        return (self.Hd, self.Wd, self.Ho, self.Wo) if self.rescaled else None

    @functools.cached_property
    def windows(self):
        """`jobs` in the form the crop launches take: (image, (y1, x1, y2, x2))."""
        return [(b, (y0, x0, y0 + self.hc, x0 + self.wc)) for b, y0, x0 in self.jobs]

    @functools.cached_property
    def tab(self):
        """`jobs` as the int [n, 3] window table of the kernels."""
        return (ctypes.c_int * (3 * self.n))(*[v for job in self.jobs for v in job])

    def _args(self, lg, out, conf=None):
        """The leading arguments the class-map entries share; the `_conf` entries take `conf` behind `out`."""
        outs = (out.data_ptr(),) if conf is None else (out.data_ptr(), conf.data_ptr())
        return (lg.data_ptr(), self.n, lg.shape[1], lg.shape[2], lg.shape[3], self.tab) + outs + (self.B, self.H, self.W, self.hc, self.wc)

    def _launch(self, lg, out, unc, o):
        """The one-pass launch of the plan, mmsa_slide_argmax[_resized], or the sibling that also writes o.conf: `_conf`; `_conf_t` with an inverse temperature
        o.it; `_score` with o.kind 1 / 2, which always takes an inverse temperature (1.0 without o.it: the untempered softmax, exactly) and 1 / log C.
        With o.topk (frame size only): mmsa_slide_argmax_topk, the K planes in the place of out / conf (`out` is plane 0 of the classes), K and the inverse
        temperature behind the uncovered-pixel word."""
        if o.topk is not None:
            lib.call("mmsa_slide_argmax_topk", *self._args(lg, o.topk.classes, o.topk.probs), unc.data_ptr(), o.topk.classes.shape[0],
                     1.0 if o.it is None else o.it, ops._stream())
            return
        if o.conf is None:
            suffix, tail = "", ()
        elif o.kind:
            suffix, tail = "_score", (o.kind, 1.0 if o.it is None else o.it, _inv_log_c(lg.shape[1]))
        elif o.it is None:
            suffix, tail = "_conf", ()
        else:
            suffix, tail = "_conf_t", (o.it,)
        lib.call("mmsa_slide_argmax" + ("_resized" if self.rescaled else "") + suffix, *self._args(lg, out, o.conf), *(self.rs or ()), unc.data_ptr(), *tail,
                 ops._stream())

    def class_map(self, lg, out, unc, labels=None, evaluator=None, case=None, fused=None, return_map=True, one_pass=None, conf=None, calibration=None,
                  selective=None, temperature=None, score="max", topk=None, topk_evaluator=None, segments=None, panoptic=None, segment_table=None, boundary=None):
        """The class-map launch of the three class-map calls, from the head-resolution logits lg [n, C, hs, ws] into out uint8 [B, Ho, Wo] and the
        uncovered-pixel word `unc`.  Without `labels`: mmsa_slide_argmax.  With `labels` (raw uint8 label maps [B, Hl, Wl]) and `evaluator`
        (mmsa.evaluate.Evaluator): the confusion counts of the map are ADDED to the evaluator's buffer as well -- by the same launch
        (mmsa_slide_argmax_eval: `fused=True`) or by a second one over the stored map (mmsa_eval_confusion_u8); `fused=None` takes mmsa.evaluate.FUSED_DEFAULT.
        The map is the same either way; `return_map=False` with the fused launch writes none.  No host sync, no allocation.
        A `rescaled` plan: mmsa_slide_argmax_resized, or the canvas path where ONE_PASS_RESCALE_DEFAULT / `one_pass=False` say so; the counts then always go
        through the stored map (no fused variant at the rescaled size).
        `conf` (a contiguous float32 [B, Ho, Wo] tensor on the map's device): the confidence map max_c softmax(logits)[c] (ED:449,460) is written too, by
        the `_conf` sibling of the launch the plan takes (mmsa_slide_argmax_conf / mmsa_slide_argmax_resized_conf; on the canvas path
        mmsa_softmax_flip_accum_nchw + mmsa_argmax_max_nchw): bit for bit probabilities(...).max(1), 0 where the map is 255.  The fused evaluation launch
        has no such sibling: `fused=True` / `return_map=False` are refused, and counts go through the stored map.
        `calibration` (mmsa.evaluate.Calibration; needs `labels` and `conf`, `evaluator` is optional with it): the reliability bins of the map and its
        confidence are ADDED to its buffer by one more launch over the stored map and confidence (mmsa_eval_calibration), whatever launch wrote them.
        `selective` (mmsa.evaluate.SelectiveEvaluator; needs `labels` and `conf`, `evaluator` and `calibration` are optional next to it): the confusion
        counts per confidence bin are ADDED to its buffer in the same way (mmsa_eval_selective).
        `temperature` (T > 0; needs `conf`): `conf` gets the confidence of softmax(logits / T), max_c of probabilities(..., temperature=T) bit for bit, from the
        `_t` sibling of the launch the plan takes (mmsa_slide_argmax_conf_t / mmsa_slide_argmax_resized_conf_t; on the canvas path
        mmsa_softmax_flip_accum_nchw_t); the map is the same for every T, and `calibration` / `selective` see the tempered confidence.  None: the launches
        above, with the arguments above.
        `score` ("max" | "margin" | "entropy"; other than "max" needs `conf`): what `conf` gets -- the confidence above, the top-2 margin P_(1) - P_(2) or the
        entropy score 1 - H / log C (csrc/softmax_px.h), each in [0, 1] with higher = more certain and 0 where the map is 255, so `calibration` / `selective`
        take any of them.  "margin" / "entropy" go to the `_score` launch in the place of the `_conf` one (mmsa_slide_argmax_score /
        mmsa_slide_argmax_resized_score; on the canvas path mmsa_argmax_score_nchw on the probabilities), with `temperature` as above: bit for bit the score of
        probabilities(..., temperature=T).  At a rescaled size `one_pass=None` follows ONE_PASS_SCORE_RESCALE_DEFAULT for them (measured: the canvas path).
        "max": the launches above, with the arguments above.
        `topk` (a TopK of contiguous buffers, classes uint8 and probs float32 [K, B, Ho, Wo], 1 <= K <= 8; `out` must be its classes[0]): the first K classes
        of every pixel and their probabilities (csrc/softmax_px.h) are written rank-major -- plane 0 is the map and its confidence, bit for bit -- by
        mmsa_slide_argmax_topk at the frame's size, and at a rescaled or cut size by the canvas path with mmsa_argmax_topk_nchw(first = the stored map) on its
        probabilities (`one_pass=True` is refused there: no one-pass launch is built).  `temperature` is accepted with it; `conf`, `score` other than "max",
        `calibration`, `selective`, `fused=True` and `return_map=False` are refused.  `topk_evaluator` (mmsa.evaluate.TopKEvaluator; needs `labels` and `topk`):
        the rank counts of the planes are ADDED to its buffer by one more launch (mmsa_eval_topk_u8).  None: the launches above, with the arguments above.
        `boundary` (mmsa.evaluate.BoundaryEvaluator; needs `labels`, refused with `return_map=False`): the boundary counts of the stored map `out` are ADDED to
        its buffer by one more launch (mmsa_eval_boundary_u8) behind whatever launch wrote the map.  None: the launches above, and no other.
        `segments` (mmsa.evaluate.SegmentEvaluator; needs `labels`, refused with `return_map=False`): the segment counts of the stored map `out` are ADDED to
        its buffer in the same way (mmsa_components_u8 for the map and for the labels, mmsa_eval_segments).  None: the launches above, and no other.
        `panoptic=` (mmsa.evaluate.PanopticEvaluator; needs `labels=`, refused with `return_map=False`): the stored map's segments are matched with the label
        segments by IoU > 1/2 and TP / FP / FN and the IoU sum are ADDED to its counts (the launches of `segments=`, mmsa_segment_pairs, mmsa_eval_panoptic).  None: no launch."""
        o = MapOptions.of("inference", conf, temperature, score, one_pass, topk=topk, labels=labels, evaluator=evaluator, case=case, calibration=calibration,
                          selective=selective, fused=fused, return_map=return_map, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table)
        o = o.at((self.B, self.Ho, self.Wo), out.device if conf is not None or topk is not None else None, "inference", make=False)
        if o.topk is not None and (out.data_ptr() != o.topk.classes.data_ptr() or tuple(out.shape) != tuple(o.topk.classes.shape[1:]) or not out.is_contiguous()):
            raise RuntimeError("mmsa.inference: with topk= the map is plane 0 of the top-k classes: pass out=topk.classes[0]")
        self._class_map(lg, out, unc, o)

    def _class_map(self, lg, out, unc, o):
        """`class_map` for the entries, which have made their MapOptions `o` under their own name: nothing of the family is checked again."""
        if self.rescaled:
            if o.fused or not o.return_map:
                raise RuntimeError("mmsa.inference: fused=True / return_map=False need the fused class-map + evaluation launch, and that launch has no variant at "
                                   "a rescaled or cut size: the counts of a rescaled map go through the stored map (drop fused= / return_map=)")
            default = ONE_PASS_SCORE_RESCALE_DEFAULT if o.kind else ONE_PASS_RESCALE_DEFAULT
            one_pass = default["up" if self.Hd * self.Wd > self.H * self.W else "down"] if o.one_pass is None else o.one_pass
            if o.topk is not None:
                if o.one_pass:
                    raise RuntimeError(f"mmsa.inference: topk= {_NO_TOPK_ONE_PASS}")
                one_pass = False
            fused = False
        else:
            if o.one_pass is not None:
                raise RuntimeError("mmsa.inference: one_pass= chooses the launch of a RESCALED class map; this map has the frame's size")
            if o.evaluator is None and not o.return_map:
                raise RuntimeError("mmsa.inference: return_map=False only makes sense with labels= and evaluator=")
            if o.fused is False and not o.return_map:
                raise RuntimeError("mmsa.inference: return_map=False needs the fused launch (two launches go through the stored map); drop fused=False")
            from . import evaluate
            one_pass = True      # fused: never with `conf`; no map wanted: only the fused launch can leave it unwritten
            fused = o.evaluator is not None and o.conf is None and o.topk is None and ((evaluate.FUSED_DEFAULT or not o.return_map) if o.fused is None else o.fused)
        if fused:
            o.evaluator.add_fused(lg, self, out if o.return_map else None, unc, o.labels, case=o.case)
            o.count_boundary(out)      # refused with return_map=False: the fused launch has stored the map
            o.count_segments(out)
            return
        if one_pass:
            self._launch(lg, out, unc, o)
        else:
            _rescaled_map_canvas(self, lg, out, unc, o.conf, o.it, o.kind, o.topk)
        o.count(out)


def _canvas_logits(plan, lg, unc):
    """The logits of a plan at its target size the long way round, from the head-resolution logits lg [n, C, hs, ws] and the plan's windows: canvas
    (accumulate, count, divide), second canvas -> [B, C, Hd, Wd] -- the launches slide_inference / encode_decode make.  `unc` gets the number of CANVAS
    pixels that no window covers (non-zero exactly when the one-pass kernels' count of output pixels may be)."""
    B, H, W, C = plan.B, plan.H, plan.W, lg.shape[1]
    canvas = torch.zeros(B, C, H, W, device=lg.device)
    count = torch.zeros(B, H, W, device=lg.device)
    for k, (b, y0, x0) in enumerate(plan.jobs):
        _resize_into(lg[k:k + 1], canvas[b:b + 1], y0, x0, plan.hc, plan.wc, count=count[b:b + 1], accumulate=True)
    unc.add_((count == 0).sum().to(torch.int32))
    lib.call("mmsa_div_count_nchw", canvas.data_ptr(), count.data_ptr(), B, C, H * W, ops._stream())
    return _rescaled_logits(canvas, (plan.Hd, plan.Wd) if plan.resized else None)


def _argmax_topk_into(prob, first, topk):
    """mmsa_argmax_topk_nchw on a canvas of probabilities [B, C, H, W] into the planes of `topk`; `first`: None, or the uint8 [B, H, W] map that names rank 0
    (it may be topk.classes[0] itself)."""
    B, C, H, W = prob.shape
    lib.call("mmsa_argmax_topk_nchw", prob.data_ptr(), None if first is None else first.data_ptr(), topk.classes.data_ptr(), topk.probs.data_ptr(), B, C, H, W,
             topk.classes.shape[0], ops._stream())


def _rescaled_map_canvas(plan, lg, out, unc, conf=None, it=None, kind=0, topk=None):
    """The rescaled class map the long way round: _canvas_logits, argmax, crop -- the launches slide_inference / encode_decode + argmax_map make.  With
    `conf`: also the softmax of the cut logits (what `probabilities` launches) and mmsa_argmax_max_nchw for its maximum.  The MAP stays the argmax of the
    logits, as without `conf` and as in the one-pass kernels: the softmax can round two distinct logits to one probability, and the first class would win.
    `it` (an inverse temperature, with `conf`): the softmax of logits / T (mmsa_softmax_flip_accum_nchw_t).
    `kind` (1 / 2, with `conf`): mmsa_argmax_score_nchw in the place of mmsa_argmax_max_nchw -- the margin or the entropy score of those probabilities.
    `topk` (a TopK whose classes[0] is `out`, without `conf`): the top-k tail -- the same softmax, then mmsa_argmax_topk_nchw with first = the stored map, in
    place: rank 0 stays the argmax of the LOGITS."""
    y = _canvas_logits(plan, lg, unc)
    out.copy_(argmax_map(y)[:, :plan.Ho, :plan.Wo])
    if conf is None and topk is None:
        return
    y = y[:, :, :plan.Ho, :plan.Wo].contiguous()
    prob = torch.empty_like(y)
    _softmax_accum(y, prob, it=it)
    if topk is not None:
        _argmax_topk_into(prob, out, topk)
    else:
        _argmax_into(prob, torch.empty_like(out), conf, kind)


def _window_logits(backbone, head, cut, windows, max_batch):
    """The windows through backbone and head in batches of `max_batch`, concatenated -> the head-resolution logits [n, classes, hs, ws]."""
    lgs = [head(backbone(cut(windows[s:s + max_batch]))[0]) for s in range(0, len(windows), max_batch)]
    return lgs[0] if len(lgs) == 1 else torch.cat(lgs, 0)


@_on_device
@torch.no_grad()
def slide_class_map(backbone, head, img, crop_size, stride, max_batch=8, preprocess=None, labels=None, evaluator=None, case=None, fused=None,
                    return_map=True, render=None, ori_shape=None, one_pass=None, confidence=False, calibration=None, selective=None, temperature=None,
                    score="max", topk=None, topk_evaluator=None, segments=None, panoptic=None, segment_table=None, boundary=None):
    """`simple_test` of a sliding-window frame (ED:191-234 + ED:449,477) -> uint8 class map [B, H, W], without the
    [B, classes, H, W] logits canvas: every window's logits stay at head resolution and ONE kernel (mmsa_slide_argmax) resizes,
    sums the overlapping windows in window order, divides by the count and takes the argmax -- the same additions in the same order
    as slide_inference + argmax_map, so the same class map bit for bit.  All windows of the frame go through the encoder in
    batches of `max_batch`; with static shapes the whole function is HIP-graph capturable (no host sync inside).
    `preprocess=` (mmsa.preprocess.Preprocess): img is the pair (rgb, aux) of raw frames; the windows are cut AND normalised by one launch.
    `labels=` + `evaluator=` (mmsa.evaluate.Evaluator; `case=` with a per-case one): the map's confusion counts are added to the evaluator on device
    (see MapPlan.class_map); the returned map is unchanged, `return_map=False` returns None in its place.
    `render=` (mmsa.render.Renderer): a second launch paints the frame's picture (test_bs.py:257-349, `show_result`) -> (map, unc, picture uint8
    [B, H, W, 3]); over the raw uint8 RGB frames with `preprocess=` (they must have the map's size), else over the de-normalised `img`.
    `ori_shape=` (h, w[, 3]): the map of `rescale=True` (ED:227-233), uint8 [B, h, w] -- the averaged logits resized once more before the argmax, by the
    same single launch (mmsa_slide_argmax_resized; `one_pass=False`: by the canvas path), bit for bit argmax_map(slide_inference(..., ori_shape=)).  None or
    the frame's own size: the launch above.  A LabelPrep for `labels=` must be built for [h, w]; `fused=True` / `return_map=False` are refused; `render=`
    needs raw uint8 frames of [h, w].
    `confidence=` True, or a contiguous float32 [B, h, w] tensor on the device to write into (nothing is allocated for it, so the launch can be captured):
    the confidence map -- the probability of the predicted class, bit for bit probabilities(...).max(1).values, 0 where the map is 255 -- is written by the
    same launch and returned as the LAST element: (map, unc[, picture], conf).  Refused with `fused=True` / `return_map=False`; `labels=` count through the
    stored map.
    `calibration=` (mmsa.evaluate.Calibration; `case=` with a per-case one): the reliability bins of the map and its confidence against `labels=` are
    added to it on device by one more launch (mmsa_eval_calibration), no host sync; it needs `labels=` and `confidence=`, `evaluator=` is optional with
    it, and what is returned does not change.
    `selective=` (mmsa.evaluate.SelectiveEvaluator; `case=` with a per-case one): one confusion matrix per confidence bin of the map and its confidence
    against `labels=` is added to it on device by one more launch (mmsa_eval_selective), no host sync; it needs `labels=` and `confidence=`, `evaluator=`
    and `calibration=` are optional next to it, and what is returned does not change.
    `temperature=` (T > 0, from mmsa.evaluate.TemperatureSweep.best(); needs `confidence=`): the confidence map is that of softmax(logits / T) --
    probabilities(..., temperature=T).max(1).values bit for bit -- written by the `_t` sibling of the same launch; the map is the same for every T, and
    `calibration=` / `selective=` see the tempered confidence.  Without `confidence=` it is refused: the map does not depend on it.
    `score=` "max" (the confidence above), "margin" (the top-2 margin P_(1) - P_(2)) or "entropy" (1 - H / log C, H the predictive entropy): what the map in
    the confidence slot holds -- each in [0, 1], higher = more certain, 0 where the map is 255, written by the launch that writes the class map
    (mmsa_slide_argmax_score) or, with `ori_shape=`, by mmsa_argmax_score_nchw on the canvas path's probabilities -- the default there, being the faster of the
    two where measured (ONE_PASS_SCORE_RESCALE_DEFAULT) -- or by mmsa_slide_argmax_resized_score (`one_pass=True`: no canvas in memory); the same bits either way.
    `temperature=` combines with it; `calibration=` / `selective=` see whatever score was written.  Other than "max" it is refused without `confidence=`.
    `topk=` K (1 .. 8), or a TopK of two buffers to write into (classes uint8, probs float32, both contiguous [K, B, h, w] on the device: nothing is allocated,
    so the launch can be captured): the first K classes of every pixel and their probabilities, rank-major -- rank 0 the class the map names, rank r >= 1 the
    largest remaining probability (the lowest class among equal ones), 255 / 0 from rank C on and where the map is 255 -- written by the launch that writes
    the class map (mmsa_slide_argmax_topk) or, with `ori_shape=`, by mmsa_argmax_topk_nchw on the canvas path's probabilities (`one_pass=True` is refused:
    no one-pass launch is built there).  Returned as the LAST element: (map, unc[, picture], topk), where map IS topk.classes[0] (the same storage),
    topk.probs[0] is the `confidence=True` map and topk.probs[0] - topk.probs[1] the `score="margin"` map, bit for bit; every plane is a map the evaluation
    passes take.  `temperature=` is accepted with it.  `confidence=`, `score=` other than "max", `calibration=`, `selective=`, `fused=True` and
    `return_map=False` are refused with it.
    `topk_evaluator=` (mmsa.evaluate.TopKEvaluator of the same K; needs `labels=` and `topk=`): the rank of the label's class is counted on device by one
    more launch (mmsa_eval_topk_u8) -- top-k pixel accuracy next to mIoU; `evaluator=` is optional with it.
    `boundary=` (mmsa.evaluate.BoundaryEvaluator; `case=` with a per-case one; needs `labels=`, `evaluator=` is optional with it): the map's confusion counts
    split by nearness to a label boundary and to a prediction boundary -- trimap mIoU and Boundary IoU -- are added to it on device by one more launch over the
    STORED map (mmsa_eval_boundary_u8): plane 0 with `topk=`, the rescaled map with `ori_shape=`.  `return_map=False` is refused with it; what is returned
    does not change.
    `segments=` (mmsa.evaluate.SegmentEvaluator; `case=` with a per-case one; needs `labels=`, `evaluator=` is optional with it): the label segments and the
    map's segments -- connected components of one class -- are counted by class, size and coverage into it on device (mmsa_components_u8 for each side,
    mmsa_eval_segments), over the same STORED map and under the same terms as `boundary=`: segment recall and precision next to mIoU.
    `panoptic=` (mmsa.evaluate.PanopticEvaluator; needs `labels=`, refused with `return_map=False`): the stored map's segments are matched with the label
    segments by IoU > 1/2 and TP / FP / FN and the IoU sum are ADDED to its counts (the launches of `segments=`, mmsa_segment_pairs, mmsa_eval_panoptic).
    `segment_table=` (mmsa.evaluate.SegmentTable made with num_classes=; needs no `labels=`, refused with `return_map=False`): the table is filled from the
    stored map -- plane 0 with `topk=`, the rescaled or cut map with `ori_shape=` -- by SegmentTable.update (mmsa_components_u8, mmsa_segment_table), its
    `values` the confidence or score map where `confidence=` was asked, probs[0] with `topk=`, nothing otherwise.  None: no launch.  Every class-map entry
    (whole_class_map, class_map, aug_class_map, MapPlan.class_map, SlideRunner.run) takes it in the same way."""
    o = MapOptions.of("slide_class_map", confidence, temperature, score, one_pass, topk=topk, labels=labels, evaluator=evaluator, case=case,
                      calibration=calibration, selective=selective, fused=fused, return_map=return_map, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table)
    return _slide_class_map(o, backbone, head, img, crop_size, stride, max_batch, preprocess, render, ori_shape)


def _slide_class_map(o, backbone, head, img, crop_size, stride, max_batch=8, preprocess=None, render=None, ori_shape=None):
    """slide_class_map behind its options (`class_map` comes here with its own)."""
    B, H, W, device, frame, cut = _intake(img, preprocess, "slide_class_map")
    plan = MapPlan.slide(B, H, W, crop_size, stride, ori_shape)
    src = None if render is None else slide_source(render, preprocess, frame, plan, o.return_map, "slide_class_map")
    plan.check_windows("slide_class_map")
    o = o.at((B, plan.Ho, plan.Wo), device, "slide_class_map")
    _pair(backbone, head)
    lg = _window_logits(backbone, head, cut, plan.windows, max_batch)
    out = o.map_buffer((B, plan.Ho, plan.Wo), device)
    unc = torch.zeros(1, dtype=torch.int32, device=device)
    plan._class_map(lg, out, unc, o)
    r = (out, unc, render(out, src)) if render is not None else ((out if o.return_map else None), unc)   # unc[0] != 0 <=> some pixel is not covered (ED:220); checked by the caller outside a capture
    if o.topk is not None:
        return r + (o.topk,)
    return r if o.conf is None else r + (o.conf,)


@_on_device
@torch.no_grad()
def whole_class_map(backbone, head, img, preprocess=None, labels=None, evaluator=None, case=None, fused=None, return_map=True, render=None,
                    ori_shape=None, dim=None, cut_dim=None, rescale=True, one_pass=None, confidence=False, calibration=None, selective=None, temperature=None,
                    score="max", topk=None, topk_evaluator=None, segments=None, panoptic=None, segment_table=None, boundary=None):
    """Whole-image `simple_test`: resize x4 (bilinear, align_corners=False) + argmax fused (ED:90-94,449,477) -> uint8 [B, H, W].
    `preprocess=` (mmsa.preprocess.Preprocess): img is the pair (rgb, aux) of raw frames, normalised (and padded) by one launch.
    `labels=` + `evaluator=` (+ `case=`): as in slide_class_map.
    `render=` (mmsa.render.Renderer): a second launch paints the frame's picture -> (map, picture uint8 [B, H, W, 3]); over the raw uint8 RGB frames where
    `preprocess=` got frames of the map's size, else over the de-normalised input tensor (a padded or device-resized frame, a float32 RGB modality, no
    `preprocess=`).
    The map at another size, by ONE launch (mmsa_slide_argmax_resized; `one_pass=False`: the canvas path), bit for bit the argmax_map of the logits call named:
      `ori_shape=` (h, w[, 3])  'whole' with rescale (ED:314-325): whole_inference(..., ori_shape=) -> uint8 [B, h, w];
      `dim=` (h, w)             'whole_dim' (ED:349-360): whole_inference_dim(..., dim) -> [B, h, w]; `rescale=False` is refused as it is there;
      `dim=` + `cut_dim=` (w, h) 'whole_dim_cut' (ED:393-414): whole_inference_dim_cut(..., dim, cut_dim, rescale) -> [B, min(cut h, .), min(cut w, .)], the
                                crop [:cut_dim[1], :cut_dim[0]] of the map at `dim` (rescale) or at the input size (`rescale=False`, the FMB configs).
    A LabelPrep for `labels=` must be built for that size; `fused=True` / `return_map=False` are refused; `render=` needs a source of the map's size: raw
    uint8 frames of the size before the cut, or -- for a cut alone -- the input tensor.
    `confidence=`: as in slide_class_map; the confidence map float32 [B, Ho, Wo] comes as the last element, (map[, picture], conf).
    `calibration=`: as in slide_class_map (needs `labels=` and `confidence=`); at a rescaled or cut size the pass reads the map and confidence stored there.
    `selective=`: as in slide_class_map (needs `labels=` and `confidence=`), over the map and confidence stored at the size returned.
    `temperature=`: as in slide_class_map (needs `confidence=`): the confidence of softmax(logits / T) at the size returned.
    `score=`: as in slide_class_map ("margin" / "entropy" need `confidence=`): the map in the confidence slot is that score, at the size returned.
    `topk=` / `topk_evaluator=`: as in slide_class_map; the TopK (planes [K, B, Ho, Wo]) comes as the last element, (map[, picture], topk), at the size
    returned: mmsa_slide_argmax_topk at the input size, the canvas path + mmsa_argmax_topk_nchw at a rescaled or cut size (`one_pass=True` is refused).
    `boundary=`: as in slide_class_map (needs `labels=`), over the map stored at the size returned (rescaled, cut).
    `segments=` and `panoptic=`: as in slide_class_map too, over the same stored map."""
    o = MapOptions.of("whole_class_map", confidence, temperature, score, one_pass, topk=topk, labels=labels, evaluator=evaluator, case=case,
                      calibration=calibration, selective=selective, fused=fused, return_map=return_map, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table)
    return _whole_class_map(o, backbone, head, img, preprocess, render, ori_shape, dim, cut_dim, rescale)


def _whole_class_map(o, backbone, head, img, preprocess=None, render=None, ori_shape=None, dim=None, cut_dim=None, rescale=True):
    """whole_class_map behind its options (`class_map` comes here with its own)."""
    rgb = None
    if preprocess is not None:
        rgb, aux, B, H, W = _raw(preprocess, img, "whole_class_map")
    else:
        _check(img)
        B, _, H, W = (int(v) for v in img.shape)
    plan = MapPlan.whole(B, H, W, ori_shape, dim, cut_dim, rescale)
    src = None if render is None else whole_source(render, rgb, plan, o.return_map, "whole_class_map")      # the raw frames, or None: the tensor below
    o = o.at((B, plan.Ho, plan.Wo), (rgb if rgb is not None else img).device, "whole_class_map")
    if preprocess is not None:
        img = preprocess(rgb, aux)
    if render is not None and src is None:
        src = img = img.contiguous()
    _pair(backbone, head)
    feats, _ = backbone(img)
    lg = head(feats)
    out = o.map_buffer((B, plan.Ho, plan.Wo), img.device)
    unc = torch.zeros(1, dtype=torch.int32, device=img.device)
    plan._class_map(lg, out, unc, o)
    if o.topk is not None:
        return (out, o.topk) if render is None else (out, render(out, src), o.topk)
    if render is not None:
        return (out, render(out, src)) if o.conf is None else (out, render(out, src), o.conf)
    if o.conf is not None:
        return out, o.conf
    return out if o.return_map else None


@_on_device
@torch.no_grad()
def whole_inference(backbone, head, img, rescale=True, ori_shape=None):
    """ED:310-327: whole-image mode = encode_decode on the full input; with `rescale` and an `ori_shape` (h, w[, 3]) other than the input's, resized once
    more to [B, classes, h, w] (ED:314-325)."""
    y = encode_decode(backbone, head, img)
    return _rescaled_logits(y, _target(ori_shape, y.shape[2], y.shape[3], "whole_inference") if rescale else None)


@_on_device
@torch.no_grad()
def whole_inference_dim(backbone, head, img, dim, rescale=True):
    """ED:329-362 -- `test_cfg.mode = 'whole_dim'`, the test mode of every DELIVER config (dim = (1024, 1024)): the logits at input size
    (encode_decode), resized once more (bilinear, align_corners=False) to `dim`.  The reference's method has no result for
    `rescale=False` (it returns None and `inference` fails on it, ED:334-346,448): that call is refused here."""
    if not rescale:
        raise RuntimeError("mmsa.whole_inference_dim: rescale=False has no defined result in the reference (encoder_decoder.py:334-346 "
                           "returns None); use whole_inference or whole_inference_dim_cut")
    y = encode_decode(backbone, head, img)
    return _rescaled_logits(y, _target(dim, y.shape[2], y.shape[3], "whole_inference_dim"))      # `dim` = the input size: y itself, no copy


@_on_device
@torch.no_grad()
def whole_inference_dim_cut(backbone, head, img, dim, cut_dim, rescale=True):
    """ED:364-413 -- `test_cfg.mode = 'whole_dim_cut'`, the test mode of every FMB config (rescale=False, dim=(600,800), cut_dim=(800,600)):
    the logits at input size, resized to `dim` when `rescale`, cropped to [:, :, :cut_dim[1], :cut_dim[0]] (a contiguous copy)."""
    y = encode_decode(backbone, head, img)
    y = _rescaled_logits(y, _target(dim, y.shape[2], y.shape[3], "whole_inference_dim_cut") if rescale else None)
    return y[:, :, :cut_dim[1], :cut_dim[0]].contiguous()


@_on_device
@torch.no_grad()
def inference(backbone, head, img, test_cfg, rescale=True, preprocess=None, ori_shape=None, max_batch=8):
    """ED:417-447 dispatch on `test_cfg['mode']` -- 'slide', 'whole', 'whole_dim', 'whole_dim_cut' ('slide_mod_sel' runs the segmentor's
    modality-selection variant, ED:236-308, which needs a backbone with a selection head: not this backbone) -- returning the logits the
    reference softmaxes (ED:448-470; `probabilities` is that softmax and the un-flip; the views come flipped from the caller, as from the reference's test
    pipeline).  `max_batch`: the windows of 'slide' per backbone call.
    `preprocess=` (mmsa.preprocess.Preprocess): img is the pair (rgb, aux) of raw frames -- 'slide' cuts its windows from them, the whole modes
    normalise the frame first.
    `ori_shape=` (h, w[, 3]) of the frame's meta: with `rescale`, 'slide' and 'whole' resize their logits to it (ED:227-233, 314-325); the `whole_dim*`
    modes rescale to `test_cfg['dim']` and ignore it, as the reference does."""
    mode = test_cfg["mode"]
    if mode == "slide":
        return slide_inference(backbone, head, img, tuple(test_cfg["crop_size"]), tuple(test_cfg["stride"]), max_batch=max_batch, preprocess=preprocess,
                               rescale=rescale, ori_shape=ori_shape)
    if preprocess is not None and mode in ("whole", "whole_dim", "whole_dim_cut"):
        img = preprocess(*_raw(preprocess, img, "inference")[:2])
    if mode == "whole":
        return whole_inference(backbone, head, img, rescale=rescale, ori_shape=ori_shape)
    if mode == "whole_dim":
        return whole_inference_dim(backbone, head, img, tuple(test_cfg["dim"]), rescale)
    if mode == "whole_dim_cut":
        return whole_inference_dim_cut(backbone, head, img, tuple(test_cfg["dim"]), tuple(test_cfg["cut_dim"]), rescale)
    raise RuntimeError(f"mmsa.inference: test_cfg.mode '{mode}' is not one of slide / whole / whole_dim / whole_dim_cut")


@_on_device
@torch.no_grad()
def class_map(backbone, head, img, test_cfg, rescale=True, ori_shape=None, preprocess=None, labels=None, evaluator=None, case=None, render=None, one_pass=None,
              confidence=False, calibration=None, selective=None, temperature=None, score="max", topk=None, topk_evaluator=None, segments=None, panoptic=None, segment_table=None, boundary=None):
    """`simple_test` (ED:471-477) by mode: the dispatch of `inference` (ED:417-447) onto the class-map calls -> uint8 map, bit for bit
    argmax_map(inference(...)) of the same arguments, without a logits canvas: [B, H, W], or at the size `rescale` gives ('slide' / 'whole': `ori_shape`;
    'whole_dim': test_cfg['dim']; 'whole_dim_cut': the crop of the map at `dim`, or at the input size without `rescale`).  What `inference` refuses is
    refused here ('slide_mod_sel'; 'whole_dim' with rescale=False).  'slide' reads the kernel's uncovered-pixel word back (one host sync, as
    slide_inference's coverage check is) and raises on a window grid that does not cover the frame (ED:220).
    `preprocess=`, `labels=` + `evaluator=` (+ `case=`; through the stored map), `render=` (-> (map, picture)), `one_pass=`: as in the calls it goes to.
    `confidence=` (True or an output tensor): the confidence map, probabilities(...).max(1).values bit for bit, as the last element: (map[, picture], conf).
    `calibration=` (mmsa.evaluate.Calibration; needs `labels=` and `confidence=`): as in the calls it goes to.
    `selective=` (mmsa.evaluate.SelectiveEvaluator; needs `labels=` and `confidence=`): as in the calls it goes to.
    `temperature=` (T > 0; needs `confidence=`): the confidence of softmax(logits / T), as in the calls it goes to.
    `score=` ("max" | "margin" | "entropy"; other than "max" needs `confidence=`): what the confidence slot holds, as in the calls it goes to.
    `topk=` (K, or a TopK of output buffers) / `topk_evaluator=` (needs `labels=` and `topk=`): the first K classes and their probabilities as rank-major
    planes, as the last element: (map[, picture], topk) with map = topk.classes[0], as in the calls it goes to.
    `boundary=` (mmsa.evaluate.BoundaryEvaluator; needs `labels=`): the boundary counts of the stored map, as in the calls it goes to.
    `segments=` (mmsa.evaluate.SegmentEvaluator; needs `labels=`): the segment counts of the stored map, likewise.
    `panoptic=` (mmsa.evaluate.PanopticEvaluator; needs `labels=`): the panoptic counts of the stored map, likewise."""
    mode = test_cfg["mode"]
    o = MapOptions.of("class_map", confidence, temperature, score, one_pass, topk=topk, labels=labels, evaluator=evaluator, case=case, calibration=calibration,
                      selective=selective, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table)
    kw = dict(preprocess=preprocess, render=render)
    if mode == "slide":
        r = _slide_class_map(o, backbone, head, img, tuple(test_cfg["crop_size"]), tuple(test_cfg["stride"]), ori_shape=ori_shape if rescale else None, **kw)
        if int(r[1].item()) != 0:
            raise RuntimeError("mmsa.class_map: windows do not cover the image")   # ED:220
        r = (r[0],) + tuple(r[2:])           # without the uncovered-pixel word: (map[, picture][, conf | topk])
        return r[0] if len(r) == 1 else r
    if mode == "whole":
        return _whole_class_map(o, backbone, head, img, ori_shape=ori_shape if rescale else None, **kw)
    if mode == "whole_dim":
        return _whole_class_map(o, backbone, head, img, dim=tuple(test_cfg["dim"]), rescale=rescale, **kw)
    if mode == "whole_dim_cut":
        return _whole_class_map(o, backbone, head, img, dim=tuple(test_cfg["dim"]), cut_dim=tuple(test_cfg["cut_dim"]), rescale=rescale, **kw)
    raise RuntimeError(f"mmsa.class_map: test_cfg.mode '{mode}' is not one of slide / whole / whole_dim / whole_dim_cut")


@_on_device
@torch.no_grad()
def argmax_map(seg_logit):
    """ED:449,477: softmax is monotonic, the prediction is the per-pixel argmax over the class axis -> uint8 [B, H, W]."""
    _check(seg_logit)
    seg_logit = seg_logit.contiguous()
    B, C, H, W = seg_logit.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=seg_logit.device)
    lib.call("mmsa_argmax_nchw", seg_logit.data_ptr(), out.data_ptr(), B, C, H * W, ops._stream())
    return out


def _argmax_max_into(prob, out, conf):
    B, C, H, W = prob.shape
    lib.call("mmsa_argmax_max_nchw", prob.data_ptr(), out.data_ptr(), conf.data_ptr(), B, C, H * W, ops._stream())


def _argmax_score_into(prob, out, score, kind):
    B, C, H, W = prob.shape
    lib.call("mmsa_argmax_score_nchw", prob.data_ptr(), out.data_ptr(), score.data_ptr(), B, C, H, W, kind, _inv_log_c(C), ops._stream())


def _argmax_into(prob, out, conf, kind=0):
    """The argmax of a canvas of probabilities into `out`, with their maximum (`kind` 0) or the score `kind` into `conf`: one launch."""
    if kind:
        _argmax_score_into(prob, out, conf, kind)
    else:
        _argmax_max_into(prob, out, conf)


def _argmax_pair(prob, kind):
    """_argmax_into with new outputs -> (uint8 [B, H, W], float32 [B, H, W])."""
    _check(prob)
    prob = prob.contiguous()
    B, C, H, W = prob.shape
    out = torch.empty(B, H, W, dtype=torch.uint8, device=prob.device)
    conf = torch.empty(B, H, W, dtype=torch.float32, device=prob.device)
    _argmax_into(prob, out, conf, kind)
    return out, conf


@_on_device
@torch.no_grad()
def argmax_max_map(prob):
    """argmax_map that also returns the maximum -> (uint8 [B, H, W], float32 [B, H, W]), one launch (mmsa_argmax_max_nchw).  On the probabilities of
    `probabilities` / `aug_inference` (ED:449,460) the second is the confidence map: the probability of the predicted class."""
    return _argmax_pair(prob, 0)


@_on_device
@torch.no_grad()
def argmax_score_map(prob, score="margin"):
    """argmax_max_map with an uncertainty score in the maximum's place -> (uint8 [B, H, W], float32 [B, H, W]), one launch (mmsa_argmax_score_nchw) on a
    canvas of probabilities (`probabilities` / `aug_inference`): `score=` "margin", the top-2 margin P_(1) - P_(2), or "entropy", 1 - H / log C with H the
    predictive entropy -- on the mean probabilities of augmented views, the usual TTA uncertainty.  Both lie in [0, 1], higher = more certain.  "max" is
    argmax_max_map itself."""
    return _argmax_pair(prob, _score_kind(score, True, "argmax_score_map"))


@_on_device
@torch.no_grad()
def argmax_topk_map(prob, k, first=None):
    """The top-k map of a canvas of probabilities [B, C, H, W] (`probabilities` / `aug_inference`) -> TopK(classes uint8 [k, B, H, W], probs float32
    [k, B, H, W]), rank-major, one launch (mmsa_argmax_topk_nchw): rank 0 is the first maximum -- or, with `first=` (a uint8 [B, H, W] class map of the same
    logits, e.g. argmax_map's: two logits can round to one probability), the class that map names, 255 / 0 at every rank where it is 255 -- and rank r >= 1
    the largest remaining probability, the lowest class among equal ones; 255 / 0 from rank C on."""
    from .evaluate import check_topk
    k = check_topk(k, "mmsa.argmax_topk_map")
    _check(prob)
    prob = prob.contiguous()
    B, C, H, W = prob.shape
    if first is not None:
        if (not isinstance(first, torch.Tensor) or first.dtype != torch.uint8 or tuple(first.shape) != (B, H, W) or first.device != prob.device
                or not first.is_contiguous()):
            raise RuntimeError(f"mmsa.argmax_topk_map: first= must be a contiguous uint8 [B, H, W] = {(B, H, W)} class map on {prob.device}")
    topk = TopK(torch.empty(k, B, H, W, dtype=torch.uint8, device=prob.device), torch.empty(k, B, H, W, dtype=torch.float32, device=prob.device))
    _argmax_topk_into(prob, first, topk)
    return topk


# ---- test-time augmentation: EncoderDecoder.aug_test (ED:509-546) -- several views of a frame (flipped, at several scales), whose probabilities are averaged

MAX_AUGS = 12          # views per call: MMSA_MAX_AUGS of csrc/augment.hip (their descriptors travel in the launch arguments)
MAX_AUG_CLASSES = 128  # classes mmsa_aug_argmax keeps per pixel in LDS; more take the canvas path
FLIPS = {None: 0, "horizontal": 1, "vertical": 2}      # img_meta's flip / flip_direction (ED:450-457) -> the kernels' code

# Which launch makes an AUGMENTED class map by default: True = the one-pass kernel (mmsa_aug_argmax), False = the canvas path (per view: canvas, second
# resize, mmsa_softmax_flip_accum_nchw; then argmax_map -- the same map bit for bit).  `one_pass=` of aug_class_map overrides it.
# Measured (profiles/aug_class_map.txt; 1080 x 1920, six 1024 x 1024 windows, 25 classes): the canvas path wins, 1.9 ms against 7.1 ms for two views and
# 4.9 ms against 8.4 ms for four, far outside its 0.02 - 0.04 ms spread -- the canvases stay in the 256 MB last-level cache, while the one-pass kernel runs
# two waves per SIMD and its pixels under 5 .. 8 windows walk the window table once per class.  One pass remains the choice where memory is: it allocates
# nothing, the canvas path three [B, C, h, w] float32 arrays per view (207 MB each at that size).
ONE_PASS_AUG_DEFAULT = False


def _flip_code(flip, what):
    if flip not in FLIPS:
        raise RuntimeError(f"mmsa.{what}: flip must be None, 'horizontal' or 'vertical' (img_meta's flip_direction, encoder_decoder.py:453), got {flip!r}")
    return FLIPS[flip]


def _softmax_accum(logits, acc, flip=0, accumulate=False, finish_div=0, it=None):
    """ED:448-469 + ED:540-541 on a logits canvas: acc (=|+=) flip(softmax(logits)) [/ finish_div]; `it` (an inverse temperature): softmax(logits * it), by
    mmsa_softmax_flip_accum_nchw_t."""
    B, C, H, W = logits.shape
    if it is None:
        lib.call("mmsa_softmax_flip_accum_nchw", logits.data_ptr(), acc.data_ptr(), B, C, H, W, flip, 1 if accumulate else 0, finish_div, ops._stream())
    else:
        lib.call("mmsa_softmax_flip_accum_nchw_t", logits.data_ptr(), acc.data_ptr(), B, C, H, W, flip, 1 if accumulate else 0, finish_div, it, ops._stream())


def _plan_of(test_cfg, B, H, W, rescale, ori_shape, what):
    """The MapPlan of one frame batch by `test_cfg['mode']`: the dispatch of `class_map` / `inference` (ED:417-447)."""
    mode = test_cfg["mode"]
    if mode == "slide":
        return MapPlan.slide(B, H, W, tuple(test_cfg["crop_size"]), tuple(test_cfg["stride"]), ori_shape if rescale else None, what=what)
    if mode == "whole":
        return MapPlan.whole(B, H, W, ori_shape=ori_shape if rescale else None, what=what)
    if mode == "whole_dim":
        return MapPlan.whole(B, H, W, dim=tuple(test_cfg["dim"]), rescale=rescale, what=what)
    if mode == "whole_dim_cut":
        return MapPlan.whole(B, H, W, dim=tuple(test_cfg["dim"]), cut_dim=tuple(test_cfg["cut_dim"]), rescale=rescale, what=what)
    raise RuntimeError(f"mmsa.{what}: test_cfg.mode '{mode}' is not one of slide / whole / whole_dim / whole_dim_cut")


@_on_device
@torch.no_grad()
def probabilities(backbone, head, img, test_cfg, rescale=True, ori_shape=None, flip=None, preprocess=None, max_batch=8, temperature=None):
    """What the reference's `inference` returns (ED:417-469): F.softmax(seg_logit, dim=1) of `inference(...)`'s logits, flipped back when the view `img`
    was flipped (`flip` = None, 'horizontal' or 'vertical': img_meta's flip_direction) -> float32 [B, classes, Ho, Wo].  One more launch
    (mmsa_softmax_flip_accum_nchw) on the logits; `inference` itself keeps returning logits.
    `temperature=` (T > 0): F.softmax(seg_logit / T, dim=1) instead, by mmsa_softmax_flip_accum_nchw_t (exponent (x - m) * float32(1 / T))."""
    code = _flip_code(flip, "probabilities")
    it = _inv_temperature(temperature, True, "probabilities")
    y = inference(backbone, head, img, test_cfg, rescale=rescale, preprocess=preprocess, ori_shape=ori_shape, max_batch=max_batch).contiguous()
    out = torch.empty_like(y)
    _softmax_accum(y, out, code, it=it)
    return out


@dataclasses.dataclass(frozen=True)
class AugPlan:
    """The MapPlan of several views of one frame batch (`aug_test`, ED:509-546), decided on the host: one MapPlan per view, made by the mode dispatch of
    `class_map`, and the views' flips as the kernels' codes.  All views end at the same [B, Ho, Wo]: the probabilities are added pixel by pixel.
    `table` is the window tables of all views one after the other (view a's rows: offsets[a] .. offsets[a] + plans[a].n - 1), built once; `table_on(device)`
    uploads it on first use and keeps it, so a second call allocates and copies nothing.  `make` / `of` own the refusals of a set of views;
    `class_map` is the launch."""
    plans: tuple
    flips: tuple

    @staticmethod
    def views(imgs, flips=None, preprocess=None, what="aug_class_map"):
        """The three per-view lists of the entries, checked for their lengths -> (imgs, flips, preprocess objects), each a list of len(imgs); `preprocess`
        may be one object for all views."""
        if not isinstance(imgs, (list, tuple)):
            raise RuntimeError(f"mmsa.{what}: imgs is the LIST of views (already flipped and resized by the caller), one tensor or (rgb, aux) pair each")
        n = len(imgs)
        flips = [None] * n if flips is None else list(flips)
        pre = list(preprocess) if isinstance(preprocess, (list, tuple)) else [preprocess] * n
        if len(flips) != n or len(pre) != n:
            raise RuntimeError(f"mmsa.{what}: {n} imgs, {len(flips)} flips and {len(pre)} preprocess objects: the lists must have the same length")
        return list(imgs), flips, pre

    @classmethod
    def make(cls, test_cfg, shapes, flips=None, ori_shape=None, rescale=True, what="aug_class_map"):
        """`shapes`: (B, H, W) of every view's canvas; `flips`: None / 'horizontal' / 'vertical' per view (None: no view is flipped)."""
        if not rescale:
            raise RuntimeError(f"mmsa.{what}: only rescale=True is supported, as in the reference (encoder_decoder.py:515 asserts it): the views are added at one size")
        shapes = [tuple(int(v) for v in s) for s in shapes]
        if not 1 <= len(shapes) <= MAX_AUGS:
            raise RuntimeError(f"mmsa.{what}: {len(shapes)} views; 1 .. {MAX_AUGS} per call")
        flips = [None] * len(shapes) if flips is None else list(flips)
        if len(flips) != len(shapes):
            raise RuntimeError(f"mmsa.{what}: {len(shapes)} imgs and {len(flips)} flips: the lists must have the same length")
        codes = tuple(_flip_code(f, what) for f in flips)
        plans = tuple(_plan_of(test_cfg, B, H, W, True, ori_shape, what) for B, H, W in shapes)
        sizes = [(p.B, p.Ho, p.Wo) for p in plans]
        if any(s != sizes[0] for s in sizes):
            raise RuntimeError(f"mmsa.{what}: the views end at different sizes (B, h, w) = {sizes}; their probabilities are added pixel by pixel -- "
                               "give ori_shape= (the frame's size before the pipeline resized it), which every view is rescaled to")
        for p in plans:
            p.check_windows(what, per="view")
        return cls(plans, codes)

    @classmethod
    def of(cls, test_cfg, shapes, flips=None, ori_shape=None, rescale=True, what="aug_class_map"):
        """`make`, remembered per geometry: the same views give the same plan object, whose window table is already on the device."""
        freeze = lambda v: tuple(freeze(x) for x in v) if isinstance(v, (list, tuple)) else v
        key = (tuple(sorted((k, freeze(v)) for k, v in dict(test_cfg).items() if k in ("mode", "crop_size", "stride", "dim", "cut_dim"))),
               freeze(shapes), None if flips is None else tuple(flips), None if ori_shape is None else freeze(ori_shape), bool(rescale))
        try:
            hash(key)
        except TypeError:
            return cls.make(test_cfg, shapes, flips, ori_shape, rescale, what)
        plan = _AUG_PLANS.get(key)
        if plan is None:
            if len(_AUG_PLANS) >= 32:
                _AUG_PLANS.clear()
            plan = _AUG_PLANS[key] = cls.make(test_cfg, shapes, flips, ori_shape, rescale, what)
        return plan

    @property
    def A(self):
        return len(self.plans)

    @property
    def size(self):
        """(B, Ho, Wo) of the class map, the same for every view."""
        return self.plans[0].B, self.plans[0].Ho, self.plans[0].Wo

    @functools.cached_property
    def offsets(self):
        """First row of every view's windows in `table`."""
        out, at = [], 0
        for p in self.plans:
            out.append(at)
            at += p.n
        return tuple(out)

    @property
    def total(self):
        return sum(p.n for p in self.plans)

    @functools.cached_property
    def table(self):
        """The window tables (image, y0, x0) of all views, concatenated: host int [total, 3]."""
        return (ctypes.c_int * (3 * self.total))(*[v for p in self.plans for job in p.jobs for v in job])

    @functools.cached_property
    def _on(self):
        return {}

    def table_on(self, device):
        """`table` on `device`, uploaded by the first call (not inside a graph capture: run the entry once before capturing it)."""
        key = str(torch.device(device))
        if key not in self._on:
            self._on[key] = torch.tensor(list(self.table), dtype=torch.int32).view(-1, 3).to(device)
        return self._on[key]

    def rows(self, lgs):
        """The [A, 11] view rows of mmsa_aug_argmax (w0, n, hs, ws, H, W, hc, wc, Hd, Wd, flip) for the head-resolution logits `lgs` (shapes only)."""
        return [(w0, p.n, int(lg.shape[2]), int(lg.shape[3]), p.H, p.W, p.hc, p.wc, p.Hd, p.Wd, f) for p, f, w0, lg in zip(self.plans, self.flips, self.offsets, lgs)]

    def mean_probabilities(self, lgs, unc):
        """The canvas path from the views' head-resolution logits: per view the logits at [B, C, Ho, Wo] (_canvas_logits + cut), softmax, un-flip and
        add (mmsa_softmax_flip_accum_nchw), the last with the division by A -> float32 [B, C, Ho, Wo]."""
        acc = None
        for a, (p, f, lg) in enumerate(zip(self.plans, self.flips, lgs)):
            y = _canvas_logits(p, lg, unc)[:, :, :p.Ho, :p.Wo].contiguous()
            if acc is None:
                acc = torch.empty_like(y)
            _softmax_accum(y, acc, f, accumulate=a > 0, finish_div=self.A if a == self.A - 1 else 0)
        return acc

    def class_map(self, lgs, out, unc, one_pass=None, conf=None, score="max", topk=None):
        """The class map of the views' head-resolution logits `lgs` (one [n_a, C, hs_a, ws_a] per view) into out uint8 [B, Ho, Wo] and the uncovered-pixel
        word `unc`: ONE launch (mmsa_aug_argmax; no host sync, no allocation once the table is on the device) where `one_pass=True` / ONE_PASS_AUG_DEFAULT
        say so and the classes fit the kernel (at most MAX_AUG_CLASSES), else the canvas path + argmax_map.  The same map bit for bit.
        `conf` (a contiguous float32 [B, Ho, Wo] tensor on the map's device): the confidence map max_c of the mean probabilities is written too, by
        mmsa_aug_argmax_conf or, on the canvas path, by mmsa_argmax_max_nchw in place of mmsa_argmax_nchw: bit for bit mean_probabilities(...).max(1).
        `score` ("margin" / "entropy", with `conf`): the top-2 margin or the entropy score of the MEAN probabilities goes to `conf` instead, by
        mmsa_argmax_score_nchw on the canvas path, whatever ONE_PASS_AUG_DEFAULT says; `one_pass=True` is refused (mmsa_aug_argmax_conf has no sibling).
        `topk` (a TopK of buffers [K, B, Ho, Wo] whose classes[0] is `out`; without `conf`): the top-k map of the MEAN probabilities, by mmsa_argmax_topk_nchw
        (first = NULL: rank 0 is their first maximum, the map above) on the canvas path, whatever ONE_PASS_AUG_DEFAULT says; `one_pass=True` is refused."""
        o = MapOptions.of("inference", conf, None, score, one_pass, aug=True, topk=topk)
        o = o.at(self.size, out.device if conf is not None or topk is not None else None, "inference", make=False)
        if o.topk is not None and (out.data_ptr() != o.topk.classes.data_ptr() or tuple(out.shape) != tuple(o.topk.classes.shape[1:]) or not out.is_contiguous()):
            raise RuntimeError("mmsa.inference: with topk= the map is plane 0 of the top-k classes: pass out=topk.classes[0]")
        self._class_map(lgs, out, unc, o)

    def _class_map(self, lgs, out, unc, o):
        """`class_map` for aug_class_map, which has made its MapOptions `o` under its own name."""
        conf = o.conf
        if len(lgs) != self.A or any(lg.shape[0] != p.n for lg, p in zip(lgs, self.plans)):
            raise RuntimeError("mmsa.inference: AugPlan.class_map takes one logits tensor per view, one row per window of that view")
        C = int(lgs[0].shape[1])
        if o.topk is not None:      # plane 0 of the classes is `out`
            _argmax_topk_into(self.mean_probabilities(lgs, unc), None, o.topk)
        elif not o.kind and ((ONE_PASS_AUG_DEFAULT and C <= MAX_AUG_CLASSES) if o.one_pass is None else o.one_pass):
            lgs = [lg.contiguous() for lg in lgs]
            ptrs = (ctypes.c_void_p * self.A)(*[lg.data_ptr() for lg in lgs])
            rows = (ctypes.c_int * (11 * self.A))(*[v for r in self.rows(lgs) for v in r])
            B, Ho, Wo = self.size
            outs = (out.data_ptr(),) if conf is None else (out.data_ptr(), conf.data_ptr())
            lib.call("mmsa_aug_argmax" if conf is None else "mmsa_aug_argmax_conf", ptrs, rows, self.A, C, self.table_on(out.device).data_ptr(), self.table,
                     self.total, *outs, B, Ho, Wo, unc.data_ptr(), ops._stream())
        elif conf is None:
            out.copy_(argmax_map(self.mean_probabilities(lgs, unc)))
        else:
            _argmax_into(self.mean_probabilities(lgs, unc), out, conf, o.kind)


_AUG_PLANS = {}


def _aug_first_tensor(imgs):
    v = imgs[0] if isinstance(imgs, (list, tuple)) and len(imgs) else None
    return v[0] if isinstance(v, (list, tuple)) and len(v) else v


def _on_views_device(fn):
    """_on_device for the entries whose frames come as a list of views."""
    @functools.wraps(fn)
    def wrapped(backbone, head, imgs, *args, **kw):
        t = _aug_first_tensor(imgs)
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            return fn(backbone, head, imgs, *args, **kw)
        with torch.cuda.device(t.device):
            return fn(backbone, head, imgs, *args, **kw)
    return wrapped


@_on_views_device
@torch.no_grad()
def aug_inference(backbone, head, imgs, test_cfg, ori_shape=None, flips=None, preprocess=None, max_batch=8):
    """`aug_test` up to its argmax (ED:517, 538-541) on logits canvases: the mean over the views of `probabilities(view)` -> float32 [B, classes, Ho, Wo].
    `imgs`: the views, normalised [B, 6, H_a, W_a] tensors -- or (rgb, aux) pairs of raw frames with `preprocess=` (one object, or one per view) -- ALREADY
    flipped and resized by the caller, as the reference's test pipeline hands them over; `flips`: None / 'horizontal' / 'vertical' per view.
    Per view: `inference`, then mmsa_softmax_flip_accum_nchw (write, then add; the last view's launch also divides by the number of views)."""
    imgs, flips, pre = AugPlan.views(imgs, flips, preprocess, "aug_inference")
    if not 1 <= len(imgs) <= MAX_AUGS:
        raise RuntimeError(f"mmsa.aug_inference: {len(imgs)} views; 1 .. {MAX_AUGS} per call")
    codes = [_flip_code(f, "aug_inference") for f in flips]
    acc = None
    for a, (img, f, p) in enumerate(zip(imgs, codes, pre)):
        y = inference(backbone, head, img, test_cfg, rescale=True, preprocess=p, ori_shape=ori_shape, max_batch=max_batch).contiguous()
        if acc is None:
            acc = torch.empty_like(y)
        elif y.shape != acc.shape:
            raise RuntimeError(f"mmsa.aug_inference: view {a} ends at {tuple(y.shape)}, the first at {tuple(acc.shape)}; give ori_shape= (the frame's size "
                               "before the pipeline resized it), which every view is rescaled to")
        _softmax_accum(y, acc, f, accumulate=a > 0, finish_div=len(imgs) if a == len(imgs) - 1 else 0)
    return acc


@_on_views_device
@torch.no_grad()
def aug_class_map(backbone, head, imgs, test_cfg, ori_shape=None, flips=None, preprocess=None, max_batch=8, labels=None, evaluator=None, case=None,
                  one_pass=None, confidence=False, calibration=None, selective=None, score="max", topk=None, topk_evaluator=None, segments=None, panoptic=None, segment_table=None, boundary=None):
    """`aug_test` (ED:509-546) -> (uint8 class map [B, Ho, Wo], uncovered-pixel word), bit for bit argmax_map(aug_inference(...)) of the same arguments.
    Every view goes through backbone and head (`max_batch` windows per call, per view); then ONE launch (mmsa_aug_argmax) resizes every view's
    head-resolution logits as `class_map` would, takes the softmax, un-flips, averages over the views and takes the argmax, with no logits or probability
    canvas in memory (`one_pass=True`), or the canvas path runs from the same logits (`one_pass=False`, more than 128 classes, and -- being the faster of
    the two where measured -- the default: ONE_PASS_AUG_DEFAULT).  No host sync either way; the one-pass launch is HIP-graph capturable once a first call
    has put the plan's window table on the device.  unc[0] != 0 <=> some view's windows do not cover its frame (ED:220): checked by the caller.
    `labels=` + `evaluator=` (+ `case=`): the map's confusion counts are added to the evaluator through the stored map, as at any rescaled size.
    `confidence=` (True or a contiguous float32 [B, Ho, Wo] output tensor): the confidence map -- the mean probability of the predicted class, bit for bit
    aug_inference(...).max(1).values, 0 where the map is 255 -- from the same launch, as the last element: (map, unc, conf).
    `calibration=` (mmsa.evaluate.Calibration; needs `labels=` and `confidence=`, `evaluator=` is optional with it): the reliability bins of the averaged map
    and its confidence are added to it by one more launch over the stored map and confidence.
    `selective=` (mmsa.evaluate.SelectiveEvaluator; needs `labels=` and `confidence=`): the averaged map's confusion counts per confidence bin, likewise.
    `score=` "max" | "margin" | "entropy" (other than "max" needs `confidence=`): the map in the confidence slot is the top-2 margin or the entropy score
    1 - H / log C of the MEAN probabilities -- the usual TTA uncertainty -- bit for bit argmax_score_map(aug_inference(...), score)[1].  Those two go through
    the canvas path (mmsa_argmax_score_nchw), whatever the default; with `one_pass=True` they are refused: mmsa_aug_argmax_conf has no score sibling.
    `topk=` K (1 .. 8) or a TopK of output buffers (uint8 / float32 [K, B, Ho, Wo]): the first K classes of the MEAN probabilities and their values, rank-major,
    bit for bit argmax_topk_map(aug_inference(...), K), as the last element: (map, unc, topk) with map = topk.classes[0].  It goes through the canvas path
    (mmsa_argmax_topk_nchw), whatever the default; `one_pass=True`, `confidence=`, `score=` other than "max", `calibration=` and `selective=` are refused
    with it.  `topk_evaluator=` (mmsa.evaluate.TopKEvaluator; needs `labels=` and `topk=`): the rank counts of the planes, by one more launch.
    `boundary=` (mmsa.evaluate.BoundaryEvaluator; needs `labels=`): the boundary counts of the averaged map, by one more launch over the stored map.
    `segments=` (mmsa.evaluate.SegmentEvaluator; needs `labels=`): the segment counts of the averaged map, over the stored map as well.
    `panoptic=` (mmsa.evaluate.PanopticEvaluator; needs `labels=`): the panoptic counts of the averaged map, likewise."""
    o = MapOptions.of("aug_class_map", confidence, None, score, one_pass, aug=True, topk=topk, labels=labels, evaluator=evaluator, case=case,
                      calibration=calibration, selective=selective, topk_evaluator=topk_evaluator, boundary=boundary, segments=segments, panoptic=panoptic, segment_table=segment_table)
    imgs, flips, pre = AugPlan.views(imgs, flips, preprocess, "aug_class_map")
    frames = [_intake(img, p, "aug_class_map") for img, p in zip(imgs, pre)]
    plan = AugPlan.of(test_cfg, [f[:3] for f in frames], flips, ori_shape)
    device = frames[0][3]
    o = o.at(plan.size, device, "aug_class_map")
    _pair(backbone, head)
    lgs = []
    for mp, p, (_, _, _, _, frame, cut) in zip(plan.plans, pre, frames):
        if test_cfg["mode"] == "slide":
            lgs.append(_window_logits(backbone, head, cut, mp.windows, max_batch))
        else:
            lgs.append(head(backbone(p(*frame) if p is not None else frame)[0]))
    out = o.map_buffer(plan.size, device)
    unc = torch.zeros(1, dtype=torch.int32, device=device)
    plan._class_map(lgs, out, unc, o)
    o.count(out)
    if o.topk is not None:
        return out, unc, o.topk
    return (out, unc) if o.conf is None else (out, unc, o.conf)


class FrameResult:
    """What SlideRunner.run() returns: the class map of ONE frame, readable once the attention logit guard of its pass has been inspected
    (mmsa.chains.Replay; a pass that ran fp16 attention out of range raises mmsa.chains.AttentionRangeError instead)."""

    def __init__(self, runner, replay, has_map=True):
        self._runner, self._replay, self._has_map = runner, replay, has_map

    def outputs(self):
        """(class map uint8 [B, H, W], uncovered-pixel flag) -- verified.  Both are the runner's static buffers: read them before the next run().
        The map is None for a run(return_map=False): that frame wrote none, the buffer still holds an earlier frame's."""
        self._replay._owner._verify(self._replay.seq)
        return (self._runner.out if self._has_map else None), self._runner.unc

    def picture(self):
        """The frame's picture uint8 [B, H, W, 3] of a runner made with render= -- verified, exactly as outputs() is.  The runner's static buffer: read it
        before the next run()."""
        if self._runner.render is None:
            raise RuntimeError("mmsa.FrameResult.picture: the SlideRunner was made without render=")
        self._replay._owner._verify(self._replay.seq)
        return self._runner.pic

    def confidence(self):
        """The frame's confidence map float32 [B, H, W] of a runner made with confidence=True -- or the score the runner was made with (`score=`) -- verified,
        exactly as outputs() is.  The runner's static buffer: read it before the next run()."""
        if self._runner.conf is None:
            raise RuntimeError("mmsa.FrameResult.confidence: the SlideRunner was made without confidence=True")
        self._replay._owner._verify(self._replay.seq)
        return self._runner.conf

    def topk(self):
        """The frame's top-k map, TopK(classes uint8 [K, B, H, W], probs float32 [K, B, H, W]), of a runner made with topk= -- verified, exactly as outputs()
        is.  The runner's static buffers (classes[0] is the map of outputs()): read them before the next run()."""
        if self._runner.topk is None:
            raise RuntimeError("mmsa.FrameResult.topk: the SlideRunner was made without topk=")
        self._replay._owner._verify(self._replay.seq)
        return self._runner.topk

    @property
    def unverified(self):
        return (self._runner.out if self._has_map else None), self._runner.unc


class SlideRunner:
    """Throughput form of slide_class_map for a fixed frame geometry: the frame's windows are cut by one kernel, go through the
    encoder + head as `chains` concurrent sub-batches (mmsa.Chains: one HIP graph per chain, shared packed weights) and one kernel
    (mmsa_slide_argmax) turns the head-resolution logits into the class map.  Same class map as slide_inference + argmax_map, bit
    for bit.  `frame` is the static [B, 6, H, W] buffer the runner reads on every run().
    With `preprocess=` (mmsa.preprocess.Preprocess) `frame` is the pair (rgb, aux) of raw [B, Hs, Ws, 3] buffers -- the runner's static inputs -- and the
    windows are cut AND normalised from them by one launch; run(frame=pair) reads another pair of the same geometry instead (mmsa.preprocess.FrameFeeder's slots).
    With `render=` (mmsa.render.Renderer) every run() also paints the frame's picture into a static buffer (one more launch): FrameResult.picture().
    With `ori_shape=` (h, w[, 3]) the class map -- and the static `out` buffer -- is the one of `rescale=True` at [B, h, w] (slide_class_map's `ori_shape=`:
    mmsa_slide_argmax_resized in place of mmsa_slide_argmax, or the canvas path with `one_pass=False`).
    With `confidence=True` every run() also writes the frame's confidence map (slide_class_map's `confidence=`) into a static float32 [B, h, w] buffer, by the
    `_conf` sibling of the class-map launch: FrameResult.confidence().  Such a runner refuses run(fused=True) and run(return_map=False).
    With `temperature=` (T > 0; needs confidence=True) that confidence is the one of softmax(logits / T) (slide_class_map's `temperature=`).  It belongs to the
    runner and not to run(): the scalar is an argument of the launch, and a captured launch keeps the one it was captured with.
    With `score=` "margin" / "entropy" (needs confidence=True) the static buffer FrameResult.confidence() returns holds that score instead (slide_class_map's
    `score=`), by the `_score` sibling of the class-map launch; it belongs to the runner for the same reason.
    With `topk=` K (or a TopK of buffers, which become the runner's) every run() also writes the frame's top-k map (slide_class_map's `topk=`) into static
    uint8 / float32 [K, B, h, w] buffers: FrameResult.topk(); the static `out` buffer is plane 0 of its classes.  `temperature=` is accepted with it; such a
    runner refuses `confidence=`, `score=` other than "max", run(fused=True), run(return_map=False), run(calibration=) and run(selective=)."""

    def __init__(self, backbone, head, frame, crop_size, stride, chains=2, check_every=1, preprocess=None, render=None, ori_shape=None, one_pass=None,
                 confidence=False, temperature=None, score="max", topk=None):
        from .chains import Chains
        o = MapOptions.of("SlideRunner", confidence, temperature, score, one_pass, topk=topk)
        self.preprocess, self.render, self.one_pass, self.temperature, self.score = preprocess, render, one_pass, temperature, score
        B, H, W, self.device, self.frame, self._cut = _intake(frame, preprocess, "SlideRunner")
        self.plan = plan = MapPlan.slide(B, H, W, tuple(crop_size), stride, ori_shape, what="SlideRunner")
        if render is not None:
            slide_source(render, preprocess, self.frame, plan, True, "SlideRunner")      # refuses a frame the picture has no source for
        _pair(backbone, head)
        plan.check_windows("SlideRunner", per="frame batch")
        if plan.n % chains:
            chains = 1
        with torch.cuda.device(self.device):
            self.crops = self._cut(plan.windows)          # also the static input buffer of the chains
            self.chains = Chains(backbone, head, n=chains, check_every=check_every).capture(self.crops)
            self.topk = o.at((B, plan.Ho, plan.Wo), self.device, "SlideRunner").topk if o.topk is not None else None
            self.out = self.topk.classes[0] if self.topk is not None else torch.empty(B, plan.Ho, plan.Wo, dtype=torch.uint8, device=self.device)
            self.unc = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.conf = torch.empty(B, plan.Ho, plan.Wo, dtype=torch.float32, device=self.device) if confidence else None
            self.options = dataclasses.replace(o, conf=self.conf, topk=self.topk)      # the runner's half of the family: the scalars a captured launch keeps; run() adds the frame's
            self.pic = None
            if render is not None:
                render.palette_on(self.device)
                self.pic = torch.empty(B, plan.Ho, plan.Wo, 3, dtype=torch.uint8, device=self.device)

    @torch.no_grad()
    def run(self, frame=None, labels=None, evaluator=None, case=None, fused=None, return_map=True, calibration=None, selective=None, topk_evaluator=None,
            segments=None, panoptic=None, segment_table=None, tracker=None, boundary=None):
        """Enqueue one frame on the current stream (asynchronous) -> FrameResult; `.outputs()` = (class map uint8 [B, H, W], uncovered-pixel flag) once the
        attention logit guard of this pass has been inspected.  The inspection costs one 4 * depth-byte copy per `check_every` frames and an event wait,
        no device sync; a frame that scored logits beyond the fp16 range raises mmsa.chains.AttentionRangeError from outputs() -- or from the next run(),
        whichever comes first -- after the blocks concerned have been moved to fp16 hi/lo pairs and the graphs captured again: run that frame again.
        `labels=` + `evaluator=` (mmsa.evaluate.Evaluator, best one made with cases=[...] and device=; `case=`): the frame's confusion counts are ADDED to the
        evaluator on device (see MapPlan.class_map); a frame that has to be run again has been counted, so reset the evaluator or subtract what it added.
        `return_map=False` (always the fused launch) leaves the runner's map buffer untouched; the FrameResult's map is then None.
        `calibration=` (mmsa.evaluate.Calibration, best one made with cases=[...] and device=; a runner made with confidence=True; needs `labels=`): the
        frame's reliability bins are ADDED to it on device by one more launch; a frame that has to be run again has been binned, as it has been counted.
        `selective=` (mmsa.evaluate.SelectiveEvaluator, made the same way; needs `labels=` and a runner made with confidence=True): the frame's confusion
        counts per confidence bin are ADDED to it on device by one more launch, under the same terms.
        `topk_evaluator=` (mmsa.evaluate.TopKEvaluator of the runner's K, made the same way; needs `labels=` and a runner made with topk=): the rank counts of
        the frame's top-k planes are ADDED to it on device by one more launch, under the same terms.
        `boundary=` (mmsa.evaluate.BoundaryEvaluator, made the same way; needs `labels=`; refused with return_map=False): the boundary counts of the frame's
        stored map are ADDED to it on device by one more launch, under the same terms.
        `segments=` (mmsa.evaluate.SegmentEvaluator, made the same way; needs `labels=`; refused with return_map=False): the segment counts of the frame's
        stored map are ADDED to it on device, under the same terms.
        `panoptic=` (mmsa.evaluate.PanopticEvaluator, made the same way; needs `labels=`; refused with return_map=False): the panoptic counts of the frame's
        stored map are ADDED to it on device, under the same terms.
        `tracker=` (mmsa.evaluate.SegmentTracker; only together with `segment_table=`, which must be the tracker's own table): `tracker.update()` runs behind
        the table's update, so consecutive run() calls are the frames of the tracker's stream; a frame that has to be run again has been tracked -- reset
        the tracker or accept the repeated frame (every segment continues itself).  None: exactly the launches made without it.  The single-frame class-map
        entries do not take it."""
        o = self.options.with_call("SlideRunner.run", labels, evaluator, case, calibration, selective, fused, return_map, topk_evaluator, segments=segments, boundary=boundary, panoptic=panoptic, segment_table=segment_table,
                                   tracker=tracker)
        o = o.at(self.out.shape, self.device, "SlideRunner.run")
        if frame is None:
            frame = self.frame
        else:
            if self.preprocess is None:
                raise RuntimeError("mmsa.SlideRunner.run(frame=...): only with preprocess= (without it the runner reads its static frame buffer)")
            frame = self.preprocess.check(*frame)
            if any(f.shape != s.shape or f.dtype != s.dtype or f.device != s.device for f, s in zip(frame, self.frame)):
                raise RuntimeError("mmsa.SlideRunner.run(frame=...): the pair must have the shape, dtypes and device of the runner's own buffers")
        src = None if self.render is None else slide_source(self.render, self.preprocess, frame, self.plan, return_map, "SlideRunner.run")
        with torch.cuda.device(self.device):
            self._cut(self.plan.windows, out=self.crops, frame=frame)
            rp = self.chains.replay()
            lg = rp.unverified          # the argmax kernel below is enqueued behind the pass; nothing is read on the host before outputs() verifies it
            self.unc.zero_()
            self.plan._class_map(lg, self.out, self.unc, o)
            if self.render is not None:
                self.render(self.out, src, out=self.pic)
        return FrameResult(self, rp, has_map=return_map)

    def check_guard(self):
        """Chains.check_guard for the runner's chains (host sync): [] = the frames since the last check ran inside the attention kernels' operand range;
        otherwise the listed ViT blocks were moved to fp16 hi/lo pairs, the graphs were captured again and run() must be repeated for
        those frames (their FrameResult.outputs() raise)."""
        return self.chains.check_guard()
