"""numpy restatement of the diagnostic pictures of mmsa.Renderer (labels / errors / heat / abstained / band; csrc/render_diag.hip), written from their
definitions and independent of the kernels' form: no paint table, no index arithmetic, no tiles -- masks and np.where -- TEST INFRASTRUCTURE ONLY.

  every pixel gets ONE paint, then show_result's blend (tests/render_ref.blend: img * (1 - opacity) + colour * opacity in float64, truncated):
    paint None      the pixel is the source pixel unchanged (black without a source)
    an RGB triple   that colour;      "pred" / "label": the palette's colour of that code, colour 0 for a code without a palette entry
    MARKED paints are blended with mark_opacity in the place of the Renderer's opacity; bgr reverses every colour
  L = the label code of tests/boundary_ref.codes: a class < C, C (kept, out of range) or 255 (ignored);  the bin of a value: tests/calibration_ref.bin_index

The checker of tests/test_render_diag_gpu.py (np.array_equal on uint8) and, against independent facts, of tests/test_render_diag_cpu.py."""
import numpy as np

from tests import boundary_ref as BR
from tests import calibration_ref as CR
from tests import render_ref as RR

IGNORE = 255


def label_codes(label, lut, C, H, W, ymap=None, xmap=None):
    """One raw label map uint8 [Hl, Wl] -> L int64 [H, W]."""
    return BR.codes(np.zeros((H, W), dtype=np.uint8), label, lut, C, ymap, xmap)[0]


def palette_colours(palette, code):
    """int codes [...] -> uint8 [..., 3] (RGB): the palette's colour, 0 for a code without an entry."""
    pal = np.zeros((max(256, len(palette)), 3), dtype=np.uint8)
    pal[:len(palette)] = np.asarray(palette)
    return pal[np.asarray(code, dtype=np.int64)]


def paint_of(what, palette, pred_code, label_code, shape):
    """A paint argument -> (colour uint8 [h, w, 3] RGB, painted bool)."""
    if what is None:
        return np.zeros(shape + (3,), dtype=np.uint8), False
    if isinstance(what, str):
        code = {"pred": pred_code, "label": label_code}[what]
        assert code is not None, f"a {what!r} paint without that map"
        return palette_colours(palette, code), True
    return np.broadcast_to(np.asarray(what, dtype=np.uint8), shape + (3,)), True


def compose(img, layers, opacity, mark_opacity, bgr):
    """img uint8 [h, w, 3]; layers: [(mask, colour RGB [h, w, 3], painted, marked)], masks disjoint -> uint8 [h, w, 3]."""
    out = img.copy()
    for mask, colour, painted, marked in layers:
        if not painted:
            continue
        col = colour[..., ::-1] if bgr else colour
        blended = RR.blend(img, col, mark_opacity if marked else opacity)
        out = np.where(mask[..., None], blended, out)
    return out


def source_of(source, b, h, w):
    return np.zeros((h, w, 3), dtype=np.uint8) if source is None else np.ascontiguousarray(source[b][:h, :w, :])


def error_states(pred, L, C):
    """0 = ignored (L == 255), 1 = correct (L < C and pred == L), 2 = wrong (everything else: L == C and pred == 255 included)."""
    pred = pred.astype(np.int64)
    return np.where(L == IGNORE, 0, np.where((L < C) & (pred == L), 1, 2))


def labels_ref(labels, lut, C, palette, opacity, H, W, source=None, ignored=(0, 0, 0), bgr=True, ymap=None, xmap=None):
    """labels uint8 [B, Hl, Wl] -> uint8 [B, H, W, 3]: the ground-truth picture."""
    out = np.empty((labels.shape[0], H, W, 3), dtype=np.uint8)
    for b in range(labels.shape[0]):
        L = label_codes(labels[b], lut, C, H, W, ymap, xmap)
        cls = L < C
        layers = [(cls,) + paint_of("label", palette, None, np.where(cls, L, 0), (H, W)) + (False,), (~cls,) + paint_of(ignored, palette, None, None, (H, W)) + (False,)]
        out[b] = compose(source_of(source, b, H, W), layers, opacity, 1.0, bgr)
    return out


def errors_ref(pred, labels, lut, C, palette, opacity, source=None, wrong=(255, 0, 0), correct=None, ignored=None, mark_opacity=1.0, bgr=True, ymap=None,
               xmap=None):
    """pred uint8 [B, H, W], labels uint8 [B, Hl, Wl] -> uint8 [B, H, W, 3]: the wrong-pixel picture."""
    B, H, W = pred.shape
    out = np.empty((B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        L = label_codes(labels[b], lut, C, H, W, ymap, xmap)
        st = error_states(pred[b], L, C)
        p = pred[b].astype(np.int64)
        layers = [(st == 0,) + paint_of(ignored, palette, p, L, (H, W)) + (False,), (st == 1,) + paint_of(correct, palette, p, L, (H, W)) + (False,),
                  (st == 2,) + paint_of(wrong, palette, p, L, (H, W)) + (True,)]
        out[b] = compose(source_of(source, b, H, W), layers, opacity, mark_opacity, bgr)
    return out


def heat_ref(values, colormap, opacity, source=None, bgr=True):
    """values float32 [B, H, W], colormap [N, 3] -> uint8 [B, H, W, 3]."""
    B, H, W = values.shape
    cm = np.asarray(colormap, dtype=np.uint8)
    out = np.empty((B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        k = CR.bin_index(values[b], len(cm))
        out[b] = compose(source_of(source, b, H, W), [(np.ones((H, W), dtype=bool), cm[k], True, False)], opacity, 1.0, bgr)
    return out


def abstain_ref(pred, conf, bins, min_bin):
    """mmsa.abstain restated: pred where the confidence's bin is >= min_bin, 255 elsewhere."""
    return np.where(CR.bin_index(conf, bins) >= min_bin, pred, 255).astype(np.uint8)


def abstained_ref(pred, conf, bins, min_bin, palette, opacity, colour=(0, 0, 0), mark_opacity=1.0, source=None, bgr=True):
    """pred uint8 / conf float32 [B, H, W] -> uint8 [B, H, W, 3]; colour: a triple or a [bins, 3] colormap."""
    B, H, W = pred.shape
    out = np.empty((B, H, W, 3), dtype=np.uint8)
    for b in range(B):
        k = CR.bin_index(conf[b], bins)
        kept = k >= min_bin
        c = np.asarray(colour, dtype=np.uint8)
        col = c[k] if c.ndim == 2 else np.broadcast_to(c, (H, W, 3))
        layers = [(kept, palette_colours(palette, pred[b]), True, False), (~kept, col, True, True)]
        out[b] = compose(source_of(source, b, H, W), layers, opacity, mark_opacity, bgr)
    return out


def band_masks(pred, label, lut, C, radius, border, where, ymap=None, xmap=None):
    """One image (pred or label may be None) -> (marked bool [H, W], P or None, L or None)."""
    if pred is not None:
        H, W = pred.shape
        P = np.minimum(pred.astype(np.int64), C)
    else:
        P = None
    if label is not None:
        if pred is None:
            H, W = (len(ymap), len(xmap)) if ymap is not None else label.shape
        L = label_codes(label, lut, C, H, W, ymap, xmap)
    else:
        L = None
    marked = np.zeros((H, W), dtype=bool)
    if where in ("pred", "both"):
        marked |= BR.near(P, radius, border)
    if where in ("label", "both"):
        marked |= BR.near(L, radius, border)
    if L is not None:
        marked &= L != IGNORE
    return marked, P, L


def band_ref(pred, labels, lut, C, palette, opacity, radius, border=False, colour=(255, 255, 255), inside="pred", where="pred", mark_opacity=1.0, source=None,
             bgr=True, ymap=None, xmap=None):
    """pred uint8 [B, H, W] or None, labels uint8 [B, Hl, Wl] or None -> uint8 [B, H, W, 3]."""
    B = (pred if pred is not None else labels).shape[0]
    outs = []
    for b in range(B):
        marked, P, L = band_masks(None if pred is None else pred[b], None if labels is None else labels[b], lut, C, radius, border, where, ymap, xmap)
        H, W = marked.shape
        layers = [(marked,) + paint_of(colour, palette, P, L, (H, W)) + (True,), (~marked,) + paint_of(inside, palette, P, L, (H, W)) + (False,)]
        outs.append(compose(source_of(source, b, H, W), layers, opacity, mark_opacity, bgr))
    return np.stack(outs)
