"""The three entries that read a code map -- mmsa.boundary_distance, mmsa.components and mmsa.segment_table -- refuse a bad `map`, `num_classes=` /
`labels_prep=` and `size=` alike, before any device is looked at: the same exception type and, word for word, the message each entry has always given.
(`segment_table` has no `size=`: a table reads labels on the grid its LabelPrep resizes them to, and the keyword itself is a TypeError.)"""
import pytest
import torch

ENTRIES = {
    "boundary_distance": (lambda mmsa, m, **kw: mmsa.boundary_distance(m, 3, **kw), "mmsa.evaluate: boundary_distance takes num_classes= (a stored class map)"),
    "components": (lambda mmsa, m, **kw: mmsa.components(m, **kw), "mmsa.evaluate: components takes num_classes= (a stored class map)"),
    "segment_table": (lambda mmsa, m, **kw: mmsa.segment_table(m, **kw), "mmsa.SegmentTable: takes num_classes= (stored class maps)"),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_bad_code_map_is_refused_alike(entry):
    import mmsa
    from mmsa.evaluate import LabelPrep
    call, takes = ENTRIES[entry]
    lp = LabelPrep(5)
    m = torch.zeros(1, 6, 8, dtype=torch.uint8)      # a CPU tensor: a call that got as far as the device would say "must be a GPU tensor"

    def refused(kind, text, m=m, **kw):
        with pytest.raises(kind) as e:
            call(mmsa, m, **kw)
        assert str(e.value) == text, (entry, kw)

    for kw in (dict(), dict(num_classes=5, labels_prep=lp)):
        refused(ValueError, takes + " or labels_prep= (raw labels), one of them", **kw)
    if entry == "segment_table":
        for kw in (dict(num_classes=5, size=(3, 4)), dict(labels_prep=lp, size=(12, 16))):
            with pytest.raises(TypeError, match="unexpected keyword argument 'size'"):
                call(mmsa, m, **kw)
    else:
        refused(RuntimeError, "mmsa.evaluate: size=(3, 4) for a stored 6 x 8 class map: only labels are resized (labels_prep=)", num_classes=5, size=(3, 4))
        refused(RuntimeError, "mmsa.evaluate: size mismatch: the label maps are 6 x 8, which the LabelPrep reads on a grid of 6 x 8, not 12 x 16",
                labels_prep=lp, size=(12, 16))
    for kw in (dict(num_classes=5), dict(labels_prep=lp)):
        refused(RuntimeError, "mmsa.evaluate: an empty map (1, 0, 8)", m=torch.zeros(1, 0, 8, dtype=torch.uint8), **kw)
        refused(RuntimeError, "mmsa.evaluate: map is torch.float32; a uint8 class map or raw uint8 labels is expected", m=m.float(), **kw)
        refused(RuntimeError, "mmsa.evaluate: map must be a GPU tensor (there is no CPU path)", **kw)      # a good call gets as far as the device, no further
