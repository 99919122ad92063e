"""The restatement of the reference's rescaled predictions (tests/rescale_ref.py) against the reference's own output (tests/golden/rescale.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import rescale_ref as RR
from tests.configs import toy_encode_decode
from tests.util import REL_TOL, assert_close


@pytest.mark.parametrize("tag", ["a", "c", "w"])
def test_restatement_equals_the_reference(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "rescale.npz"))
    hw, crop, stride, ori = RR.case_of(g[f"{tag}_cfg"])
    want = torch.from_numpy(g[f"{tag}_out"])
    got = RR.rescaled_logits(toy_encode_decode(RR.NUM_CLASSES, seed=RR.TOY_SEED), RR.frame(hw), ori, crop, stride)
    r, m = assert_close(got, want, what=f"rescale case {tag}")
    share = RR.near_ties(want, REL_TOL).float().mean().item()
    print(f"rescale {tag}: rel_l2 {r:.2e} max_rel {m:.2e}; near-tie pixels {share:.4%}; classes present {sorted(set(want.argmax(1).flatten().tolist()))}")
    assert share <= 0.01, "the fixture itself must stay inside the 1 % the class-map test may exclude"
    assert len(set(want.argmax(1).flatten().tolist())) >= 2, "a fixture with one class everywhere pins no class map"


def test_tap_tables():
    """rescale_ref.taps: identity, exact half and the clamps at both ends."""
    t0, t1 = RR.taps(7, 7)
    assert t0.tolist() == list(range(7)) and t1.tolist() == [1, 2, 3, 4, 5, 6, 6]
    t0, t1 = RR.taps(8, 4)
    assert t0.tolist() == [0, 2, 4, 6] and t1.tolist() == [1, 3, 5, 7]
    t0, t1 = RR.taps(4, 10)
    assert t0[0] == 0 and t1[-1] == 3 and t0[-1] == 3
    cnt = np.ones((1, 4, 6))
    cnt[:, :, 4:] = 0
    bad = RR.touches_uncovered(cnt, 4, 6)
    assert bad[0, 0].tolist() == [False, False, False, True, True, True]       # column 3's second tap is column 4
