"""Oracle-side premises of the class-count tests (tests/test_classes_gpu.py), checked on the CPU: the real-valued
dense heads of tests/class_cases.py are lively at the tests' thresholds and have few pixels near a cut, and the
oracle's masks take per-class thresholds without changing what they are by default."""
import numpy as np
import pytest

import class_cases as cc
from oracle import unet_oracle as orc


@pytest.mark.parametrize("index", range(len(cc.SHAPES)), ids=[str(s) for s in cc.SHAPES])
@pytest.mark.parametrize("n_classes", [1, 2, 4])
def test_dense_head_cases_on_the_oracle(n_classes, index):
    """Per (class count, shape): with the shifted bias every class's oracle mask covers 10 .. 90 % of the pixels
    and at most 8 pixels per class lie in the band around the cut that the fp32 plans' masks are not compared
    in."""
    case = cc.dense_case(n_classes, index)
    share, near = case.masks.mean(axis=(0, 2, 3)), case.near.sum(axis=(0, 2, 3))
    print(f"{n_classes} classes {cc.SHAPES[index]}: unshifted {np.round(case.raw_share, 3)}, shifted "
          f"{np.round(share, 3)}, near a cut {near} of {case.masks[:, 0].size}, max |logit| {np.abs(case.ref).max():.2f}")
    case.check_oracle()
    assert np.abs(case.ref).max() < 50


def test_unshifted_heads_are_degenerate():
    """Why the biases are shifted: unshifted, several (shape, class) pairs have >= 98 % of their pixels on, a
    mask that could hide a stray plane."""
    shares = np.concatenate([cc.dense_case(4, i).raw_share for i in range(len(cc.SHAPES))])
    assert (shares >= 0.98).sum() >= 2, shares


def test_masks_from_logits_thresholds_argument():
    """orc.masks_from_logits: unchanged by default (the three fields' constants, keyed by field); with
    ``thresholds`` one strict fp32 '>' per plane, keyed by class index, for any class count."""
    rng = np.random.default_rng(5)
    lg = rng.normal(0, 2, (4, 8, 16)).astype(np.float32)
    lg[:, 0, 0] = 0.0                            # sigmoid(0) = 0.5 is not > 0.5
    default = orc.masks_from_logits(lg[:3])
    assert list(default) == orc.FIELDS
    same = orc.masks_from_logits(lg[:3], [orc.THRESHOLDS[k] for k in orc.FIELDS])
    assert all(np.array_equal(default[k], same[i]) for i, k in enumerate(orc.FIELDS))
    for ncls in (1, 2, 4):
        got = orc.masks_from_logits(lg[:ncls], (0.35, 0.5, 0.1, 0.9))
        assert list(got) == list(range(ncls))
        p = 1.0 / (1.0 + np.exp(-lg[:ncls].astype(np.float64)))
        for c, t in enumerate((0.35, 0.5, 0.1, 0.9)[:ncls]):
            firm = np.abs(p[c] - t) > 1e-6
            assert np.array_equal(got[c][firm], (p[c] > t)[firm])
    assert not orc.masks_from_logits(lg[:2], (0.35, 0.5))[1][0, 0]
    with pytest.raises(ValueError):
        orc.masks_from_logits(lg, (0.5, 0.5))
