"""numpy restatement of unet_head_score (include/unet_mi355x.h): out_conv's logits by
unet_head_forward's chain (head_step_ref.logits_chain), scored as unet_score scores them (score_ref.score).  Shared
by the CPU and GPU tests of the head score.  The cases are head_step_ref.CASES -- the reference loss of each is
already held in tests/golden/head_step_cases.npz -- and one more shape with no reference loss: 33 x 130 with C = 4,
the unaligned tail of score_ref.CASES."""
import numpy as np

import head_step_ref
import score_ref
from head_step_ref import WEIGHTS, bar, case_tensors, fixture, target_f32  # noqa: F401
from score_ref import SWEEP  # noqa: F401

from unet_mi355x.metrics import Score

# name, (N, C, H, W), seed, target density, soft: head_step_ref.generate's arguments
TAIL = ("tail", (1, 4, 33, 130), 407, 0.2, True)
SWEEP_1 = [0.5]
SWEEP_64 = [float(v) for v in np.linspace(0.01, 0.99, 64)]


def score(feat, w, b, target, cuts, sweep_cuts=None):
    """feat fp32 [N, 64, H, W], target fp32 [N, C, H, W]: (entries [N, C], hist or None) as score_ref.score."""
    return score_ref.score(head_step_ref.logits_chain(feat, w, b), target, cuts, sweep_cuts)


def loss(entries, weights=WEIGHTS) -> float:
    """InvoiceLoss of the entries as one batch: metrics.Score.loss with unet_loss_config's four weights."""
    dw, fw, alpha, smooth = weights
    return Score(entries).loss(dw, fw, None, smooth, alpha)


def sum_bar(hw: int, value: float) -> float:
    """The first-order bound between two fp64 summation trees over hw non-negative fp32 terms."""
    return 2.0 * hw * 2.0 ** -53 * abs(value)
