"""Real-valued dense heads at 1, 2 and 4 classes (tests/test_classes_cpu.py, tests/test_classes_gpu.py): structured
weights whose out_conv bias is shifted so that every class's mask is lively at the class-count tests' thresholds,
with the fp32 oracle's logits and masks and the pixels too close to a cut to be compared across arithmetics.

A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.  Built once per
(class count, shape) and shared (cached): treat the arrays as read-only."""
from __future__ import annotations

import functools

import numpy as np
import torch

import exact_nets as en
from oracle import unet_oracle as orc
from unet_mi355x import synthetic as syn

# (n, h, w) of exact_nets.ROUTING_CLASSES, all on 3 input channels; seed 301 + index
SHAPES = [tuple(c[2:]) for c in en.ROUTING_CLASSES]
SEED0 = 301
THRESHOLDS = en.CLASS_THRESHOLDS
# tests/test_forward_gpu.py TOL["fp32"] (asserted equal there and in test_classes_gpu.py): the band of oracle
# logits around a cut, relative to max(1, max |logit|), inside which an fp32 plan's mask may differ
FP32_TOL = 2e-5
MAX_NEAR = 8      # pixels per (case, class) that band may hold
QUANTILE = 0.5    # the share of each class's oracle logits the shifted bias leaves below its cut


class DenseCase:
    """sd: the state_dict (numpy); x: fp32 [n, 3, h, w] invoice-like pages; raw_share: per class, the share of
    pixels above the cut BEFORE the bias shift; ref: the oracle's logits; masks: its sigmoid > thr (bool);
    near: the pixels whose oracle logit lies within FP32_TOL * max(1, max |ref|) of the class's cut."""

    def __init__(self, n_classes: int, index: int, thresholds=THRESHOLDS):
        n, h, w = SHAPES[index]
        seed = SEED0 + index
        thr = np.asarray(thresholds[:n_classes], dtype=np.float64)
        assert len(thr) == n_classes
        cuts = np.log(thr / (1.0 - thr))
        sd = syn.make_state_dict(seed, 3, n_classes, "structured")
        self.x = syn.invoice_pages(seed, n, h, w, 3)
        xt = torch.from_numpy(self.x)
        raw = orc.unet_forward(sd, xt).numpy()
        self.raw_share = en.reference_masks(raw, thresholds[:n_classes]).mean(axis=(0, 2, 3))
        # tests/test_forward_gpu.py _recentred, per class and at these thresholds: the bias moves the QUANTILE of
        # the class's logits onto its cut
        q = np.quantile(raw.transpose(1, 0, 2, 3).reshape(n_classes, -1), QUANTILE, axis=1)
        sd["out_conv.bias"] = (sd["out_conv.bias"] + (cuts - q)).astype(np.float32)
        self.sd = sd
        self.thresholds = tuple(float(t) for t in thresholds[:n_classes])
        self.ref = orc.unet_forward(sd, xt).numpy()
        self.masks = en.reference_masks(self.ref, self.thresholds)
        self.band = FP32_TOL * max(1.0, float(np.abs(self.ref).max()))
        self.near = np.abs(self.ref.astype(np.float64) - cuts.reshape(1, -1, 1, 1)) <= self.band
        for a in (self.x, self.ref, self.masks, self.near):
            a.setflags(write=False)

    def check_oracle(self) -> None:
        """The oracle-side premises, asserted before a GPU is used: every class's mask covers 10 .. 90 % of the
        pixels, and at most MAX_NEAR pixels per class are too close to the cut to compare."""
        share = self.masks.mean(axis=(0, 2, 3))
        near = self.near.sum(axis=(0, 2, 3))
        assert ((share >= 0.1) & (share <= 0.9)).all(), share
        assert (near <= MAX_NEAR).all(), near


@functools.lru_cache(maxsize=None)
def dense_case(n_classes: int, index: int, thresholds=THRESHOLDS) -> DenseCase:
    return DenseCase(n_classes, index, thresholds)
