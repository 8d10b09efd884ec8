"""numpy restatement of unet_score (include/unet_mi355x.h): fp32 per element, op by op as the reference's
InvoiceLoss (train.py:58, 24-29, 40-45), fp64 sums, integer counts and histogram.  Shared by the CPU and GPU
score tests, together with the seeded generator of the fixture's cases (tests/golden/score_cases.npz holds the
generator parameters and the reference's results, not the tensors)."""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd")
for _p in (PKG_DIR, REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from unet_mi355x.metrics import ENTRY_DTYPE  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "score_cases.npz")
SPREAD_FACTOR = 8.0   # the bar of every float comparison: this many times the fixture's largest spread

# (N, C, H, W), logit scale, logit shift, target density, seed: one element, odd widths and vector tails, one
# plane over several spans (96 x 160 = 3.75 spans of 4096), logits wide enough to reach the clamp
CASES = [
    ((2, 1, 1, 1), 4.0, -1.0, 0.5, 101),
    ((2, 1, 5, 7), 4.0, -1.0, 0.3, 102),
    ((3, 3, 16, 16), 3.0, -4.0, 0.1, 103),
    ((1, 4, 33, 130), 5.0, -3.0, 0.2, 104),
    ((2, 3, 64, 48), 6.0, -2.0, 0.2, 105),
    ((1, 3, 96, 160), 10.0, 0.0, 0.3, 106),
]
SWEEP = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]


def generate(shape, scale, shift, density, seed):
    """(logits fp32 NCHW, target uint8 NHWC): logits = scale * randn + shift; target 255 with probability
    ``density``, else 0, and one pixel in ten a uniform byte (soft labels: v / 255 and the 0.5 cut matter)."""
    n, c, h, w = shape
    rs = np.random.RandomState(seed)
    logits = (scale * rs.randn(n, c, h, w) + shift).astype(np.float32)
    hard = np.where(rs.rand(n, h, w, c) < density, 255, 0)
    soft = rs.randint(0, 256, size=(n, h, w, c))
    target = np.where(rs.rand(n, h, w, c) < 0.1, soft, hard).astype(np.uint8)
    return logits, target


def target_f32(target_u8):
    """uint8 NHWC -> fp32 NCHW, v / 255.0f (dataset.py:33-34)."""
    return np.ascontiguousarray((target_u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))


def sha256(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def elementwise(x, t):
    """fp32 per-element terms of unet_score: (p, p * t, focal term u * u * bce)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    t = np.asarray(t, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        p = f32(1) / (f32(1) + np.exp(-x))
        pt = p * t
        lo, hi = f32(1e-7), f32(1.0 - 1e-7)
        pc = np.where(p < lo, lo, np.where(p > hi, hi, p))   # NaN stays NaN
        l1 = np.log(f32(1) - pc)
        l1 = np.where(l1 < f32(-100), f32(-100), l1)
        l0 = np.log(pc)
        l0 = np.where(l0 < f32(-100), f32(-100), l0)
        bce = (t - f32(1)) * l1 - t * l0
        q = np.exp(-bce)
        u = f32(1) - q
        f = u * u * bce
    assert p.dtype == pt.dtype == f.dtype == f32
    return p, pt, f


def score(logits, target, cuts, sweep_cuts=None):
    """logits fp32 [N, C, H, W]; target fp32 [N, C, H, W]; cuts: C logit cuts (unet_logit_cut of the
    thresholds); sweep_cuts: K non-decreasing logit cuts or None.  Returns (entries [N, C] of ENTRY_DTYPE,
    hist int64 [N, C, 2, K + 1] or None)."""
    logits = np.asarray(logits, np.float32)
    target = np.asarray(target, np.float32)
    n, c, h, w = logits.shape
    p, pt, f = elementwise(logits, target)
    e = np.zeros((n, c), ENTRY_DTYPE)
    flat = lambda a: a.reshape(n, c, -1)   # noqa: E731
    nan = np.isnan(flat(logits))
    e["sum_p"] = flat(p).astype(np.float64).sum(-1)
    e["sum_t"] = np.where(nan, np.float64("nan"), flat(target).astype(np.float64)).sum(-1)   # a NaN logit marks it too
    e["sum_pt"] = flat(pt).astype(np.float64).sum(-1)
    e["sum_focal"] = flat(f).astype(np.float64).sum(-1)
    with np.errstate(invalid="ignore"):
        pred = flat(logits) > np.asarray(cuts, np.float32).reshape(1, c, 1)
    tgt = flat(target) > np.float32(0.5)
    e["n_pred"] = pred.sum(-1)
    e["n_tgt"] = tgt.sum(-1)
    e["n_both"] = (pred & tgt).sum(-1)
    e["n_px"] = h * w
    hist = None
    if sweep_cuts is not None:
        sc = np.asarray(sweep_cuts, np.float32)
        k = len(sc)
        with np.errstate(invalid="ignore"):
            b = (flat(logits)[..., None] > sc).sum(-1)
        hist = np.zeros((n, c, 2, k + 1), np.int64)
        for i in range(n):
            for j in range(c):
                for tv in (0, 1):
                    hist[i, j, tv] = np.bincount(b[i, j][tgt[i, j] == bool(tv)], minlength=k + 1)
    return e, hist


def rel(a, b) -> float:
    """Relative distance of two scalars (0 when both are 0)."""
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(a), abs(b))


def fixture():
    """The committed cases: list of dicts with the generator parameters and the reference's results."""
    z = np.load(FIXTURE)
    out = []
    for i in range(int(z["n_cases"])):
        out.append(dict(shape=tuple(int(v) for v in z[f"shape_{i}"]), scale=float(z[f"scale_{i}"]),
                        shift=float(z[f"shift_{i}"]), density=float(z[f"density_{i}"]), seed=int(z[f"seed_{i}"]),
                        logits_sha256=str(z[f"logits_sha256_{i}"]), dice=float(z[f"dice_{i}"]),
                        focal=float(z[f"focal_{i}"]), loss=float(z[f"loss_{i}"]),
                        loss_b1=float(z[f"loss_b1_{i}"]), loss_b2=float(z[f"loss_b2_{i}"]),
                        spread=float(z[f"spread_{i}"])))
    return out


def case_tensors(case):
    logits, target = generate(case["shape"], case["scale"], case["shift"], case["density"], case["seed"])
    assert sha256(logits) == case["logits_sha256"], "the seeded generator no longer reproduces the fixture's logits"
    return logits, target
