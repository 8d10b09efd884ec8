"""numpy restatement of unet_loss_grad (include/unet_mi355x.h): the reference's InvoiceLoss (train.py:18-59) and
autograd's backward of it at the logits.  fp32 per element with separately rounded operations (numpy has no fused
multiply-add), fp64 sums and Dice coefficients, as the device.  Shared by the CPU and GPU loss tests, together
with the seeded generator of the fixture's cases (tests/golden/loss_cases.npz holds the generator parameters and
the reference's loss and gradient, not the inputs)."""
import os

import numpy as np

import score_ref
from score_ref import sha256, target_f32  # noqa: F401

FIXTURE = os.path.join(score_ref.REPO, "tests", "golden", "loss_cases.npz")
SPREAD_FACTOR = 8.0    # the bar of a case: this many times its own spread (fp32 against fp64 reference autograd)
SPREAD_LIMIT = 1e-5    # the generator refuses a case whose spread is larger
WEIGHTS = (0.85, 0.15, 0.8, 1.0)   # dice_weight, focal_weight, focal_alpha, smooth: the reference's

# name, (N, C, H, W), logit scale, logit shift, target density, soft (one target in ten a uniform byte), seed,
# index of a NaN logit or None
CASES = [
    ("one", (1, 1, 1, 1), 3.0, -2.0, 0.5, False, 201, None),             # a single element
    ("odd", (1, 3, 5, 7), 3.0, -2.0, 0.3, False, 202, None),             # planes 2, 3 unaligned, scalar tails
    ("spans", (2, 3, 48, 96), 10.0, -4.0, 0.1, False, 203, None),        # 4608 px: two spans, the second partial
    ("c4", (2, 4, 16, 16), 3.0, -2.0, 0.1, True, 204, None),             # uint8 NHWC words of 4 classes
    ("c1", (3, 1, 16, 16), 3.0, -2.0, 0.2, True, 205, None),             # ... and of one
    ("far", (2, 3, 64, 64), 10.0, 0.0, 0.5, False, 206, None),           # both far bands |x| >= 20 populated
    ("nan", (2, 3, 16, 16), 3.0, -2.0, 0.2, False, 207, (1, 2, 3, 5)),   # one NaN logit
]


def generate(shape, scale, shift, density, soft, seed, nan_at=None):
    """(logits fp32 NCHW, target uint8 NHWC).  logits = scale * randn + shift, and any with 14 < |x| < 20 pushed
    out to |x| + 6: in that band the clamp of train.py:41 makes two correct fp32 implementations disagree element
    by element, so it has a test of its own.  target: 255 with probability ``density``
    else 0; with ``soft`` one pixel in ten a uniform byte."""
    n, c, h, w = shape
    rs = np.random.RandomState(seed)
    x = (scale * rs.randn(n, c, h, w) + shift).astype(np.float32)
    band = (np.abs(x) > 14) & (np.abs(x) < 20)
    x = np.where(band, x + np.copysign(np.float32(6), x), x).astype(np.float32)
    target = np.where(rs.rand(n, h, w, c) < density, 255, 0)
    if soft:
        target = np.where(rs.rand(n, h, w, c) < 0.1, rs.randint(0, 256, size=(n, h, w, c)), target)
    if nan_at is not None:
        x[tuple(nan_at)] = np.nan
    assert not ((np.abs(x) > 14) & (np.abs(x) < 20)).any()
    return x, target.astype(np.uint8)


def loss_grad(x, t, weights=WEIGHTS, upstream=1.0):
    """x, t: fp32 [N, C, H, W].  Returns (loss fp32, gradient fp32 [N, C, H, W])."""
    f32, f64 = np.float32, np.float64
    x = np.asarray(x, f32)
    t = np.asarray(t, f32)
    n, c, h, w = x.shape
    dw, fw, alpha, smooth = (f32(v) for v in weights)
    up = f32(upstream)
    numel = n * c * h * w
    with np.errstate(all="ignore"):
        # forward chain: score_ref.elementwise, keeping what autograd saves
        p = f32(1) / (f32(1) + np.exp(-x))
        lo, hi = f32(1e-7), f32(1.0 - 1e-7)
        pc = np.where(p < lo, lo, np.where(p > hi, hi, p))
        l1 = np.log(f32(1) - pc)
        l1 = np.where(l1 < f32(-100), f32(-100), l1)
        l0 = np.log(pc)
        l0 = np.where(l0 < f32(-100), f32(-100), l0)
        bce = (t - f32(1)) * l1 - t * l0
        q = np.exp(-bce)
        u = f32(1) - q
        focal = u * u * bce
        # the sums and what follows from them, fp64
        flat = lambda a: a.reshape(n, c, -1).astype(f64)   # noqa: E731
        nan = np.isnan(x).reshape(n, c, -1)
        sum_p = flat(p).sum(-1)
        sum_t = np.where(nan, f64("nan"), flat(t)).sum(-1)
        sum_pt = flat(p * t).sum(-1)
        sum_f = flat(focal).sum(-1)
        den = sum_p + sum_t + f64(smooth)
        num = 2.0 * sum_pt + f64(smooth)
        loss = f64(dw) * np.mean(1.0 - num / den) + f64(fw) * f64(alpha) * sum_f.sum() / f64(numel)
        scale = f64(dw) / f64(n * c) * f64(up)
        A = (-2.0 / den * scale).astype(f32)[:, :, None, None]
        B = (num / (den * den) * scale).astype(f32)[:, :, None, None]
        # autograd's backward, fp32, in the engine's order
        g0 = up * fw / f32(numel)
        m1 = alpha * (u * u)
        g_m1 = g0 * bce
        g_bce = g0 * m1
        g_u2 = g_m1 * alpha
        g_u = g_u2 * (f32(2) * u)
        g_nb = (-g_u) * q
        g_bce = g_bce + (-g_nb)
        d = (f32(1) - pc) * pc
        d = np.where(d < f32(1e-12), f32(1e-12), d)
        g_pc = g_bce * (pc - t) / d
        g_p = np.where((p >= lo) & (p <= hi), g_pc, f32(0))
        g_p = g_p + (A * t + B)
        g = g_p * (f32(1) - p) * p
    assert g.dtype == f32 and g_pc.dtype == f32 and A.dtype == f32
    return f32(loss), g


def ulps(a, b) -> int:
    """Distance of two finite fp32 numbers of one sign in units in the last place."""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    return abs(ia - ib)


def grad_distance(g, ref) -> float:
    """max |g - ref| / max |ref| over the elements where the reference is finite."""
    ok = np.isfinite(ref)
    return float(np.abs(g[ok].astype(np.float64) - ref[ok]).max() / np.abs(ref[ok]).max())


def fixture():
    """The committed cases: list of dicts with the generator parameters and the reference's results."""
    z = np.load(FIXTURE)
    out = []
    for i in range(int(z["n_cases"])):
        nan_at = tuple(int(v) for v in z[f"nan_at_{i}"])
        out.append(dict(name=str(z[f"name_{i}"]), shape=tuple(int(v) for v in z[f"shape_{i}"]),
                        scale=float(z[f"scale_{i}"]), shift=float(z[f"shift_{i}"]), density=float(z[f"density_{i}"]),
                        soft=bool(z[f"soft_{i}"]), seed=int(z[f"seed_{i}"]), nan_at=nan_at if nan_at else None,
                        logits_sha256=str(z[f"logits_sha256_{i}"]), loss=np.float32(z[f"loss_{i}"]),
                        grad=z[f"grad_{i}"], spread=float(z[f"spread_{i}"])))
    return out


def case_tensors(case):
    """(logits fp32 NCHW, target uint8 NHWC) of a fixture case."""
    x, t = generate(case["shape"], case["scale"], case["shift"], case["density"], case["soft"], case["seed"],
                    case["nan_at"])
    assert sha256(x) == case["logits_sha256"], "the seeded generator no longer reproduces the fixture's logits"
    return x, t
