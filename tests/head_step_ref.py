"""numpy restatement of unet_head_step (include/unet_mi355x.h): out_conv's logits, the
reference's InvoiceLoss (train.py:18-59), its gradient at the head's 64 C + C parameters from the one-pass sums
F, T, S, and AdamW.  fp32 per element with separately rounded operations, everything after the element chain in
fp64, as the device.  Shared by the CPU and GPU tests of the fused step, together with the seeded generator of the
fixture's cases (tests/golden/head_step_cases.npz holds the generator parameters and the reference's results, not
the inputs)."""
import os

import numpy as np

import head_ref
import score_ref
from loss_ref import SPREAD_FACTOR, SPREAD_LIMIT, WEIGHTS  # noqa: F401
from score_ref import sha256, target_f32  # noqa: F401

FIXTURE = os.path.join(score_ref.REPO, "tests", "golden", "head_step_cases.npz")
K = head_ref.K
OUTPUTS = ("loss", "grad_w", "grad_b")
FLOOR = 2.0 ** -23      # the bar of an output is SPREAD_FACTOR x max(its spread, this): the one-element case's
                        # reference spread is near zero

# name, (N, C, H, W), seed, target density, soft (one target in ten a uniform byte)
CASES = [
    ("one", (1, 1, 1, 1), 401, 0.5, False),       # a single element
    ("odd", (1, 3, 5, 7), 402, 0.3, False),       # unaligned planes, scalar tails
    ("spans", (2, 3, 48, 96), 403, 0.1, False),   # 4608 px: two spans per page, the second ragged
    ("c4", (2, 4, 16, 16), 404, 0.1, True),       # C = 4, soft targets
    ("c1", (3, 1, 16, 16), 405, 0.2, True),       # C = 1
    ("big", (2, 3, 64, 64), 406, 0.2, False),     # a full span per page
]


def generate(shape, seed, density, soft):
    """(feat fp32 [N, 64, H, W] as head_ref's, w fp32 [C, 64] and b fp32 [C] as train.py:106-108 leaves out_conv,
    target uint8 [N, H, W, C]: 255 with probability ``density`` else 0; with ``soft`` one in ten a uniform byte)."""
    n, c, h, w = shape
    rs = np.random.RandomState(seed)
    feat = head_ref.features(rs, n, h, w)
    wt, b = head_ref.head_init(rs, c)
    target = np.where(rs.rand(n, h, w, c) < density, 255, 0)
    if soft:
        target = np.where(rs.rand(n, h, w, c) < 0.1, rs.randint(0, 256, size=(n, h, w, c)), target)
    return feat, wt, b, target.astype(np.uint8)


def logits_chain(feat, w, b):
    """unet_head_forward's chain: fp32 fmaf from the bias, k ascending (each step formed in fp64 -- the product of
    two fp32 values is exact there -- and rounded to fp32)."""
    f32, f64 = np.float32, np.float64
    feat, w, b = np.asarray(feat, f32), np.asarray(w, f32), np.asarray(b, f32)
    n, _, hh, ww = feat.shape
    x = np.broadcast_to(b[None, :, None, None], (n, w.shape[0], hh, ww)).astype(f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            x = (w[None, :, k, None, None].astype(f64) * feat[:, None, k].astype(f64) + x.astype(f64)).astype(f32)
    return x


def in_clamp_band(x) -> bool:
    """a logit with 14 < |x| < 20: there the clamp of train.py:41 makes two correct fp32 implementations disagree
    element by element"""
    a = np.abs(x)
    return bool(((a > 14) & (a < 20)).any())


def step(feat, w, b, t, weights=WEIGHTS):
    """feat fp32 [N, 64, H, W], t fp32 [N, C, H, W].  Returns (loss fp32, grad_w fp32 [C, 64], grad_b fp32 [C]) by
    the one-pass sums."""
    f32, f64 = np.float32, np.float64
    x = logits_chain(feat, w, b)
    t = np.asarray(t, f32)
    n, c, h, ww = x.shape
    dw, fw, alpha, smooth = (f32(v) for v in weights)
    numel = n * c * h * ww
    with np.errstate(all="ignore"):
        # the element chain, fp32: loss_chain, then the focal branch's backward for an upstream gradient of 1
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
        m1 = alpha * (u * u)
        g_u = (bce * alpha) * (f32(2) * u)
        g_bce = m1 + (-((-g_u) * q))
        d = (f32(1) - pc) * pc
        d = np.where(d < f32(1e-12), f32(1e-12), d)
        g_pc = g_bce * (pc - t) / d
        e = np.where((p >= lo) & (p <= hi), g_pc, f32(0))
        assert e.dtype == f32 and focal.dtype == f32
        # everything else fp64
        flat = lambda a: a.reshape(n, c, -1).astype(f64)   # noqa: E731
        s = flat(f32(1) - p) * flat(p)
        es, ts = flat(e) * s, flat(t) * s
        sum_p = flat(p).sum(-1)
        sum_t = np.where(np.isnan(x).reshape(n, c, -1), f64("nan"), flat(t)).sum(-1)
        sum_pt = flat(p * t).sum(-1)
        sum_f = flat(focal).sum(-1)
        den = sum_p + sum_t + f64(smooth)
        num = 2.0 * sum_pt + f64(smooth)
        loss = f64(dw) * np.mean(1.0 - num / den) + f64(fw) * f64(alpha) * sum_f.sum() / f64(numel)
        scale = f64(dw) / f64(n * c)
        A, B = -2.0 / den * scale, num / (den * den) * scale
        g0 = f64(fw / f32(numel))
        ff = np.asarray(feat, f64).reshape(n, K, -1)
        F, T, S = (np.einsum("ncp,nkp->nck", v, ff) for v in (es, ts, s))
        grad_w = (g0 * F + A[:, :, None] * T + B[:, :, None] * S).sum(0)
        grad_b = (g0 * es.sum(-1) + A * ts.sum(-1) + B * s.sum(-1)).sum(0)
    return f32(loss), grad_w.astype(f32), grad_b.astype(f32)


def adamw(theta, m, v, g, lr, step_no, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4):
    """torch.optim.AdamW's update on the fp32 gradient ``g``, in float64 with the constants as the C struct carries
    them (fp32), each of (theta, m, v) rounded to fp32 once."""
    f32, f64 = np.float32, np.float64
    lr, b1, b2, eps, wd = (f64(f32(a)) for a in (lr, betas[0], betas[1], eps, weight_decay))
    g, m, v, theta = (np.asarray(a, f32).astype(f64) for a in (g, m, v, theta))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    th = theta * (1.0 - lr * wd)
    th = th - lr / (1.0 - b1 ** step_no) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** step_no) + eps)
    return th.astype(f32), m1.astype(f32), v1.astype(f32)


def distance(a, ref) -> float:
    """max |a - ref| / max |ref| (0 when they are equal; a scalar: its relative distance)"""
    return head_ref.distance(np.atleast_1d(a), np.atleast_1d(ref))


def bar(case, output) -> float:
    return SPREAD_FACTOR * max(case[f"spread_{output}"], FLOOR)


def fixture():
    """The committed cases: list of dicts with the generator parameters, the reference's fp32 loss, grad_w and
    grad_b, and spread_<output> beside each."""
    z = np.load(FIXTURE)
    out = []
    for i in range(int(z["n_cases"])):
        case = dict(name=str(z[f"name_{i}"]), shape=tuple(int(v) for v in z[f"shape_{i}"]), seed=int(z[f"seed_{i}"]),
                    density=float(z[f"density_{i}"]), soft=bool(z[f"soft_{i}"]), feat_sha256=str(z[f"feat_sha256_{i}"]))
        for k in OUTPUTS:
            case[k] = z[f"{k}_{i}"]
            case[f"spread_{k}"] = float(z[f"spread_{k}_{i}"])
        out.append(case)
    return out


def case_tensors(case):
    """(feat, w, b, target uint8 NHWC) of a fixture case."""
    feat, w, b, t = generate(case["shape"], case["seed"], case["density"], case["soft"])
    assert sha256(feat) == case["feat_sha256"], "the seeded generator no longer reproduces the fixture's features"
    return feat, w, b, t
