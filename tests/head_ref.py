"""float64 numpy restatement of unet_head_forward / unet_head_backward (include/unet_mi355x.h): out_conv =
Conv2d(64, C, 1) (unet_model.py:50) on a stored feature map, and its backward.  Shared by the CPU and GPU head
tests, together with the seeded generator of the fixture's cases (tests/golden/head_cases.npz holds the generator
parameters and the reference's results, not the inputs) and of the trajectory case (a head fitted by train.py's
loop on seeded features)."""
import os

import numpy as np

import score_ref
from loss_ref import SPREAD_FACTOR, SPREAD_LIMIT  # noqa: F401
from score_ref import sha256  # noqa: F401

FIXTURE = os.path.join(score_ref.REPO, "tests", "golden", "head_cases.npz")
K = 64                  # out_conv's input channels
FEAT_SCALE = 2.5        # relu(normal) * this: the oracle's range of conv1's output (max about 11)
GRAD_SCALE = 1e-3       # scale of grad_logits (what InvoiceLoss leaves at the logits of a small batch)
SAMPLES = 4096          # grad_feat positions the fixture keeps per case
OUTPUTS = ("logits", "grad_w", "grad_b", "grad_feat")

# name, (N, C, H, W), seed, feature channels that are zero everywhere
CASES = [
    ("one", (1, 1, 1, 1), 301, ()),           # a single element
    ("odd", (1, 3, 5, 7), 302, ()),           # unaligned planes, scalar tails
    ("spans", (2, 3, 48, 96), 303, ()),       # 4608 px: more than one tile and span per image, the last partial
    ("c4", (2, 4, 16, 16), 304, ()),          # C = 4
    ("c1", (3, 1, 16, 16), 305, ()),          # C = 1
    ("big", (2, 3, 64, 64), 306, ()),         # several tiles, several images
    ("dead", (2, 3, 16, 16), 307, (5, 40)),   # channels 5 and 40 of feat all zero
]

# the trajectory case: (N, C, H, W), seed, the feature channels whose cut makes the 0/1 targets, the cut, and the
# loop of train.py:119-160 on the head alone: epochs, batch, weight decay, the two learning rates
TRAJ_SHAPE, TRAJ_SEED, TRAJ_CHANNELS, TRAJ_CUT = (4, 3, 32, 32), 311, (3, 17, 42), 2.0
TRAJ_EPOCHS, TRAJ_BATCH, TRAJ_WD, TRAJ_LRS = 20, 2, 1e-4, (1e-2, 1e-3)


def features(rs, n, h, w, dead=()):
    f = (FEAT_SCALE * np.maximum(rs.randn(n, K, h, w), 0.0)).astype(np.float32)
    for k in dead:
        f[:, k] = 0.0
    return f


def head_init(rs, c):
    """out_conv as train.py:106-108 leaves it: Conv2d's default uniform weight (+-1/sqrt(64)), bias -4."""
    return rs.uniform(-0.125, 0.125, size=(c, K)).astype(np.float32), np.full((c,), -4.0, np.float32)


def generate(shape, seed, dead=()):
    """(feat fp32 [N, 64, H, W], w fp32 [C, 64], b fp32 [C], grad_logits fp32 [N, C, H, W])."""
    n, c, h, w = shape
    rs = np.random.RandomState(seed)
    feat = features(rs, n, h, w, dead)
    wt = rs.uniform(-0.125, 0.125, size=(c, K)).astype(np.float32)
    b = (-4.0 + 0.5 * rs.randn(c)).astype(np.float32)
    g = (GRAD_SCALE * rs.randn(n, c, h, w)).astype(np.float32)
    return feat, wt, b, g


def sample_positions(shape, seed):
    """SAMPLES flat indices into grad_feat [N, 64, H, W] (fewer for a smaller tensor: all of it, in order)."""
    n, _, h, w = shape
    numel = n * K * h * w
    if numel <= SAMPLES:
        return np.arange(numel, dtype=np.int64)
    return np.random.RandomState(seed + 1000).randint(0, numel, size=SAMPLES).astype(np.int64)


def trajectory_tensors():
    """(feat fp32 [4, 64, 32, 32], target fp32 0/1 [4, 3, 32, 32], w0 fp32 [3, 64], b0 fp32 [3])."""
    n, c, h, w = TRAJ_SHAPE
    rs = np.random.RandomState(TRAJ_SEED)
    feat = features(rs, n, h, w)
    target = (feat[:, list(TRAJ_CHANNELS)] > TRAJ_CUT).astype(np.float32)
    w0, b0 = head_init(rs, c)
    return feat, np.ascontiguousarray(target), w0, b0


def head(feat, w, b, g=None):
    """float64 throughout, rounded to fp32 once: (logits, grad_w, grad_b, grad_feat); without ``g`` the logits
    alone.  IEEE propagation as numpy's einsum gives it."""
    f64 = np.float64
    f, wt, bb = np.asarray(feat, f64), np.asarray(w, f64), np.asarray(b, f64)
    with np.errstate(all="ignore"):
        logits = (np.einsum("ck,nkhw->nchw", wt, f) + bb[None, :, None, None]).astype(np.float32)
        if g is None:
            return logits
        gg = np.asarray(g, f64)
        grad_w = np.einsum("nchw,nkhw->ck", gg, f).astype(np.float32)
        grad_b = gg.sum((0, 2, 3)).astype(np.float32)
        grad_feat = np.einsum("ck,nchw->nkhw", wt, gg).astype(np.float32)
    return logits, grad_w, grad_b, grad_feat


def distance(a, ref) -> float:
    """max |a - ref| / max |ref| over the elements where the reference is finite (0 when they are equal)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    d = np.abs(a[ok] - ref[ok]).max() if ok.any() else 0.0
    return 0.0 if d == 0.0 else float(d / np.abs(ref[ok]).max())


def fixture():
    """The committed cases: list of dicts with the generator parameters and the reference's results
    (logits / grad_w / grad_b in full, grad_feat at ``positions``; spread_<output> beside each)."""
    z = np.load(FIXTURE)
    out = []
    for i in range(int(z["n_cases"])):
        case = dict(name=str(z[f"name_{i}"]), shape=tuple(int(v) for v in z[f"shape_{i}"]), seed=int(z[f"seed_{i}"]),
                    dead=tuple(int(v) for v in z[f"dead_{i}"]), feat_sha256=str(z[f"feat_sha256_{i}"]),
                    positions=z[f"positions_{i}"])
        for k in OUTPUTS:
            case[k] = z[f"{k}_{i}"]
            case[f"spread_{k}"] = float(z[f"spread_{k}_{i}"])
        out.append(case)
    return out


def trajectory_fixture():
    """{lr: dict(losses fp32 [steps], spread)}: the reference loop's per-step loss in fp32, and the largest relative
    distance of its fp32 trajectory from its fp64 one."""
    z = np.load(FIXTURE)
    assert sha256(trajectory_tensors()[0]) == str(z["traj_feat_sha256"]), \
        "the seeded generator no longer reproduces the trajectory's features"
    return {float(lr): dict(losses=z[f"traj_losses_{j}"], spread=float(z[f"traj_spread_{j}"]))
            for j, lr in enumerate(z["traj_lrs"])}


def case_tensors(case):
    """(feat, w, b, grad_logits) of a fixture case."""
    feat, w, b, g = generate(case["shape"], case["seed"], case["dead"])
    assert sha256(feat) == case["feat_sha256"], "the seeded generator no longer reproduces the fixture's features"
    return feat, w, b, g
