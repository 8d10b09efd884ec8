"""The differentiable InvoiceLoss, the parts that need no GPU: the numpy restatement of unet_loss_grad (loss_ref)
against the reference's fp32 loss and autograd gradient of the fixture (tests/golden/loss_cases.npz) and against
metrics.Score's loss, the new symbols and their argument checks (made before any HIP call), and the criterion's
refusals.

Bar of every comparison with the reference: 8 x the case's own spread (the reference's fp32 autograd against its
fp64 autograd)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_ref
import score_ref
from loss_ref import SPREAD_FACTOR

CASES = loss_ref.fixture()
IDS = [c["name"] for c in CASES]
HEADER = os.path.join(score_ref.REPO, "include", "unet_mi355x.h")


def test_fixture_holds_the_issue_cases():
    assert [(c["name"], c["shape"], c["scale"], c["shift"], c["density"], c["soft"], c["seed"], c["nan_at"])
            for c in CASES] == loss_ref.CASES
    shapes = [c["shape"] for c in CASES]
    for want in ((1, 1, 1, 1), (1, 3, 5, 7), (2, 3, 48, 96), (2, 4, 16, 16), (3, 1, 16, 16), (2, 3, 64, 64)):
        assert want in shapes
    assert sum(c["nan_at"] is not None for c in CASES) == 1
    for c in CASES:
        assert 0 < c["spread"] <= loss_ref.SPREAD_LIMIT
        assert c["grad"].dtype == np.float32 and c["grad"].shape == c["shape"]
    far, _ = loss_ref.case_tensors(CASES[IDS.index("far")])
    assert (far >= 20).any() and (far <= -20).any()          # both far bands are populated
    assert os.path.getsize(loss_ref.FIXTURE) < (1 << 20)


@pytest.fixture(scope="module")
def restated():
    """Per case, once: (logits, target uint8 NHWC, target fp32 NCHW, restatement's loss, restatement's gradient)."""
    out = []
    for case in CASES:
        x, tu8 = loss_ref.case_tensors(case)
        tf = loss_ref.target_f32(tu8)
        out.append((x, tu8, tf) + loss_ref.loss_grad(x, tf))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_reproduces_reference_gradient(i, restated):
    case = CASES[i]
    _, _, _, loss, g = restated[i]
    bar = SPREAD_FACTOR * case["spread"]
    assert np.array_equal(np.isnan(g), np.isnan(case["grad"]))
    d = loss_ref.grad_distance(g, case["grad"])
    print(f"{IDS[i]}: gradient {d:.3e} (bar {bar:.3e}); loss {loss!r} reference {case['loss']!r}")
    assert d <= bar
    if case["nan_at"] is None:
        assert score_ref.rel(loss, case["loss"]) <= bar
        assert np.isfinite(g).all()
    else:
        n, c = case["nan_at"][:2]
        assert np.isnan(loss) and np.isnan(case["loss"])
        assert np.isnan(g[n, c]).all() and np.isnan(g).sum() == g[n, c].size


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_loss_is_the_scores_loss(i, restated):
    """The loss of the restatement equals metrics.Score.loss() of score_ref's entries, to 1 fp32 ulp."""
    from unet_mi355x.metrics import Score
    x, _, tf, loss, _ = restated[i]
    entries, _ = score_ref.score(x, tf, [0.0] * x.shape[1])
    want = np.float32(Score(entries).loss())
    if CASES[i]["nan_at"] is not None:
        assert np.isnan(want) and np.isnan(loss)
    else:
        assert loss_ref.ulps(loss, want) <= 1, (loss, want)


def test_upstream_scales_the_restatement():
    x, tu8 = loss_ref.case_tensors(CASES[IDS.index("odd")])
    tf = loss_ref.target_f32(tu8)
    _, g1 = loss_ref.loss_grad(x, tf)
    _, g2 = loss_ref.loss_grad(x, tf, upstream=2.0)
    assert np.array_equal(g2, np.float32(2) * g1)   # a power of two scales every product exactly


# ---------------------------------------------------------------- the library, no GPU
def test_new_symbols_match_the_header():
    from unet_mi355x import native
    lib = native.load_library()
    assert lib.unet_abi_version() == native.ABI_VERSION == 5
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert ("typedef struct unet_loss_config { float dice_weight, focal_weight, focal_alpha, smooth; } "
            "unet_loss_config;") in src
    assert "int unet_loss_reserve(unet_handle* h, int N, int H, int W);" in src
    assert ("int unet_loss_grad(unet_handle* h, const float* logits, const void* target, int target_kind, int N, "
            "int C, int H, int W, const unet_loss_config* cfg, const float* grad_out, float* loss, "
            "float* grad_logits, void* hip_stream);") in src
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert native.SIGNATURES["unet_loss_reserve"] == (i, [vp, i, i, i])
    assert native.SIGNATURES["unet_loss_grad"] == (i, [vp, vp, vp, i, i, i, i, i, ctypes.POINTER(native.LossConfig),
                                                       vp, vp, vp, vp])
    assert [f for f, _ in native.LossConfig._fields_] == ["dice_weight", "focal_weight", "focal_alpha", "smooth"]
    assert ctypes.sizeof(native.LossConfig) == 16
    for name in ("unet_loss_reserve", "unet_loss_grad"):
        assert hasattr(lib, name)


def _call_loss(lib, **kw):
    from unet_mi355x import native
    dummy = ctypes.create_string_buffer(1 << 16)   # stands for every non-NULL pointer; never read by a refused call
    ptr = ctypes.cast(dummy, ctypes.c_void_p).value
    cfg = native.LossConfig(0.85, 0.15, 0.8, 1.0)
    a = dict(h=ptr, logits=ptr, target=ptr + 4096, kind=native.TGT_F32_NCHW, N=1, C=3, H=16, W=16,
             cfg=ctypes.byref(cfg), grad_out=None, loss=ptr + 8192, grad=ptr + 12288)
    a.update(kw)
    return lib.unet_loss_grad(a["h"], a["logits"], a["target"], a["kind"], a["N"], a["C"], a["H"], a["W"], a["cfg"],
                              a["grad_out"], a["loss"], a["grad"], None)


@pytest.mark.parametrize("kw, word", [
    (dict(h=None), b"handle"),
    (dict(logits=None), b"NULL"),
    (dict(target=None), b"NULL"),
    (dict(cfg=None), b"NULL"),
    (dict(loss=None), b"NULL"),
    (dict(C=0), b"C must be 1..4"),
    (dict(C=5), b"C must be 1..4"),
    (dict(kind=2), b"target_kind"),
    (dict(kind=-1), b"target_kind"),
    (dict(N=0), b"positive"),
    (dict(N=-3), b"positive"),
    (dict(H=0), b"positive"),
    (dict(W=-1), b"positive"),
    (dict(alias=True), b"alias"),
])
def test_loss_grad_rejects_bad_arguments_without_gpu(kw, word):
    from unet_mi355x import native
    lib = native.load_library()
    if kw.pop("alias", False):
        buf = ctypes.create_string_buffer(64)
        p = ctypes.cast(buf, ctypes.c_void_p).value
        kw = dict(logits=p, grad=p)
    assert _call_loss(lib, **kw) == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


@pytest.mark.parametrize("args, word", [
    ((None, 1, 16, 16), b"handle"),
    ((1, 0, 16, 16), b"positive"),
    ((1, 1, 0, 16), b"positive"),
    ((1, 1, 16, -1), b"positive"),
])
def test_loss_reserve_rejects_bad_arguments_without_gpu(args, word):
    from unet_mi355x import native
    lib = native.load_library()
    dummy = ctypes.create_string_buffer(1 << 16)
    h = None if args[0] is None else ctypes.cast(dummy, ctypes.c_void_p).value
    assert lib.unet_loss_reserve(h, *args[1:]) == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


# ---------------------------------------------------------------- the criterion, no GPU
def test_criterion_has_the_references_constructor():
    from unet_mi355x.metrics import InvoiceLoss
    crit = InvoiceLoss()
    assert isinstance(crit, torch.nn.Module) and crit.weights == (0.85, 0.15, 0.8, 1.0)
    crit = InvoiceLoss(dice_weight=0.7, focal_weight=0.3, focal_alpha=0.5, gamma=2.0)
    assert crit.weights == (0.7, 0.3, 0.5, 1.0)
    assert list(crit.parameters()) == [] and crit.state_dict() == {}
    with pytest.raises(ValueError, match="gamma"):
        InvoiceLoss(gamma=3)
    with pytest.raises(ValueError, match="gamma"):
        InvoiceLoss(0.85, 0.15, 0.8, 1.5)


def test_criterion_refuses_cpu_tensors_and_bad_shapes():
    import copy
    from unet_mi355x.metrics import InvoiceLoss
    crit = InvoiceLoss()
    x = torch.zeros(1, 3, 4, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(x, torch.zeros(1, 3, 4, 4))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(x, torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match=r"\[N, C, H, W\]"):
        crit(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    with pytest.raises(RuntimeError, match="C in 1..4"):
        crit(torch.zeros(1, 5, 4, 4), torch.zeros(1, 5, 4, 4))
    assert copy.deepcopy(crit).weights == crit.weights   # a criterion copies without its native handles
