"""The output head (unet_head_forward / unet_head_backward, head.head_conv, UNet.fit_head), the parts that need no
GPU: the fixture (tests/golden/head_cases.npz) holds the issue's cases, the float64 numpy restatement (head_ref)
reproduces the reference's out_conv and autograd on every output, the new symbols match the header, every bad
argument is refused before any HIP call, and the Python entry points refuse CPU tensors.

Bar of every comparison with the reference: 8 x the output's own spread (the reference's fp32 results against its
fp64 ones)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import head_ref
import score_ref
from head_ref import SPREAD_FACTOR

CASES = head_ref.fixture()
IDS = [c["name"] for c in CASES]
HEADER = os.path.join(score_ref.REPO, "include", "unet_mi355x.h")


def test_fixture_holds_the_issue_cases():
    assert [(c["name"], c["shape"], c["seed"], c["dead"]) for c in CASES] == head_ref.CASES
    assert [(c["name"], c["shape"]) for c in CASES] == [
        ("one", (1, 1, 1, 1)), ("odd", (1, 3, 5, 7)), ("spans", (2, 3, 48, 96)), ("c4", (2, 4, 16, 16)),
        ("c1", (3, 1, 16, 16)), ("big", (2, 3, 64, 64)), ("dead", (2, 3, 16, 16))]
    assert CASES[IDS.index("dead")]["dead"] == (5, 40)
    for c in CASES:
        n, cc, h, w = c["shape"]
        feat, wt, b, g = head_ref.case_tensors(c)
        assert feat.shape == (n, 64, h, w) and wt.shape == (cc, 64) and b.shape == (cc,) and g.shape == c["shape"]
        assert feat.min() == 0.0 and feat.max() < 13.0            # relu(normal) in the oracle's range
        assert 0 < np.abs(g).max() < 1e-2                         # grad_logits of scale 1e-3
        for k in c["dead"]:
            assert not feat[:, k].any()
        assert c["logits"].shape == c["shape"] and c["grad_w"].shape == (cc, 64) and c["grad_b"].shape == (cc,)
        assert len(c["positions"]) == min(head_ref.SAMPLES, feat.size) == len(c["grad_feat"])
        assert np.array_equal(c["positions"], head_ref.sample_positions(c["shape"], c["seed"]))
        for k in head_ref.OUTPUTS:
            assert c[k].dtype == np.float32 and 0 <= c[f"spread_{k}"] <= head_ref.SPREAD_LIMIT
    traj = head_ref.trajectory_fixture()
    assert sorted(traj) == [1e-3, 1e-2]
    for lr, t in traj.items():
        assert t["losses"].dtype == np.float32 and len(t["losses"]) == 40 and 0 < t["spread"] <= head_ref.SPREAD_LIMIT
        assert t["losses"][-1] < t["losses"][0]
    feat, target, w0, b0 = head_ref.trajectory_tensors()
    assert feat.shape == (4, 64, 32, 32) and target.shape == (4, 3, 32, 32) and set(np.unique(target)) == {0.0, 1.0}
    assert np.abs(w0).max() <= 0.125 and (b0 == -4).all()
    assert os.path.getsize(head_ref.FIXTURE) < (1 << 20)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_reproduces_the_reference(i):
    case = CASES[i]
    feat, w, b, g = head_ref.case_tensors(case)
    ours = dict(zip(head_ref.OUTPUTS, head_ref.head(feat, w, b, g)))
    ours["grad_feat"] = ours["grad_feat"].reshape(-1)[case["positions"]]
    for k in head_ref.OUTPUTS:
        d, bar = head_ref.distance(ours[k], case[k]), SPREAD_FACTOR * case[f"spread_{k}"]
        print(f"{IDS[i]} {k}: {d:.3e} (bar {bar:.3e})")
        assert ours[k].dtype == np.float32 and d <= bar
    for k in case["dead"]:
        assert (ours["grad_w"][:, k] == 0.0).all() and (case["grad_w"][:, k] == 0.0).all()


def test_restatement_propagates_nan_as_the_issue_states():
    feat, w, b, g = head_ref.case_tensors(CASES[IDS.index("dead")])
    clean = head_ref.head(feat, w, b, g)
    f2 = feat.copy()
    f2[1, 7, 3, 5] = np.nan
    logits, gw, gb, gf = head_ref.head(f2, w, b, g)
    nan = np.isnan(logits)
    assert nan[1, :, 3, 5].all() and nan.sum() == 3
    assert np.isnan(gw[:, 7]).all() and np.isnan(gw).sum() == 3
    assert np.array_equal(gb, clean[2]) and np.array_equal(gf, clean[3])
    g2 = g.copy()
    g2[0, 1, 2, 9] = np.nan
    _, gw, gb, gf = head_ref.head(feat, w, b, g2)
    assert np.isnan(gw[1]).all() and np.isnan(gw).sum() == 64
    assert np.isnan(gb[1]) and np.isnan(gb).sum() == 1
    assert np.isnan(gf[0, :, 2, 9]).all() and np.isnan(gf).sum() == 64


# ---------------------------------------------------------------- the library, no GPU
def test_new_symbols_match_the_header():
    from unet_mi355x import native
    lib = native.load_library()
    assert lib.unet_abi_version() == native.ABI_VERSION == 5
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert "#define UNET_ABI_VERSION 5" in src
    assert "int unet_head_reserve(unet_handle* h, int N, int H, int W);" in src
    assert ("int unet_head_forward(unet_handle* h, const float* feat, const float* w, const float* b, float* logits, "
            "int N, int C, int H, int W, void* hip_stream);") in src
    assert ("int unet_head_backward(unet_handle* h, const float* feat, const float* grad_logits, const float* w, "
            "float* grad_w, float* grad_b, float* grad_feat, int N, int C, int H, int W, void* hip_stream);") in src
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert native.SIGNATURES["unet_head_reserve"] == (i, [vp, i, i, i])
    assert native.SIGNATURES["unet_head_forward"] == (i, [vp, vp, vp, vp, vp, i, i, i, i, vp])
    assert native.SIGNATURES["unet_head_backward"] == (i, [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp])
    for name in ("unet_head_reserve", "unet_head_forward", "unet_head_backward"):
        assert hasattr(lib, name)
    for name in ("head_reserve", "head_forward", "head_backward"):
        assert callable(getattr(native.Handle, name))


def _pointers():
    """Distinct non-NULL host addresses standing for every pointer; a refused call reads none of them."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    return buf, {k: p + 4096 * j for j, k in enumerate(("h", "feat", "w", "b", "logits", "g", "gw", "gb", "gf"))}


@pytest.mark.parametrize("kw, word", [
    (dict(h=None), b"handle"),
    (dict(feat=None), b"NULL"),
    (dict(w=None), b"NULL"),
    (dict(b=None), b"NULL"),
    (dict(logits=None), b"NULL"),
    (dict(C=0), b"C must be 1..4"),
    (dict(C=5), b"C must be 1..4"),
    (dict(N=0), b"positive"),
    (dict(N=-2), b"positive"),
    (dict(H=0), b"positive"),
    (dict(W=-1), b"positive"),
    (dict(N=1 << 30, H=1 << 12, W=1 << 12), b"too large"),
    (dict(alias="logits"), b"alias"),
])
def test_head_forward_rejects_bad_arguments_without_gpu(kw, word):
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    a.update(N=1, C=3, H=16, W=16)
    if kw.get("alias"):
        a["logits"] = a["feat"]
    else:
        a.update(kw)
    rc = lib.unet_head_forward(a["h"], a["feat"], a["w"], a["b"], a["logits"], a["N"], a["C"], a["H"], a["W"], None)
    assert rc == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(h=None), b"handle"),
    (dict(feat=None), b"NULL"),
    (dict(g=None), b"NULL"),
    (dict(w=None), b"NULL"),
    (dict(gw=None), b"pair"),
    (dict(gb=None), b"pair"),
    (dict(gw=None, gb=None, gf=None), b"no output"),
    (dict(C=0), b"C must be 1..4"),
    (dict(C=5), b"C must be 1..4"),
    (dict(N=0), b"positive"),
    (dict(H=-4), b"positive"),
    (dict(W=0), b"positive"),
    (dict(alias="feat"), b"alias"),
    (dict(alias="g"), b"alias"),
])
def test_head_backward_rejects_bad_arguments_without_gpu(kw, word):
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    a.update(N=1, C=3, H=16, W=16)
    if kw.get("alias"):
        a["gf"] = a[kw["alias"]]
    else:
        a.update(kw)
    rc = lib.unet_head_backward(a["h"], a["feat"], a["g"], a["w"], a["gw"], a["gb"], a["gf"], a["N"], a["C"], a["H"],
                                a["W"], None)
    assert rc == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


@pytest.mark.parametrize("args, word", [
    ((None, 1, 16, 16), b"handle"),
    ((1, 0, 16, 16), b"positive"),
    ((1, 1, 0, 16), b"positive"),
    ((1, 1, 16, -1), b"positive"),
])
def test_head_reserve_rejects_bad_arguments_without_gpu(args, word):
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    assert lib.unet_head_reserve(None if args[0] is None else a["h"], *args[1:]) == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


# ---------------------------------------------------------------- the Python entry points, no GPU
def test_head_conv_refuses_cpu_tensors_and_bad_shapes():
    from unet_mi355x.head import head_conv
    feat, w, b = torch.zeros(1, 64, 4, 4), torch.zeros(3, 64, 1, 1, requires_grad=True), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head_conv(feat, w, b)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        head_conv(feat, w.view(3, 64), b)
    with pytest.raises(TypeError):
        head_conv(feat.numpy(), w, b)


def test_fit_head_and_features_refuse_cpu_tensors():
    from unet_mi355x.model import UNet
    m = UNet(3, 3, compute_dtype="fp32")
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.fit_head(x, t, epochs=1, batch=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.features(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.head(torch.zeros(1, 64, 16, 16))
    with pytest.raises(TypeError, match="InvoiceLoss"):
        m.fit_head(x, t, criterion=torch.nn.BCEWithLogitsLoss())
    assert m.training   # the mode is left as found
