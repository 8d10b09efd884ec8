"""The head score without a GPU: unet_head_score as numpy restates it
(tests/head_score_ref.py) against the reference's loss, the C boundary's new symbols and argument checks, and the
validation arguments of the Python front ends.  The device tests are tests/test_head_score_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import head_score_ref as ref
import head_step_ref
import score_ref

HEADER = os.path.join(score_ref.REPO, "include", "unet_mi355x.h")
CASES = ref.fixture()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_meets_the_reference_loss(i):
    """head_score_ref.score is score_ref.score of head_step_ref.logits_chain; the loss of its entries lies within
    8 x max(spread, 2^-23) of the reference's fp32 loss (tests/golden/head_step_cases.npz)."""
    case = CASES[i]
    feat, w, b, tu8 = ref.case_tensors(case)
    t = ref.target_f32(tu8)
    cuts = [0.0] * case["shape"][1]
    entries, hist = ref.score(feat, w, b, t, cuts)
    want, _ = score_ref.score(head_step_ref.logits_chain(feat, w, b), t, cuts)
    assert hist is None and entries.tobytes() == want.tobytes()
    d = head_step_ref.distance(np.float32(ref.loss(entries)), case["loss"])
    print(f"{case['name']} loss: {d:.3e} (bar {ref.bar(case, 'loss'):.3e})")
    assert d <= ref.bar(case, "loss")
    assert (entries["n_px"] == case["shape"][2] * case["shape"][3]).all()


def test_header_library_and_binding_agree():
    from unet_mi355x import native
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = native.load_library()
    for f in ("unet_head_score_reserve", "unet_head_score"):
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert hasattr(lib, f) and f in native.SIGNATURES
    assert "#define UNET_ABI_VERSION 5" in src and lib.unet_abi_version() == 5 == native.ABI_VERSION
    comment = re.search(r"#define UNET_ABI_VERSION 5\s*/\*(.*?)\*/", text, flags=re.S).group(1)
    assert re.search(r"then\s+unet_head_score_reserve,\s+unet_head_score\b", comment)
    assert "unet_head_step_reserve, unet_head_step, unet_adamw_config" in comment
    i, vp, fp = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    assert native.SIGNATURES["unet_head_score_reserve"] == (i, [vp, i, i, i, i])
    assert native.SIGNATURES["unet_head_score"] == (i, [vp, vp, i, vp, vp, vp, i, vp, i, i, i, i, i, fp, vp, fp, i, vp,
                                                        vp])


def test_bad_arguments_are_refused_before_any_hip_call():
    """Every check comes before the first HIP call and before the handle is read: the handle of these calls is a
    block of host memory that is no handle, and the pointers are host addresses no one reads."""
    from unet_mi355x import native
    lib = native.load_library()
    einval = native.UNET_EINVAL
    assert lib.unet_head_score_reserve(None, 1, 16, 16, 0) == einval and b"null" in lib.unet_last_error()
    block = ctypes.create_string_buffer(1 << 16)
    h = ctypes.addressof(block)
    assert lib.unet_head_score_reserve(h, 1, 16, 16, 65) == einval and b"K" in lib.unet_last_error()
    assert lib.unet_head_score_reserve(h, 0, 16, 16, 0) == einval
    bufs = [ctypes.create_string_buffer(64) for _ in range(7)]
    feat, w, b, target, entries, hist, pages = (ctypes.addressof(x) for x in bufs)
    probs = (ctypes.c_float * 3)(0.25, 0.5, 0.75)
    good = dict(h=h, feat=feat, dt=native.DTYPES["fp32"], w=w, b=b, target=target, kind=native.TGT_U8_NHWC, pages=None,
                P=2, N=2, C=3, H=16, W=16, thr=None, entries=entries, probs=None, K=0, hist=None)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.unet_head_score(a["h"], a["feat"], a["dt"], a["w"], a["b"], a["target"], a["kind"], a["pages"], a["P"],
                                 a["N"], a["C"], a["H"], a["W"], a["thr"], a["entries"], a["probs"], a["K"], a["hist"],
                                 None)
        return rc, lib.unet_last_error()

    for name in ("h", "feat", "w", "b", "target", "entries"):
        rc, msg = call(**{name: None})
        assert rc == einval and msg, name
    for c in (0, 5):
        rc, msg = call(C=c)
        assert rc == einval and b"C must be 1..4" in msg
    many = (ctypes.c_float * 65)(*np.linspace(0.01, 0.99, 65))
    rc, msg = call(probs=many, K=65, hist=hist)
    assert rc == einval and b"K" in msg
    for bad in ((0.5, 0.5, 0.75), (0.5, 0.25, 0.75), (0.25, float("nan"), 0.75)):
        rc, msg = call(probs=(ctypes.c_float * 3)(*bad), K=3, hist=hist)
        assert rc == einval and b"ascending" in msg, bad
    rc, msg = call(hist=hist)
    assert rc == einval and b"hist given without sweep_probs" in msg
    rc, msg = call(probs=probs, K=3)
    assert rc == einval and b"sweep_probs given without hist" in msg
    for dt in (native.DTYPES["mixed"], native.DTYPES["fp32_exact"], -1, 99):
        rc, msg = call(dt=dt)
        assert rc == einval and b"feat_dtype" in msg, dt
    rc, msg = call(kind=7)
    assert rc == einval and b"target_kind" in msg
    for name in ("feat", "w", "b", "target"):
        rc, msg = call(entries=good[name])
        assert rc == einval and b"alias" in msg, name
    rc, msg = call(pages=pages, entries=pages)
    assert rc == einval and b"alias" in msg
    rc, msg = call(probs=probs, K=3, hist=feat)
    assert rc == einval and b"alias" in msg
    rc, msg = call(P=0)
    assert rc == einval and b"P" in msg
    rc, msg = call(N=3)
    assert rc == einval and b"N exceeds P" in msg
    rc, msg = call(H=0)
    assert rc == einval


def test_front_ends_accept_validation():
    from unet_mi355x import head, inference, native
    from unet_mi355x.model import UNet
    prm = inspect.signature(UNet.fit_head).parameters
    assert prm["val_pages"].default is None and prm["keep_best"].default is False
    assert prm["sweep"].default is None and prm["report"].default is None
    prm = inspect.signature(inference.finetune_head).parameters
    assert prm["val_fraction"].default == 0.0 and prm["val_seed"].default == 0 and prm["keep_best"].default is False
    assert prm["sweep"].default is None and prm["report"].default is None
    assert list(inspect.signature(head.head_score).parameters) == ["feats", "weight", "bias", "target", "pages",
                                                                   "thresholds", "sweep", "handle"]
    assert list(inspect.signature(native.Handle.head_score).parameters)[:9] == [
        "self", "feat", "target", "weight", "bias", "stream", "pages", "thresholds", "sweep"]
    assert {"feature_cache", "score_features"} <= set(dir(UNet)) and hasattr(native.Handle, "head_score_reserve")
    assert list(inspect.signature(UNet.feature_cache).parameters) == ["self", "x", "batch", "feature_dtype"]
    assert list(inspect.signature(UNet.score_features).parameters) == ["self", "feats", "target", "pages", "sweep"]


def test_fit_head_refuses_bad_val_pages_before_any_device_work():
    """On host tensors: the val_pages checks come before the device check, which a host tensor would fail."""
    from unet_mi355x.model import UNet
    m = UNet(3, 3, compute_dtype="fp32")
    x, t = torch.zeros(4, 3, 16, 16), torch.zeros(4, 3, 16, 16)
    with pytest.raises(ValueError, match="repeats"):
        m.fit_head(x, t, epochs=1, batch=2, val_pages=[1, 1])
    for bad in ([4], [-1], [0, 7]):
        with pytest.raises(IndexError, match="val_pages"):
            m.fit_head(x, t, epochs=1, batch=2, val_pages=bad)
    with pytest.raises(ValueError, match="no page for training"):
        m.fit_head(x, t, epochs=1, batch=2, val_pages=[3, 1, 0, 2])
    with pytest.raises(ValueError, match="empty"):
        m.fit_head(x, t, epochs=1, batch=2, val_pages=[])
    for kw in (dict(keep_best=True), dict(sweep=[0.5])):
        with pytest.raises(ValueError, match="need val_pages"):
            m.fit_head(x, t, epochs=1, batch=2, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # good val_pages: the next check is the device's
        m.fit_head(x, t, epochs=1, batch=2, val_pages=[3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.feature_cache(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score_features(torch.zeros(1, 64, 16, 16), torch.zeros(1, 3, 16, 16))
