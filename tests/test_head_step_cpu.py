"""The fused head training step without a GPU: the one-pass algebra of unet_head_step as
numpy restates it (tests/head_step_ref.py) against the reference's autograd, the C boundary's new symbols, and the
``fused`` switch of the Python front ends.  The device tests are tests/test_head_step_gpu.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import head_step_ref as ref

HEADER = os.path.join(ref.score_ref.REPO, "include", "unet_mi355x.h")
CASES = ref.fixture()
IDS = [c["name"] for c in CASES]


def test_fixture_holds_the_issue_cases():
    assert [(c["name"], c["shape"]) for c in CASES] == [(n, s) for n, s, *_ in ref.CASES]
    assert [c["shape"] for c in CASES] == [(1, 1, 1, 1), (1, 3, 5, 7), (2, 3, 48, 96), (2, 4, 16, 16), (3, 1, 16, 16),
                                           (2, 3, 64, 64)]
    for c in CASES:
        assert all(c[f"spread_{k}"] <= ref.SPREAD_LIMIT for k in ref.OUTPUTS)
        assert c["grad_w"].shape == (c["shape"][1], 64) and c["grad_b"].shape == (c["shape"][1],)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_one_pass_sums_meet_the_reference(i):
    """grad_w = sum_n (g0 F + A T + B S) from the three per-(page, class) vectors, fp32 element chain and fp64 sums:
    within 8 x max(spread, 2^-23) of the reference's fp32 autograd, per output."""
    case = CASES[i]
    feat, w, b, tu8 = ref.case_tensors(case)
    x = ref.logits_chain(feat, w, b)
    assert not ref.in_clamp_band(x)
    got = dict(zip(ref.OUTPUTS, ref.step(feat, w, b, ref.target_f32(tu8))))
    for k in ref.OUTPUTS:
        d = ref.distance(got[k], case[k])
        print(f"{case['name']} {k}: {d:.3e} (bar {ref.bar(case, k):.3e})")
        assert got[k].dtype == np.float32 and d <= ref.bar(case, k)


def test_one_pass_sums_equal_the_two_pass_gradient():
    """The same numbers the other way round: out_conv's backward (head_ref.head) of loss_ref's gradient at the
    logits, which forms A, B first and then walks the elements."""
    import head_ref
    import loss_ref
    case = CASES[IDS.index("spans")]
    feat, w, b, tu8 = ref.case_tensors(case)
    t = ref.target_f32(tu8)
    loss, gw, gb = ref.step(feat, w, b, t)
    l2, g = loss_ref.loss_grad(ref.logits_chain(feat, w, b), t)
    _, gw2, gb2, _ = head_ref.head(feat, w, b, g)
    assert loss_ref.ulps(loss, l2) <= 1
    assert ref.distance(gw, gw2) <= ref.bar(case, "grad_w") and ref.distance(gb, gb2) <= ref.bar(case, "grad_b")


def test_adamw_restatement_matches_torch():
    """head_step_ref.adamw against torch.optim.AdamW on the CPU, three steps, torch given the constants as the C
    struct carries them (fp32): fp32 torch and the fp64 restatement then differ by rounding only."""
    import torch
    rs = np.random.RandomState(3)
    theta = rs.uniform(-0.125, 0.125, size=(195,)).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(theta.copy()))
    lr, b1, b2, eps, wd = (float(np.float32(a)) for a in (1e-2, 0.9, 0.999, 1e-8, 1e-4))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    for step_no in (1, 2, 3):
        g = (1e-3 * rs.randn(195)).astype(np.float32)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        theta, m, v = ref.adamw(theta, m, v, g, 1e-2, step_no)
        st = opt.state[p]
        assert np.abs(theta - p.detach().numpy()).max() <= 4 * 2.0 ** -24 * 0.125
        assert ref.distance(m, st["exp_avg"].numpy()) <= 2.0 ** -22
        assert ref.distance(v, st["exp_avg_sq"].numpy()) <= 2.0 ** -22


def test_header_library_and_binding_agree():
    from unet_mi355x import native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = native.load_library()
    for f in ("unet_head_step_reserve", "unet_head_step"):
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert hasattr(lib, f) and f in native.SIGNATURES
    assert "unet_adamw_config" in src and "#define UNET_ABI_VERSION 5" in src
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert native.SIGNATURES["unet_head_step_reserve"] == (i, [vp, i, i, i])
    assert native.SIGNATURES["unet_head_step"] == (
        i, [vp, vp, i, vp, i, vp, i, i, i, i, i, ctypes.POINTER(native.LossConfig), vp, vp, vp, vp, vp,
            ctypes.POINTER(native.AdamWConfig), vp, vp])
    assert [n for n, _ in native.AdamWConfig._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay", "step"]
    assert ctypes.sizeof(native.AdamWConfig) == 24


def test_bad_arguments_are_refused_before_any_hip_call():
    from unet_mi355x import native
    lib = native.load_library()
    assert lib.unet_head_step_reserve(None, 1, 16, 16) == native.UNET_EINVAL
    assert b"null" in lib.unet_last_error()
    cfg = native.LossConfig(0.85, 0.15, 0.8, 1.0)
    rc = lib.unet_head_step(None, None, 0, None, 0, None, 1, 1, 3, 16, 16, ctypes.byref(cfg), None, None, None, None,
                            None, None, None, None)
    assert rc == native.UNET_EINVAL and b"null" in lib.unet_last_error()


def test_front_ends_accept_fused():
    from unet_mi355x import head, inference
    from unet_mi355x.model import UNet
    for fn in (UNet.fit_head, inference.finetune_head):
        prm = inspect.signature(fn).parameters["fused"]
        assert prm.default is False
    assert {"step", "loss_and_grads"} <= set(dir(head.HeadFit))
    prm = inspect.signature(head.HeadFit.__init__).parameters
    assert prm["betas"].default == (0.9, 0.999) and prm["eps"].default == 1e-8 and prm["weight_decay"].default == 1e-4
