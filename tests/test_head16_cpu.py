"""The head on 16-bit features (unet_head_forward_typed / unet_head_backward_typed, head.head_conv on float16 /
bfloat16 maps, UNet.features(dtype=), UNet.fit_head(feature_dtype=)), the parts that need no GPU: the two symbols
match the header, the ABI is still 5, every bad argument -- a feat_dtype outside F32 / BF16 / F16 included -- is
refused before any HIP call, and the Python entry points check feature_dtype before they look for a device."""
import ctypes
import os
import re

import pytest
import torch

import score_ref

HEADER = os.path.join(score_ref.REPO, "include", "unet_mi355x.h")
F32, BF16, F16 = 0, 1, 2


def test_typed_symbols_match_the_header():
    from unet_mi355x import native
    lib = native.load_library()
    assert lib.unet_abi_version() == native.ABI_VERSION == 5
    text = open(HEADER).read()
    assert "unet_head_forward_typed, unet_head_backward_typed" in text   # the list in the ABI comment
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    src = re.sub(r"\s+", " ", src)
    assert "#define UNET_ABI_VERSION 5" in src
    assert "#define UNET_DTYPE_F32 0" in src and "#define UNET_DTYPE_BF16 1" in src and "#define UNET_DTYPE_F16 2" in src
    assert ("int unet_head_forward_typed(unet_handle* h, const void* feat, int feat_dtype, const float* w, "
            "const float* b, float* logits, int N, int C, int H, int W, void* hip_stream);") in src
    assert ("int unet_head_backward_typed(unet_handle* h, const void* feat, int feat_dtype, const float* grad_logits, "
            "const float* w, float* grad_w, float* grad_b, float* grad_feat, int N, int C, int H, int W, "
            "void* hip_stream);") in src
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert native.SIGNATURES["unet_head_forward_typed"] == (i, [vp, vp, i, vp, vp, vp, i, i, i, i, vp])
    assert native.SIGNATURES["unet_head_backward_typed"] == (i, [vp, vp, i, vp, vp, vp, vp, vp, i, i, i, i, vp])
    for name in ("unet_head_forward_typed", "unet_head_backward_typed"):
        assert hasattr(lib, name)
    assert native.HEAD_FEAT_DTYPES == {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}


def _pointers():
    """Distinct non-NULL host addresses standing for every pointer; a refused call reads none of them."""
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    return buf, {k: p + 4096 * j for j, k in enumerate(("h", "feat", "w", "b", "logits", "g", "gw", "gb", "gf"))}


BAD_DTYPES = [(dict(dt=v), b"feat_dtype") for v in (-1, 3, 4, 7)]


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
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
] + BAD_DTYPES)
def test_typed_forward_rejects_bad_arguments_without_gpu(kw, word, dtype):
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    a.update(N=1, C=3, H=16, W=16, dt=dtype)
    if kw.get("alias"):
        a["logits"] = a["feat"]
    else:
        a.update(kw)
    rc = lib.unet_head_forward_typed(a["h"], a["feat"], a["dt"], a["w"], a["b"], a["logits"], a["N"], a["C"], a["H"],
                                     a["W"], None)
    assert rc == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
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
    (dict(N=1 << 30, H=1 << 12, W=1 << 12), b"too large"),
    (dict(alias="feat"), b"alias"),
    (dict(alias="g"), b"alias"),
] + BAD_DTYPES)
def test_typed_backward_rejects_bad_arguments_without_gpu(kw, word, dtype):
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    a.update(N=1, C=3, H=16, W=16, dt=dtype)
    if kw.get("alias"):
        a["gf"] = a[kw["alias"]]
    else:
        a.update(kw)
    rc = lib.unet_head_backward_typed(a["h"], a["feat"], a["dt"], a["g"], a["w"], a["gw"], a["gb"], a["gf"], a["N"],
                                      a["C"], a["H"], a["W"], None)
    assert rc == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


def test_too_large_is_counted_in_elements_not_bytes():
    """The largest N x H x W the fp32 call takes is taken in 16 bits too, and the first one it refuses is refused:
    the bound is on tiles of pixels, whatever an element's size.  (The accepted geometry is then stopped at the
    next check, the alias, still before any HIP call.)"""
    from unet_mi355x import native
    lib = native.load_library()
    _keep, a = _pointers()
    fits, over = (1 << 21, 1 << 10, 1023), (1 << 21, 1 << 10, 1024)   # 2^31 - 2^21 and 2^31 tiles of 1024 pixels
    for dt in (F32, BF16, F16):
        rc = lib.unet_head_forward_typed(a["h"], a["feat"], dt, a["w"], a["b"], a["feat"], *fits[:1], 3, *fits[1:], None)
        assert rc == native.UNET_EINVAL and b"alias" in lib.unet_last_error(), lib.unet_last_error()
        rc = lib.unet_head_forward_typed(a["h"], a["feat"], dt, a["w"], a["b"], a["feat"], *over[:1], 3, *over[1:], None)
        assert rc == native.UNET_EINVAL and b"too large" in lib.unet_last_error(), lib.unet_last_error()
    rc = lib.unet_head_forward(a["h"], a["feat"], a["w"], a["b"], a["feat"], over[0], 3, over[1], over[2], None)
    assert rc == native.UNET_EINVAL and b"too large" in lib.unet_last_error()


# ---------------------------------------------------------------- the Python entry points, no GPU
def test_fit_head_checks_feature_dtype_before_the_device():
    from unet_mi355x.model import UNet
    m = UNet(3, 3, compute_dtype="fp32")
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    for bad in ("fp8", "float16", "mixed", None, torch.float16):
        with pytest.raises(ValueError, match="feature_dtype"):
            m.fit_head(x, t, epochs=1, batch=2, feature_dtype=bad)
    for ok in ("fp32", "fp16", "bf16"):   # a good one gets as far as the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.fit_head(x, t, epochs=1, batch=2, feature_dtype=ok)
    with pytest.raises(ValueError, match="dtype"):
        m.features(x, dtype=torch.float64)
    for ok in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.features(x, dtype=ok)
    assert m.training   # the mode is left as found


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_head_conv_refuses_16_bit_cpu_tensors(dtype):
    from unet_mi355x.head import head_conv
    feat, w, b = torch.zeros(1, 64, 4, 4, dtype=dtype), torch.zeros(3, 64, 1, 1, requires_grad=True), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head_conv(feat, w, b)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        head_conv(feat, w.view(3, 64), b)


def test_finetune_head_takes_feature_dtype():
    import inspect

    from unet_mi355x import inference
    from unet_mi355x.model import UNet
    assert inspect.signature(inference.finetune_head).parameters["feature_dtype"].default == "fp32"
    assert inspect.signature(UNet.fit_head).parameters["feature_dtype"].default == "fp32"
    assert inspect.signature(UNet.features).parameters["dtype"].default is torch.float32
