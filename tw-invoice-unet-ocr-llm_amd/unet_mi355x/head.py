"""The output head as a differentiable operator: ``out_conv = Conv2d(64, n_classes, 1)`` (unet_model.py:50) on a
stored feature map, forward and backward on the native kernels (unet_head_forward / unet_head_backward,
include/unet_mi355x.h).  With ``metrics.InvoiceLoss`` it closes the loop
``loss = criterion(head_conv(feat, w, b), mask); loss.backward()`` for the 64 C + C parameters of the head: a
linear probe on frozen features (``UNet.fit_head``).  There is no CPU fallback.
"""
from __future__ import annotations

import threading

import torch
from torch.autograd.function import once_differentiable

from . import native

_handles: dict = {}
_lock = threading.Lock()


def _handle(device: torch.device) -> native.Handle:
    """The module's weightless native handle for ``device`` (the head calls take their weights as pointers)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _lock:
        h = _handles.get(idx)
        if h is None:
            h = _handles[idx] = native.Handle(3, 4, "fp32", idx)
    return h


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t


def _feat(t: torch.Tensor) -> torch.Tensor:
    """The features as the kernels read them: float16 / bfloat16 in place (contiguous in their own dtype, never
    widened: the typed kernels widen each value in registers), every other dtype as contiguous fp32."""
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.detach().contiguous()
    return _f32(t)


class _HeadConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, weight, bias, handle):
        f, w, b = _feat(feat), _f32(weight), _f32(bias)
        ctx.handle = handle
        ctx.shapes = (feat.shape, weight.shape, bias.shape, feat.dtype, weight.dtype, bias.dtype)
        ctx.save_for_backward(f, w)
        with torch.cuda.device(f.device):
            return handle.head_forward(f, w, b, torch.cuda.current_stream(f.device).cuda_stream)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_logits):
        f, w = ctx.saved_tensors
        fs, ws, bs, fdt, wdt, bdt = ctx.shapes
        want_feat = ctx.needs_input_grad[0]
        want_params = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (want_feat or want_params):
            return None, None, None, None
        with torch.cuda.device(f.device):
            gw, gb, gf = ctx.handle.head_backward(f, _f32(grad_logits), w,
                                                  torch.cuda.current_stream(f.device).cuda_stream,
                                                  want_params=want_params, want_feat=want_feat)
        return (gf.view(fs).to(fdt) if want_feat else None,
                gw.view(ws).to(wdt) if ctx.needs_input_grad[1] else None,
                gb.view(bs).to(bdt) if ctx.needs_input_grad[2] else None, None)


def head_conv(feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, handle: native.Handle | None = None):
    """``F.conv2d(feat, weight, bias)`` for the 1x1 head on the device, with autograd.

    feat: [N, 64, H, W]; weight: [C, 64, 1, 1] or [C, 64] with C in 1..4; bias: [C]; all on one ROCm device
    (a CPU tensor raises).  A float16 / bfloat16 ``feat`` is used in place -- made contiguous in its own dtype if it
    is not, never widened to an fp32 copy, and saved for backward as it is: the kernels widen each value exactly as
    they read it, so every output is bitwise that of the call on ``feat.float()``.  Other non-contiguous or non-fp32
    inputs are made contiguous fp32 first.  Returns the logits, fp32 [N, C, H, W]: one fp32 fmaf chain per element
    from the bias, k ascending.  ``backward`` computes only the gradients autograd asks for: grad_weight /
    grad_bias (fp64 sums over a fixed tree, bitwise reproducible) and grad_feat (computed in fp32, returned in
    ``feat``'s dtype).  ``handle``: the native handle to run on (default: one of this module's per device)."""
    for name, t in (("feat", feat), ("weight", weight), ("bias", bias)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"head_conv: {name} must be a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"unet_mi355x: head_conv runs only on ROCm GPU tensors (got {name} on {t.device}); "
                               "there is no CPU fallback")
    if feat.dim() != 4 or feat.shape[1] != 64:
        raise RuntimeError("head_conv expects features [N, 64, H, W]")
    c = weight.shape[0] if weight.dim() in (2, 4) else 0
    if not 1 <= c <= 4 or tuple(weight.shape[1:]) not in ((64,), (64, 1, 1)):
        raise RuntimeError("head_conv expects a weight [C, 64, 1, 1] or [C, 64] with C in 1..4")
    if tuple(bias.shape) != (c,):
        raise RuntimeError(f"head_conv expects a bias [{c}]")
    if weight.device != feat.device or bias.device != feat.device:
        raise RuntimeError("head_conv: feat, weight and bias must be on one device")
    return _HeadConvFn.apply(feat, weight, bias, handle if handle is not None else _handle(feat.device))
