"""The output head as a differentiable operator: ``out_conv = Conv2d(64, n_classes, 1)`` (unet_model.py:50) on a
stored feature map, forward and backward on the native kernels (unet_head_forward / unet_head_backward,
include/unet_mi355x.h).  With ``metrics.InvoiceLoss`` it closes the loop
``loss = criterion(head_conv(feat, w, b), mask); loss.backward()`` for the 64 C + C parameters of the head: a
linear probe on frozen features (``UNet.fit_head``).  ``HeadFit`` is the same step as one native call: logits, loss,
gradient and AdamW from one pass over the feature cache (unet_head_step).  There is no CPU
fallback.
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


def _page_list(feats: torch.Tensor, pages, who: str):
    """``pages`` as the kernels read it: a device int32 tensor as it is, a host list range-checked first."""
    if pages is None or isinstance(pages, torch.Tensor) and pages.device.type == "cuda":
        return pages if pages is None or pages.dtype == torch.int32 else pages.to(torch.int32)
    idx = [int(i) for i in (pages.tolist() if isinstance(pages, torch.Tensor) else pages)]
    if not idx or min(idx) < 0 or max(idx) >= feats.shape[0]:
        raise IndexError(f"{who}: pages must be a non-empty list of indices in [0, {feats.shape[0]})")
    return torch.tensor(idx, dtype=torch.int32).to(feats.device)


def head_score(feats: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, target: torch.Tensor, pages=None,
               thresholds=None, sweep=None, handle: native.Handle | None = None):
    """Score the head on pages of a feature cache without forming the logits in memory (unet_head_score,
    include/unet_mi355x.h): what ``score_logits(head_conv(feats[pages], w, b), target[pages])``
    computes, from one pass over the cache, with no gathered copy.

    feats: the cache [P, 64, H, W] (fp32, fp16 or bf16; 16-bit features are read in place); weight: fp32
    [C, 64, 1, 1] or [C, 64] with C in 1..4; bias: fp32 [C]; target: fp32 [P, C, H, W] or uint8 [P, H, W, C]; all on
    one ROCm device (a CPU tensor raises).  ``pages``: the pages to score, in the order of the returned entries
    (None: all, in order) -- a host list is range-checked here (IndexError), a device tensor goes to the kernel as
    it is, where an index outside [0, P) is never used as an address and gives that slot NaN sums.
    ``thresholds``: C probabilities (None: the handle's); ``sweep``: up to 64 ascending probabilities.  Returns a
    ``metrics.Score``; the 64 bytes per (page, field) and the histogram are copied to the host, which synchronises.
    ``handle``: the native handle to run on (default: one of this module's per device)."""
    from .metrics import Score
    for name, t in (("feats", feats), ("weight", weight), ("bias", bias), ("target", target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"head_score: {name} must be a tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"unet_mi355x: head_score runs only on ROCm GPU tensors (got {name} on {t.device}); "
                               "there is no CPU fallback")
    if feats.dim() != 4 or feats.shape[1] != 64:
        raise RuntimeError("head_score expects features [P, 64, H, W]")
    f = _feat(feats)
    probs = None if sweep is None else [float(p) for p in sweep]
    h = handle if handle is not None else _handle(f.device)
    with torch.cuda.device(f.device):
        entries, hist = h.head_score(f, target.detach().contiguous(), _f32(weight), _f32(bias),
                                     torch.cuda.current_stream(f.device).cuda_stream,
                                     pages=_page_list(f, pages, "head_score"), thresholds=thresholds, sweep=probs)
    return Score(entries.cpu().numpy(), None if hist is None else hist.cpu().numpy(), probs)


class HeadFit:
    """``loss = criterion(head_conv(feat, w, b), mask); loss.backward(); AdamW.step()`` as one native call per step
    (unet_head_step, include/unet_mi355x.h): one pass over the features, no logits, no gathered
    batch, three launches.  It owns AdamW's moments and step count; ``weight`` and ``bias`` stay the caller's and are
    updated in place.

    weight: contiguous fp32 [C, 64, 1, 1] or [C, 64] with C in 1..4, bias: contiguous fp32 [C], on one ROCm device
    (tensors or parameters; autograd is not involved).  lr, betas, eps, weight_decay: torch.optim.AdamW's.
    criterion: a ``metrics.InvoiceLoss`` whose weights to use (default: the reference's).  handle: the native handle
    to run on (default: one of this module's per device)."""

    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-4, criterion=None, handle: native.Handle | None = None):
        from .metrics import InvoiceLoss
        crit = criterion if criterion is not None else InvoiceLoss()
        if not isinstance(crit, InvoiceLoss):
            raise TypeError("criterion must be a unet_mi355x.metrics.InvoiceLoss")
        for name, t in (("weight", weight), ("bias", bias)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"HeadFit: {name} must be a tensor")
            if t.device.type != "cuda":
                raise RuntimeError(f"unet_mi355x: HeadFit runs only on ROCm GPU tensors (got {name} on {t.device}); "
                                   "there is no CPU fallback")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"HeadFit: {name} must be contiguous float32 (it is updated in place)")
        c = weight.shape[0] if weight.dim() in (2, 4) else 0
        if not 1 <= c <= 4 or tuple(weight.shape[1:]) not in ((64,), (64, 1, 1)):
            raise ValueError("HeadFit expects a weight [C, 64, 1, 1] or [C, 64] with C in 1..4")
        if tuple(bias.shape) != (c,) or bias.device != weight.device:
            raise ValueError(f"HeadFit expects a bias [{c}] on {weight.device}")
        self.weight, self.bias, self.n_classes = weight, bias, c
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), \
            float(weight_decay)
        self.loss_weights = crit.weights
        self.handle = handle if handle is not None else _handle(weight.device)
        self.state = torch.zeros((2 * (64 * c + c),), device=weight.device, dtype=torch.float32)   # m_w, m_b, v_w, v_b
        self.steps = 0

    def _pages(self, feats: torch.Tensor, pages):
        """``pages`` as the kernel reads it: a device int32 tensor as it is, a host list range-checked first."""
        return _page_list(feats, pages, "HeadFit")

    def _call(self, feats, target, pages, opt, want_grads):
        if not isinstance(feats, torch.Tensor) or feats.device != self.weight.device:
            raise RuntimeError(f"HeadFit: feats must be a tensor on {self.weight.device}; there is no CPU fallback")
        f = _feat(feats)
        with torch.cuda.device(f.device):
            return self.handle.head_step(f, target.detach().contiguous(), self.weight.detach(), self.bias.detach(),
                                         torch.cuda.current_stream(f.device).cuda_stream,
                                         pages=self._pages(f, pages), weights=self.loss_weights, opt=opt,
                                         state=self.state, want_grads=want_grads)

    def step(self, feats: torch.Tensor, target: torch.Tensor, pages=None, lr: float | None = None) -> torch.Tensor:
        """One update on the batch ``pages`` (None: every page, in order) of the cache ``feats`` [P, 64, H, W] (fp32,
        fp16 or bf16) and its masks ``target`` (fp32 [P, C, H, W] or uint8 [P, H, W, C]).  ``lr``: this step's
        learning rate (default: the constructor's; a scheduler's value goes here).  Returns the batch's loss
        before the update, a 0-dim fp32 device tensor.  The version counters of ``weight`` and ``bias`` move, so
        whatever keys on them (``UNet``'s weight signature) sees the update."""
        opt = (self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps, self.weight_decay,
               self.steps + 1)
        loss, _, _ = self._call(feats, target, pages, opt, False)
        self.steps += 1
        torch.autograd.graph.increment_version(self.weight)   # the native call wrote behind autograd's back
        torch.autograd.graph.increment_version(self.bias)
        return loss

    def loss_and_grads(self, feats: torch.Tensor, target: torch.Tensor, pages=None):
        """(loss, grad_w [C, 64], grad_b [C]) of the same batch, fp32 device tensors; nothing is updated."""
        return self._call(feats, target, pages, None, True)
