"""Host side of the device scoring (unet_score, include/unet_mi355x.h): the reference's training loss
(InvoiceLoss, train.py:18-59), Dice, mask IoU and the threshold sweep, assembled in float64 from the 64-byte
entries the device returns per (image, field) -- pure numpy, nothing there needs a GPU -- and ``InvoiceLoss``, the
same loss as a criterion: a device scalar with a gradient at the logits (unet_loss_grad).
"""
from __future__ import annotations

import threading

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

# unet_score_entry (native.ScoreEntry is the same record as a ctypes struct)
ENTRY_DTYPE = np.dtype([("sum_p", "<f8"), ("sum_t", "<f8"), ("sum_pt", "<f8"), ("sum_focal", "<f8"),
                        ("n_pred", "<i8"), ("n_tgt", "<i8"), ("n_both", "<i8"), ("n_px", "<i8")])


def _ratio(inter: np.ndarray, union: np.ndarray) -> np.ndarray:
    """inter / union in float64, 1.0 where the union is empty (oracle.mask_iou's convention)."""
    out = np.ones(union.shape, np.float64)
    np.divide(inter, union, out=out, where=union != 0)
    return out


class Score:
    """Scores of N pages x C fields.

    entries: structured array [N, C] of ENTRY_DTYPE (or the raw bytes [N, C, 64]).
    hist:    optional int64 [N, C, 2, K + 1] of a sweep over ``probs`` (K ascending probabilities):
             hist[n, c, t, b] = pixels of target class t (t > 0.5) whose logit passes exactly b of the cuts.
    """

    def __init__(self, entries, hist=None, probs=None):
        e = np.asarray(entries)
        if e.dtype != ENTRY_DTYPE:
            if e.dtype != np.uint8 or e.ndim != 3 or e.shape[-1] != ENTRY_DTYPE.itemsize:
                raise ValueError("entries must be a [N, C] array of ENTRY_DTYPE or its bytes [N, C, 64]")
            e = np.ascontiguousarray(e).view(ENTRY_DTYPE)[..., 0]
        if e.ndim != 2:
            raise ValueError("entries must be [N, C]")
        self.entries = e
        if (hist is None) != (probs is None):
            raise ValueError("hist and probs come together")
        self.hist = self.probs = None
        if hist is not None:
            self.probs = np.asarray(probs, np.float64).reshape(-1)
            self.hist = np.asarray(hist, np.int64)
            if self.hist.shape != e.shape + (2, len(self.probs) + 1):
                raise ValueError(f"hist must be {e.shape + (2, len(self.probs) + 1)}, got {self.hist.shape}")

    def __len__(self) -> int:
        return self.entries.shape[0]

    @staticmethod
    def concat(scores) -> "Score":
        """Scores of consecutive chunks as one, along N (all with the same sweep, or all without)."""
        scores = list(scores)
        if not scores:
            raise ValueError("nothing to concatenate")
        first = scores[0]
        for s in scores[1:]:
            if (s.probs is None) != (first.probs is None) or \
                    (s.probs is not None and not np.array_equal(s.probs, first.probs)):
                raise ValueError("scores with different sweeps do not concatenate")
        entries = np.concatenate([s.entries for s in scores], axis=0)
        if first.probs is None:
            return Score(entries)
        return Score(entries, np.concatenate([s.hist for s in scores], axis=0), first.probs)

    def __add__(self, other: "Score") -> "Score":
        return Score.concat([self, other])

    def __getitem__(self, idx) -> "Score":
        if not isinstance(idx, slice):
            raise TypeError("Score is sliced along N")
        return Score(self.entries[idx], None if self.hist is None else self.hist[idx], self.probs)

    # ---------------------------------------------------------------- the reference's means
    def dice(self, smooth: float = 1.0) -> float:
        """MultiLabelDiceLoss (train.py:23-30): mean over (n, c) of 1 - (2 inter + smooth) / (union + smooth)."""
        e = self.entries
        return float(np.mean(1.0 - (2.0 * e["sum_pt"] + smooth) / (e["sum_p"] + e["sum_t"] + smooth)))

    def focal(self, alpha: float = 0.8) -> float:
        """MultiLabelFocalLoss (train.py:39-46, gamma = 2): alpha x the mean over every element."""
        e = self.entries
        return float(alpha * e["sum_focal"].sum() / e["n_px"].sum())

    def loss(self, dice_weight: float = 0.85, focal_weight: float = 0.15, batch: int | None = None,
             smooth: float = 1.0, alpha: float = 0.8) -> float:
        """InvoiceLoss (train.py:57-59) of the whole set as one batch, or with ``batch`` = b the mean of the
        per-batch losses of consecutive batches of b pages (a shorter last one), train.py:133-151's average."""
        if batch is None:
            return dice_weight * self.dice(smooth) + focal_weight * self.focal(alpha)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        parts = [self[i:i + batch].loss(dice_weight, focal_weight, None, smooth, alpha)
                 for i in range(0, len(self), batch)]
        return float(np.mean(parts))

    # ---------------------------------------------------------------- masks
    def iou(self) -> np.ndarray:
        """Mask IoU [N, C] at the scored thresholds; 1.0 where both masks are empty."""
        e = self.entries
        return _ratio(e["n_both"], e["n_pred"] + e["n_tgt"] - e["n_both"])

    def pooled_iou(self) -> np.ndarray:
        """IoU [C] of the pixels of all pages pooled."""
        e = self.entries
        both = e["n_both"].sum(0)
        return _ratio(both, e["n_pred"].sum(0) + e["n_tgt"].sum(0) - both)

    def sweep_counts(self):
        """(n_pred [N, C, K], n_both [N, C, K], n_tgt [N, C]) at every candidate threshold: suffix sums of hist."""
        if self.hist is None:
            raise ValueError("this Score holds no sweep")
        suffix = np.cumsum(self.hist[..., ::-1], axis=-1)[..., ::-1][..., 1:]   # passes more than k cuts, k = 0..K-1
        return suffix.sum(-2), suffix[..., 1, :], self.hist[..., 1, :].sum(-1)

    def sweep_iou(self) -> np.ndarray:
        """Pooled IoU [C, K] at every candidate threshold."""
        pred, both, tgt = self.sweep_counts()
        both = both.sum(0)
        return _ratio(both, pred.sum(0) + tgt.sum(0)[:, None] - both)

    def best_thresholds(self) -> np.ndarray:
        """Per class, the candidate probability of the highest pooled IoU (ties: the lowest probability)."""
        return self.probs[np.argmax(self.sweep_iou(), axis=1)]


# ---------------------------------------------------------------- the loss as a criterion
class _InvoiceLossFn(torch.autograd.Function):
    """loss = InvoiceLoss(pred, target) on the device.  The gradient at the logits is computed in forward (upstream
    1, one more launch over tensors the loss has just read) and kept; backward multiplies it by the upstream
    scalar on the device."""

    @staticmethod
    def forward(ctx, pred, target, crit, want_grad):
        loss, grad = crit.loss_and_grad(pred, target, want_grad=want_grad)
        if want_grad:
            ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None


class InvoiceLoss(nn.Module):
    """train.InvoiceLoss (train.py:49-59) on the device: ``criterion(logits, mask)`` returns a 0-dim fp32 device
    tensor, and ``loss.backward()`` leaves in ``logits.grad`` what the reference's autograd leaves there (fp32, op
    by op).  ``pred``: fp32 logits [N, C, H, W] (C <= 4) on a ROCm device; ``target``: fp32
    [N, C, H, W] with values in [0, 1], or uint8 [N, H, W, C] read as v / 255 (the .npy masks as stored).  The
    target gets no gradient.  gamma is 2 (the kernels square); anything else raises ValueError.  There is no CPU
    fallback."""

    def __init__(self, dice_weight=0.85, focal_weight=0.15, focal_alpha=0.8, gamma=2.0):
        super().__init__()
        if float(gamma) != 2.0:
            raise ValueError(f"unet_mi355x.InvoiceLoss supports gamma = 2 only (the reference's setting), got {gamma}")
        self.dw, self.fw, self.alpha, self.gamma = float(dice_weight), float(focal_weight), float(focal_alpha), 2.0
        self.smooth = 1.0   # MultiLabelDiceLoss's default, which InvoiceLoss does not expose
        self._handles = {}
        self._lock = threading.Lock()

    @property
    def weights(self):
        """(dice_weight, focal_weight, focal_alpha, smooth): unet_loss_config."""
        return self.dw, self.fw, self.alpha, self.smooth

    def __getstate__(self):   # copies and pickles start without native handles
        state = self.__dict__.copy()
        state["_handles"], state["_lock"] = {}, None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._lock = threading.Lock()

    def _handle(self, device: torch.device):
        """This criterion's weightless native handle for ``device``."""
        from . import native
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._lock:
            h = self._handles.get(idx)
            if h is None:
                h = self._handles[idx] = native.Handle(3, 4, "fp32", idx)
        return h

    @staticmethod
    def check_pred(pred):
        if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or not 1 <= pred.shape[1] <= 4:
            raise RuntimeError("InvoiceLoss expects logits [N, C, H, W] with C in 1..4")
        if pred.device.type != "cuda":
            raise RuntimeError("unet_mi355x: InvoiceLoss runs only on a ROCm GPU tensor "
                               f"(got device {pred.device}); there is no CPU fallback")

    def loss_and_grad(self, pred, target, want_grad=True, handle=None):
        """(loss, gradient at the logits or None) as device tensors, outside autograd: what ``forward`` and
        ``UNet.loss_grad`` run.  ``handle``: the native handle to run on (default: this criterion's own)."""
        self.check_pred(pred)
        if not isinstance(target, torch.Tensor):
            raise ValueError("target must be float32 [N, C, H, W] or uint8 [N, H, W, C]")
        h = handle if handle is not None else self._handle(pred.device)
        with torch.cuda.device(pred.device):
            return h.loss_grad(pred.detach().contiguous(), target.detach().contiguous(),
                               torch.cuda.current_stream(pred.device).cuda_stream, self.weights, want_grad=want_grad)

    def forward(self, pred, target):
        self.check_pred(pred)
        want = bool(pred.requires_grad and torch.is_grad_enabled())
        return _InvoiceLossFn.apply(pred, target, self, want)

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles.clear()
