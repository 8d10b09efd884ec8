"""Drop-in ``UNet`` for the reference ``unet_model.UNet`` (unet_model.py:23-86).

Same constructor, same sub-module tree and therefore the same 136 ``state_dict`` keys
and shapes, so ``load_state_dict(torch.load("checkpoints/best_unet_model.pth"))``
works unchanged (inference.py:20-21).  ``forward`` runs the MI355X native path
(libunet_mi355x.so): the parameters held by the torch sub-modules are only the
weight *container*; they are BN-folded and pre-packed into the native handle the
first time a forward runs on a device, and again whenever a parameter changes.

There is no CPU / eager fallback: a CPU input raises.  The network's own backward pass is not part of this
project, except for ``out_conv``: ``UNet.features`` / ``head`` / ``fit_head`` fit the output head on frozen
features (unet_mi355x/head.py).
"""
from __future__ import annotations

import os
import threading

import torch
import torch.nn as nn

from . import native

DEFAULT_DTYPE = os.environ.get("UNET_MI355X_DTYPE", "fp32")
# storage types of a feature map the head kernels read (features' dtype, fit_head's feature_dtype)
_FEATURE_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# Bumped whenever a module of a UNet's tree (the _Tracked classes below) changes its parameters, buffers or
# children -- attribute assignment, register_parameter / register_buffer / add_module, deletion -- or converts
# its tensors (_apply: .to / .cuda / .half): the cached list of tensors whose (data_ptr, _version) signature
# decides re-packing is then rebuilt.  Between such events the per-forward check reads 136 cached tensors
# instead of rebuilding state_dict().  Scoped to these classes: no process-global torch hooks, so other
# modules of the app process (EasyOCR's) are never touched.
_TREE_EPOCH = [0]


def _bump_epoch(*_args):
    _TREE_EPOCH[0] += 1


class _Tracked:
    """Mixin of every module class in the UNet tree: any change to this module's own tensors or children
    bumps _TREE_EPOCH.  A tree holding a module without it (a user-assigned plain nn.Module) makes
    UNet._signature walk the live tree on every call instead of trusting the cached list."""

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        _bump_epoch()

    def __delattr__(self, name):
        super().__delattr__(name)
        _bump_epoch()

    def register_parameter(self, name, param):
        super().register_parameter(name, param)
        _bump_epoch()

    def register_buffer(self, name, tensor, persistent=True):
        super().register_buffer(name, tensor, persistent)
        _bump_epoch()

    def add_module(self, name, module):
        super().add_module(name, module)
        _bump_epoch()

    def register_module(self, name, module):
        self.add_module(name, module)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        _bump_epoch()
        return out


# the reference's layer classes (same constructor, parameters, state_dict keys and repr), tracked
class Conv2d(_Tracked, nn.Conv2d):
    pass


class BatchNorm2d(_Tracked, nn.BatchNorm2d):
    pass


class ReLU(_Tracked, nn.ReLU):
    pass


class Sequential(_Tracked, nn.Sequential):
    pass


class MaxPool2d(_Tracked, nn.MaxPool2d):
    pass


class ConvTranspose2d(_Tracked, nn.ConvTranspose2d):
    pass


class DoubleConv(_Tracked, nn.Module):
    """unet_model.py:6-20: (conv3x3, BN, ReLU) x 2 -- the same parameters (and state_dict keys).

    Inside UNet.forward the blocks run fused with pooling / concat / head (the whole-network native
    path).  Called on its own, forward runs the block on the native library too (unet_block_*: the
    first-conv kernel or the MFMA rings, BN folded, eval semantics), for every block shape of the
    reference network; ``compute_dtype`` as UNet's (None: the UNET_MI355X_DTYPE default, fp32).
    """

    def __init__(self, in_ch: int, out_ch: int, compute_dtype: str | None = None):
        super().__init__()
        self.net = Sequential(
            Conv2d(in_ch, out_ch, kernel_size=3, padding=1),
            BatchNorm2d(out_ch),
            ReLU(inplace=True),
            Conv2d(out_ch, out_ch, kernel_size=3, padding=1),
            BatchNorm2d(out_ch),
            ReLU(inplace=True),
        )
        self.in_ch, self.out_ch = in_ch, out_ch
        self.compute_dtype = compute_dtype
        self._blocks: dict = {}
        self._packed_sig: dict = {}
        self._lock = threading.Lock()

    def forward(self, x):
        """unet_model.py:19-20 on the native path: NCHW in -> NCHW fp32 out [N, out_ch, H, W]."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise RuntimeError("DoubleConv.forward expects a 4-D NCHW tensor")
        if x.shape[1] != self.in_ch:
            raise RuntimeError(f"expected input with {self.in_ch} channels, got {x.shape[1]}")
        if x.device.type != "cuda":
            raise RuntimeError("unet_mi355x: DoubleConv runs only on a ROCm GPU tensor "
                               f"(got device {x.device}); there is no CPU fallback")
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("unet_mi355x.DoubleConv is inference-only (eval BatchNorm folded, no autograd); "
                               "call .eval() or run under torch.no_grad()")
        blk = self.native_block(x.device)
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        n, _, h, w = x.shape
        y = torch.empty((n, self.out_ch, h, w), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            blk.forward(x, y, torch.cuda.current_stream(x.device).cuda_stream)
        return y

    def native_block(self, device: torch.device) -> native.Block:
        """The packed native block for ``device`` (re-packs if any parameter changed)."""
        dtype = self.compute_dtype or DEFAULT_DTYPE
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._lock:
            blk = self._blocks.get((idx, dtype))
            if blk is None:
                blk = self._blocks[(idx, dtype)] = native.Block(self.in_ch, self.out_ch, dtype, idx)
            sd = self.state_dict(keep_vars=True)
            sig = tuple((t.data_ptr(), t._version) for t in sd.values())
            if self._packed_sig.get((idx, dtype)) != sig:
                blk.load_weights(sd)
                self._packed_sig[(idx, dtype)] = sig
        return blk

    def reserve(self, n: int, h: int, w: int, device=None) -> None:
        """Pre-allocate the native block's workspace for up to (n, h, w)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        self.native_block(dev).reserve(n, h, w)

    def debug_fill(self, byte: int, device=None) -> None:
        """Set the native block's workspace to ``byte`` (unet_block_debug_fill; tests of history independence)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        with torch.cuda.device(dev):
            self.native_block(dev).debug_fill(byte, torch.cuda.current_stream(dev).cuda_stream)

    def close(self):
        for b in self._blocks.values():
            b.close()
        self._blocks.clear()
        self._packed_sig.clear()


class UNet(_Tracked, nn.Module):
    """unet_model.UNet(n_channels=3, n_classes=3) with an MI355X forward.

    compute_dtype: "fp32" (default; fp32 storage, every product as three bf16 terms per operand
    on the bf16 MFMA with fp32 accumulation -- fp32 accuracy, not bitwise fp32 products),
    "fp32_exact" (fp32 storage with true fp32 products on the fp32 MFMA, reference semantics), "bf16" or
    "fp16" (16-bit activations/weights, fp32 accumulation, fp32 head), or "mixed" (bf16 at
    resolution levels 2-4, fp16 at the full-resolution levels 0-1; the benchmark's plan, chosen
    so the masks meet IoU >= 0.999 against fp32).  Default from the UNET_MI355X_DTYPE
    environment variable.

    Non-finite input pixels: NaN propagates as through the reference in every plan.  +-inf does so
    by kind and sign in "fp32_exact" and the 16-bit plans (a +inf logit gives a True mask; a weight
    that rounds to zero in the 16-bit type makes inf * 0 = NaN of it).  The
    three-term "fp32" plan evaluates inf * w as inf * w_hi + inf * w_mid + inf * w_lo, which is
    inf - inf or inf * 0, so there every logit an infinity reaches is NaN: the set of non-finite
    logits is the reference's, each of them gives a False mask.

    The forward is inference only: it folds eval-mode BatchNorm and builds no autograd graph, so calling it
    in training mode with grad enabled raises (use the reference module to train the network).  The one layer
    that does train here is the output head: ``features`` returns the 64-channel map ``out_conv`` reads,
    ``head`` applies ``out_conv`` to it with autograd (``head.head_conv``, native forward and backward), and
    ``fit_head`` fits ``out_conv`` on labelled pages with the backbone frozen -- a linear probe.  What training
    keeps a checkpoint by -- the reference's InvoiceLoss on labelled pages -- is computed on the device by
    ``score`` / ``score_logits`` (with mask IoU and a threshold sweep), see ``metrics.Score``; the same loss as a
    device scalar with its gradient at the logits by ``loss_grad``, see ``metrics.InvoiceLoss``.
    """

    def __init__(self, n_channels: int = 3, n_classes: int = 3, compute_dtype: str | None = None,
                 thresholds=(0.25, 0.40, 0.30)):
        super().__init__()
        self.n_channels = n_channels
        self.n_classes = n_classes
        self.compute_dtype = compute_dtype or DEFAULT_DTYPE
        if self.compute_dtype not in native.DTYPES:
            raise ValueError(f"compute_dtype must be one of {sorted(native.DTYPES)}")
        self.thresholds = tuple(float(t) for t in thresholds)

        cd = self.compute_dtype   # the blocks' own forward (called stand-alone) uses the model's precision plan
        self.down1 = DoubleConv(n_channels, 64, cd)
        self.down2 = DoubleConv(64, 128, cd)
        self.down3 = DoubleConv(128, 256, cd)
        self.down4 = DoubleConv(256, 512, cd)
        self.pool = MaxPool2d(2)
        self.bottleneck = DoubleConv(512, 1024, cd)
        self.up4 = ConvTranspose2d(1024, 512, 2, stride=2)
        self.conv4 = DoubleConv(1024, 512, cd)
        self.up3 = ConvTranspose2d(512, 256, 2, stride=2)
        self.conv3 = DoubleConv(512, 256, cd)
        self.up2 = ConvTranspose2d(256, 128, 2, stride=2)
        self.conv2 = DoubleConv(256, 128, cd)
        self.up1 = ConvTranspose2d(128, 64, 2, stride=2)
        self.conv1 = DoubleConv(128, 64, cd)
        self.out_conv = Conv2d(64, n_classes, kernel_size=1)
        nn.init.constant_(self.out_conv.bias, -4)  # unet_model.py:52-53

        self._handles: dict[int, native.Handle] = {}
        self._packed_sig: dict[int, tuple] = {}
        self._lock = threading.Lock()
        self._sig_tensors = None
        self._sig_epoch = -1
        self._sig_tracked = False
        # set by the drop-in's private model cache (inference._cached_model), whose model nobody can
        # reach to modify: once packed, its handle skips the per-call weight signature (136 tensors,
        # ~40-50 us of host time on the batch-1 call path)
        self._frozen = False

    # ------------------------------------------------------------------ native plumbing
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """nn.Module.load_state_dict; every packed handle re-packs at its next use (also when frozen)."""
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        with self._lock:
            self._packed_sig.clear()
        _bump_epoch()
        return out

    def _signature(self):
        """(data_ptr, _version) of every state_dict tensor: changes on any in-place update
        (load_state_dict, optimizer steps, ``with no_grad(): p.add_``), on .to() / .data
        replacement and on re-registration (the cached tensor list is rebuilt then)."""
        if self._sig_epoch != _TREE_EPOCH[0] or self._sig_tensors is None or not self._sig_tracked:
            self._sig_tracked = all(isinstance(m, _Tracked) for m in self.modules())
            self._sig_tensors = list(self.state_dict(keep_vars=True).values())
            self._sig_epoch = _TREE_EPOCH[0]
        return tuple((t.data_ptr(), t._version) for t in self._sig_tensors)

    def native_handle(self, device: torch.device) -> native.Handle:
        """The packed native handle for ``device`` (re-packs if any parameter changed)."""
        if device.type != "cuda":
            raise RuntimeError("unet_mi355x: UNet.forward runs only on a ROCm GPU tensor "
                               f"(got device {device}); there is no CPU fallback")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._lock:
            h = self._handles.get(idx)
            # frozen (the drop-in's private cache): skip the 136-tensor signature while nothing was
            # re-registered or converted anywhere (_TREE_EPOCH) and no load_state_dict ran (it clears
            # _packed_sig); otherwise check it as usual
            if (h is not None and self._frozen and idx in self._packed_sig and self._sig_epoch == _TREE_EPOCH[0]
                    and self._sig_tracked):
                return h
            if h is None:
                h = native.Handle(self.n_channels, self.n_classes, self.compute_dtype, idx,
                                  self.thresholds)
                self._handles[idx] = h
            sig = self._signature()
            if self._packed_sig.get(idx) != sig:
                h.load_weights(self.state_dict())
                self._packed_sig[idx] = sig
        return h

    def _prepack(self, device: torch.device, host_state) -> None:
        """Pack the native handle for ``device`` from ``host_state``: host copies of exactly the module's
        current weights (inference.load_model passes the checkpoint it just assigned), so the pack reads
        no weight back from the device.  The handle then counts as packed for the current weights."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._lock:
            h = self._handles.get(idx)
            if h is None:
                h = native.Handle(self.n_channels, self.n_classes, self.compute_dtype, idx, self.thresholds)
                self._handles[idx] = h
            h.load_weights(host_state)
            self._packed_sig[idx] = self._signature()

    def _check_input(self, x: torch.Tensor):
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise RuntimeError("UNet.forward expects a 4-D NCHW tensor")
        if x.shape[1] != self.n_channels:
            raise RuntimeError(f"expected input with {self.n_channels} channels, got {x.shape[1]}")
        if x.shape[2] % 16 or x.shape[3] % 16:
            # the reference fails inside torch.cat for such sizes
            raise RuntimeError(f"UNet input H and W must be divisible by 16, got {tuple(x.shape[2:])}")

    def _run(self, x: torch.Tensor, want_logits: bool, mask_kind: int, want_boxes: bool = False,
             out_masks: torch.Tensor | None = None, out_boxes: torch.Tensor | None = None):
        self._check_input(x)
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("unet_mi355x.UNet is inference-only (eval BatchNorm folded, no autograd); "
                               "call .eval() or run under torch.no_grad()")
        h = self.native_handle(x.device)
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        n, _, hh, ww = x.shape
        logits = masks = None
        if want_logits:
            logits = torch.empty((n, self.n_classes, hh, ww), device=x.device, dtype=torch.float32)
        if mask_kind != native.MASK_NONE:
            shape = (n, self.n_classes, hh, ww if mask_kind == native.MASK_U8 else ww // 8)
            if out_masks is not None:   # a caller-owned buffer reused across calls (run_unet)
                if (out_masks.dtype != torch.uint8 or tuple(out_masks.shape) != shape or
                        not out_masks.is_contiguous() or out_masks.device != x.device):
                    raise ValueError(f"out masks must be a contiguous uint8 {shape} tensor on {x.device}")
                masks = out_masks
            else:
                masks = torch.empty(shape, device=x.device, dtype=torch.uint8)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        boxes = None
        h.reserve(n, hh, ww)   # grows the workspace if needed (a no-op otherwise); forwards never allocate
        with torch.cuda.device(x.device):
            if want_boxes:
                boxes = out_boxes if out_boxes is not None else \
                    torch.empty((n, self.n_classes, 4), device=x.device, dtype=torch.int32)
                h.forward_boxes(x, logits, masks, mask_kind, boxes, stream)
            else:
                h.forward(x, logits, masks, mask_kind, stream)
        if want_boxes:
            return logits, masks, boxes
        return logits, masks

    # ------------------------------------------------------------------ public API
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """unet_model.py:55-86: NCHW fp32 in -> NCHW fp32 logits [N, n_classes, H, W]."""
        logits, _ = self._run(x, True, native.MASK_NONE)
        return logits

    def forward_masks(self, x: torch.Tensor, packed: bool = False, with_logits: bool = False):
        """Fused sigmoid + per-class threshold (inference.py:72-79) on the device.

        Returns uint8 masks [N, n_classes, H, W] (0/1), or bit-packed [N, n_classes, H, W/8]
        (bit b of byte j = pixel 8j+b) when ``packed``; with ``with_logits`` also the logits.
        """
        logits, masks = self._run(x, with_logits, native.MASK_BITS if packed else native.MASK_U8)
        return (masks, logits) if with_logits else masks

    def forward_boxes(self, x: torch.Tensor, masks: str | None = None, out=None):
        """Fused masks + per-(image, field) bounding boxes on the device (inference.py:72-90).

        Returns int32 boxes [N, n_classes, 4] = (x_min, y_min, x_max, y_max) in mask pixels,
        inclusive, (-1, -1, -1, -1) for an empty mask -- the np.where -> min/max of run_unet.
        ``masks`` = None (boxes only), "u8" or "bits": also return that mask tensor first.
        ``out`` = (masks tensor or None, boxes tensor): caller-owned device buffers to fill.
        """
        kind = {None: native.MASK_NONE, "u8": native.MASK_U8, "bits": native.MASK_BITS}[masks]
        om, ob = out if out is not None else (None, None)
        _, m, boxes = self._run(x, False, kind, want_boxes=True, out_masks=om, out_boxes=ob)
        return boxes if masks is None else (m, boxes)

    def score_logits(self, logits: torch.Tensor, target: torch.Tensor, sweep=None):
        """Score logits [N, n_classes, H, W] (e.g. ``model(x)``) against ground-truth masks on the device
        (unet_score): ``target`` is a device tensor, fp32 NCHW with values in [0, 1] (what dataset.py:33-34
        hands the loss) or uint8 NHWC read as v / 255 (the .npy mask files as stored).  Returns a
        ``metrics.Score``: the reference's InvoiceLoss / Dice / focal means (train.py:18-59), per-field IoU at
        the model's thresholds and, with ``sweep`` = up to 64 ascending probabilities, IoU at each of them.
        Only 64 bytes per (image, field) (and the sweep histogram) are copied to the host; that copy
        synchronises."""
        from .metrics import Score
        if not isinstance(logits, torch.Tensor) or logits.dim() != 4 or logits.shape[1] != self.n_classes:
            raise RuntimeError(f"score_logits expects logits [N, {self.n_classes}, H, W]")
        h = self.native_handle(logits.device)
        logits = logits.detach()
        if logits.dtype != torch.float32 or not logits.is_contiguous():
            logits = logits.to(torch.float32).contiguous()
        target = target.detach().contiguous()
        probs = None if sweep is None else [float(p) for p in sweep]
        with torch.cuda.device(logits.device):
            entries, hist = h.score(logits, target, torch.cuda.current_stream(logits.device).cuda_stream,
                                    sweep=probs)
        return Score(entries.cpu().numpy(), None if hist is None else hist.cpu().numpy(), probs)

    def score(self, x: torch.Tensor, target: torch.Tensor, sweep=None):
        """Forward + ``score_logits`` on one stream: the logits never leave the device."""
        logits, _ = self._run(x, True, native.MASK_NONE)
        return self.score_logits(logits, target, sweep)

    def loss_grad(self, x: torch.Tensor, target: torch.Tensor, criterion=None):
        """Forward + InvoiceLoss + its gradient at the logits on one stream (unet_loss_grad), the companion of
        ``score``: returns (loss, grad_logits), a 0-dim fp32 device tensor and fp32 [N, n_classes, H, W].
        ``criterion``: a ``metrics.InvoiceLoss`` whose weights to use (default: the reference's).  The forward
        itself stays inference-only; the gradient is the first operator of a backward pass, not the whole of it."""
        from .metrics import InvoiceLoss
        crit = criterion if criterion is not None else InvoiceLoss()
        if not isinstance(crit, InvoiceLoss):
            raise TypeError("criterion must be a unet_mi355x.metrics.InvoiceLoss")
        logits, _ = self._run(x, True, native.MASK_NONE)
        return crit.loss_and_grad(logits, target, handle=self.native_handle(logits.device))

    # ------------------------------------------------------------------ the output head on frozen features
    def features(self, x: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """The 64-channel map ``out_conv`` reads (conv1's output, unet_model.py:83), fp32 [N, 64, H, W].
        ``dtype``: ``torch.float16`` or ``torch.bfloat16`` return exactly ``features(x).to(dtype)`` (round to nearest
        even; fp16 overflows to inf above 65504), the storage of a 16-bit feature cache (``fit_head``).

        The fused forward never stores it (conv1.3 and the head are one launch), so it is rebuilt from what
        the forward does store: ``conv1(cat(u1, c1))`` on the stand-alone DoubleConv, in the model's precision
        plan and with eval BatchNorm whatever the module's mode -- one forward plus one conv1 block per call,
        which a frozen backbone pays once per page.  The handle is held from the forward to the fetches, so
        another thread's forward cannot replace the intermediates in between."""
        if dtype not in _FEATURE_DTYPES.values():
            raise ValueError("features: dtype must be torch.float32, torch.float16 or torch.bfloat16")
        self._check_input(x)
        if x.device.type != "cuda":
            raise RuntimeError("unet_mi355x: UNet.features runs only on a ROCm GPU tensor "
                               f"(got device {x.device}); there is no CPU fallback")
        n, _, hh, ww = x.shape
        h = self.native_handle(x.device)
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        logits = torch.empty((n, self.n_classes, hh, ww), device=x.device, dtype=torch.float32)
        cat = torch.empty((2, n * 64 * hh * ww), device=x.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device), h.lock:   # the handle's (re-entrant) lock, forward to last fetch
            h.reserve(n, hh, ww)
            h.forward(x, logits, None, native.MASK_NONE, stream)
            for i, name in enumerate(("u1", "c1")):
                if h.debug_fetch(name, stream) != cat.shape[1]:
                    raise RuntimeError(f"unet_mi355x: intermediate {name} is not [N, 64, H, W]")
                h.debug_fetch_into(name, cat[i], stream)
        u1c1 = torch.cat([cat[0].view(n, 64, hh, ww), cat[1].view(n, 64, hh, ww)], 1)
        with torch.no_grad():
            feat = self.conv1(u1c1)
        return feat if dtype == torch.float32 else feat.to(dtype)

    def head(self, feat: torch.Tensor) -> torch.Tensor:
        """``out_conv`` on a stored feature map (``features``' output): fp32 logits [N, n_classes, H, W], with
        autograd to ``out_conv.weight`` / ``out_conv.bias`` (and to ``feat`` if it asks) -- ``head.head_conv``."""
        from .head import head_conv
        return head_conv(feat, self.out_conv.weight, self.out_conv.bias)

    def feature_cache(self, x: torch.Tensor, batch: int = 4, feature_dtype: str = "fp32") -> torch.Tensor:
        """The feature cache ``fit_head`` trains on, built once: ``features`` of all pages of ``x``
        [P, n_channels, H, W], computed in chunks of ``batch`` and kept on the device as [P, 64, H, W] in
        ``feature_dtype`` (``"fp32"``, or ``"fp16"`` / ``"bf16"``: each chunk's fp32 features rounded to nearest even
        as they are stored).  RuntimeError if the cache does not fit the device's free memory, or if a 16-bit cache
        holds a non-finite value (a feature above 65504 stored as fp16, or a NaN / inf from the backbone).  What
        ``score_features`` and ``head.head_score`` read."""
        if feature_dtype not in _FEATURE_DTYPES:
            raise ValueError(f"feature_cache: feature_dtype must be one of {sorted(_FEATURE_DTYPES)}, "
                             f"got {feature_dtype!r}")
        fdt = _FEATURE_DTYPES[feature_dtype]
        self._check_input(x)
        if x.device.type != "cuda":
            raise RuntimeError("unet_mi355x: feature_cache runs only on a ROCm GPU tensor "
                               f"(got device {x.device}); there is no CPU fallback")
        if batch < 1:
            raise ValueError("batch must be >= 1")
        pages, _, hh, ww = x.shape
        need = pages * 64 * hh * ww * torch.empty((), dtype=fdt).element_size()
        with torch.cuda.device(x.device):
            free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
        if need > free:
            raise RuntimeError(f"fit_head: the feature cache of {pages} pages of {hh}x{ww} needs {need / 2**30:.2f} "
                               f"GiB, {free / 2**30:.2f} GiB are free on {x.device}; fit on fewer pages at a time")
        feats = torch.empty((pages, 64, hh, ww), device=x.device, dtype=fdt)
        for lo in range(0, pages, batch):   # the fp32 transient is one chunk; the copy rounds to nearest even
            feats[lo:lo + batch] = self.features(x[lo:lo + batch])
        # one reduction over the finished cache, read once; the fp32 cache is taken as it comes
        if fdt != torch.float32 and not bool(torch.isfinite(feats).all()):
            raise RuntimeError(f"fit_head: the {feature_dtype} feature cache holds non-finite values (a feature beyond "
                               "fp16's 65504, or a NaN / inf from the backbone); use feature_dtype=\"bf16\" (fp32's "
                               "range) or \"fp32\"")
        return feats

    def _head_thresholds(self):
        """The model's thresholds for its n_classes fields, padded as the native handle pads them (0.5)."""
        return (list(self.thresholds) + [0.5] * 4)[:self.n_classes]

    def score_features(self, feats: torch.Tensor, target: torch.Tensor, pages=None, sweep=None):
        """Score ``out_conv`` on pages of a feature cache (``feature_cache``'s output, [P, 64, H, W]) against their
        masks ``target`` (fp32 [P, C, H, W] or uint8 [P, H, W, C]) at the model's thresholds: ``head.head_score``
        with ``out_conv``'s parameters -- what ``score`` computes for those pages, without running the backbone
        again, without storing logits and without gathering ``pages`` (None: all, in order) out of the cache.
        Returns a ``metrics.Score``, one entry per listed page."""
        from .head import head_score
        return head_score(feats, self.out_conv.weight, self.out_conv.bias, target, pages=pages,
                          thresholds=self._head_thresholds(), sweep=sweep)

    def fit_head(self, x: torch.Tensor, target: torch.Tensor, epochs: int = 50, batch: int = 4, lr: float = 1e-3,
                 weight_decay: float = 1e-4, criterion=None, shuffle_seed: int | None = None,
                 feature_dtype: str = "fp32", fused: bool = False, val_pages=None, keep_best: bool = False,
                 sweep=None, report: dict | None = None) -> list:
        """Fit ``out_conv`` alone on labelled pages, the backbone frozen: a linear probe on frozen features
        (64 C + C parameters), not train.py's training -- no other parameter moves, BatchNorm runs in eval mode
        and its statistics stay.  The loop is train.py:119-160 restricted to the head: ``metrics.InvoiceLoss``,
        AdamW on the two parameters, CosineAnnealingWarmRestarts(T_0=10, T_mult=2) stepped per epoch.

        x: device pages [P, n_channels, H, W]; target: device fp32 [P, C, H, W] in [0, 1] or uint8 [P, H, W, C]
        (the .npy masks as stored).  The features of all pages are computed once, in chunks of ``batch``, and kept
        on the device (``feature_cache``: P x 64 x H x W in ``feature_dtype``; RuntimeError if that does not fit).
        ``feature_dtype``:
        ``"fp32"``, or ``"fp16"`` / ``"bf16"`` for a cache of half the size and half the bytes per step: each chunk's
        fp32 features are rounded to nearest even as they are stored, and the head kernels read the 16-bit cache
        directly (bitwise the fit on the rounded features held as fp32; DESIGN.md section 11 has what the rounding
        costs).  A non-finite value in a 16-bit cache -- a feature above 65504 stored as fp16, or a NaN from the
        backbone -- raises RuntimeError before the first step.  Batches are consecutive pages, the
        last one possibly short, reshuffled every epoch with ``shuffle_seed`` (None: never).  Returns the
        per-epoch mean of the batch losses; the losses are summed on the device and read once per epoch.  The
        module's train / eval mode is left as found.  The next fused forward uses the new head (the weight
        signature re-packs the handle).

        ``fused``: run every step as one native call (``head.HeadFit``, unet_head_step: logits, loss, gradient and
        AdamW from one pass over the batch's features) in place of head_conv + criterion +
        torch's AdamW.  No logits are stored and a shuffled batch is not gathered: the shuffled order goes to the
        kernel as page indices.  The learning rate of each epoch is read from torch's own
        CosineAnnealingWarmRestarts, stepped on a stand-in optimizer.  The losses agree with the unfused loop within
        the trajectory bar of the tests, not bitwise (the gradient is summed in another order, AdamW runs in fp64).

        Validation, the other half of train.py:129-160.  ``val_pages``: distinct page
        indices into ``x``, held out: training runs on the other pages in ascending order (reshuffled per epoch as
        ``train_idx[randperm(len(train_idx))]``), and after every epoch the held-out pages are scored from the cache
        in one native call (unet_head_score) at the model's thresholds.  The entries and the head of every epoch
        stay on the device and are read once after the last epoch: validation adds no host synchronisation.
        ``keep_best``: leave in ``out_conv`` the head of the epoch with the lowest validation ``Score.loss()`` (the
        criterion's weights), the first on ties, instead of the last epoch's.  ``sweep``: ascending probabilities for
        one final sweep of the held-out pages with the head that is kept.  ``report``: a dict to fill with
        ``val_loss`` (list of floats), ``val_iou`` ([epochs][C] pooled IoU), ``best_epoch``, ``heads`` (the
        [epochs][65 C] array: weight then bias) and, with ``sweep``, ``thresholds`` (``Score.best_thresholds()``).
        ``keep_best`` and ``sweep`` need ``val_pages``.  Without ``val_pages`` the fit is what it was."""
        import numpy as np
        from .head import HeadFit, _handle, head_conv
        from .metrics import InvoiceLoss, Score
        crit = criterion if criterion is not None else InvoiceLoss()
        if not isinstance(crit, InvoiceLoss):
            raise TypeError("criterion must be a unet_mi355x.metrics.InvoiceLoss")
        if not isinstance(x, torch.Tensor) or not isinstance(target, torch.Tensor):
            raise TypeError("fit_head expects device tensors")
        if feature_dtype not in _FEATURE_DTYPES:
            raise ValueError(f"fit_head: feature_dtype must be one of {sorted(_FEATURE_DTYPES)}, "
                             f"got {feature_dtype!r}")
        val = train = None
        if val_pages is not None:   # host lists, checked before any device work
            val = [int(i) for i in (val_pages.tolist() if isinstance(val_pages, torch.Tensor) else val_pages)]
            total = x.shape[0] if x.dim() else 0
            if not val:
                raise ValueError("fit_head: val_pages is empty (None: no validation)")
            if len(set(val)) != len(val):
                raise ValueError("fit_head: val_pages repeats a page")
            if min(val) < 0 or max(val) >= total:
                raise IndexError(f"fit_head: val_pages must be indices in [0, {total})")
            held = set(val)
            train = [i for i in range(total) if i not in held]
            if not train:
                raise ValueError("fit_head: val_pages leaves no page for training")
        elif keep_best or sweep is not None:
            raise ValueError("fit_head: keep_best and sweep need val_pages")
        if report is not None and not isinstance(report, dict):
            raise TypeError("fit_head: report must be a dict")
        if x.device.type != "cuda" or target.device != x.device:
            raise RuntimeError("unet_mi355x: fit_head runs only on ROCm GPU tensors "
                               f"(got x on {x.device}, target on {target.device}); there is no CPU fallback")
        self._check_input(x)
        if epochs < 1 or batch < 1:
            raise ValueError("epochs and batch must be >= 1")
        pages, _, hh, ww = x.shape
        c = self.n_classes
        want = (pages, hh, ww, c) if target.dtype == torch.uint8 else (pages, c, hh, ww)
        if target.dtype not in (torch.uint8, torch.float32) or tuple(target.shape) != want:
            raise ValueError(f"target must be float32 {(pages, c, hh, ww)} or uint8 {(pages, hh, ww, c)}")
        weight, bias = self.out_conv.weight, self.out_conv.bias
        if not (weight.requires_grad and bias.requires_grad):
            raise RuntimeError("fit_head: out_conv's parameters must require grad")
        feats = self.feature_cache(x, batch, feature_dtype)
        target = target.detach().contiguous()
        gen = None if shuffle_seed is None else torch.Generator().manual_seed(int(shuffle_seed))
        n_train = pages if train is None else len(train)
        train_host = None if train is None else torch.tensor(train, dtype=torch.int64)
        steps = (n_train + batch - 1) // batch

        def shuffled():   # this epoch's pages on the host: randperm, through the training pages when some are held out
            perm = torch.randperm(n_train, generator=gen)
            return perm if train_host is None else train_host[perm]

        validate = None
        if val is not None:
            vh = _handle(x.device)
            val_dev = torch.tensor(val, dtype=torch.int32).to(x.device)
            val_entries = torch.empty((epochs, len(val), c, native.SCORE_DTYPE.itemsize), device=x.device,
                                      dtype=torch.uint8)
            heads = torch.empty((epochs, 65 * c), device=x.device, dtype=torch.float32)
            thr = self._head_thresholds()
            with torch.cuda.device(x.device):
                vh.head_score_reserve(len(val), hh, ww, 0 if sweep is None else len(sweep))

            def validate(ep):   # one native call and two small copies on the stream; nothing is read here
                with torch.cuda.device(x.device):
                    vh.head_score(feats, target, weight.detach(), bias.detach(),
                                  torch.cuda.current_stream(x.device).cuda_stream, pages=val_dev, thresholds=thr,
                                  entries=val_entries[ep])
                heads[ep, :64 * c].copy_(weight.detach().reshape(-1))
                heads[ep, 64 * c:].copy_(bias.detach())

        losses = []
        if fused:
            fit = HeadFit(weight, bias, lr, weight_decay=weight_decay, criterion=crit)
            # the schedule is torch's by construction: its scheduler on an optimizer that never steps a parameter
            stand_in = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
            sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(stand_in, T_0=10, T_mult=2)
            in_order = (torch.arange(pages, dtype=torch.int32, device=x.device) if train_host is None
                        else train_host.to(x.device, torch.int32))
            for ep in range(epochs):
                order = in_order if gen is None else shuffled().to(x.device, torch.int32)
                total = torch.zeros((), device=x.device, dtype=torch.float32)
                for lo in range(0, n_train, batch):
                    total += fit.step(feats, target, order[lo:lo + batch], lr=stand_in.param_groups[0]["lr"])
                if validate is not None:
                    validate(ep)
                losses.append(float(total.item()) / steps)
                stand_in.step()
                sched.step()
        else:
            opt = torch.optim.AdamW([weight, bias], lr=lr, weight_decay=weight_decay)
            sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2)
            in_order = None if train_host is None else train_host.to(x.device)
            with torch.enable_grad():
                for ep in range(epochs):
                    order = in_order if gen is None else shuffled().to(x.device)
                    total = torch.zeros((), device=x.device, dtype=torch.float32)
                    for lo in range(0, n_train, batch):
                        if order is None:
                            f, t = feats[lo:lo + batch], target[lo:lo + batch]
                        else:
                            f, t = feats[order[lo:lo + batch]], target[order[lo:lo + batch]]
                        loss = crit(head_conv(f, weight, bias), t)
                        opt.zero_grad()
                        loss.backward()
                        opt.step()
                        total += loss.detach()
                    if validate is not None:
                        validate(ep)
                    losses.append(float(total.item()) / steps)
                    sched.step()
        if val is None:
            return losses
        # the one read of the validation record
        entries, heads_host = val_entries.cpu().numpy(), heads.cpu().numpy()
        dw, fw, alpha, smooth = crit.weights
        scores = [Score(entries[ep]) for ep in range(epochs)]
        val_loss = [s.loss(dw, fw, None, smooth, alpha) for s in scores]
        finite = [v for v in val_loss if v == v]   # a NaN loss never wins; all NaN: the last epoch stays
        best = val_loss.index(min(finite)) if finite else epochs - 1
        if keep_best and best != epochs - 1:
            with torch.no_grad():
                weight.copy_(heads[best, :64 * c].view_as(weight))
                bias.copy_(heads[best, 64 * c:])
        if report is not None:
            report["val_loss"] = val_loss
            report["val_iou"] = np.stack([s.pooled_iou() for s in scores])
            report["best_epoch"] = best
            report["heads"] = heads_host
            if sweep is not None:
                report["thresholds"] = self.score_features(feats, target, pages=val, sweep=sweep).best_thresholds()
        return losses

    def preprocess(self, img: torch.Tensor, size: int = 512, out: torch.Tensor | None = None) -> torch.Tensor:
        """inference.py:62-64 + :30-44 on the device: a photo as uint8 [H, W, 3] (RGB) or
        [H, W] / [H, W, 1] (L) device tensor -> fp32 [1, 3, size, size] network input, with
        Pillow's default BICUBIC resize reproduced bit-exactly (csrc/unet_preprocess.hip).
        ``out`` (optional, fp32 [3, size, size] contiguous, e.g. a slot of a batch) is filled
        in place.

        The passes run horizontal first, then vertical, as Pillow's resampler runs one resize.  The one
        exception to bit-exactness: a newer Pillow's ``Image.resize`` (12.2; not the reference's 10.2) runs the
        vertical pass first on a photo with H > 100 * W that it makes less tall, and its bytes differ there;
        ``run_unet`` sends such photos down the host path (``inference.resizes_on_host``)."""
        if img.dim() == 2:
            img = img.unsqueeze(-1)
        if img.device.type != "cuda":
            raise RuntimeError("unet_mi355x: preprocess runs on a ROCm GPU tensor; there is no CPU fallback")
        img = img.contiguous()
        h = self.native_handle(img.device)
        dst = out if out is not None else torch.empty((3, size, size), device=img.device, dtype=torch.float32)
        with torch.cuda.device(img.device):
            h.preprocess(img, dst, torch.cuda.current_stream(img.device).cuda_stream)
        return dst.unsqueeze(0) if out is None else out

    def reserve(self, n: int, h: int, w: int, device=None) -> None:
        """Pre-allocate the native workspace (so forwards do not allocate)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        self.native_handle(dev).reserve(n, h, w)

    def intermediate(self, name: str, device=None) -> torch.Tensor:
        """Intermediate activation of the last forward as fp32 NCHW (debug / per-layer parity)."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        h = self.native_handle(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        numel = h.debug_fetch(name, stream)
        out = torch.empty(numel, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            h.debug_fetch_into(name, out, stream)
        return out

    def debug_fill(self, byte: int, device=None) -> None:
        """Set every scratch allocation of the native handle to ``byte`` (unet_debug_fill; tests of history
        independence).  Not between a forward and ``intermediate``, which reads the workspace."""
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        with torch.cuda.device(dev):
            self.native_handle(dev).debug_fill(byte, torch.cuda.current_stream(dev).cuda_stream)

    def close(self):
        for h in self._handles.values():
            h.close()
        self._handles.clear()
        self._packed_sig.clear()
        for m in self.modules():
            if isinstance(m, DoubleConv):
                m.close()
