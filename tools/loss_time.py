#!/usr/bin/env python3
"""Time unet_loss_grad (HIP events) at the headline batch: 256 x 3 x 512 x 512 logits, both target forms, beside
unet_score alone (what the gradient pass adds) and eager torch autograd of the same formula on the device (what a
user runs without it).

    python tools/loss_time.py [--n 256] [--size 512] [--reps 20] [--rounds 7] [--out FILE.json]

Each figure is the median over ``rounds`` of (one event pair around ``reps`` back-to-back calls) / reps, after a
warm-up of every variant; the spread (min .. max over the rounds) is printed beside it.  Bytes moved, from the
shapes: the score reads the logits (4 B) and the target (4 B or 1 B) per element; the loss reads both twice (the
sums, then the gradient) and writes 4 B.  The eager line is this tool's own statement of InvoiceLoss
(train.py:18-59) in torch ops, forward + backward on an fp32 target; its bytes are not counted (about ten
element-wise passes and four reductions).  Needs a GPU.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))


def eager_loss(torch, x, t, dw=0.85, fw=0.15, alpha=0.8, smooth=1.0):
    p = torch.sigmoid(x)
    pf, tf = p.flatten(2), t.flatten(2)
    dice = (1 - (2 * (pf * tf).sum(-1) + smooth) / (pf.sum(-1) + tf.sum(-1) + smooth)).mean()
    bce = torch.nn.functional.binary_cross_entropy(p.clamp(1e-7, 1 - 1e-7), t, reduction="none")
    focal = (alpha * (1 - torch.exp(-bce)) ** 2 * bce).mean()
    return dw * dice + fw * focal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from unet_mi355x import native
    if not torch.cuda.is_available():
        raise SystemExit("loss_time: needs a ROCm GPU (there is no CPU timing)")
    dev = "cuda:0"
    n, c, s = a.n, 3, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((n, c, s, s), device=dev, generator=g) * 4.0 - 3.0
    tu8 = torch.where(torch.rand((n, s, s, c), device=dev, generator=g) < 0.1, 255, 0).to(torch.uint8)
    tf = (tu8.to(torch.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
    h = native.Handle(3, c, "mixed", 0)
    h.score_reserve(n, s, s, 0)
    h.loss_reserve(n, s, s)
    st = torch.cuda.current_stream(dev).cuda_stream
    loss = torch.zeros((), device=dev)
    grad = torch.empty_like(logits)
    leaf = logits.clone().requires_grad_()

    def eager():
        leaf.grad = None
        eager_loss(torch, leaf, tf).backward()

    el = logits.numel()
    variants = [
        ("loss_grad u8_nhwc", lambda: h.loss_grad(logits, tu8, st, loss=loss, grad=grad), el * (2 * 5 + 4)),
        ("loss_grad f32_nchw", lambda: h.loss_grad(logits, tf, st, loss=loss, grad=grad), el * (2 * 8 + 4)),
        ("loss only u8_nhwc", lambda: h.loss_grad(logits, tu8, st, loss=loss, want_grad=False), el * 5),
        ("score u8_nhwc", lambda: h.score(logits, tu8, st), el * 5),
        ("score f32_nchw", lambda: h.score(logits, tf, st), el * 8),
        ("eager torch autograd f32_nchw", eager, None),
    ]
    for _, fn, _ in variants:   # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    rows = []
    for name, fn, nbytes in variants:
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        ms.sort()
        med = ms[len(ms) // 2]
        rows.append(dict(variant=name, ms=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                         bytes_moved=nbytes, tb_per_s=None if nbytes is None else round(nbytes / med / 1e9, 3),
                         gelem_per_s=round(el / med / 1e6, 1)))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(n=n, classes=c, size=s, reps=a.reps, rounds=a.rounds, results=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    h.close()


if __name__ == "__main__":
    main()
