#!/usr/bin/env python3
"""Time the output head's kernels (HIP events) at the headline batch: 256 x 64 x 512 x 512 fp32 features (17 GB),
C = 3 -- unet_head_forward, unet_head_backward without and with grad_feat -- beside the same forward and
grad_w + grad_b on the features rounded to fp16 and to bf16 (unet_head_*_typed, 8.6 GB each) and beside eager torch
on the fp32 tensors (F.conv2d and its autograd backward: what a user runs without them).

    python tools/head_time.py [--n 256] [--size 512] [--reps 5] [--rounds 7] [--out FILE.json]

Every variant is warmed first; then ``rounds`` rounds, each timing every variant in turn (one event pair around
``reps`` back-to-back calls) / reps.  A figure is the median over the rounds, the spread (min .. max) beside it.
Bytes moved, from the shapes: the forward reads feat (64 elements per pixel, 4 or 2 bytes each) and writes C fp32
logits; the parameter backward reads feat and C fp32 gradients; grad_feat reads C gradients and writes 64 fp32
more.  The yardstick is the HBM floor these bytes set, with eager torch beside it; the 16-bit rows also carry their
time as a fraction of the fp32 row of the same call (``vs_fp32``); no ratio is fixed in advance.  Needs a GPU with
about 60 GB free at the default size.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from unet_mi355x import native
    if not torch.cuda.is_available():
        raise SystemExit("head_time: needs a ROCm GPU (there is no CPU timing)")
    dev = "cuda:0"
    n, c, s = a.n, 3, a.size
    gen = torch.Generator(device=dev).manual_seed(0)
    feat = torch.empty((n, 64, s, s), device=dev)
    for i in range(n):   # image by image: no second 17 GB temporary
        feat[i] = torch.relu(torch.randn((64, s, s), device=dev, generator=gen)) * 2.5
    g = torch.randn((n, c, s, s), device=dev, generator=gen) * 1e-3
    w = (torch.rand((c, 64, 1, 1), device=dev, generator=gen) - 0.5) * 0.25
    b = torch.full((c,), -4.0, device=dev)
    h = native.Handle(3, c, "fp32", 0)
    h.head_reserve(n, s, s)
    st = torch.cuda.current_stream(dev).cuda_stream
    logits = torch.empty((n, c, s, s), device=dev)
    gw, gb = torch.empty((c, 64), device=dev), torch.empty((c,), device=dev)
    gf = torch.empty_like(feat)

    wl, bl = w.clone().requires_grad_(), b.clone().requires_grad_()
    out_p = F.conv2d(feat, wl, bl)                      # graph to the parameters only
    fl = feat.requires_grad_()
    out_f = F.conv2d(fl, wl, bl)                        # ... and to the features

    def eager_forward():
        with torch.no_grad():
            F.conv2d(feat, w, b)

    px = n * s * s * 4
    px16 = n * s * s * (64 * 2 + c * 4)   # 16-bit features, fp32 logits / gradients
    f16 = {}
    for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        f16[name] = torch.empty((n, 64, s, s), device=dev, dtype=dt)
        for i in range(n):   # image by image, as above
            f16[name][i] = feat[i]

    def fwd16(f):
        return lambda: h.head_forward(f, w, b, st, logits=logits)

    def bwd16(f):
        return lambda: h.head_backward(f, g, w, st, grad_w=gw, grad_b=gb)

    variants = [
        ("native forward", lambda: h.head_forward(feat, w, b, st, logits=logits), px * (64 + c)),
        ("native forward, fp16 features", fwd16(f16["fp16"]), px16),
        ("native forward, bf16 features", fwd16(f16["bf16"]), px16),
        ("native backward, no grad_feat", lambda: h.head_backward(feat, g, w, st, grad_w=gw, grad_b=gb),
         px * (64 + c)),
        ("native backward, no grad_feat, fp16 features", bwd16(f16["fp16"]), px16),
        ("native backward, no grad_feat, bf16 features", bwd16(f16["bf16"]), px16),
        ("native backward with grad_feat",
         lambda: h.head_backward(feat, g, w, st, want_feat=True, grad_w=gw, grad_b=gb, grad_feat=gf),
         px * (64 + c + c + 64)),
        ("eager F.conv2d forward", eager_forward, px * (64 + c)),
        ("eager autograd backward, no grad_feat",
         lambda: torch.autograd.grad(out_p, [wl, bl], g, retain_graph=True), px * (64 + c)),
        ("eager autograd backward with grad_feat",
         lambda: torch.autograd.grad(out_f, [wl, bl, fl], g, retain_graph=True), px * (64 + c + c + 64)),
    ]
    for _, fn, _ in variants:   # warm-up: code objects, the allocator's blocks, the library's algorithm choice
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in variants]
    for _ in range(a.rounds):
        for i, (_, fn, _) in enumerate(variants):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1) / a.reps)
    rows, medians = [], {}
    for (name, _, nbytes), m in zip(variants, ms):
        m.sort()
        med = medians[name] = m[len(m) // 2]
        rows.append(dict(variant=name, ms=round(med, 4), ms_min=round(m[0], 4), ms_max=round(m[-1], 4),
                         bytes_moved=nbytes, tb_per_s=round(nbytes / med / 1e9, 3)))
        base = name.split(", fp16 features")[0].split(", bf16 features")[0]
        if base != name:   # a 16-bit row: its time against the fp32 row of the same call (listed before it)
            rows[-1]["vs_fp32"] = round(med / medians[base], 3)
        print(json.dumps(rows[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), n=n, classes=c, size=s, reps=a.reps, rounds=a.rounds,
               results=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    h.close()


if __name__ == "__main__":
    main()
