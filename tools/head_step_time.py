#!/usr/bin/env python3
"""Time the fused head training step (unet_head_step, HIP events) against the sequence it replaces, in one process
with the variants alternating.

    python tools/head_step_time.py [--n 256] [--size 512] [--reps 3] [--rounds 7] [--pages 64] [--out FILE.json]

(a) one step at the headline batch, n x 64 x size x size features with C = 3 and uint8 masks, on an fp32 and an fp16
    cache: ``unet_head_step`` with AdamW against unet_head_forward_typed + unet_loss_grad + unet_head_backward_typed
    + torch.optim.AdamW, and against the same sequence behind the gather of a shuffled batch
    (``feats[order]``, ``target[order]``), where the fused step takes the order as page indices.
(b) ``UNet.fit_head``'s own loop at batch 4 on ``pages`` pages of size x size, ``fused=True`` against
    ``fused=False``: the time of a fit of 21 epochs less that of a fit of 1 (the feature cache is built in both), per
    step.

Every variant is warmed first; then ``rounds`` rounds, each timing every variant in turn.  A figure is the median
over the rounds with min .. max beside it; a fused row carries its median as a fraction of the row it replaces
(``vs``) and whether the two min .. max ranges are disjoint (``disjoint``).  Bytes moved, from the shapes, are
carried for part (a).  Nothing is fixed in advance.  Needs a GPU with about 70 GB free at the default size.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))


def timed(torch, variants, rounds, reps):
    """{name: sorted ms per call}: every variant warmed, then ``rounds`` rounds over all of them in turn"""
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    return {k: sorted(v) for k, v in ms.items()}


def row(name, m, **extra):
    r = dict(variant=name, ms=round(m[len(m) // 2], 4), ms_min=round(m[0], 4), ms_max=round(m[-1], 4))
    r.update(extra)
    return r


def versus(r, base):
    r["vs"] = round(r["ms"] / base["ms"], 3)
    r["disjoint"] = bool(r["ms_max"] < base["ms_min"] or base["ms_max"] < r["ms_min"])
    return r


def step_rows(torch, native, n, s, rounds, reps):
    dev, c = "cuda:0", 3
    gen = torch.Generator(device=dev).manual_seed(0)
    caches = {"fp32": torch.empty((n, 64, s, s), device=dev)}
    for i in range(n):   # page by page: no second 17 GB temporary
        caches["fp32"][i] = torch.relu(torch.randn((64, s, s), device=dev, generator=gen)) * 2.5
    caches["fp16"] = torch.empty((n, 64, s, s), device=dev, dtype=torch.float16)
    for i in range(n):
        caches["fp16"][i] = caches["fp32"][i]
    target = (torch.rand((n, s, s, c), device=dev, generator=gen) < 0.2).to(torch.uint8) * 255
    order = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(dev)
    order32 = order.to(torch.int32)
    h = native.Handle(3, c, "fp32", 0)
    h.head_reserve(n, s, s)
    h.loss_reserve(n, s, s)
    h.head_step_reserve(n, s, s)
    st = torch.cuda.current_stream(dev).cuda_stream
    logits, grad = torch.empty((n, c, s, s), device=dev), torch.empty((n, c, s, s), device=dev)
    loss = torch.empty((), device=dev)
    w0 = (torch.rand((c, 64, 1, 1), device=dev, generator=gen) - 0.5) * 0.25
    b0 = torch.full((c,), -4.0, device=dev)

    # the parent's sequence: its own parameters, torch's AdamW on gradients the native backward fills
    wp, bp = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
    wp.grad, bp.grad = torch.zeros_like(wp), torch.zeros_like(bp)
    opt = torch.optim.AdamW([wp, bp], lr=1e-5, weight_decay=1e-4)
    gw, gb = wp.grad.view(c, 64), bp.grad

    def three_calls(f, t):
        h.head_forward(f, wp.detach(), bp.detach(), st, logits=logits)
        h.loss_grad(logits, t, st, loss=loss, grad=grad)
        h.head_backward(f, grad, wp.detach(), st, grad_w=gw, grad_b=gb)
        opt.step()

    # the fused step: its own parameters and moments
    wf, bf = w0.clone(), b0.clone()
    state = torch.zeros(2 * (64 * c + c), device=dev)
    count = [0]

    def fused(f, pages):
        count[0] += 1
        h.head_step(f, target, wf, bf, st, pages=pages, opt=(1e-5, 0.9, 0.999, 1e-8, 1e-4, count[0]), state=state,
                    loss=loss)

    px = n * s * s
    variants, nbytes = [], {}
    for name, f in caches.items():
        es = f.element_size()
        variants += [
            (f"fused step, {name} cache", lambda f=f: fused(f, None)),
            (f"three calls + AdamW, {name} cache", lambda f=f: three_calls(f, target)),
            (f"fused step, shuffled pages, {name} cache", lambda f=f: fused(f, order32)),
            (f"gather + three calls + AdamW, {name} cache", lambda f=f: three_calls(f[order], target[order])),
        ]
        feat_b, logit_b = px * 64 * es, px * c * 4
        nbytes[variants[-4][0]] = nbytes[variants[-2][0]] = feat_b + px * c
        # forward: feat in, logits out; loss: logits and masks twice, gradient out; backward: feat and gradient in
        nbytes[variants[-3][0]] = 2 * feat_b + 5 * logit_b + 2 * px * c
        nbytes[variants[-1][0]] = nbytes[variants[-3][0]] + 2 * feat_b + 2 * px * c
    ms = timed(torch, variants, rounds, reps)
    rows = []
    for i, (name, _) in enumerate(variants):
        r = row(name, ms[name], bytes_moved=nbytes[name])
        r["tb_per_s"] = round(nbytes[name] / r["ms"] / 1e9, 3)
        rows.append(r)
        if i % 2:   # the pair (fused, what it replaces) is complete
            versus(rows[-2], rows[-1])
    h.close()
    return rows


def loop_rows(torch, pages, s, rounds):
    import numpy as np
    from unet_mi355x import synthetic as syn
    from unet_mi355x.model import UNet
    dev, batch, epochs = "cuda:0", 4, (1, 21)
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()}
    x = torch.from_numpy(syn.invoice_pages(5, pages, s, s, 3)).to(dev)
    t = torch.from_numpy((syn.invoice_fields(5, pages, s, s) > 0).astype(np.float32)).to(dev)
    model = UNet(3, 3)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    head0 = {k: v.detach().clone() for k, v in model.out_conv.state_dict().items()}

    def fit(fused, e):
        model.out_conv.load_state_dict(head0)   # every fit starts from the same head
        model.fit_head(x, t, epochs=e, batch=batch, lr=1e-3, shuffle_seed=1, fused=fused)

    variants = [(f"fit_head fused={f}, {e} epochs", lambda f=f, e=e: fit(f, e)) for e in epochs for f in (True, False)]
    for _, fn in variants[:2]:
        fn()
    torch.cuda.synchronize()
    steps = (epochs[1] - epochs[0]) * ((pages + batch - 1) // batch)
    per_step = {True: [], False: []}
    for _ in range(rounds):
        ms = {}
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name] = e0.elapsed_time(e1)
        for f in (True, False):
            per_step[f].append((ms[f"fit_head fused={f}, {epochs[1]} epochs"] -
                                ms[f"fit_head fused={f}, {epochs[0]} epochs"]) / steps)
    rows = [row(f"fit_head loop per step, batch {batch}, {pages} pages, fused={f}", sorted(per_step[f]))
            for f in (True, False)]
    versus(rows[0], rows[1])
    model.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from unet_mi355x import native
    if not torch.cuda.is_available():
        raise SystemExit("head_step_time: needs a ROCm GPU (there is no CPU timing)")
    rows = []
    for r in step_rows(torch, native, a.n, a.size, a.rounds, a.reps):
        rows.append(r)
        print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    for r in loop_rows(torch, a.pages, a.size, a.rounds):
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), n=a.n, classes=3, size=a.size, reps=a.reps, rounds=a.rounds,
               pages=a.pages, results=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
