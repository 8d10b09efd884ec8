#!/usr/bin/env python3
"""Time the head score (unet_head_score, HIP events) against the path it replaces, in one process with the variants
alternating.

    python tools/head_score_time.py [--n 256] [--size 512] [--subset 64] [--reps 3] [--rounds 7] [--pages 64]
                                    [--held 16] [--out FILE.json]

(a) scoring at the headline batch, n x 64 x size x size features with C = 3 and uint8 masks, on an fp32 and an fp16
    cache, without a sweep (K = 0) and with the 19-point sweep: ``unet_head_score`` on all pages in order against
    unet_head_forward_typed + unet_score, and ``unet_head_score`` on a shuffled subset of ``subset`` pages, given as
    page indices, against the same two calls behind the gather ``feats[idx]``, ``target[idx]``.
(b) what validation adds to ``UNet.fit_head``'s loop (fused steps, batch 4): ``pages`` pages of size x size with the
    last ``held`` held out and scored after every epoch, against the same loop on the other pages alone; per epoch,
    the time of a fit of 21 epochs less that of a fit of 1 (the feature cache is built in both).

Every variant is warmed first; then ``rounds`` rounds, each timing every variant in turn.  A figure is the median
over the rounds with min .. max beside it; a fused row carries its median as a fraction of the row it replaces
(``vs``) and whether the two min .. max ranges are disjoint (``disjoint``).  Bytes moved, from the shapes, are
carried for part (a).  Nothing is fixed in advance.  Needs a GPU with about 40 GB free at the default size.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))

SWEEP = [0.05 * i for i in range(1, 20)]


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


def score_rows(torch, native, n, s, subset, rounds, reps):
    dev, c = "cuda:0", 3
    gen = torch.Generator(device=dev).manual_seed(0)
    caches = {"fp32": torch.empty((n, 64, s, s), device=dev)}
    for i in range(n):   # page by page: no second 17 GB temporary
        caches["fp32"][i] = torch.relu(torch.randn((64, s, s), device=dev, generator=gen)) * 2.5
    caches["fp16"] = torch.empty((n, 64, s, s), device=dev, dtype=torch.float16)
    for i in range(n):
        caches["fp16"][i] = caches["fp32"][i]
    target = (torch.rand((n, s, s, c), device=dev, generator=gen) < 0.2).to(torch.uint8) * 255
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:subset].to(dev)
    idx32 = idx.to(torch.int32)
    h = native.Handle(3, c, "fp32", 0)
    h.score_reserve(n, s, s, len(SWEEP))
    h.head_score_reserve(n, s, s, len(SWEEP))
    st = torch.cuda.current_stream(dev).cuda_stream
    logits = torch.empty((n, c, s, s), device=dev)
    w = ((torch.rand((c, 64), device=dev, generator=gen) - 0.5) * 0.25).contiguous()
    b = torch.full((c,), -4.0, device=dev)

    def two_calls(f, t, sweep):
        h.score(h.head_forward(f, w, b, st, logits=logits[:f.shape[0]]), t, st, sweep=sweep)

    def fused(f, pages, sweep):
        h.head_score(f, target, w, b, st, pages=pages, sweep=sweep)

    variants, nbytes = [], {}
    for name, f in caches.items():
        es = f.element_size()
        for k, sweep in ((0, None), (len(SWEEP), SWEEP)):
            tag = f"{name} cache, K = {k}"
            variants += [
                (f"head score, in order, {tag}", lambda f=f, sweep=sweep: fused(f, None, sweep)),
                (f"forward + score, in order, {tag}", lambda f=f, sweep=sweep: two_calls(f, target, sweep)),
                (f"head score, {subset} shuffled pages, {tag}", lambda f=f, sweep=sweep: fused(f, idx32, sweep)),
                (f"gather + forward + score, {subset} shuffled pages, {tag}",
                 lambda f=f, sweep=sweep: two_calls(f[idx], target[idx], sweep)),
            ]
            for j, pages in ((-4, n), (-2, subset)):
                px = pages * s * s
                feat_b, logit_b = px * 64 * es, px * c * 4
                nbytes[variants[j][0]] = feat_b + px * c
                # forward: feat in, logits out; score: logits and masks in; the gather reads and writes both
                nbytes[variants[j + 1][0]] = feat_b + 2 * logit_b + px * c + (0 if pages == n else 2 * (feat_b + px * c))
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


def loop_rows(torch, pages, held, s, rounds):
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
    train = pages - held
    val = list(range(train, pages))

    def fit(validate, e):
        model.out_conv.load_state_dict(head0)   # every fit starts from the same head
        if validate:
            model.fit_head(x, t, epochs=e, batch=batch, lr=1e-3, shuffle_seed=1, fused=True, val_pages=val, report={})
        else:
            model.fit_head(x[:train], t[:train], epochs=e, batch=batch, lr=1e-3, shuffle_seed=1, fused=True)

    variants = [(f"validate={v}, {e} epochs", lambda v=v, e=e: fit(v, e)) for e in epochs for v in (True, False)]
    for _, fn in variants[:2]:
        fn()
    torch.cuda.synchronize()
    per_epoch = {True: [], False: []}
    for _ in range(rounds):
        ms = {}
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name] = e0.elapsed_time(e1)
        for v in (True, False):
            per_epoch[v].append((ms[f"validate={v}, {epochs[1]} epochs"] - ms[f"validate={v}, {epochs[0]} epochs"])
                                / (epochs[1] - epochs[0]))
    rows = [row(f"fit_head loop per epoch, batch {batch}, {train} training pages, "
                + (f"{held} held out and scored" if v else "no validation"), sorted(per_epoch[v])) for v in (True, False)]
    versus(rows[0], rows[1])
    rows[0]["added_ms"] = round(rows[0]["ms"] - rows[1]["ms"], 4)
    model.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--held", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from unet_mi355x import native
    if not torch.cuda.is_available():
        raise SystemExit("head_score_time: needs a ROCm GPU (there is no CPU timing)")
    rows = []
    for r in score_rows(torch, native, a.n, a.size, a.subset, a.rounds, a.reps):
        rows.append(r)
        print(json.dumps(r), flush=True)
    torch.cuda.empty_cache()
    for r in loop_rows(torch, a.pages, a.held, a.size, a.rounds):
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), n=a.n, classes=3, size=a.size, subset=a.subset, reps=a.reps,
               rounds=a.rounds, pages=a.pages, held=a.held, results=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
