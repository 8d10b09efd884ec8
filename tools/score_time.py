#!/usr/bin/env python3
"""Time unet_score alone (HIP events) at the headline batch: 256 x 3 x 512 x 512 logits, with a sweep of
K = 19 candidates and without, for both target forms.

    python tools/score_time.py [--n 256] [--size 512] [--reps 20] [--rounds 7] [--out FILE.json]

Each figure is the median over ``rounds`` of (one event pair around ``reps`` back-to-back scores) / reps, after
a warm-up of every variant; the spread (min .. max over the rounds) is printed beside it.  Bytes read = the
logits (4 B) plus the target (4 B or 1 B) per element; the slabs written are under 1 % of that.  The share is
of the parent commit's headline forward step (BENCH_r06.json: 74.65 ms at batch 256, mixed).  Needs a GPU.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tw-invoice-unet-ocr-llm_amd"))

HEADLINE_FORWARD_MS = 74.65   # BENCH_r06.json, value (ms per step of 256 pages)
SWEEP = [0.05 * k for k in range(1, 20)]


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
        raise SystemExit("score_time: needs a ROCm GPU (there is no CPU timing)")
    dev = "cuda:0"
    n, c, s = a.n, 3, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn((n, c, s, s), device=dev, generator=g) * 4.0 - 3.0
    tu8 = torch.where(torch.rand((n, s, s, c), device=dev, generator=g) < 0.1, 255, 0).to(torch.uint8)
    tf = (tu8.to(torch.float32) / 255.0).permute(0, 3, 1, 2).contiguous()
    h = native.Handle(3, c, "mixed", 0)
    h.score_reserve(n, s, s, len(SWEEP))
    st = torch.cuda.current_stream(dev).cuda_stream
    variants = [("u8_nhwc", tu8, None), ("u8_nhwc+sweep19", tu8, SWEEP), ("f32_nchw", tf, None),
                ("f32_nchw+sweep19", tf, SWEEP)]
    for _, t, sw in variants:   # warm-up: code objects, the allocator's blocks of the outputs
        for _ in range(3):
            h.score(logits, t, st, sweep=sw)
    torch.cuda.synchronize()
    rows = []
    for name, t, sw in variants:
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                h.score(logits, t, st, sweep=sw)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.reps)
        ms.sort()
        med = ms[len(ms) // 2]
        nbytes = logits.numel() * 4 + t.numel() * t.element_size()
        rows.append(dict(variant=name, ms=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                         bytes_read=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                         gelem_per_s=round(logits.numel() / med / 1e6, 1),
                         share_of_forward=round(med / HEADLINE_FORWARD_MS, 4)))
        print(json.dumps(rows[-1]))
    out = dict(n=n, classes=c, size=s, reps=a.reps, rounds=a.rounds, headline_forward_ms=HEADLINE_FORWARD_MS,
               results=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    h.close()


if __name__ == "__main__":
    main()
