"""Generate tests/golden/head_cases.npz by running the REFERENCE's out_conv and torch autograd (survey container
only).

Usage (from the repo root, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_golden.py

It imports ``unet_model`` from /root/reference as make_golden.py does, builds its ``UNet(3, C)`` and calls that
model's ``out_conv`` (unet_model.py:50) and ``backward`` on the CPU, in fp32 and in fp64, on the seeded cases of
tests/head_ref.py.  No reference source is copied; per case the file keeps the generator parameters, a checksum of
the generated features, the reference's fp32 logits, grad_w and grad_b, its grad_feat at head_ref.SAMPLES seeded
positions, and per output ``spread`` = max |fp32 - fp64| / max |fp64|: the distance of the reference's own fp32
results from its fp64 ones, which the tests' bar scales.  A case whose spread exceeds head_ref.SPREAD_LIMIT is
refused.

The trajectory case: the reference's out_conv, re-initialised as train.py:106-108 does, fitted on seeded features
and 0/1 targets by train.py's loop (its InvoiceLoss, AdamW with weight decay 1e-4, CosineAnnealingWarmRestarts(10,
2), 20 epochs of two batches of 2, not shuffled) at two learning rates, in fp32 and in fp64: the fp32 run's loss at
every step, and the largest relative distance of the two trajectories.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import head_ref  # noqa: E402
from make_score_golden import REF, ref_train  # noqa: E402


def ref_out_conv(c, w, b, dtype):
    """the reference UNet's out_conv holding (w, b), as ``dtype``"""
    sys.path.insert(0, REF)
    import unet_model as ref_unet  # noqa: E402
    sys.path.remove(REF)
    conv = ref_unet.UNet(n_channels=3, n_classes=c).out_conv
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(w).view(c, head_ref.K, 1, 1))
        conv.bias.copy_(torch.from_numpy(b))
    return conv.to(dtype)


def ref_head(feat, w, b, g, dtype):
    conv = ref_out_conv(w.shape[0], w, b, dtype)
    x = torch.from_numpy(feat).to(dtype).requires_grad_()
    logits = conv(x)
    logits.backward(torch.from_numpy(g).to(dtype))
    return dict(logits=logits.detach().numpy(), grad_w=conv.weight.grad.numpy().reshape(w.shape),
                grad_b=conv.bias.grad.numpy(), grad_feat=x.grad.numpy())


def ref_trajectory(crit, feat, target, w0, b0, lr, dtype):
    conv = ref_out_conv(w0.shape[0], w0, b0, dtype)
    x, t = torch.from_numpy(feat).to(dtype), torch.from_numpy(target).to(dtype)
    opt = torch.optim.AdamW(conv.parameters(), lr=lr, weight_decay=head_ref.TRAJ_WD)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2)
    losses = []
    for _ in range(head_ref.TRAJ_EPOCHS):
        for lo in range(0, x.shape[0], head_ref.TRAJ_BATCH):
            loss = crit(conv(x[lo:lo + head_ref.TRAJ_BATCH]), t[lo:lo + head_ref.TRAJ_BATCH])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        sched.step()
    return np.array(losses, np.float64)


def main():
    torch.set_num_threads(1)
    payload = dict(n_cases=np.int64(len(head_ref.CASES)))
    for i, (name, shape, seed, dead) in enumerate(head_ref.CASES):
        feat, w, b, g = head_ref.generate(shape, seed, dead)
        r32, r64 = ref_head(feat, w, b, g, torch.float32), ref_head(feat, w, b, g, torch.float64)
        ours = dict(zip(head_ref.OUTPUTS, head_ref.head(feat, w, b, g)))
        pos = head_ref.sample_positions(shape, seed)
        payload.update({f"name_{i}": np.array(name), f"shape_{i}": np.array(shape, np.int64), f"seed_{i}": np.int64(seed),
                        f"dead_{i}": np.array(dead, np.int64), f"feat_sha256_{i}": np.array(head_ref.sha256(feat)),
                        f"positions_{i}": pos})
        line = [f"{name} {shape}: max |feat| {feat.max():.2f}"]
        for k in head_ref.OUTPUTS:
            assert r32[k].dtype == np.float32 and np.isfinite(r32[k]).all() and np.isfinite(r64[k]).all()
            spread = head_ref.distance(r32[k], r64[k])
            if not spread <= head_ref.SPREAD_LIMIT:
                raise SystemExit(f"case {name}: {k} spread {spread:.3e} > {head_ref.SPREAD_LIMIT}: refused")
            line.append(f"{k} spread {spread:.2e} restatement {head_ref.distance(ours[k], r32[k]):.2e}")
            keep = r32[k].reshape(-1)[pos] if k == "grad_feat" else r32[k]
            payload.update({f"{k}_{i}": keep, f"spread_{k}_{i}": np.float64(spread)})
        print(", ".join(line))

    crit = ref_train().InvoiceLoss()
    feat, target, w0, b0 = head_ref.trajectory_tensors()
    payload.update(traj_feat_sha256=np.array(head_ref.sha256(feat)), traj_lrs=np.array(head_ref.TRAJ_LRS, np.float64))
    for j, lr in enumerate(head_ref.TRAJ_LRS):
        l32 = ref_trajectory(crit, feat, target, w0, b0, lr, torch.float32)
        l64 = ref_trajectory(crit, feat, target, w0, b0, lr, torch.float64)
        spread = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
        print(f"trajectory lr {lr}: first {l64[0]:.4f} last {l64[-1]:.4f}, target density {target.mean():.3f}, "
              f"fp32 against fp64 {spread:.2e} over {len(l32)} steps")
        payload.update({f"traj_losses_{j}": l32.astype(np.float32), f"traj_spread_{j}": np.float64(spread)})
    np.savez_compressed(os.path.join(HERE, "head_cases.npz"), **payload)


if __name__ == "__main__":
    main()
