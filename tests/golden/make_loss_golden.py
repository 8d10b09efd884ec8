"""Generate tests/golden/loss_cases.npz by running the REFERENCE's InvoiceLoss and torch autograd (survey
container only).

Usage (from the repo root, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_loss_golden.py

It imports ``train`` from /root/reference as make_score_golden.py does (an empty stand-in module named cv2 is
registered before the import) and calls its InvoiceLoss (train.py:18-59) and ``backward`` on CPU, in fp32 and in
fp64, on the seeded cases of tests/loss_ref.py.  No reference source is copied; per case the file keeps the
generator parameters, a checksum of the generated logits, the reference's fp32 loss and fp32 gradient at the
logits, and ``spread`` = max |g32 - g64| / max |g64|: the distance of the reference's own fp32 autograd from its
fp64 autograd, which the tests' bar scales.  A case whose spread exceeds loss_ref.SPREAD_LIMIT is refused: its
inputs are ill-conditioned (the clamp edge of train.py:41), not a fixture.

The case with a NaN logit: torch's CPU binary_cross_entropy refuses a NaN input outright, so the reference runs
on the same logits with the NaN replaced by 0.  Every other (n, c) plane's gradient does not depend on that element
(the focal term is element-wise, the Dice term per plane), so those planes are the reference's; the NaN logit's
own plane and the loss are stored as NaN, the IEEE propagation unet_score already follows.
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
import loss_ref  # noqa: E402
from make_score_golden import ref_train  # noqa: E402


def ref_loss_grad(crit, logits, target, dtype):
    x = torch.from_numpy(logits).to(dtype).requires_grad_()
    loss = crit(x, torch.from_numpy(target).to(dtype))
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def main():
    torch.set_num_threads(1)
    crit = ref_train().InvoiceLoss()
    payload = dict(n_cases=np.int64(len(loss_ref.CASES)))
    for i, (name, shape, scale, shift, density, soft, seed, nan_at) in enumerate(loss_ref.CASES):
        logits, tu8 = loss_ref.generate(shape, scale, shift, density, soft, seed, nan_at)
        tf = loss_ref.target_f32(tu8)
        finite = np.where(np.isnan(logits), np.float32(0), logits)
        l32, g32 = ref_loss_grad(crit, finite, tf, torch.float32)
        l64, g64 = ref_loss_grad(crit, finite, tf, torch.float64)
        assert g32.dtype == np.float32 and np.isfinite(g32).all() and np.isfinite(g64).all()
        spread = loss_ref.grad_distance(g32, g64)
        if nan_at is not None:
            l32 = np.float32("nan")
            g32[nan_at[0], nan_at[1]] = np.nan
        if not spread <= loss_ref.SPREAD_LIMIT:
            raise SystemExit(f"case {name}: spread {spread:.3e} > {loss_ref.SPREAD_LIMIT}: refused")
        ours_l, ours_g = loss_ref.loss_grad(logits, tf)
        print(f"{name} {shape}: loss {l32!r} (restatement {ours_l!r}), max|g| {np.nanmax(np.abs(g32)):.3e}, "
              f"spread {spread:.3e}, restatement {loss_ref.grad_distance(ours_g, g32):.3e}")
        payload.update({f"name_{i}": np.array(name), f"shape_{i}": np.array(shape, np.int64),
                        f"scale_{i}": np.float64(scale), f"shift_{i}": np.float64(shift),
                        f"density_{i}": np.float64(density), f"soft_{i}": np.bool_(soft), f"seed_{i}": np.int64(seed),
                        f"nan_at_{i}": np.array(nan_at if nan_at is not None else (), np.int64),
                        f"logits_sha256_{i}": np.array(loss_ref.sha256(logits)), f"loss_{i}": np.float32(l32),
                        f"grad_{i}": g32, f"spread_{i}": np.float64(spread)})
    np.savez_compressed(os.path.join(HERE, "loss_cases.npz"), **payload)


if __name__ == "__main__":
    main()
