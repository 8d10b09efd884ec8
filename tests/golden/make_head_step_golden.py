"""Generate tests/golden/head_step_cases.npz by running the REFERENCE's out_conv, InvoiceLoss and torch autograd
(survey container only).

Usage (from the repo root, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_head_step_golden.py

It imports ``train`` and ``unet_model`` from /root/reference as make_loss_golden.py and make_head_golden.py do (an
empty stand-in module named cv2 is registered before the import), holds the seeded head of tests/head_step_ref.py in
the reference UNet's ``out_conv`` (unet_model.py:50), and runs ``loss = InvoiceLoss()(out_conv(feat), mask);
loss.backward()`` (train.py:137-142) on the CPU, in fp32 and in fp64.  No reference source is copied; per case the
file keeps the generator parameters, a checksum of the generated features, the reference's fp32 loss, grad_w and
grad_b, and per output ``spread`` = max |fp32 - fp64| / max |fp64|: the distance of the reference's own fp32
autograd from its fp64 autograd, which the tests' bar scales.  A case whose spread exceeds loss_ref.SPREAD_LIMIT, or
whose logits fall in the clamp band 14 < |x| < 20 of train.py:41, is refused: its inputs are ill-conditioned, not a
fixture.
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
import head_step_ref as ref  # noqa: E402
from make_head_golden import ref_out_conv  # noqa: E402
from make_score_golden import ref_train  # noqa: E402


def ref_step(crit, feat, w, b, target, dtype):
    conv = ref_out_conv(w.shape[0], w, b, dtype)
    loss = crit(conv(torch.from_numpy(feat).to(dtype)), torch.from_numpy(target).to(dtype))
    loss.backward()
    return dict(loss=loss.detach().numpy(), grad_w=conv.weight.grad.numpy().reshape(w.shape),
                grad_b=conv.bias.grad.numpy())


def main():
    torch.set_num_threads(1)
    crit = ref_train().InvoiceLoss()
    payload = dict(n_cases=np.int64(len(ref.CASES)))
    for i, (name, shape, seed, density, soft) in enumerate(ref.CASES):
        feat, w, b, tu8 = ref.generate(shape, seed, density, soft)
        tf = ref.target_f32(tu8)
        if ref.in_clamp_band(ref.logits_chain(feat, w, b)):
            raise SystemExit(f"case {name}: a logit in the clamp band 14 < |x| < 20: refused")
        r32, r64 = ref_step(crit, feat, w, b, tf, torch.float32), ref_step(crit, feat, w, b, tf, torch.float64)
        ours = dict(zip(ref.OUTPUTS, ref.step(feat, w, b, tf)))
        payload.update({f"name_{i}": np.array(name), f"shape_{i}": np.array(shape, np.int64), f"seed_{i}": np.int64(seed),
                        f"density_{i}": np.float64(density), f"soft_{i}": np.bool_(soft),
                        f"feat_sha256_{i}": np.array(ref.sha256(feat))})
        line = [f"{name} {shape}: loss {float(r32['loss']):.6f}"]
        for k in ref.OUTPUTS:
            assert r32[k].dtype == np.float32 and np.isfinite(r32[k]).all() and np.isfinite(r64[k]).all()
            spread = ref.distance(r32[k], r64[k])
            if not spread <= ref.SPREAD_LIMIT:
                raise SystemExit(f"case {name}: {k} spread {spread:.3e} > {ref.SPREAD_LIMIT}: refused")
            line.append(f"{k} spread {spread:.2e} restatement {ref.distance(ours[k], r32[k]):.2e} "
                        f"(against fp64 {ref.distance(ours[k], r64[k]):.2e})")
            payload.update({f"{k}_{i}": r32[k], f"spread_{k}_{i}": np.float64(spread)})
        print(", ".join(line))
    np.savez_compressed(os.path.join(HERE, "head_step_cases.npz"), **payload)


if __name__ == "__main__":
    main()
