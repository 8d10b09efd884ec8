"""Generate tests/golden/score_cases.npz by running the REFERENCE's losses (survey container only).

Usage (from the repo root, where /root/reference exists):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_score_golden.py

It imports ``train`` from /root/reference and calls its InvoiceLoss, MultiLabelDiceLoss and
MultiLabelFocalLoss (train.py:18-59) on CPU fp32 on the seeded cases of tests/score_ref.py.  ``train``
imports ``dataset``, which imports cv2 (not needed by the losses, not installed here): an empty stand-in
module named cv2 is registered before the import.  No reference source is copied; the file keeps only the
generator parameters, a checksum of the generated logits and the reference's results, and per case the
largest relative distance between the reference's fp32 result and the numpy restatement (score_ref) as
``spread`` -- the distance of two fp32 implementations of the same arithmetic, which the tests' bar scales.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import score_ref  # noqa: E402
from unet_mi355x.metrics import Score  # noqa: E402

REF = "/root/reference"


def ref_train():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, REF)
    import train  # noqa: E402
    sys.path.remove(REF)
    return train


def main():
    torch.set_num_threads(1)
    train = ref_train()
    crit, dice, focal = train.InvoiceLoss(), train.MultiLabelDiceLoss(), train.MultiLabelFocalLoss()

    def ref_loss(x, t, b):
        """the reference called per batch of b and averaged (train.py:133-151)"""
        parts = [float(crit(x[i:i + b], t[i:i + b])) for i in range(0, x.shape[0], b)]
        return sum(parts) / len(parts)

    payload = dict(n_cases=np.int64(len(score_ref.CASES)))
    for i, (shape, scale, shift, density, seed) in enumerate(score_ref.CASES):
        logits, target = score_ref.generate(shape, scale, shift, density, seed)
        x = torch.from_numpy(logits)
        t = torch.from_numpy(score_ref.target_f32(target))
        with torch.no_grad():
            p = torch.sigmoid(x)
            ref = dict(dice=float(dice(p, t)), focal=float(focal(p, t)), loss=float(crit(x, t)),
                       loss_b1=ref_loss(x, t, 1), loss_b2=ref_loss(x, t, 2))
        entries, _ = score_ref.score(logits, t.numpy(), [0.0] * shape[1])
        s = Score(entries)
        ours = dict(dice=s.dice(), focal=s.focal(), loss=s.loss(), loss_b1=s.loss(batch=1), loss_b2=s.loss(batch=2))
        spread = max(score_ref.rel(ref[k], ours[k]) for k in ("dice", "focal", "loss"))
        payload.update({f"shape_{i}": np.array(shape, np.int64), f"scale_{i}": np.float64(scale),
                        f"shift_{i}": np.float64(shift), f"density_{i}": np.float64(density),
                        f"seed_{i}": np.int64(seed), f"logits_sha256_{i}": np.array(score_ref.sha256(logits)),
                        f"spread_{i}": np.float64(spread)})
        payload.update({f"{k}_{i}": np.float64(v) for k, v in ref.items()})
        print(shape, {k: (ref[k], ours[k]) for k in ref}, "spread %.3e" % spread)
    np.savez_compressed(os.path.join(HERE, "score_cases.npz"), **payload)


if __name__ == "__main__":
    main()
