"""bench.py on the GPU: a plain run times the headline only (at 512^2, where --full would add every other
leg), and --dump-outputs writes the masks a caller of the timed step receives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_only_and_dumped_masks_equal_the_forward(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    from unet_mi355x import synthetic as syn
    from unet_mi355x.model import UNet
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--batch", "4", "--steps", "2",
                        "--warmup", "1", "--detail-out", "", "--dump-outputs", str(tmp_path)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dtype"] == "bf16+fp16"
    assert out["value"] == pytest.approx(4 / (1e-3 * out["ms_per_step"]), rel=1e-2)
    assert out["strong_scaling"] == [] and out["roofline"] is None and out["cpu_baseline"] is None
    assert out["fp32"] is None and out["cfg5"] is None and out["latency_bs1"] is None
    got = np.load(tmp_path / "masks.npy")
    assert got.dtype == np.float32 and got.shape == (4, 3, 512, 512)
    m = UNet(3, 3, compute_dtype="mixed")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()})
    m = m.to("cuda:0").eval()
    with torch.no_grad():
        ref = m.forward_masks(torch.from_numpy(bench.gen_pages(1000, 4, 512, 3)).to("cuda:0"), packed=True).cpu().numpy()
    m.close()
    assert np.array_equal(got, np.unpackbits(ref, axis=-1, bitorder="little").astype(np.float32))
    assert 0 < got.mean() < 1    # the pretrained-like weights find fields on the pages
