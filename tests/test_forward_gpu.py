"""Parity of the native MI355X forward (through the C-ABI) against the golden vectors the
reference produced and against the CPU oracle.  Needs a GPU: run with -m gpu.

Logit tolerances, max |err| / max(1, max|ref|) (TOL; measured on MI355X in round 2, see
profiles/gpu_tests_r2*.log, and set at about 2x the largest value measured over the goldens):
  fp32  (exact-fp32 MFMA, different summation order)             measured <= 5e-6
  fp16  (fp16 storage, fp32 accumulate)                          measured <= 2.2e-3
  bf16  (bf16 storage, fp32 accumulate)                          measured <= 1.7e-2
  mixed (bf16 at levels 2-4, fp16 at levels 0-1: the bench plan)
Masks: fp32 must match the oracle to IoU >= 0.999 (north_star); on trained-like weights the
bench plan ("mixed") and fp16 meet 0.999 too, pure bf16 does not (0.998).
"""
import glob
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import unet_oracle as orc
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
# max|err| / max(1, max|ref|) bounds, about 2x the largest measured on MI355X (round 2 logs:
# fp32 6.2e-6, fp16 2.7e-3, bf16 2.1e-2, mixed 1.6e-2, all on the reference's own 512x512 logits)
TOL = {"fp32": 2e-5, "fp32_exact": 2e-5, "fp16": 5e-3, "bf16": 3.5e-2, "mixed": 3e-2}
DEV = "cuda:0"
HALO_CFGS, RING_CFGS, UP_CFGS = [0, 1, 2], [3, 4, 5, 8, 9, 10, 11], [2, 6, 7]   # csrc/unet_internal.h Cfg
# bitwise families: the 4-wave ring (zero-initialised accumulators, bias added in the epilogue) and the
# 8-wave ring (accumulators start at the bias, round 3) accumulate in the same K order but add the bias
# at different ends, so each agrees bitwise only within itself
RING4_CFGS, RING8_CFGS = [3, 4, 5], [8, 9, 10, 11]
UP_RING_CFGS = [6, 7]                   # convT_ring_kernel (accumulators start at the bias)


def make_model(sd_np, c, dtype):
    m = UNet(c, 3, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
    return m.to(DEV).eval()


def rel_err(out, ref):
    return float(np.abs(out - ref).max()) / max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("dtype", ["fp32", "fp32_exact", "fp16", "bf16", "mixed"])
@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "unet_*.npz"))), ids=os.path.basename)
def test_golden_logits(path, dtype):
    z = np.load(path)
    c = int(z["n_channels"])
    sd = syn.make_state_dict(int(z["seed"]), c, 3, profile=str(z["profile"]))
    m = make_model(sd, c, dtype)
    with torch.no_grad():
        out = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
    err = rel_err(out, z["logits"])
    print(f"{os.path.basename(path)} {dtype}: rel err {err:.3e}")
    assert out.shape == z["logits"].shape
    assert np.isfinite(out).all()
    assert err <= TOL[dtype]
    m.close()


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "mixed"])
def test_golden_intermediates(dtype, fuse, monkeypatch):
    """Per-layer localisation: skips, pools, bottleneck and up-convs vs the reference hooks.  With
    up1 fused into conv2.3 (the 16-bit default) conv2.3's output c7 is never stored, and fetching
    it is an error; UNET_MI355X_FUSE_UP1=0 keeps the two launches."""
    monkeypatch.setenv("UNET_MI355X_FUSE_UP1", fuse)
    fused = fuse == "1" and dtype != "fp32"
    z = np.load(os.path.join(GOLD, "unet_c3_h16w16_n3_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    m = make_model(sd, 3, dtype)
    x = torch.from_numpy(z["x"]).to(DEV)
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    for name, key in (("c1", "inter_c1"), ("c2", "inter_c2"), ("c3", "inter_c3"), ("c4", "inter_c4"),
                      ("bn", "inter_bn"), ("u1", "inter_u1_up"), ("u4", "inter_u4_up"), ("c7", "inter_c7")):
        if name == "c7" and fused:
            with pytest.raises(RuntimeError, match="not stored"):
                m.intermediate(name)
            continue
        ref = z[key]
        got = m.intermediate(name).cpu().numpy().reshape(ref.shape)
        err = rel_err(got, ref)
        print(f"{name} {dtype}: rel err {err:.3e}")
        assert err <= TOL[dtype], name
    m.close()


def _golden_photo_input(m):
    """The 600x400 golden photo through the device preprocessing (inference.py:62-64)."""
    from PIL import Image
    z = np.load(os.path.join(GOLD, "run_unet_600x400.npz"))
    img = torch.from_numpy(np.ascontiguousarray(np.asarray(Image.fromarray(z["image"], mode="RGB")))).to(DEV)
    return z, m.preprocess(img, 512)


def test_preprocess_equals_reference_input_bitwise():
    """unet_preprocess of the golden photo is the reference's own network input, byte for byte
    (sha256 of inference.preprocess(pil.resize((512, 512))), make_golden.py)."""
    m = make_model(syn.make_state_dict(0, 3, 3), 3, "bf16")
    z, x = _golden_photo_input(m)
    xh = x.cpu().numpy()
    assert xh.shape == (1, 3, 512, 512) and xh.dtype == np.float32
    assert hashlib.sha256(xh.tobytes()).hexdigest() == str(z["x_sha256"])
    assert np.array_equal(xh[0, :, ::8, ::8], z["x_sub8"])
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16", "mixed"])
def test_reference_512_logits(dtype):
    """Full-size (512x512) logits pinned to the REFERENCE's own forward on its run_unet input:
    the stored 1/4-subsampled grid and rows 0 and 257 (make_golden.py, inference.py:62-67)."""
    z = np.load(os.path.join(GOLD, "run_unet_600x400.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile="structured")
    sd["out_conv.bias"] = sd["out_conv.bias"] + z["out_bias_delta"]
    m = make_model(sd, 3, dtype)
    _, x = _golden_photo_input(m)
    with torch.no_grad():
        lg = m(x).cpu().numpy()[0]
    errs = {"sub4": rel_err(lg[:, ::4, ::4], z["logits_sub4"]), "row0": rel_err(lg[:, 0, :], z["logits_row0"]),
            "row257": rel_err(lg[:, 257, :], z["logits_row257"])}
    print(f"512x512 reference logits {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) <= TOL[dtype]
    m.close()


@pytest.mark.parametrize("c,n,h,w", [(3, 2, 64, 128), (1, 3, 96, 32), (3, 1, 160, 48), (3, 2, 16, 16), (1, 1, 16, 80)])
def test_fp32_vs_oracle_odd_shapes(c, n, h, w):
    sd = syn.make_state_dict(100 + h, c, 3, profile="structured")
    x = syn.uniform_batch(5 + w, n, c, h, w)
    ref = orc.unet_forward(sd, torch.from_numpy(x)).numpy()
    m = make_model(sd, c, "fp32")
    with torch.no_grad():
        out = m(torch.from_numpy(x).to(DEV)).cpu().numpy()
    err = rel_err(out, ref)
    print(f"fp32 {c}x{h}x{w} n={n}: rel err {err:.3e}")
    assert err <= TOL["fp32"]
    m.close()


@pytest.mark.parametrize("dtype", ["mixed", "bf16", "fp16"])
@pytest.mark.parametrize("n,h,w", [(2, 16, 16), (1, 16, 112), (6, 16, 16)])
def test_16bit_plans_at_the_minimum_size(dtype, n, h, w):
    """The smallest input the reference accepts (H, W = 16: the bottleneck is 1 x 1 pixel, every tile
    of every level is partial, the small-batch split-K plan at N <= 4 and the large-batch plan at N = 6)
    against the fp32 oracle within the plan's tolerance."""
    sd = syn.make_state_dict(200 + w, 3, 3, profile="structured")
    x = syn.uniform_batch(7 + n, n, 3, h, w)
    ref = orc.unet_forward(sd, torch.from_numpy(x)).numpy()
    m = make_model(sd, 3, dtype)
    with torch.no_grad():
        out = m(torch.from_numpy(x).to(DEV)).cpu().numpy()
    err = rel_err(out, ref)
    print(f"{dtype} 3x{h}x{w} n={n}: rel err {err:.3e}")
    assert err <= TOL[dtype]
    m.close()


def _recentred(seed, x, c=3):
    """Structured weights with out_conv bias shifted so ~10% of pixels pass each threshold."""
    sd = syn.make_state_dict(seed, c, 3, profile="structured")
    logits = orc.unet_forward(sd, torch.from_numpy(x)).numpy()
    thr = np.array([0.25, 0.40, 0.30])
    q = np.quantile(logits.transpose(1, 0, 2, 3).reshape(3, -1), 0.9, axis=1)
    sd["out_conv.bias"] = (sd["out_conv.bias"] + (np.log(thr / (1 - thr)) - q)).astype(np.float32)
    return sd, orc.unet_forward(sd, torch.from_numpy(x)).numpy()


def test_masks_512_all_dtypes():
    """Full-size 512x512 pages, untrained (structured) weights: logits within tolerance of the
    oracle, fused masks (u8 and bit-packed agree) vs the oracle's masks.  Untrained weights put
    ~20 % of the pixels near a threshold, so the 16-bit IoU bounds here are loose; the
    trained-like case is test_masks_512_pretrained_weights."""
    x = syn.invoice_pages(21, 2, 512, 512, 3)
    sd, ref_logits = _recentred(21, x)
    ref_masks = np.stack([np.stack(list(orc.masks_from_logits(ref_logits[i]).values())) for i in range(2)])
    xd = torch.from_numpy(x).to(DEV)
    for dtype, min_iou in (("fp32", 0.999), ("fp16", 0.99), ("mixed", 0.97), ("bf16", 0.95)):
        m = make_model(sd, 3, dtype)
        with torch.no_grad():
            masks, logits = m.forward_masks(xd, with_logits=True)
            bits = m.forward_masks(xd, packed=True)
        masks = masks.cpu().numpy().astype(bool)
        unpacked = np.unpackbits(bits.cpu().numpy(), axis=-1, bitorder="little").astype(bool)
        assert np.array_equal(unpacked, masks), "bit-packed and u8 masks disagree"
        err = rel_err(logits.cpu().numpy(), ref_logits)
        ious = [orc.mask_iou(masks[i, k], ref_masks[i, k]) for i in range(2) for k in range(3)]
        print(f"512x512 {dtype}: logits rel err {err:.3e}, mask IoU min {min(ious):.5f} mean {np.mean(ious):.5f}")
        assert err <= TOL[dtype]
        assert min(ious) >= min_iou
        m.close()


def test_masks_512_pretrained_weights():
    """Trained-like weights (synthetic profile "pretrained": bimodal logits, as a trained net
    has): fused masks of every dtype vs the fp32 CPU oracle at 512x512 (north_star IoU
    target 0.999, met by fp32, fp16 and the bench's mixed plan)."""
    x = syn.invoice_pages(1000, 2, 512, 512, 3)
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    ref_logits = orc.unet_forward(sd, torch.from_numpy(x)).numpy()
    ref_masks = np.stack([np.stack(list(orc.masks_from_logits(ref_logits[i]).values())) for i in range(2)])
    assert 0.02 < ref_masks.mean() < 0.5
    xd = torch.from_numpy(x).to(DEV)
    for dtype, min_iou in (("fp32", 0.9999), ("fp16", 0.999), ("mixed", 0.999), ("bf16", 0.995)):
        m = make_model(sd, 3, dtype)
        with torch.no_grad():
            bits = m.forward_masks(xd, packed=True)
        masks = np.unpackbits(bits.cpu().numpy(), axis=-1, bitorder="little").astype(bool)
        ious = [orc.mask_iou(masks[i, k], ref_masks[i, k]) for i in range(2) for k in range(3)]
        print(f"512x512 pretrained {dtype}: mask IoU min {min(ious):.5f} mean {np.mean(ious):.5f}")
        assert min(ious) >= min_iou
        m.close()


def test_batch256_bench_shape_invariance_and_iou(monkeypatch):
    """The batch the bench times (256 pages of 512x512, the bench's mixed plan, bit-packed
    masks): image i of the N=256 forward equals the same image run alone (N=1) and in the
    second half-batch (N=128, rank 1's shard of a 2-GPU run) bit for bit -- the persistent
    walkers wrap ~100x more often at N=256 than in the small tests --, and the masks of 16
    distinct pages (a quarter of the batch's 64 unique pages, spread over its positions) match
    the fp32 oracle at IoU >= 0.999.  (N = 1 with the small-batch split-K plan switched off: that
    plan accumulates in another order, test_small_batch_split_k_plan.)"""
    import bench
    monkeypatch.setenv("UNET_MI355X_KSPLIT", "0")
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    m = make_model(sd, 3, "mixed")
    x = torch.from_numpy(bench.gen_pages(1000, 256, 512, 3, unique=64)).to(DEV)
    with torch.no_grad():
        full = m.forward_masks(x, packed=True).clone()
        half = m.forward_masks(x[128:].contiguous(), packed=True)
    assert torch.equal(half, full[128:]), "N=128 shard differs from the N=256 batch"
    with torch.no_grad():   # rank 1's shard of global batch 256 over 8 GPUs (the strong-scaling shape)
        eighth = m.forward_masks(x[32:64].contiguous(), packed=True)
    assert torch.equal(eighth, full[32:64]), "N=32 shard differs from the N=256 batch"
    for i in (0, 77, 128, 255):
        with torch.no_grad():
            one = m.forward_masks(x[i:i + 1].contiguous(), packed=True)
        assert torch.equal(one, full[i:i + 1]), f"image {i}: N=1 differs from N=256"
    pos = [4 * k + 64 * (k % 4) for k in range(16)]   # page i is unique page i % 64: 0, 4, .., 60
    logits = orc.unet_forward(sd, x[pos].cpu()).numpy()
    ious = []
    for j, i in enumerate(pos):
        ref = orc.masks_from_logits(logits[j])
        got = np.unpackbits(full[i].cpu().numpy(), axis=-1, bitorder="little").astype(bool)
        ious += [orc.mask_iou(got[k], ref[f]) for k, f in enumerate(orc.FIELDS)]
    print(f"bs256 mixed: IoU vs oracle over {len(pos)} pages: min {min(ious):.5f} mean {np.mean(ious):.5f}")
    assert min(ious) >= 0.999
    m.close()


@pytest.mark.parametrize("dtype", ["fp32", "mixed"])
def test_nan_input_propagates_like_torch(dtype):
    """A NaN input pixel propagates exactly as through the reference's aten ops: conv spreads it
    over the 3x3 neighbourhood, ReLU and MaxPool2d keep it (unet_model.py:12,16,34), so the NaN
    logits form the same receptive-field pattern as the oracle's; the other logits stay within
    tolerance and a NaN logit gives a False mask (sigmoid(NaN) > thr is False)."""
    sd = syn.make_state_dict(3, 3, 3, profile="structured")
    x = syn.uniform_batch(8, 1, 3, 320, 320)
    x[0, 1, 7, 9] = np.nan
    x[0, 0, 300, 170] = np.nan
    ref = orc.unet_forward(sd, torch.from_numpy(x)).numpy()
    m = make_model(sd, 3, dtype)
    with torch.no_grad():
        masks, lg = m.forward_masks(torch.from_numpy(x).to(DEV), with_logits=True)
    lg, masks = lg.cpu().numpy(), masks.cpu().numpy()
    nan_ref, nan_got = np.isnan(ref), np.isnan(lg)
    print(f"{dtype}: NaN logits {int(nan_got.sum())} (oracle {int(nan_ref.sum())}) of {lg.size}")
    assert 0 < nan_ref.sum() < ref.size
    assert np.array_equal(nan_got, nan_ref)
    ok = ~nan_ref
    assert rel_err(lg[ok], ref[ok]) <= TOL[dtype]
    assert not masks[nan_got].any()
    m.close()


FLOOR = 1e-4   # folded weights of _positive_state_dict are raised towards this; asserted: normal fp16 numbers
F16_MIN_NORMAL = 2.0 ** -14


def _positive_state_dict(seed, probe):
    """Structured weights made to carry an infinity through to the logits: |w| on every 3x3 conv and
    ConvTranspose, and every BatchNorm re-calibrated on ``probe`` (running statistics = the layer's own
    pre-BN statistics, gamma 1, beta 0.5) so that activations stay O(1) although all weights are positive.
    inf * w is then +inf in every layer and never meets a -inf.  out_conv: class 0 all positive (+inf),
    class 1 all negative (-inf), class 2 alternating signs (NaN).  Every folded weight is raised
    to a normal fp16 number (>= 2^-14, aiming at 1e-4), so that none rounds to zero in fp16 storage:
    a zero weight would make inf * 0 = NaN of it (without the floor sixteen folded weights of down2 and conv2
    fall below fp16's smallest subnormal, and the mixed plan then has NaN where the oracle has +-inf)."""
    import torch.nn.functional as F
    sd = {k: np.array(v) for k, v in syn.make_state_dict(seed, 3, 3, profile="structured").items()}
    for k, v in sd.items():
        if k.endswith("weight") and v.ndim == 4:
            sd[k] = np.maximum(np.abs(v) / (16.0 if k.startswith("up") else 1.0), FLOOR if k.startswith("up") else 0.0)
    sd["out_conv.weight"][1] *= -1
    sd["out_conv.weight"][2, ::2] *= -1
    t = lambda k: torch.from_numpy(sd[k])   # noqa: E731

    def dc(name, v):
        for conv, bn in ((0, 1), (3, 4)):
            wk = f"{name}.net.{conv}.weight"
            for _ in range(6):   # raising weights raises the variance, which lowers the fold's scale: iterate
                y = F.conv2d(v, t(wk), t(f"{name}.net.{conv}.bias"), padding=1)
                scale = 1.0 / np.sqrt(y.var((0, 2, 3)).numpy() + 1e-3)           # the fold's scale, gamma = 1
                if (sd[wk] * scale.reshape(-1, 1, 1, 1)).min() >= 1.2 * FLOOR:
                    break
                sd[wk] = np.maximum(sd[wk], (2 * FLOOR / scale).astype(np.float32).reshape(-1, 1, 1, 1))
            y = F.conv2d(v, t(wk), t(f"{name}.net.{conv}.bias"), padding=1)
            sd[f"{name}.net.{bn}.running_mean"] = y.mean((0, 2, 3)).numpy()
            sd[f"{name}.net.{bn}.running_var"] = (y.var((0, 2, 3)) + 1e-3).numpy()
            sd[f"{name}.net.{bn}.weight"] = np.ones(y.shape[1], np.float32)
            sd[f"{name}.net.{bn}.bias"] = np.full(y.shape[1], 0.5, np.float32)
            v = F.relu(F.batch_norm(y, t(f"{name}.net.{bn}.running_mean"), t(f"{name}.net.{bn}.running_var"),
                                    t(f"{name}.net.{bn}.weight"), t(f"{name}.net.{bn}.bias"), training=False, eps=1e-5))
            folded = sd[wk] / np.sqrt(sd[f"{name}.net.{bn}.running_var"].astype(np.float64) + 1e-5).reshape(-1, 1, 1, 1)
            assert folded.min() >= F16_MIN_NORMAL, (wk, folded.min())
        return v

    with torch.no_grad():
        skips, v = [], torch.from_numpy(probe)
        for name in ("down1", "down2", "down3", "down4"):
            skips.append(dc(name, v))
            v = F.max_pool2d(skips[-1], 2)
        v = dc("bottleneck", v)
        for k in (4, 3, 2, 1):
            v = dc(f"conv{k}", torch.cat([orc.up(sd, f"up{k}", v), skips[k - 1]], 1))
    return sd


_INF_CASES = {}


def _inf_case(weights):
    """(state_dict, input with one +inf and one -inf pixel, oracle logits), computed once per weight set."""
    if weights not in _INF_CASES:
        x = syn.uniform_batch(8, 1, 3, 320, 320)
        sd = syn.make_state_dict(3, 3, 3, profile="structured") if weights == "structured" else \
            _positive_state_dict(3, np.ascontiguousarray(x[:, :, :64, 64:192]))
        x[0, 1, 7, 9] = np.inf
        x[0, 0, 300, 170] = -np.inf
        _INF_CASES[weights] = (sd, x, orc.unet_forward(sd, torch.from_numpy(x)).numpy())
    return _INF_CASES[weights]


@pytest.mark.parametrize("dtype", ["fp32_exact", "mixed", "fp32"])
@pytest.mark.parametrize("weights", ["structured", "positive"])
def test_inf_input_pixels(weights, dtype):
    """One +inf and one -inf input pixel.  The exact-fp32 plan and the 16-bit plans multiply the infinity by
    the weight itself, as the reference does: the logits are +inf, -inf or NaN exactly where the oracle's are,
    a +inf logit gives a True mask (sigmoid(+inf) = 1), NaN and -inf a False one.  The three-term fp32 plan
    cannot keep the kind: it evaluates inf * w as inf * w_hi + inf * w_mid + inf * w_lo, which is inf - inf
    when w_mid has the other sign and inf * 0 when w is a bf16 value, so every logit the infinity reaches is
    NaN -- the SET of non-finite logits is the oracle's, the finite ones are within tolerance,
    and a non-finite logit gives a False mask.

    "structured": dense weights of both signs; the oracle's own infinities meet as inf - inf in the second
    conv already, so its non-finite logits are all NaN.  "positive" (_positive_state_dict): the +inf pixel
    reaches the logits as +inf in class 0, -inf in class 1 and NaN in class 2 (asserted), and the -inf pixel
    ends at the first ReLU, as in the reference.  There the finite logits are held to the tolerance in the
    fp32 plans only: the re-calibrated BatchNorm subtracts a mean many times the spread, which multiplies a
    16-bit storage error by that ratio, and the 16-bit tolerances were set on zero-mean weights."""
    sd, x, ref = _inf_case(weights)
    m = make_model(sd, 3, dtype)
    with torch.no_grad():
        masks, lg = m.forward_masks(torch.from_numpy(x).to(DEV), with_logits=True)
    lg, masks = lg.cpu().numpy(), masks.cpu().numpy().astype(bool)
    bad_ref, bad_got = ~np.isfinite(ref), ~np.isfinite(lg)
    err = rel_err(lg[~bad_ref & ~bad_got], ref[~bad_ref & ~bad_got])
    print(f"{weights} {dtype}: non-finite logits {int(bad_got.sum())} (oracle {int(bad_ref.sum())}: "
          f"{int(np.isnan(ref).sum())} NaN, {int(np.isposinf(ref).sum())} +inf, {int(np.isneginf(ref).sum())} -inf) "
          f"of {lg.size}; finite logits rel err {err:.3e}")
    assert 0 < bad_ref.sum() < ref.size
    if weights == "positive":
        assert np.isposinf(ref[0, 0]).sum() > 1000 and np.isneginf(ref[0, 1]).sum() > 1000 and np.isnan(ref[0, 2]).sum() > 1000
        assert np.isfinite(ref[0, :, 300, 170]).all()        # the -inf pixel: relu(-inf) = 0
    assert np.array_equal(bad_got, bad_ref)
    if weights == "structured" or dtype != "mixed":
        assert err <= TOL[dtype]
    if dtype == "fp32":
        assert not masks[bad_got].any()
    else:
        assert np.array_equal(np.isnan(lg), np.isnan(ref))
        assert np.array_equal(np.isposinf(lg), np.isposinf(ref))
        assert np.array_equal(np.isneginf(lg), np.isneginf(ref))
        assert masks[np.isposinf(lg)].all() and not masks[np.isnan(lg) | np.isneginf(lg)].any()
    m.close()


def test_logit_cut_matches_torch_sigmoid_on_gpu():
    """The fused masks threshold logits at the host-bisected cut (unet_logit_cut); the reference
    thresholds torch.sigmoid.  Against ROCm's own sigmoid on the GPU, every fp32 logit within
    4096 ulps of each field's cut classifies the same way, except at most a hair from the cut
    (the ulp-level disagreement of two fp32 sigmoid implementations)."""
    lib = native.load_library()
    for thr in (0.25, 0.40, 0.30):
        cut = np.float32(lib.unet_logit_cut(thr))
        bits = cut.view(np.int32).astype(np.int64) + np.arange(-4096, 4097)
        x = torch.from_numpy(bits.astype(np.int32).view(np.float32)).to(DEV)
        theirs = (torch.sigmoid(x) > thr).cpu().numpy()
        ours = (x > float(cut)).cpu().numpy()
        diff = np.nonzero(ours != theirs)[0] - 4096
        print(f"thr {thr}: cut {float(cut)!r}, ulps that disagree with torch.sigmoid on the GPU: {diff.tolist()}")
        assert np.all(np.abs(diff) <= 2)


def test_two_streams_share_one_handle():
    """forwards issued on two torch streams against ONE handle (one workspace) give
    bitwise the results of the same forwards issued back to back on one stream -- the library
    orders a call after the previous call on another stream (hipStreamWaitEvent)."""
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    m = make_model(sd, 3, "mixed")
    xa = torch.from_numpy(syn.invoice_pages(31, 8, 512, 512, 3)).to(DEV)
    xb = torch.from_numpy(syn.invoice_pages(32, 8, 512, 512, 3)).to(DEV)
    with torch.no_grad():
        ra = m.forward_masks(xa, packed=True).clone()
        rb = m.forward_masks(xb, packed=True).clone()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        sa.wait_stream(torch.cuda.current_stream())
        sb.wait_stream(torch.cuda.current_stream())
        outs = []
        for _ in range(3):
            with torch.cuda.stream(sa):
                a = m.forward_masks(xa, packed=True)
            with torch.cuda.stream(sb):
                b = m.forward_masks(xb, packed=True)
            outs.append((a, b))
        torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, ra) and torch.equal(b, rb)
    m.close()


def test_graph_replay_equals_eager():
    """unet_graph_create / unet_graph_launch (the hipGraph-captured forward, batch 1 and 4)
    produce bitwise the eager forward's logits, masks and boxes; a weight reload makes the graph
    stale (UNET_ESTATE) instead of replaying freed pointers."""
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    m = make_model(sd, 3, "mixed")
    h = m.native_handle(torch.device(DEV))
    stream = torch.cuda.current_stream().cuda_stream
    for n in (1, 4):
        x = torch.from_numpy(syn.invoice_pages(40 + n, n, 512, 512, 3)).to(DEV)
        lg = torch.empty((n, 3, 512, 512), device=DEV)
        mk = torch.empty((n, 3, 512, 64), dtype=torch.uint8, device=DEV)
        bx = torch.empty((n, 3, 4), dtype=torch.int32, device=DEV)
        h.reserve(n, 512, 512)
        h.forward_boxes(x, lg, mk, native.MASK_BITS, bx, stream)
        ref = (lg.clone(), mk.clone(), bx.clone())
        g = h.graph(x, lg, mk, native.MASK_BITS, boxes=bx)
        for t in (lg, mk, bx):
            t.zero_()
        for _ in range(3):
            g.launch(stream)
        torch.cuda.synchronize()
        assert torch.equal(lg, ref[0]) and torch.equal(mk, ref[1]) and torch.equal(bx, ref[2])
    h.load_weights(m.state_dict())
    with pytest.raises(RuntimeError, match="stale"):
        g.launch(stream)
    g.close()
    m.close()


def test_rccl_allgather_c_abi_single_rank():
    """unet_comm_init + unet_allgather (the C-ABI's RCCL all-gather of per-rank masks, SURVEY
    §8b) on a one-rank communicator: the gathered buffer is the rank's masks, stream-ordered
    after the forward that produced them."""
    m = make_model(syn.make_state_dict(0, 3, 3, profile="pretrained"), 3, "mixed")
    h = m.native_handle(torch.device(DEV))
    x = torch.from_numpy(syn.invoice_pages(9, 2, 512, 512, 3)).to(DEV)
    with torch.no_grad():
        ref = m.forward_masks(x, packed=True).clone()
    h.comm_init(0, 1, native.Handle.comm_unique_id())
    masks = torch.empty_like(ref)
    out = torch.zeros_like(ref)
    stream = torch.cuda.current_stream().cuda_stream
    h.forward(x, None, masks, native.MASK_BITS, stream)
    h.allgather(masks, out, stream)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match="recv"):   # a short recv buffer is refused, not overrun
        h.allgather(masks, out[:1], stream)
    h.comm_destroy()
    m.close()


def test_u8_nhwc_input_equals_f32_nchw():
    """unet_forward's other input formats (include/unet_mi355x.h): uint8 NHWC photos (value/255)
    give bitwise the result of the same values as fp32 NCHW, on the 16-bit and the fp32 path."""
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (2, 128, 96, 3), dtype=np.uint8)
    f32 = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    sd = syn.make_state_dict(0, 3, 3, profile="structured")
    for dtype in ("mixed", "fp32"):
        m = make_model(sd, 3, dtype)
        h = m.native_handle(torch.device(DEV))
        stream = torch.cuda.current_stream().cuda_stream
        h.reserve(2, 128, 96)
        outs = []
        for x, layout in ((torch.from_numpy(f32).to(DEV), native.LAYOUT_NCHW),
                          (torch.from_numpy(u8).to(DEV), native.LAYOUT_NHWC),
                          (torch.from_numpy(f32.transpose(0, 2, 3, 1).copy()).to(DEV), native.LAYOUT_NHWC)):
            lg = torch.empty((2, 3, 128, 96), device=DEV)
            h.forward(x, lg, None, native.MASK_NONE, stream, layout=layout)
            outs.append(lg)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), dtype
        m.close()


def test_u8_nhwc_input_with_unfused_first_layer(monkeypatch):
    """a 16-bit handle whose down1.3 is overridden to a non-fused configuration converts
    a uint8 NHWC input to fp32 NCHW (12 B per pixel) inside the workspace; the buffer must hold it
    (it was sized 8 B per pixel) and the result must equal the fp32 NCHW input's bitwise."""
    monkeypatch.setenv("UNET_MI355X_CFG", "0:10")   # CFG_RING8_R64_WS: the unfused weight-stationary ring
    rng = np.random.default_rng(6)
    u8 = rng.integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)
    f32 = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2))
    sd = syn.make_state_dict(0, 3, 3, profile="structured")
    m = make_model(sd, 3, "mixed")
    h = m.native_handle(torch.device(DEV))
    assert not h.launch_labels()[0].startswith("x_to_px4")
    stream = torch.cuda.current_stream().cuda_stream
    h.reserve(3, 64, 96)
    lg = [torch.empty((3, 3, 64, 96), device=DEV) for _ in range(2)]
    h.forward(torch.from_numpy(u8).to(DEV), lg[0], None, native.MASK_NONE, stream, layout=native.LAYOUT_NHWC)
    h.forward(torch.from_numpy(f32).to(DEV), lg[1], None, native.MASK_NONE, stream)
    torch.cuda.synchronize()
    assert torch.equal(lg[0], lg[1])
    ref = orc.unet_forward(sd, torch.from_numpy(f32)).numpy()
    assert rel_err(lg[0].cpu().numpy(), ref) <= TOL["mixed"]
    m.close()


def test_fp16_range_refused_at_load():
    """fp16 storage holds |v| <= 65504.  A checkpoint whose BN fold leaves a conv weight
    beyond that at an fp16 level (here a running_var of 1e-12 at down1.3: scale ~316 x gamma) is
    refused by the fp16 / mixed plans (ValueError) instead of producing inf; bf16 and fp32 load it."""
    sd = syn.make_state_dict(0, 3, 3, profile="structured")
    sd["down1.net.4.weight"] = np.full_like(np.asarray(sd["down1.net.4.weight"]), 1e5)
    sd["down1.net.4.running_var"] = np.full_like(np.asarray(sd["down1.net.4.running_var"]), 1e-12)
    x = torch.from_numpy(syn.uniform_batch(1, 1, 3, 32, 32)).to(DEV)
    for dtype in ("fp16", "mixed"):
        m = make_model(sd, 3, dtype)
        with pytest.raises(ValueError, match="fp16 range"), torch.no_grad():
            m(x)
        m.close()
    for dtype in ("bf16", "fp32"):
        m = make_model(sd, 3, dtype)
        with torch.no_grad():
            m(x)
        m.close()
    # the 16-bit head rounds the out_conv weights to conv1.3's type, so they are checked too
    sd = syn.make_state_dict(0, 3, 3, profile="structured")
    sd["out_conv.weight"] = np.full_like(np.asarray(sd["out_conv.weight"]), 1e5)
    for dtype, refused in (("fp16", True), ("mixed", True), ("bf16", False)):
        m = make_model(sd, 3, dtype)
        if refused:
            with pytest.raises(ValueError, match="out_conv"), torch.no_grad():
                m(x)
        else:
            with torch.no_grad():
                m(x)
        m.close()


def test_torch_graph_capture_on_side_stream():
    """torch.cuda.graph captures on its own side stream, after eager forwards on the
    default stream; the library must not wait on (or record) its stream-order event inside the
    capture.  The replayed masks equal the eager ones."""
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    m = make_model(sd, 3, "mixed")
    x = torch.from_numpy(syn.invoice_pages(61, 2, 256, 256, 3)).to(DEV)
    m.reserve(2, 256, 256)
    with torch.no_grad():
        ref = m.forward_masks(x, packed=True).clone()       # eager, default stream: the event is pending
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m.forward_masks(x, packed=True)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m.forward_masks(x, packed=True)
        out.zero_()
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, ref)
    with torch.no_grad():   # the handle is usable eagerly afterwards
        assert torch.equal(m.forward_masks(x, packed=True), ref)
    del g
    m.close()


def test_bf16_cast_model_loads():
    """a UNet cast with .to(torch.bfloat16) still loads (its parameters are read back
    in fp32, as the reference module's would be) and gives the fp32-weights result of that cast."""
    sd = syn.make_state_dict(0, 3, 3, profile="structured")
    m = make_model(sd, 3, "bf16").to(torch.bfloat16)
    x = torch.from_numpy(syn.uniform_batch(1, 1, 3, 32, 32)).to(DEV)
    with torch.no_grad():
        out = m(x)
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    m.close()


def test_errors_and_no_fallback():
    m = make_model(syn.make_state_dict(0, 3, 3), 3, "bf16")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 40, 32, device=DEV))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 32, 32, device=DEV))
    h = m.native_handle(torch.device(DEV))   # forwards never allocate: an unreserved shape is refused
    x = torch.zeros(64, 3, 512, 512, device=DEV)
    with pytest.raises(RuntimeError, match="unet_reserve"):
        h.forward(x, None, torch.empty((64, 3, 512, 64), dtype=torch.uint8, device=DEV), native.MASK_BITS,
                  torch.cuda.current_stream().cuda_stream)
    m.close()


def test_weight_update_repacks():
    """Parameter changes re-pack the handle: in-place updates, a replaced Parameter object, and a
    .to() round trip (the cached signature tensors are rebuilt on re-registration / conversion)."""
    sd = syn.make_state_dict(4, 3, 3)
    m = make_model(sd, 3, "fp32")
    x = torch.from_numpy(syn.uniform_batch(1, 1, 3, 32, 32)).to(DEV)
    with torch.no_grad():
        a = m(x).clone()
        m.out_conv.bias.add_(1.0)
        b = m(x).clone()
        m.out_conv.bias = torch.nn.Parameter(m.out_conv.bias.detach() + 1.0)
        c = m(x).clone()
        m.to("cpu")
        m.out_conv.bias.add_(1.0)
        m.to(DEV)
        d = m(x)
    assert torch.allclose(b - a, torch.ones_like(a), atol=1e-4)
    assert torch.allclose(c - b, torch.ones_like(a), atol=1e-4)
    assert torch.allclose(d - c, torch.ones_like(a), atol=1e-4)
    m.close()


@pytest.mark.parametrize("cfg", HALO_CFGS + RING_CFGS)
def test_every_kernel_config(cfg, monkeypatch):
    """Each 3x3 configuration (csrc/unet_internal.h Cfg) forced on every layer it supports,
    checked against the reference golden (the exact-fp32 plan and bf16; the three-term fp32 plan has one
    configuration of its own, tested everywhere else)."""
    monkeypatch.setenv("UNET_MI355X_CFG", ",".join(f"{i}:{cfg}" for i in range(17)))
    z = np.load(os.path.join(GOLD, "unet_c3_h64w64_n2_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    for dtype in ("fp32_exact", "bf16"):
        m = make_model(sd, 3, dtype)
        with torch.no_grad():
            out = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
        err = rel_err(out, z["logits"])
        print(f"cfg {cfg} {dtype}: rel err {err:.3e}")
        assert err <= TOL[dtype]
        m.close()


@pytest.mark.parametrize("cfg", UP_CFGS)
def test_convtranspose_configs(cfg, monkeypatch):
    """ConvTranspose2d (up4..up1) on every supported kernel configuration vs the golden (up1 as
    its own launch, not fused into conv2.3)."""
    monkeypatch.setenv("UNET_MI355X_UPCFG", ",".join(f"{i}:{cfg}" for i in range(4)))
    monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    z = np.load(os.path.join(GOLD, "unet_c3_h16w16_n3_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    for dtype in ("fp32_exact", "bf16"):
        m = make_model(sd, 3, dtype)
        with torch.no_grad():
            out = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
        for name, key in (("u1", "inter_u1_up"), ("u4", "inter_u4_up")):
            ref = z[key]
            got = m.intermediate(name).cpu().numpy().reshape(ref.shape)
            assert rel_err(got, ref) <= TOL[dtype], (cfg, dtype, name)
        assert rel_err(out, z["logits"]) <= TOL[dtype]
        m.close()


INTER = ["c1", "p1", "c2", "p2", "c3", "p3", "c4", "p4", "bn", "u4", "u3", "u2", "c7", "u1", "c8a"]


def _forward_state(m, x):
    with torch.no_grad():
        lg = m(x)
    torch.cuda.synchronize()
    out = {}
    for k in INTER:
        try:
            out[k] = m.intermediate(k).clone()
        except RuntimeError:   # c7 with up1 fused into conv2.3: never stored
            assert k == "c7"
    out["logits"] = lg.clone()
    return out


def _first_diff(a, b):
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k], b[k])]


def _forced(cfg, up, sd, x, dtype, monkeypatch):
    """Configuration families compared unfused: the fused conv2.3 + up1 launch accumulates the
    ConvTranspose in another K order than the up1 kernel (test_fused_up1_matches_unfused)."""
    monkeypatch.setenv("UNET_MI355X_CFG", ",".join(f"{i}:{cfg}" for i in range(17)) if cfg is not None else "")
    monkeypatch.setenv("UNET_MI355X_UPCFG", ",".join(f"{i}:{up}" for i in range(4)) if up is not None else "")
    monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    # families compared on the unsplit kernels: the small-batch split-K plan (N = 2 here) picks its
    # slice count from each configuration's tile grid
    monkeypatch.setenv("UNET_MI355X_KSPLIT", "0")
    m = make_model(sd, 3, dtype)
    st = _forward_state(m, x)
    m.close()
    monkeypatch.delenv("UNET_MI355X_KSPLIT")
    return st


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "mixed"])
def test_forward_deterministic_and_config_invariant(dtype, monkeypatch):
    """Full-size pages (persistent kernels walk several tiles per block, rings wrap): repeated
    forwards are bitwise identical, and within each kernel family every configuration --
    forced on all 3x3 layers, or on all ConvTranspose layers -- gives bitwise the same
    activations: the 128-byte LDS-halo configurations (K order chunk64-major / tap-minor) agree
    with each other, the 64-byte ring configurations (chunk32-major; 5 = down1.0 fused) agree
    with each other within the 4-wave ring (3-5) and within the 8-wave ring (8-11), and the two
    ConvTranspose ring configurations (6, 7) agree with each other (the LDS-halo ConvTranspose, 2,
    starts its accumulators at zero, the rings at the bias: checked against the reference in
    test_convtranspose_configs).  A missed
    wait in a DMA ring shows up here as a run-to-run or config-to-config difference."""
    x = torch.from_numpy(syn.invoice_pages(3, 2, 512, 512, 3)).to(DEV)
    sd = syn.make_state_dict(3, 3, 3, profile="structured")
    m = make_model(sd, 3, dtype)
    base = _forward_state(m, x)
    for r in range(2):
        assert _first_diff(_forward_state(m, x), base) == [], f"run {r + 1} differs"
    m.close()
    if dtype == "mixed":
        return
    bad = []
    for family in (HALO_CFGS, RING4_CFGS, RING8_CFGS):
        fbase = _forced(family[0], None, sd, x, dtype, monkeypatch)
        for cfg in family[1:]:
            d = _first_diff(_forced(cfg, None, sd, x, dtype, monkeypatch), fbase)
            if d:
                bad.append((cfg, None, d[:3]))
    ubase = _forced(None, UP_RING_CFGS[0], sd, x, dtype, monkeypatch)
    for up in UP_RING_CFGS[1:]:
        d = _first_diff(_forced(None, up, sd, x, dtype, monkeypatch), ubase)
        if d:
            bad.append((None, up, d[:3]))
    print(bad)
    assert bad == []


@pytest.mark.parametrize("dtype", ["mixed", "bf16", "fp16"])
def test_fused_up1_matches_unfused(dtype, monkeypatch):
    """conv2.3 + up1 in one launch (EPI_UPFUSE, the 16-bit default) vs the two launches: the same
    products, only the ConvTranspose's fp32 accumulation order differs (its K order follows the
    conv accumulators' lanes), so u1 agrees to a few 16-bit ulps and the logits / masks agree; the
    fused run is bitwise repeatable.  Full-size pages (the persistent walker wraps) and a ragged
    shape (partial tiles at 24 x 40)."""
    sd = syn.make_state_dict(3, 3, 3, profile="structured")
    for n, h, w in ((2, 512, 512), (3, 48, 80)):
        x = torch.from_numpy(syn.invoice_pages(5, n, h, w, 3)).to(DEV)
        st = {}
        for fuse in ("1", "0"):
            monkeypatch.setenv("UNET_MI355X_FUSE_UP1", fuse)
            m = make_model(sd, 3, dtype)
            st[fuse] = _forward_state(m, x)
            labels = m.native_handle(torch.device(DEV)).launch_labels()
            assert (labels[19] == "") == (fuse == "1"), labels[19]   # up1's slot: fused -> no launch
            if fuse == "1":
                epi_arg = 3 if labels[18].startswith("conv3x3_ring8_kernel") else 5
                assert labels[18].split(",")[epi_arg].strip() == "4", labels[18]   # conv2.3: EPI_UPFUSE
                assert "c7" not in st[fuse]
                assert _first_diff(_forward_state(m, x), st[fuse]) == []
            m.close()
        u_f, u_u = st["1"]["u1"].float(), st["0"]["u1"].float()
        du = rel_err(u_f.cpu().numpy(), u_u.cpu().numpy())
        dl = rel_err(st["1"]["logits"].cpu().numpy(), st["0"]["logits"].cpu().numpy())
        print(f"{dtype} {n}x{h}x{w}: u1 rel diff {du:.2e}, logits rel diff {dl:.2e}")
        assert du <= (1e-2 if dtype == "bf16" else 2e-3)
        assert dl <= TOL[dtype]


def _np_boxes(masks):
    """[N, C, H, W] bool -> int32 [N, C, 4] (x_min, y_min, x_max, y_max), -1s if empty."""
    out = np.full(masks.shape[:2] + (4,), -1, dtype=np.int32)
    for i in range(masks.shape[0]):
        for c in range(masks.shape[1]):
            ys, xs = np.where(masks[i, c])
            if len(xs):
                out[i, c] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


@pytest.mark.parametrize("kind", [None, "u8", "bits"])
def test_mask_boxes_match_numpy(kind):
    """Device per-(image, field) boxes (unet_forward_boxes) == np.where min/max of the masks the
    same forward produced (inference.py:84-90), with and without caller mask buffers; empty
    masks (torch_default weights: logits ~ -4) give -1s; W = 48 exercises a 16-bit word row;
    1280 x 1024 has more 1024-word strips than blocks per mask (blocks loop).  Every handle runs
    three forwards (page, mirrored page, page again): the strips' sync entries must be back in
    their idle state after each launch."""
    cases = [(syn.make_state_dict(0, 3, 3, "pretrained"), syn.invoice_pages(1000, 2, 512, 512, 3)),
             (syn.make_state_dict(1, 3, 3, "torch_default"), syn.invoice_pages(2, 1, 64, 64, 3)),
             (syn.make_state_dict(5, 3, 3, "structured", out_bias=0.0), syn.uniform_batch(3, 3, 3, 32, 48)),
             (syn.make_state_dict(0, 3, 3, "pretrained"), syn.invoice_pages(3, 1, 1280, 1024, 3))]
    for sd, x in cases:
        m = make_model(sd, 3, "mixed")
        for xd in (torch.from_numpy(x).to(DEV), torch.from_numpy(x[..., ::-1].copy()).to(DEV),
                   torch.from_numpy(x).to(DEV)):
            with torch.no_grad():
                ref_masks = m.forward_masks(xd).cpu().numpy().astype(bool)
                got = m.forward_boxes(xd, masks=kind)
            boxes = (got if kind is None else got[1]).cpu().numpy()
            assert np.array_equal(boxes, _np_boxes(ref_masks))
            if kind is not None:
                mk = got[0].cpu().numpy()
                if kind == "bits":
                    mk = np.unpackbits(mk, axis=-1, bitorder="little")
                assert np.array_equal(mk.astype(bool), ref_masks)
        m.close()


def test_config5_1024_fp16():
    """BASELINE config 5 shape (1024x1024, 3 channels, 5 resolution levels, fp16 storage with
    fp32 accumulation) against the REFERENCE's own forward of a 1024x1024 page on the trained-like
    weights (tests/golden/pretrained_1024_page.npz): 1/8-subsampled logits within TOL["fp16"] and
    fused masks at north_star's IoU >= 0.999; a batch of 3 agrees with the single-image forward
    bitwise (no cross-image coupling)."""
    z = np.load(os.path.join(GOLD, "pretrained_1024_page.npz"))
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    assert syn.state_dict_checksum(sd) == str(z["sd_sha256"])
    x = np.repeat(z["page_u8"][None, None].astype(np.float32) / 255.0, 3, axis=1)
    ref_masks = _ref_maskbits(z, "")
    m = make_model(sd, 3, "fp16")
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        bits, logits = m.forward_masks(xd, packed=True, with_logits=True)
        x3 = torch.cat([torch.from_numpy(syn.invoice_pages(7, 1, 1024, 1024, 3)).to(DEV), xd,
                        torch.from_numpy(syn.uniform_batch(2, 1, 3, 1024, 1024)).to(DEV)])
        lg3 = m(x3)
    err = rel_err(logits.cpu().numpy()[0][:, ::8, ::8], z["logits_sub8"])
    got = np.unpackbits(bits.cpu().numpy()[0], axis=-1, bitorder="little").astype(bool)
    ious = [orc.mask_iou(got[k], ref_masks[k]) for k in range(3)]
    print(f"1024x1024 fp16 vs reference: logits rel err {err:.3e}, mask IoU {ious}")
    assert err <= TOL["fp16"]
    assert min(ious) >= 0.999
    assert torch.equal(lg3[1:2], logits)
    m.close()


def _ref_maskbits(z, suffix):
    """[3, H, W] bool masks the reference produced (bit-packed in the fixture)."""
    return np.stack([np.unpackbits(z[f"maskbits_{k}{suffix}"], axis=-1, bitorder="little").astype(bool)
                     for k in orc.FIELDS])


def _embed_reference_pages(base, positions):
    """The 4 reference pages of pretrained_512_pages.npz (u8 / 255, gray x3) written into the
    batch `base` [N, 3, 512, 512] at `positions`; returns (batch, fixture)."""
    z = np.load(os.path.join(GOLD, "pretrained_512_pages.npz"))
    pages = np.repeat(z["pages_u8"][:, None].astype(np.float32) / 255.0, 3, axis=1)
    x = base.copy()
    for j, i in enumerate(positions):
        x[i] = pages[j]
        assert hashlib.sha256(x[i:i + 1].tobytes()).hexdigest() == str(z[f"x_sha256_{j}"])
    return x, z


def _check_against_reference_pages(bits, logits, z, positions, dtype, min_iou):
    ious, errs = [], []
    for j, i in enumerate(positions):
        got = np.unpackbits(bits[i], axis=-1, bitorder="little").astype(bool)
        ref = _ref_maskbits(z, f"_{j}")
        ious += [orc.mask_iou(got[k], ref[k]) for k in range(3)]
        if logits is not None:
            errs.append(rel_err(logits[i][:, ::8, ::8], z[f"logits_sub8_{j}"]))
    print(f"{dtype} vs reference pages {list(positions)}: mask IoU min {min(ious):.5f} mean {np.mean(ious):.5f}"
          + (f", logits rel err max {max(errs):.3e}" if errs else ""))
    assert min(ious) >= min_iou
    if errs:
        assert max(errs) <= TOL[dtype]


def test_reference_pages_in_bs256_mixed_batch():
    """The headline shape pinned to the REFERENCE: 4 pages whose masks the
    reference's run_unet produced on the trained-like weights (make_golden.pretrained_cases) sit
    at positions 0, 77, 128, 255 of the bench's 256-page batch; the bench plan (mixed, bit-packed
    masks, the timed kernels) meets north_star's IoU >= 0.999 against the reference's masks, and
    its logits sit within TOL["mixed"] of the reference's."""
    import bench
    pos = (0, 77, 128, 255)
    x, z = _embed_reference_pages(bench.gen_pages(1000, 256, 512, 3, unique=64), pos)
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    assert syn.state_dict_checksum(sd) == str(z["sd_sha256"])
    m = make_model(sd, 3, "mixed")
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        bits = m.forward_masks(xd, packed=True)
        bits2, logits = m.forward_masks(xd, packed=True, with_logits=True)
    assert torch.equal(bits, bits2), "masks with and without the logits output differ"
    _check_against_reference_pages(bits.cpu().numpy(), logits.cpu().numpy(), z, pos, "mixed", 0.999)
    m.close()


def test_reference_pages_in_bs32_fp32_batch_and_batch_invariance(monkeypatch):
    """BASELINE config 2's shape at the drop-in's default precision (fp32, batch 32), pinned to the
    reference: the 4 reference pages at positions 0, 9, 20, 31 of the fp32 leg's batch meet IoU >=
    0.9999 and the fp32 logit tolerance; and every image of the N = 32 forward equals the same image
    run alone (N = 1) bit for bit (the small-batch split-K plan off: it is another accumulation order,
    test_small_batch_split_k_plan)."""
    import bench
    monkeypatch.setenv("UNET_MI355X_KSPLIT", "0")
    pos = (0, 9, 20, 31)
    x, z = _embed_reference_pages(bench.gen_pages(2000, 32, 512, 3), pos)
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    m = make_model(sd, 3, "fp32")
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        bits, logits = m.forward_masks(xd, packed=True, with_logits=True)
        bits, logits = bits.clone(), logits.clone()
        for i in range(32):
            b1, l1 = m.forward_masks(xd[i:i + 1].contiguous(), packed=True, with_logits=True)
            assert torch.equal(b1, bits[i:i + 1]) and torch.equal(l1, logits[i:i + 1]), f"image {i}: N=1 != N=32"
    _check_against_reference_pages(bits.cpu().numpy(), logits.cpu().numpy(), z, pos, "fp32", 0.9999)
    m.close()


@pytest.mark.parametrize("h,w,c", [(400, 600, 3), (1333, 1000, 3), (200, 300, 3), (700, 512, 3),
                                   (512, 900, 3), (512, 512, 3), (390, 517, 1), (37, 23, 3), (3024, 4032, 3)])
def test_preprocess_bit_exact_with_pillow(h, w, c):
    """unet_preprocess (GPU) == PIL Image.resize((512, 512)) (default BICUBIC) + convert("RGB")
    + /255, bit for bit: down / up / one-axis / identity geometries, RGB and L, a 12 MP photo; and the
    same RGB photos uploaded as RGBX (Pillow's in-memory layout, run_unet's upload) with a random 4th
    byte, which must be ignored."""
    from PIL import Image
    rng = np.random.default_rng(h + 3 * w)
    arr = rng.integers(0, 256, (h, w, 3) if c == 3 else (h, w), dtype=np.uint8)
    if h == 3024:   # smooth photo-like content (strong low-pass response, clip8 at both ends)
        yy, xx = np.mgrid[0:h, 0:w]
        arr = (127.5 + 127.5 * (np.sin(yy / 37.0) * np.cos(xx / 53.0))[..., None] + rng.normal(0, 20, (h, w, 3))
               ).clip(0, 255).astype(np.uint8)
    pil = Image.fromarray(arr)
    ref = np.array(pil.resize((512, 512)).convert("RGB")).astype(np.float32) / 255.0
    m = make_model(syn.make_state_dict(0, 3, 3), 3, "bf16")
    got = m.preprocess(torch.from_numpy(arr).to(DEV)).cpu().numpy()[0]
    assert got.shape == (3, 512, 512)
    assert np.array_equal(got, ref.transpose(2, 0, 1))
    if c == 3:
        rgbx = np.concatenate([arr, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
        got4 = m.preprocess(torch.from_numpy(rgbx).to(DEV)).cpu().numpy()[0]
        assert np.array_equal(got4, got)
    if h < 2000:   # the numpy restatement agrees too (checker of the checker)
        from oracle import pil_resample as pr
        assert np.array_equal(got, pr.to_input(arr))
    m.close()


def test_preprocess_geometry_cache_is_bounded():
    """the per-geometry resize tables live in a bounded LRU; 20 distinct photo sizes
    (more than the cache holds) still resize bit-exactly, including a geometry revisited after
    its eviction."""
    from PIL import Image
    m = make_model(syn.make_state_dict(0, 3, 3), 3, "bf16")
    rng = np.random.default_rng(2)
    sizes = [(100 + 7 * i, 120 + 5 * i) for i in range(20)] + [(100, 120)]
    for h, w in sizes:
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.array(Image.fromarray(arr).resize((512, 512))).astype(np.float32) / 255.0
        got = m.preprocess(torch.from_numpy(arr).to(DEV)).cpu().numpy()[0]
        assert np.array_equal(got, ref.transpose(2, 0, 1)), (h, w)
    m.close()


@pytest.mark.parametrize("pillow", ["current", "pillow_10_2"])
def test_run_unet_boundary_matches_reference_golden(pillow, monkeypatch):
    """inference.run_unet (drop-in) on the golden 600x400 photo vs the reference's masks/crops.
    "pillow_10_2": the reference's pinned Pillow (requirements.txt:3) has no Arrow export, and the photo is
    packed by plain np.asarray (no raw-encoder pass), so run_unet's photo graph takes the packed-photo path
    (3 bytes per pixel) -- same masks and crops."""
    from PIL import Image
    from unet_mi355x import inference as inf
    if pillow == "pillow_10_2":
        monkeypatch.setattr(inf, "copy_rgbx", lambda *a, **k: None)          # no Arrow export
        monkeypatch.setattr(inf, "photo_array", lambda im: np.asarray(im))   # the plain packing, no raw-encoder pass
        calls = []
        real_stage = inf._Staging.stage
        monkeypatch.setattr(inf._Staging, "stage", lambda self, arr: calls.append(arr.shape) or real_stage(self, arr))
    z = np.load(os.path.join(GOLD, "run_unet_600x400.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile="structured")
    sd["out_conv.bias"] = sd["out_conv.bias"] + z["out_bias_delta"]
    assert syn.state_dict_checksum(sd) == str(z["sd_sha256"])
    pil = Image.fromarray(z["image"], mode="RGB")
    with tempfile.TemporaryDirectory() as td:
        ck = os.path.join(td, "best_unet_model.pth")
        torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ck)
        inf.DEVICE = DEV
        masks, crops = inf.run_unet(pil, ck, compute_dtype="fp32")
    if pillow == "pillow_10_2":
        assert calls == [(400, 600, 3)]   # the packed photo went through the graph, not the RGBX export
    for k in inf.FIELDS:
        ref = np.unpackbits(z["maskbits_" + k], axis=-1, bitorder="little").astype(bool)
        iou = orc.mask_iou(masks[k], ref)
        print(f"run_unet {k}: IoU {iou:.6f}, differing pixels {int((masks[k] != ref).sum())}")
        assert iou >= 0.999
        # the crop rules (inference.py:92-127) applied to the box of the REFERENCE's mask reproduce
        # its crop byte for byte; our own crop must too whenever our mask has the same box (a mask
        # pixel off inside the box changes nothing downstream)
        ref_box = _np_box(ref)
        from_ref = inf.crop_from_box(pil, ref_box)
        if bool(z["crop_none_" + k]):
            assert crops[k] is None and from_ref is None
            continue
        want = str(z["crop_sha256_" + k])
        assert hashlib.sha256(np.asarray(from_ref).tobytes()).hexdigest() == want
        arr = np.asarray(crops[k])
        assert list(arr.shape) == list(z["crop_shape_" + k])
        if _np_box(masks[k]) == ref_box:
            assert hashlib.sha256(arr.tobytes()).hexdigest() == want, k
        else:
            print(f"run_unet {k}: box {_np_box(masks[k])} vs reference {ref_box}")


def _np_box(mask):
    """inference.py:84-90: np.where -> (x_min, y_min, x_max, y_max), None for an empty mask."""
    ys, xs = np.where(mask)
    return None if len(xs) == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


@pytest.mark.parametrize("h,w,c", [(400, 600, 3), (700, 300, 1), (3024, 4032, 3), (23, 37, 3)])
def test_crop_stats_match_host_crop_rules(h, w, c):
    """unet_crop_stats (device) == the reference's crop arithmetic (inference.py:92-127, restated
    by inference.crop_rect) and numpy's crop pixel sums, for empty / 1-pixel / border / whole-mask /
    random boxes; and crop_from_stats on them == crop_from_box (incl. the near-black rejection, on
    a dark photo whose crop means straddle 3)."""
    from PIL import Image
    from unet_mi355x import inference as inf, native
    rng = np.random.default_rng(h * 7 + w)
    for dark in (False, True):
        arr = rng.integers(0, 7 if dark else 256, (h, w, c) if c == 3 else (h, w), dtype=np.uint8)
        pil = Image.fromarray(arr)
        boxes = [(-1, -1, -1, -1), (0, 0, 0, 0), (511, 511, 511, 511), (0, 0, 511, 511), (3, 500, 9, 511)]
        for _ in range(59):
            x0, y0 = rng.integers(0, 512, 2)
            boxes.append((x0, y0, min(511, x0 + rng.integers(0, 200)), min(511, y0 + rng.integers(0, 200))))
        b = torch.tensor(np.array(boxes, dtype=np.int32)).to(DEV)
        rects = torch.empty((len(boxes), 4), dtype=torch.int32, device=DEV)
        sums = torch.empty((len(boxes),), dtype=torch.int64, device=DEV)
        img = torch.from_numpy(arr.reshape(h, w, c)).to(DEV)
        native.crop_stats(img, b, 512, 512, inf.CROP_PAD, rects, sums, torch.cuda.current_stream().cuda_stream)
        if c == 3:   # the RGBX upload: the same rectangles and sums over R, G, B (the 4th byte ignored)
            img4 = torch.from_numpy(np.concatenate([arr, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)).to(DEV)
            r4, s4 = torch.empty_like(rects), torch.empty_like(sums)
            native.crop_stats(img4, b, 512, 512, inf.CROP_PAD, r4, s4, torch.cuda.current_stream().cuda_stream)
            assert torch.equal(r4, rects) and torch.equal(s4, sums)
        for off in (1, 3):   # a photo not 4-byte aligned (the kernel walks aligned words and masks the ends)
            for img_u in (img, img4 if c == 3 else None):
                if img_u is None:
                    continue
                blk = torch.empty(img_u.numel() + 8, dtype=torch.uint8, device=DEV)
                v = blk[off:off + img_u.numel()].view(img_u.shape)
                v.copy_(img_u)
                ru, su = torch.empty_like(rects), torch.empty_like(sums)
                native.crop_stats(v, b, 512, 512, inf.CROP_PAD, ru, su, torch.cuda.current_stream().cuda_stream)
                assert torch.equal(ru, rects) and torch.equal(su, sums), off
        rects, sums = rects.cpu().numpy(), sums.cpu().numpy()
        for i, box in enumerate(boxes):
            if box[2] < 0:
                assert tuple(rects[i]) == (-1, -1, -1, -1)
                want = None
            else:
                r = inf.crop_rect(box, w, h)
                assert tuple(int(v) for v in rects[i]) == r, (box, rects[i], r)
                assert int(sums[i]) == int(arr[r[1]:r[3], r[0]:r[2]].astype(np.int64).sum()), box
                want = inf.crop_from_box(pil, box)
            got = inf.crop_from_stats(pil, rects[i], sums[i], c)
            assert (got is None) == (want is None), (box, dark)
            if got is not None:
                assert np.array_equal(np.asarray(got), np.asarray(want))


def test_run_unet_batch_equals_per_photo_calls():
    """inference.run_unet_batch (one forward over N photos of mixed sizes / modes) returns, for
    every photo, exactly run_unet's masks and crops."""
    from PIL import Image
    from unet_mi355x import inference as inf
    rng = np.random.default_rng(9)
    pages = syn.invoice_pages(1000, 3, 512, 512, 1)
    photos = [Image.fromarray((pages[0, 0] * 255).astype(np.uint8)).resize((600, 400)).convert("RGB"),
              Image.fromarray((pages[1, 0] * 255).astype(np.uint8)).resize((300, 700)),            # mode L
              Image.fromarray(rng.integers(0, 256, (333, 517, 4), dtype=np.uint8), mode="RGBA")]  # host path
    sd = syn.make_state_dict(0, 3, 3, "pretrained")
    with tempfile.TemporaryDirectory() as td:
        ck = os.path.join(td, "best_unet_model.pth")
        torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ck)
        inf.DEVICE = DEV
        single = [inf.run_unet(p, ck, compute_dtype="mixed") for p in photos]
        batch = inf.run_unet_batch(photos, ck, compute_dtype="mixed")
    assert len(batch) == len(photos)
    for (m1, c1), (m2, c2) in zip(single, batch):
        for k in inf.FIELDS:
            assert np.array_equal(m1[k], m2[k]), k
            assert (c1[k] is None) == (c2[k] is None), k
            if c1[k] is not None:
                assert np.array_equal(np.asarray(c1[k]), np.asarray(c2[k])), k


@pytest.mark.parametrize("dtype", ["fp32", "mixed", "bf16"])
def test_small_batch_split_k_plan(dtype, monkeypatch):
    """The small-batch plan (csrc/unet_capi.cpp layer_split: the deep layers whose tile grid under-fills
    the 256 CUs at N <= 4 run as K slices into fp32 partials + a slice-ordered reduction): engaged at
    N = 1 (its partial buffer enlarges the workspace), bitwise repeatable, bitwise the same image at N =
    1, 3 and 4 (the slice counts depend on the layer only), pinned to the reference masks and logits of
    the trained-like pages (pretrained_512_pages.npz), and within TOL of the unsplit kernels
    (UNET_MI355X_KSPLIT=0)."""
    z = np.load(os.path.join(GOLD, "pretrained_512_pages.npz"))
    x = torch.from_numpy(np.repeat(z["pages_u8"][:, None].astype(np.float32) / 255.0, 3, axis=1)).to(DEV)
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    monkeypatch.setenv("UNET_MI355X_KSPLIT", "0")
    m0 = make_model(sd, 3, dtype)
    ws_unsplit = m0.native_handle(torch.device(DEV)).workspace_bytes(1, 512, 512)
    with torch.no_grad():
        lg_unsplit = m0(x[:1]).cpu().numpy()
    m0.close()
    monkeypatch.delenv("UNET_MI355X_KSPLIT")
    m = make_model(sd, 3, dtype)
    h = m.native_handle(torch.device(DEV))
    assert h.workspace_bytes(1, 512, 512) > ws_unsplit, "no layer split at batch 1"
    with torch.no_grad():
        bits4, lg4 = m.forward_masks(x, packed=True, with_logits=True)
        bits4, lg4 = bits4.clone(), lg4.clone()
        b3, l3 = m.forward_masks(x[1:].contiguous(), packed=True, with_logits=True)
        assert torch.equal(b3, bits4[1:]) and torch.equal(l3, lg4[1:]), "N=3 != N=4"
        for i in range(4):
            b1, l1 = m.forward_masks(x[i:i + 1].contiguous(), packed=True, with_logits=True)
            assert torch.equal(b1, bits4[i:i + 1]) and torch.equal(l1, lg4[i:i + 1]), f"image {i}: N=1 != N=4"
        b1b, l1b = m.forward_masks(x[:1], packed=True, with_logits=True)
        assert torch.equal(l1b, lg4[:1]), "split-K forward not repeatable"
    err = rel_err(lg4[:1].cpu().numpy(), lg_unsplit)
    print(f"{dtype}: split vs unsplit logits rel err {err:.3e}")
    assert err <= TOL[dtype]
    _check_against_reference_pages(bits4.cpu().numpy(), lg4.cpu().numpy(), z, range(4), dtype,
                                   {"fp32": 0.9999, "mixed": 0.999, "bf16": 0.995}[dtype])
    m.close()


def test_product_configs_build_no_spilling_kernels(monkeypatch):
    """The configurations whose instantiation would spill (the fp32 128-row 8-wave ring, the pooled
    128-row 4-wave ring) are not built: a forced override lands on the 64-row tiles of the same family
    (csrc/unet_capi.cpp), so the labels name those and the forward matches the golden."""
    z = np.load(os.path.join(GOLD, "unet_c3_h64w64_n2_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    for cfg, dtype, want in ((8, "fp32_exact", "conv3x3_ring8_kernel<float, 4, 2,"),
                             (3, "bf16", "conv3x3_ring_kernel<__bf16, 1, 4, 4,"),
                             # the three-term fp32 plan runs only on its own tiles: split-once 128-row
                             # tiles where Cout >= 128 (down2.3), the pre-split 64-row halo tiles elsewhere
                             (8, "fp32", "conv3x3_x3s_kernel<1>")):
        monkeypatch.setenv("UNET_MI355X_CFG", ",".join(f"{i}:{cfg}" for i in range(17)))
        m = make_model(sd, 3, dtype)
        labels = m.native_handle(torch.device(DEV)).launch_labels()
        assert labels[3].startswith(want), (cfg, dtype, labels[3])     # down2.3, a pooled 128-channel layer
        with torch.no_grad():
            out = m(torch.from_numpy(z["x"]).to(DEV)).cpu().numpy()
        assert rel_err(out, z["logits"]) <= TOL[dtype]
        m.close()


def test_small_batch_convtranspose_halves_bitwise(monkeypatch):
    """The batch-1 plan's ConvTranspose on 128-row halves of the 256-row packing (up4, up3: the 4-wave
    128-row ring reading the 8-wave ring's packing, csrc/unet_capi.cpp layer_split) is bitwise the
    256-row ring: with the 3x3 layers forced unsplit (UNET_MI355X_KSPLIT_FORCE=i:1) the batch-1 forward
    equals the one with the whole small-batch plan off (UNET_MI355X_KSPLIT=0), u4, u3 and logits."""
    sd = syn.make_state_dict(0, 3, 3, profile="pretrained")
    x = torch.from_numpy(syn.invoice_pages(1000, 1, 512, 512, 3)).to(DEV)
    st = {}
    for name, env in (("halves", {"UNET_MI355X_KSPLIT_FORCE": ",".join(f"{i}:1" for i in range(17))}),
                      ("off", {"UNET_MI355X_KSPLIT": "0"})):
        for k in ("UNET_MI355X_KSPLIT_FORCE", "UNET_MI355X_KSPLIT"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = make_model(sd, 3, "mixed")
        with torch.no_grad():
            lg = m(x)
        torch.cuda.synchronize()
        st[name] = {"u4": m.intermediate("u4").clone(), "u3": m.intermediate("u3").clone(), "logits": lg.clone()}
        m.close()
    assert _first_diff(st["halves"], st["off"]) == []


def _photos(n, seed=21):
    from PIL import Image
    pages = syn.invoice_pages(seed, n, 512, 512, 1)
    sizes = [(600, 400), (300, 700), (517, 333), (640, 480), (400, 600), (1024, 768), (256, 256), (333, 517)]
    out = []
    for i in range(n):
        im = Image.fromarray((pages[i, 0] * 255).astype(np.uint8)).resize(sizes[i % len(sizes)])
        out.append(im if i % 3 == 1 else im.convert("RGB"))
    return out


def _save_ckpt(td, profile="pretrained"):
    sd = syn.make_state_dict(0, 3, 3, profile)
    ck = os.path.join(td, "best_unet_model.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ck)
    return ck


def _same_result(a, b, fields):
    (m1, c1), (m2, c2) = a, b
    for k in fields:
        assert np.array_equal(m1[k], m2[k]), k
        assert (c1[k] is None) == (c2[k] is None), k
        if c1[k] is not None:
            assert np.array_equal(np.asarray(c1[k]), np.asarray(c2[k])), k


def test_run_unet_batch_exact_above_the_small_batch_limit():
    """run_unet_batch over more photos than the small-batch plan's limit (6 > 4) still returns
    exactly run_unet's masks and crops for every photo (exact=True: chunks of at most the limit, whose
    outputs are bitwise the batch-1 ones); exact=False (one large-batch forward) agrees within the
    accumulation tolerance: mask IoU >= 0.999 against the per-photo calls."""
    from unet_mi355x import inference as inf
    photos = _photos(6)
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        single = [inf.run_unet(p, ck, compute_dtype="mixed") for p in photos]
        assert inf._cached_model(ck, "mixed").native_handle(torch.device(DEV)).small_batch_limit() == 4
        batch = inf.run_unet_batch(photos, ck, compute_dtype="mixed")
        loose = inf.run_unet_batch(photos, ck, compute_dtype="mixed", exact=False)
    for a, b in zip(single, batch):
        _same_result(a, b, inf.FIELDS)
    for (m1, _), (m2, _) in zip(single, loose):
        for k in inf.FIELDS:
            assert orc.mask_iou(m1[k], m2[k]) >= 0.999, k


@pytest.mark.parametrize("dtype", ["mixed", "bf16"])
def test_run_unet_photo_graphs_equal_eager_calls(dtype):
    """run_unet replays one photo graph per geometry (upload + resize + forward + boxes + crop statistics +
    copies back, unet_photo_graph_create).  Alternating geometries (RGB and L), a photo larger than the
    staging buffer (its graphs are re-captured over the new buffers) and a stale graph (the cached model's
    workspace grown by a batch call) all return what the eager device path returns, bit for bit.  The
    16-bit plans' graphs resize straight into the first conv's pre-cast input (fp16 / bf16) when the
    photo's height is not 512; 512-high, 512-wide and 512 x 512 photos take the fp32 planes + pre-cast;
    1 x 1 and 3 x 2 photos (one-pixel crops, rectangles clamped at every edge) too."""
    from unet_mi355x import inference as inf
    extra = _photos(7)
    photos = _photos(4) + [_photos(6)[5].resize((1800, 1400)), extra[6].resize((700, 512)),
                           extra[6].resize((512, 300)), extra[6].resize((512, 512)),
                           extra[6].convert("L").resize((333, 512)),
                           extra[6].resize((1, 1)), extra[6].convert("L").resize((3, 2))]   # tiny photos
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        model = inf._cached_model(ck, dtype)
        dev = torch.device(DEV)

        def eager(pil):   # the round-4 device path: separate preprocess / forward_boxes / crop_stats calls
            arr = np.asarray(pil)
            img = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
            x = torch.empty((1, 3, 512, 512), dtype=torch.float32, device=dev)
            with torch.no_grad():
                model.preprocess(img, 512, out=x[0])
                m, b = model.forward_boxes(x, masks="u8")
            img3 = img if img.dim() == 3 else img.unsqueeze(-1)
            r = torch.empty((3, 4), dtype=torch.int32, device=dev)
            s = torch.empty((3,), dtype=torch.int64, device=dev)
            native.crop_stats(img3, b[0], 512, 512, inf.CROP_PAD, r, s, torch.cuda.current_stream(dev).cuda_stream)
            m, r, s = m.cpu().numpy()[0].astype(bool), r.cpu().numpy(), s.cpu().numpy()
            ch = 3 if arr.ndim == 3 else 1
            return ({k: m[i] for i, k in enumerate(inf.FIELDS)},
                    {k: inf.crop_from_stats(pil, r[i], s[i], ch) for i, k in enumerate(inf.FIELDS)})

        want = [eager(p) for p in photos]
        for rep in range(2):
            for p, w in zip(photos, want):
                _same_result(inf.run_unet(p, ck, compute_dtype=dtype), w, inf.FIELDS)
        st = inf._staging[str(inf.DEVICE)]
        assert 1 <= len(st.graphs) <= st.MAX_GRAPHS
        assert all(m is model for m, _ in st.graphs.values())   # another model's graphs were dropped
        inf.run_unet_batch(photos[:2], ck, compute_dtype=dtype, exact=False)   # may grow the workspace
        model.native_handle(dev).reserve(8, 512, 512)                        # grows it: graphs stale
        for p, w in zip(photos, want):
            _same_result(inf.run_unet(p, ck, compute_dtype=dtype), w, inf.FIELDS)


def test_launch_labels_at_name_the_small_batch_kernels():
    """unet_launch_label_at names the kernels a forward of that shape runs -- at batch 1 the
    split layers' partial kernel + reduction and the finer row tiles; above the limit the large-batch
    labels of unet_launch_label."""
    sd = syn.make_state_dict(0, 3, 3, "pretrained")
    m = make_model(sd, 3, "mixed")
    h = m.native_handle(torch.device(DEV))
    big = h.launch_labels()
    assert h.launch_labels_at(256, 512, 512) == big == h.launch_labels_at(0, 0, 0)
    small = h.launch_labels_at(1, 512, 512)
    assert small[9].startswith("conv3x3_ring8_kernel<__bf16, ") and "+ splitk_reduce_kernel<__bf16, __bf16, 0>" in small[9], small[9]
    assert small[10].startswith("convT_ring_kernel<__bf16, 8, 3, 1,"), small[10]      # up4 on 128-row halves
    assert small[21] == big[21]                                                       # the head is never split
    m.close()


def test_fp32_plan_kernels_per_layer():
    """The three-term fp32 plan's kernel per launch: the VALU first conv; split-per-tap 64-row
    tiles on the short-K layers (down1.3, down2.0, conv1.0); split-once 128-row tiles on the long-K layers;
    the 16x32 split-once tile with the head on conv1.3; the ConvTranspose on 128-row tiles splitting both
    operands at large batch and on pre-split 64-row tiles at batch 1."""
    sd = syn.make_state_dict(0, 3, 3, "pretrained")
    m = make_model(sd, 3, "fp32")
    h = m.native_handle(torch.device(DEV))
    big = h.launch_labels()
    assert big[0] == "first_conv_kernel<float, 3>", big[0]
    for i, epi in ((1, 1), (2, 0), (20, 0)):    # down1.3 (+ pool), down2.0, conv1.0
        assert big[i] == f"conv3x3_halo_kernel<float, 1, 4, 4, 2, 3, {epi}, 2>", (i, big[i])
    assert big[3] == "conv3x3_x3s_kernel<1>" and big[9] == "conv3x3_x3s_kernel<0>", (big[3], big[9])
    assert big[21] == "conv3x3_x3w_kernel<2>", big[21]
    for i in (10, 13, 16, 19):                   # up4 .. up1
        assert big[i] == "conv3x3_halo_kernel<float, 1, 4, 8, 2, 1, 3, 1>", (i, big[i])
    small = h.launch_labels_at(1, 512, 512)
    for i in (10, 13, 16, 19):
        assert small[i].startswith("conv3x3_halo_kernel<float, 1, 4, 4, 2, 1, ") and small[i].count(", 2>") >= 1, \
            (i, small[i])
    assert small[21] == big[21]
    m.close()


def _pool2(a):
    n, c, h, w = a.shape
    return a.reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "mixed"])
def test_doubleconv_standalone_matches_reference_hooks(dtype):
    """VERDICT r4 missing #4: DoubleConv called on its own (unet_model.py:19-20) runs natively
    (unet_block_*) and reproduces the reference's own block outputs -- the hook intermediates of
    tests/golden/unet_c3_h16w16_n3_structured.npz, each block fed the reference's own input (its pooled
    or concatenated hook tensors): down1 .. down4, bottleneck (1 x 1 pixels), conv4, conv1; conv3 and
    conv2 (no reference hook for their up-sampled half) against the oracle on seeded inputs at an odd
    37 x 50 size (partial tiles)."""
    z = np.load(os.path.join(GOLD, "unet_c3_h16w16_n3_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    m = make_model(sd, 3, dtype)
    cases = [("down1", z["x"], z["inter_c1"]),
             ("down2", _pool2(z["inter_c1"]), z["inter_c2"]),
             ("down3", _pool2(z["inter_c2"]), z["inter_c3"]),
             ("down4", _pool2(z["inter_c3"]), z["inter_c4"]),
             ("bottleneck", _pool2(z["inter_c4"]), z["inter_bn"]),
             ("conv4", np.concatenate([z["inter_u4_up"], z["inter_c4"]], 1), z["inter_c5"]),
             ("conv1", np.concatenate([z["inter_u1_up"], z["inter_c1"]], 1), z["inter_c8"])]
    sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    rng = np.random.default_rng(5)
    for name, cin in (("conv3", 512), ("conv2", 256)):
        xin = rng.standard_normal((2, cin, 37, 50)).astype(np.float32)
        cases.append((name, xin, orc.double_conv(sdt, name, torch.from_numpy(xin)).numpy()))
    with torch.no_grad():
        for name, xin, ref in cases:
            got = getattr(m, name)(torch.from_numpy(np.ascontiguousarray(xin)).to(DEV)).cpu().numpy()
            err = rel_err(got, ref)
            print(f"{dtype} {name}: {tuple(xin.shape)} -> rel err {err:.3e}")
            assert got.shape == ref.shape and err <= TOL[dtype], (name, err)
    m.close()


def test_run_unet_masks_survive_later_calls():
    """run_unet hands out its masks as views of pinned mask blocks (no host copy); a block is reused only
    once no returned mask of it is alive, and with every block held the call falls back to copying.  So
    masks kept across many later calls (more than the pool holds) never change, and dropped ones free
    their block for the next call."""
    from unet_mi355x import inference as inf
    photos = _photos(3)
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        kept = []
        for i in range(inf._Staging.MASK_POOL + 3):   # the first calls hold every block, then fall back
            masks, _ = inf.run_unet(photos[i % 3], ck, compute_dtype="mixed")
            kept.append((i % 3, masks, {k: v.copy() for k, v in masks.items()}))
        for _ in range(3):                           # more calls while all of those are alive
            inf.run_unet(photos[1], ck, compute_dtype="mixed")
        for j, masks, snap in kept:
            for k in inf.FIELDS:
                assert masks[k].dtype == np.bool_ and masks[k].shape == (512, 512)
                assert np.array_equal(masks[k], snap[k]), (j, k)
            again, _ = inf.run_unet(photos[j], ck, compute_dtype="mixed")
            for k in inf.FIELDS:
                assert np.array_equal(again[k], snap[k]), (j, k)
        st = inf._staging[str(inf.DEVICE)]
        assert len(st.masks.blocks) == inf._Staging.MASK_POOL
        # one photo graph per geometry (three photos), its masks copy retargeted to each block lent
        assert len(st.graphs) == len({(p.size, p.mode) for p in photos}) and st.retarget_error is None, st.retarget_error
        del kept, masks, again
        import gc
        gc.collect()
        assert all(st.masks.idle)   # every returned mask dropped: every block is free again


def test_photo_graph_retargets_between_blocks_and_the_shared_buffer():
    """One photo geometry, one graph: its masks copy is retargeted (unet_photo_graph_set_masks) from a lent
    pinned block to the shared pinned buffer (every block held: run_unet copies out of it) and back, and
    every call returns the same masks and crops."""
    import gc
    from unet_mi355x import inference as inf
    photo = _photos(1)[0]
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        first = inf.run_unet(photo, ck, compute_dtype="mixed")
        first = ({k: v.copy() for k, v in first[0].items()}, first[1])
        gc.collect()
        st = inf._staging[str(inf.DEVICE)]
        st.drop_graphs()
        st.retarget_error = None
        held = [inf.run_unet(photo, ck, compute_dtype="mixed") for _ in range(inf._Staging.MASK_POOL + 2)]
        assert not any(st.masks.idle)                     # every block lent: the last calls used the shared buffer
        for r in held:
            _same_result(r, first, inf.FIELDS)
        del held, r
        gc.collect()
        again = inf.run_unet(photo, ck, compute_dtype="mixed")   # back onto a block
        _same_result(again, first, inf.FIELDS)
        assert len(st.graphs) == 1
        assert st.retarget_error is None, st.retarget_error


def test_photo_graph_eviction_beside_batch_calls_on_another_thread():
    """evicting photo graphs (unet_graph_destroy drains the handle) while run_unet_batch runs on
    another thread and another stream: the destroy takes the handle's lock, so it never clears the
    stream-order state under a forward in flight.  Every batch result equals the single-threaded one, and
    every run_unet result too, while the LRU (shrunk to 1 geometry) evicts a graph on every call."""
    import threading
    from unet_mi355x import inference as inf
    photos = _photos(4)
    sizes = [(600, 400), (640, 480), (500, 700), (800, 600)]
    singles = [p.resize(sz) for p, sz in zip(photos, sizes)]
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        want_batch = inf.run_unet_batch(photos, ck, compute_dtype="mixed")
        want_single = [inf.run_unet(p, ck, compute_dtype="mixed") for p in singles]
        st = inf._staging[str(inf.DEVICE)]
        old_max = st.MAX_GRAPHS
        st.MAX_GRAPHS = 1
        st.drop_graphs()    # (the LRU evicts on insertion: start from none, so every call below inserts)
        errors, stop = [], threading.Event()

        def batch_worker():
            side = torch.cuda.Stream(device=DEV)
            try:
                with torch.cuda.stream(side):
                    while not stop.is_set():
                        for a, b in zip(inf.run_unet_batch(photos, ck, compute_dtype="mixed"), want_batch):
                            _same_result(a, b, inf.FIELDS)
            except Exception as e:   # noqa: BLE001 - reported below
                errors.append(repr(e))
        th = threading.Thread(target=batch_worker)
        th.start()
        try:
            for r in range(12):
                i = r % len(singles)
                _same_result(inf.run_unet(singles[i], ck, compute_dtype="mixed"), want_single[i], inf.FIELDS)
                assert len(st.graphs) == 1, (len(st.graphs), st.retarget_error)
        finally:
            stop.set()
            th.join(120)
            st.MAX_GRAPHS = old_max
        assert not th.is_alive() and errors == []


def test_run_unet_batch_loose_chunks_equal_one_large_forward():
    """run_unet_batch(exact=False) pipelines 16+ photos as chunks of 8 or more (every chunk above the
    small-batch limit): its masks equal one forward over all the photos at once bit for bit (the
    large-batch kernels' outputs do not depend on N)."""
    from unet_mi355x import inference as inf
    photos = _photos(17)
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        loose = inf.run_unet_batch(photos, ck, compute_dtype="mixed", exact=False)
        model = inf._cached_model(ck, "mixed")
        x = torch.empty((len(photos), 3, 512, 512), dtype=torch.float32, device=DEV)
        for i, p in enumerate(photos):
            model.preprocess(torch.from_numpy(np.array(p)).to(DEV), 512, out=x[i])
        with torch.no_grad():
            m, _ = model.forward_boxes(x, masks="u8")
        m = m.cpu().numpy().astype(bool)
    for i, (masks, _) in enumerate(loose):
        for j, k in enumerate(inf.FIELDS):
            assert np.array_equal(masks[k], m[i, j]), (i, k)


def test_run_unet_from_several_threads():
    """A Streamlit server may call run_unet from several session threads at once: the calls serialise on
    the device's staging lock and every thread gets exactly the single-threaded result for its photo
    (photo graphs, mask blocks and the cached model are shared state)."""
    import threading
    from unet_mi355x import inference as inf
    photos = _photos(4)
    with tempfile.TemporaryDirectory() as td:
        ck = _save_ckpt(td)
        inf.DEVICE = DEV
        want = [inf.run_unet(p, ck, compute_dtype="mixed") for p in photos]
        errors = []

        def worker(t):
            try:
                for r in range(6):
                    i = (t + r) % len(photos)
                    _same_result(inf.run_unet(photos[i], ck, compute_dtype="mixed"), want[i], inf.FIELDS)
            except Exception as e:   # noqa: BLE001 - reported below
                errors.append(repr(e))

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(120)
        assert not any(th.is_alive() for th in threads)
        assert errors == []
