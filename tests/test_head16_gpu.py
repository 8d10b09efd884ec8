"""The output head on 16-bit features on the GPU: unet_head_forward_typed / unet_head_backward_typed through
native.Handle, head.head_conv on float16 / bfloat16 maps, UNet.features(dtype=), UNet.fit_head(feature_dtype=) and
inference.finetune_head(feature_dtype=).

The oracle is the existing fp32 entry points on the widened tensor (``feat16.float()``: widening fp16 or bf16 to fp32
is exact), which tests/test_head_gpu.py pins to the reference.  No tolerance appears here: every comparison is
bitwise, except that where a feature is NaN the NaN positions are compared, not the payloads, and that the two-tree
comparison past 2^31 elements reuses the bar of test_head_gpu.test_elements_past_2_31."""
import numpy as np
import pytest
import torch

import head_ref
import test_head_gpu as thg
from head_ref import SPREAD_FACTOR
from test_head_gpu import DEV, dev, probe_setup, stream
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.head import head_conv
from unet_mi355x.metrics import InvoiceLoss
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu

CASES, IDS = thg.CASES, thg.IDS
D16 = {"fp16": torch.float16, "bf16": torch.bfloat16}
BOTH = pytest.mark.parametrize("d", sorted(D16))


@pytest.fixture(scope="module")
def handle():
    h = native.Handle(3, 4, "fp32", 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def tensors():
    """Per fixture case, once: (feat, w, b, grad_logits) as fp32 device tensors."""
    return [tuple(dev(t) for t in head_ref.case_tensors(case)) for case in CASES]


def bits(t):
    """The tensor's bytes (numpy has no bfloat16: 16-bit tensors go as their integer view)."""
    t = t.detach().contiguous()
    if t.element_size() == 2:
        t = t.view(torch.int16)
    return t.cpu().numpy().tobytes()


def run(h, f, w, b, g, want_params=True, want_feat=True):
    """(logits, grad_w, grad_b, grad_feat) of device tensors straight through the handle: the typed symbols for a
    16-bit ``f``, the untyped ones for an fp32 ``f``."""
    logits = h.head_forward(f, w, b, stream())
    return (logits,) + h.head_backward(f, g, w, stream(), want_params=want_params, want_feat=want_feat)


def shifted(t, k):
    """The same tensor k elements into a larger buffer: its base 2 k bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=DEV, dtype=t.dtype)
    o = buf[k:k + t.numel()].view(t.shape).copy_(t)
    assert buf.data_ptr() % 16 == 0 and o.data_ptr() % 16 == k * t.element_size() and o.is_contiguous()
    return o


def same(a, r, what):
    """Bitwise equal, except that NaNs need only sit in the same places."""
    a, r = a.detach().cpu().float().numpy(), r.detach().cpu().float().numpy()
    assert a.shape == r.shape, what
    na, nr = np.isnan(a), np.isnan(r)
    assert np.array_equal(na, nr), what
    assert a[~na].tobytes() == r[~nr].tobytes(), what


# ---------------------------------------------------------------- 1. fixture cases
@BOTH
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixture_cases(i, d, handle, tensors):
    """Every fixture case with its features rounded to 16 bits: the typed path's four outputs are the bits of the
    fp32 path on the widened features, through the handle and through head_conv with autograd (grad_feat comes back
    in feat's dtype, cast from the fp32 result); grad_w of a dead channel is exactly 0."""
    feat, w, b, g = tensors[i]
    f16 = feat.to(D16[d])
    wide = f16.float()
    assert f16.dtype == D16[d] and f16.is_contiguous() and wide.dtype == torch.float32
    want = run(handle, wide, w, b, g)
    got = run(handle, f16, w, b, g)
    for k, a, r in zip(head_ref.OUTPUTS, got, want):
        assert a.dtype == torch.float32 and bits(a) == bits(r), k
        assert torch.isfinite(a).all(), k
    fa, wa, ba = f16.clone().requires_grad_(), w.view(-1, 64, 1, 1).clone().requires_grad_(), b.clone().requires_grad_()
    la = head_conv(fa, wa, ba)
    la.backward(g)
    assert fa.grad.dtype == D16[d] and la.dtype == torch.float32
    assert bits(la) == bits(want[0]) and bits(wa.grad.view(-1, 64)) == bits(want[1]) and bits(ba.grad) == bits(want[2])
    assert bits(fa.grad) == bits(want[3].to(D16[d]))
    gw = got[1].cpu().numpy()
    for k in CASES[i]["dead"]:
        assert (gw[:, k] == 0.0).all()
    if CASES[i]["dead"]:
        assert np.count_nonzero(gw) == gw.size - gw.shape[0] * len(CASES[i]["dead"])


# ---------------------------------------------------------------- 2. geometry edges
EDGES = [(1, 1, 1, 1), (1, 3, 5, 7), (2, 2, 2, 6), (1, 4, 3, 8), (2, 3, 48, 96)]


@BOTH
@pytest.mark.parametrize("shape", EDGES, ids=["x".join(map(str, s)) for s in EDGES])
def test_geometry_edges_and_base_alignment(shape, d, handle):
    """The smallest shapes at which the 16-byte loads of 8 pixels can go wrong -- H W odd (every image base
    misaligned), divisible by 4 but not by 8, by 8, and one full span plus a 512-pixel tail -- each also with the
    feature tensor's base 2, 4 and 8 bytes off a 16-byte boundary: always the bits of the fp32 path."""
    feat, w, b, g = (dev(t) for t in head_ref.generate(shape, 400 + EDGES.index(shape)))
    f16 = feat.to(D16[d])
    want = run(handle, f16.float(), w, b, g)
    assert f16.data_ptr() % 16 == 0
    for k in (0, 1, 2, 4):
        got = run(handle, shifted(f16, k) if k else f16, w, b, g)
        for name, a, r in zip(head_ref.OUTPUTS, got, want):
            assert bits(a) == bits(r), (name, k)


# ---------------------------------------------------------------- 3. special values
def specials(d):
    """(bit patterns of the finite special values, of the non-finite ones) of the 16-bit type."""
    if d == "fp16":   # 1-5-10
        finite = dict(pzero=0x0000, nzero=0x8000, sub_min=0x0001, sub_max=0x03FF, norm_min=0x0400, fin_max=0x7BFF,
                      neg_sub_min=0x8001, neg_fin_max=0xFBFF)
        nonfinite = dict(pinf=0x7C00, ninf=0xFC00, nan=0x7E00)
    else:             # 1-8-7
        finite = dict(pzero=0x0000, nzero=0x8000, sub_min=0x0001, sub_max=0x007F, norm_min=0x0080, fin_max=0x7F7F,
                      neg_sub_min=0x8001, neg_fin_max=0xFF7F)
        nonfinite = dict(pinf=0x7F80, ninf=0xFF80, nan=0x7FC0)
    return finite, nonfinite


def put(f16, spots, patterns):
    raw = f16.view(torch.int16)
    for (k, y, x), v in zip(spots, patterns.values()):
        raw[0, k, y, x] = v - 0x10000 if v >= 0x8000 else v
    return f16


@BOTH
def test_special_values(d, handle):
    """Signed zeros, the smallest and largest subnormal, the smallest normal, the largest finite value, then also
    +-inf and NaN in a (1, 3, 4, 8) map: widened exactly (the outputs are the bits of the fp32 path on
    ``feat.float()``), and a non-finite feature reaches the logits of its pixel and grad_w[:, k] of its channel
    only -- DESIGN.md section 11's NaN rule."""
    feat, w, b, g = (dev(t) for t in head_ref.generate((1, 3, 4, 8), 410))
    finite, nonfinite = specials(d)
    spots = [(0, 0, 0), (1, 0, 1), (2, 1, 7), (3, 2, 0), (63, 3, 7), (17, 1, 3), (40, 2, 5), (41, 3, 0)]
    f16 = put(feat.to(D16[d]), spots, finite)
    wide = f16.float()
    for (k, y, x), (name, v) in zip(spots, finite.items()):   # the widened tensor holds the value meant
        sign, mag = (-1.0 if v & 0x8000 else 1.0), v & 0x7FFF
        if d == "fp16":
            val = np.float64(np.array(mag, np.uint16).view(np.float16))
        else:
            val = np.float64(np.array(mag << 16, np.uint32).view(np.float32))
        assert float(wide[0, k, y, x]) == sign * val and (mag == 0 or val > 0), name
        assert np.signbit(wide[0, k, y, x].item()) == (sign < 0), name
    assert float(wide.abs().max()) == (65504.0 if d == "fp16" else float(np.array(0x7F7F0000, np.uint32).view(np.float32)))
    clean_want, clean = run(handle, wide, w, b, g), run(handle, f16, w, b, g)
    for name, a, r in zip(head_ref.OUTPUTS, clean, clean_want):
        assert bits(a) == bits(r) and torch.isfinite(a).all(), name
    bad_spots = [(5, 0, 4), (22, 2, 2), (50, 3, 6)]   # other channels and pixels than the finite specials
    f_bad = put(f16.clone(), bad_spots, nonfinite)
    wide_bad = f_bad.float()
    assert int((~torch.isfinite(wide_bad)).sum()) == 3 and int(torch.isnan(wide_bad).sum()) == 1
    want, got = run(handle, wide_bad, w, b, g), run(handle, f_bad, w, b, g)
    for name, a, r in zip(head_ref.OUTPUTS, got, want):
        same(a, r, name)
    reach_logits = torch.zeros_like(got[0], dtype=torch.bool)
    reach_gw = torch.zeros_like(got[1], dtype=torch.bool)
    for k, y, x in bad_spots:
        reach_logits[0, :, y, x] = True
        reach_gw[:, k] = True
    assert not torch.isfinite(got[0][reach_logits]).any() and not torch.isfinite(got[1][reach_gw]).any()
    assert torch.isnan(got[0][0, :, 3, 6]).all() and torch.isnan(got[1][:, 50]).all()   # the NaN itself
    assert bits(got[0][~reach_logits]) == bits(clean[0][~reach_logits])
    assert bits(got[1][~reach_gw]) == bits(clean[1][~reach_gw])
    assert bits(got[2]) == bits(clean[2]) and bits(got[3]) == bits(clean[3])


# ---------------------------------------------------------------- 4. no hidden fp32 copy
@BOTH
def test_head_conv_makes_no_fp32_copy_of_the_features(d):
    """Forward and backward (weight and bias gradients) of head_conv on a 16-bit (2, 64, 64, 64) map: the allocator's
    peak rises by less than an fp32 copy of the map would take."""
    gen = torch.Generator(device=DEV).manual_seed(4)
    feat = (torch.relu(torch.randn((2, 64, 64, 64), device=DEV, generator=gen)) * 2.5).to(D16[d])
    g = torch.randn((2, 3, 64, 64), device=DEV, generator=gen) * 1e-3
    w = ((torch.rand((3, 64, 1, 1), device=DEV, generator=gen) - 0.5) * 0.25).requires_grad_()
    b = torch.full((3,), -4.0, device=DEV).requires_grad_()
    with torch.no_grad():
        head_conv(feat[:1], w, b)   # the module's handle exists before the measurement
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    before = torch.cuda.memory_allocated(DEV)
    out = head_conv(feat, w, b)
    out.backward(g)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - before
    print(f"{d}: peak rise {rise} bytes, an fp32 copy of the features {feat.numel() * 4}")
    assert w.grad is not None and b.grad is not None and float(w.grad.abs().max()) > 0
    assert rise < feat.numel() * 4


# ---------------------------------------------------------------- 5. capture
@BOTH
def test_capture_replays_to_the_eager_result(d, tensors):
    """One torch.cuda.graph capture (a single stream, no parallel branches) of a typed forward and backward after
    head_reserve: the replay equals the eager calls bitwise, also on new contents of the captured buffers; a
    backward whose scratch would have to grow under capture is refused (UNET_ESTATE) before it launches."""
    feat, wd, bd, g = tensors[IDS.index("spans")]
    fd, gd = feat.to(D16[d]), g.clone()
    h, small = native.Handle(3, 3, "fp32", 0), native.Handle(3, 3, "fp32", 0)
    c = g.shape[1]
    outs = (torch.zeros(g.shape, device=DEV), torch.zeros((c, 64), device=DEV), torch.zeros((c,), device=DEV),
            torch.zeros(feat.shape, device=DEV))
    h.head_reserve(2, 48, 96)
    eager = run(h, fd, wd, bd, gd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="unet_head_reserve"):
            small.head_backward(fd, gd, wd, stream())
        h.head_forward(fd, wd, bd, stream(), logits=outs[0])
        h.head_backward(fd, gd, wd, stream(), want_feat=True, grad_w=outs[1], grad_b=outs[2], grad_feat=outs[3])
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(x) == bits(y) for x, y in zip(outs, eager))
    gd.copy_(-2 * gd)   # the graph reads the buffers it captured
    fd.copy_(fd.flip(0))
    e2 = run(h, fd, wd, bd, gd)
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(x) == bits(y) for x, y in zip(outs, e2)) and bits(e2[1]) != bits(eager[1])
    assert all(bits(x) == bits(y) for x, y in zip(e2, run(h, fd.float(), wd, bd, gd)))
    del graph
    h.close()
    small.close()


# ---------------------------------------------------------------- 6. indices past 2^31
def test_elements_past_2_31(handle):
    """fp16 features of 129 x 64 x 512 x 512 = 2^31 + 2^24 elements (8.7 GB).  The last image's logits equal the
    one-image calls on its slice bitwise, typed and fp32-on-widened; grad_w / grad_b from a gradient that is zero on
    every other image agree with the one-image call within the bar test_head_gpu.test_elements_past_2_31 uses (the
    two sums run over different trees: 8256 slabs against 64)."""
    n, c, s = 129, 3, 512
    need = n * 64 * s * s * 2 + 3 * n * c * s * s * 4 + (2 << 30)
    free = torch.cuda.mem_get_info(DEV)[0] + torch.cuda.memory_reserved(DEV) - torch.cuda.memory_allocated(DEV)
    if free < need:
        pytest.skip(f"the device has {free / 2**30:.1f} GiB free, the case needs {need / 2**30:.1f} GiB")
    gen = torch.Generator(device=DEV).manual_seed(5)
    base = torch.relu(torch.randn((64, s, s), device=DEV, generator=gen)) * 2.5
    feat = torch.empty((n, 64, s, s), device=DEV, dtype=torch.float16)
    for i, scale in enumerate(torch.linspace(0.5, 1.5, n).tolist()):
        feat[i] = base * scale
    assert feat.numel() > 2 ** 31 and feat.is_contiguous()
    w, b = dev(head_ref.generate((1, c, 1, 1), 99)[1]), torch.full((c,), -4.0, device=DEV)
    g = torch.zeros((n, c, s, s), device=DEV)
    g[-1] = torch.randn((c, s, s), device=DEV, generator=gen) * 1e-3
    logits = handle.head_forward(feat, w, b, stream())
    gw, gb, _ = handle.head_backward(feat, g, w, stream())
    last = feat[-1:].contiguous()
    one, one_wide = handle.head_forward(last, w, b, stream()), handle.head_forward(last.float(), w, b, stream())
    gw1, gb1, _ = handle.head_backward(last, g[-1:].contiguous(), w, stream())
    gw1_wide, gb1_wide, _ = handle.head_backward(last.float(), g[-1:].contiguous(), w, stream())
    assert torch.isfinite(logits[-1]).all() and float(one.abs().max()) > 0
    assert torch.equal(logits[-1], one[0]) and torch.equal(one, one_wide)
    assert not torch.equal(logits[0], one[0])
    assert torch.equal(gw1, gw1_wide) and torch.equal(gb1, gb1_wide)
    bar = SPREAD_FACTOR * CASES[IDS.index("big")]["spread_grad_w"]
    dw = head_ref.distance(gw.cpu().numpy(), gw1.cpu().numpy())
    db = head_ref.distance(gb.cpu().numpy(), gb1.cpu().numpy())
    print(f"past 2^31, fp16 features: grad_w {dw:.3e}, grad_b {db:.3e} (bar {bar:.3e})")
    assert float(gw1.abs().max()) > 0 and dw <= bar and db <= bar
    del logits, one, one_wide, feat, g, base, last
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. scratch history
@BOTH
def test_typed_backward_after_fill(d, tensors):
    """After unet_debug_fill(0xFF) of a scratch reserved for a larger call, a typed backward equals the one on a
    handle that was never filled."""
    feat, w, b, g = tensors[IDS.index("spans")]
    f16 = feat.to(D16[d])
    fresh, filled = native.Handle(3, 3, "fp32", 0), native.Handle(3, 3, "fp32", 0)
    filled.head_reserve(4, 128, 96)
    run(filled, f16, w, b, g)   # a past of its own, then the fill
    filled.debug_fill(0xFF, stream())
    got, want = run(filled, f16, w, b, g), run(fresh, f16, w, b, g)
    for name, a, r in zip(head_ref.OUTPUTS, got, want):
        assert bits(a) == bits(r) and torch.isfinite(a).all(), name
    fresh.close()
    filled.close()


# ---------------------------------------------------------------- 8. features(dtype=)
@pytest.fixture(scope="module")
def structured():
    sd_np = syn.make_state_dict(11, 3, 3, profile="structured")
    return sd_np, torch.from_numpy(syn.invoice_pages(11, 2, 64, 64, 3))


@pytest.mark.parametrize("plan", ["fp32", "mixed"])
def test_features_dtype(plan, structured):
    """features(x, dtype) is features(x).to(dtype) bit for bit (torch's round to nearest even); the default is the
    fp32 map as before.  Prints the share of the features the rounding changes."""
    sd_np, x = structured
    m = UNet(3, 3, compute_dtype=plan)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    f32 = m.features(xd)
    assert f32.dtype == torch.float32 and bits(m.features(xd, dtype=torch.float32)) == bits(f32)
    for d, dt in sorted(D16.items()):
        f16 = m.features(xd, dtype=dt)
        assert f16.dtype == dt and f16.shape == f32.shape and f16.is_contiguous()
        assert bits(f16) == bits(f32.to(dt))
        changed = float((f16.float() != f32).float().mean())
        print(f"{plan}: rounding to {d} changes {100 * changed:.1f} % of the features (max {float(f32.max()):.2f})")
    with pytest.raises(ValueError, match="dtype"):
        m.features(xd, dtype=torch.float64)
    m.close()


# ---------------------------------------------------------------- 9. fit_head equivalence
def probe_model(sd):
    m = UNet(3, 3, compute_dtype="fp32")
    m.load_state_dict(sd)
    return m.to(DEV).eval()


@BOTH
def test_fit_head_on_a_16_bit_cache_is_the_fit_on_the_rounded_features(d):
    """fit_head(feature_dtype=d) against the same loop written out here on ``features(x).to(d).float()`` through the
    fp32 head_conv: equal epoch losses, bitwise equal out_conv parameters."""
    sd, x, t = probe_setup()
    xd, td = dev(x), dev(t)
    a, b = probe_model(sd), probe_model(sd)
    losses_a = a.fit_head(xd, td, epochs=3, batch=2, lr=1e-2, shuffle_seed=1, feature_dtype=d)
    feats = b.features(xd).to(D16[d]).float()
    assert feats.dtype == torch.float32
    weight, bias = b.out_conv.weight, b.out_conv.bias
    crit = InvoiceLoss()
    opt = torch.optim.AdamW([weight, bias], lr=1e-2, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2)
    gen = torch.Generator().manual_seed(1)
    pages, batch = xd.shape[0], 2
    steps = (pages + batch - 1) // batch
    losses_b = []
    for _ in range(3):
        order = torch.randperm(pages, generator=gen).to(DEV)
        total = torch.zeros((), device=DEV, dtype=torch.float32)
        for lo in range(0, pages, batch):
            f, tt = feats[order[lo:lo + batch]], td[order[lo:lo + batch]]
            loss = crit(head_conv(f, weight, bias), tt)
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += loss.detach()
        losses_b.append(float(total.item()) / steps)
        sched.step()
    crit.close()
    print(f"{d}: fit_head {losses_a}, written out {losses_b}")
    assert losses_a == losses_b and len(losses_a) == 3
    assert bits(a.out_conv.weight) == bits(weight) and bits(a.out_conv.bias) == bits(bias)
    assert not torch.equal(weight.detach().cpu(), sd["out_conv.weight"])
    a.close()
    b.close()


# ---------------------------------------------------------------- 10. end to end
def test_fit_head_end_to_end_on_an_fp16_cache():
    """The conditions of test_head_gpu.test_fit_head_end_to_end with feature_dtype="fp16"."""
    sd, x, t = probe_setup()
    m = probe_model(sd)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    xd, td = dev(x), dev(t)
    losses = m.fit_head(xd, td, epochs=20, batch=2, lr=1e-2, feature_dtype="fp16")
    after_fit = m.score(xd, td).loss(batch=2)   # the fused forward: the new head reached the handle
    print(f"fit_head on fp16 features: epoch losses {losses[0]:.6f} -> {losses[-1]:.9f} "
          f"({losses[-1] / losses[0]:.4f} of the first), fused forward afterwards {after_fit:.4f}")
    assert len(losses) == 20 and not m.training
    assert losses[-1] < 0.5 * losses[0]
    assert after_fit < 0.5 * losses[0]
    changed = sorted(k for k, v in m.state_dict().items() if not torch.equal(v, before[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"]
    m.close()


def test_finetune_head_on_a_directory_with_an_fp16_cache(tmp_path):
    from PIL import Image
    from unet_mi355x import inference
    sd, x, t = probe_setup()
    img_dir, mask_dir = tmp_path / "images", tmp_path / "masks"
    img_dir.mkdir()
    mask_dir.mkdir()
    for i in range(4):
        page = np.round(x[i].transpose(1, 2, 0) * 255.0).astype(np.uint8)
        Image.fromarray(page).save(img_dir / f"page{i}.png")
        np.save(mask_dir / f"page{i}.npy", (t[i].transpose(1, 2, 0) * 255).astype(np.uint8))
    ckpt, out = str(tmp_path / "start.pth"), str(tmp_path / "probed.pth")
    torch.save(sd, ckpt)
    losses = inference.finetune_head(str(img_dir), str(mask_dir), ckpt, out, epochs=20, batch=2, lr=1e-2,
                                     compute_dtype="fp32", feature_dtype="fp16")
    assert len(losses) == 20 and losses[-1] < 0.5 * losses[0]
    saved = torch.load(out, map_location="cpu", weights_only=True)
    assert len(saved) == 136
    changed = sorted(k for k in saved if not torch.equal(saved[k], sd[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"]
    after = inference.evaluate(str(img_dir), str(mask_dir), out, batch=2, compute_dtype="fp32").loss(batch=2)
    print(f"finetune_head on fp16 features: epoch losses {losses[0]:.4f} -> {losses[-1]:.4f}, evaluate afterwards "
          f"{after:.4f}")
    assert after < 0.5 * losses[0]


# ---------------------------------------------------------------- 11. the overflow rule
def test_fp16_cache_refuses_features_beyond_its_range():
    """conv1's last BatchNorm scaled by 1e6 on the fp32 plan: the features leave fp16's range.  feature_dtype="fp16"
    raises, naming fp16, before any parameter moves; "bf16" (fp32's range) and "fp32" run."""
    sd, x, t = probe_setup()
    sd["conv1.net.4.weight"] = sd["conv1.net.4.weight"] * 1e6
    xd, td = dev(x), dev(t)
    m = probe_model(sd)
    assert float(m.features(xd).max()) > 65504.0
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    with pytest.raises(RuntimeError, match="fp16") as info:
        m.fit_head(xd, td, epochs=1, batch=2, lr=1e-2, feature_dtype="fp16")
    assert "bf16" in str(info.value) and "fp32" in str(info.value)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    for ok in ("bf16", "fp32"):
        losses = m.fit_head(xd, td, epochs=1, batch=2, lr=1e-2, feature_dtype=ok)
        assert len(losses) == 1
    assert not torch.equal(m.out_conv.weight.detach(), before["out_conv.weight"])
    m.close()
