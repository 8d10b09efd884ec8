"""The output head on the GPU: unet_head_forward / unet_head_backward through native.Handle and through
head.head_conv's autograd, UNet.features / head / fit_head and inference.finetune_head.

Bar of every comparison with the reference's out_conv (tests/golden/head_cases.npz): 8 x the output's own spread
(the reference's fp32 results against its fp64 ones), as max |a - ref| / max |ref|; the distance to the float64
restatement (head_ref.head) is printed beside it."""
import os

import numpy as np
import pytest
import torch

import head_ref
from head_ref import SPREAD_FACTOR
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.head import head_conv
from unet_mi355x.metrics import InvoiceLoss
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = head_ref.fixture()
IDS = [c["name"] for c in CASES]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def handle():
    h = native.Handle(3, 4, "fp32", 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def refs():
    """Per case, once: (feat, w, b, grad_logits) and the restatement's four outputs."""
    out = []
    for case in CASES:
        t = head_ref.case_tensors(case)
        out.append((t, head_ref.head(*t)))
    return out


def run(h, feat, w, b, g, want_params=True, want_feat=True):
    """(logits, grad_w, grad_b, grad_feat) as device tensors, straight through the handle."""
    f, wd = dev(feat), dev(w)
    logits = h.head_forward(f, wd, dev(b), stream())
    return (logits,) + h.head_backward(f, dev(g), wd, stream(), want_params=want_params, want_feat=want_feat)


def offset_copy(t):
    """The same tensor one float into a larger buffer: every row's alignment moves by 4 bytes."""
    o = torch.empty(t.numel() + 1, device=DEV)[1:].view(t.shape).copy_(t)
    assert o.data_ptr() % 16 == 4 and o.is_contiguous()
    return o


# ---------------------------------------------------------------- 1. fixture parity
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixture_cases(i, handle, refs):
    """Every fixture case through native.Handle and through head_conv with autograd (bitwise the same four
    outputs): each output within 8 x its own spread of the reference's, grad_w of a dead channel exactly 0.
    Observed on an MI355X (DESIGN.md section 11 has the table): logits at most 4.8e-7 (c1, bar 2.5e-6) and at most
    0.46 of the bar (dead); grad_w at most 2.7e-7, grad_b 2.6e-7 (spans, bars 2.2e-6 and 2.1e-6), both bitwise the
    restatement's; grad_feat bitwise the reference's at every sampled position."""
    case = CASES[i]
    (feat, w, b, g), restated = refs[i]
    outs = run(handle, feat, w, b, g)
    fa, wa, ba = dev(feat).requires_grad_(), dev(w).view(-1, 64, 1, 1).requires_grad_(), dev(b).requires_grad_()
    la = head_conv(fa, wa, ba)
    la.backward(dev(g))
    auto = (la, wa.grad.view(-1, 64), ba.grad, fa.grad)
    for k, native_out, auto_out, ours in zip(head_ref.OUTPUTS, outs, auto, restated):
        assert bits(native_out) == bits(auto_out), k
        got = native_out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all()
        ref = case[k]
        if k == "grad_feat":
            got, ours = got.reshape(-1)[case["positions"]], ours.reshape(-1)[case["positions"]]
        d, bar = head_ref.distance(got, ref), SPREAD_FACTOR * case[f"spread_{k}"]
        print(f"{IDS[i]} {k}: reference {d:.3e} (bar {bar:.3e}), restatement {head_ref.distance(got, ours):.3e}")
        assert d <= bar, (k, d, bar)
    gw = outs[1].cpu().numpy()
    for k in case["dead"]:
        assert (gw[:, k] == 0.0).all()
    if case["dead"]:
        assert np.count_nonzero(gw) == gw.size - gw.shape[0] * len(case["dead"])


def test_head_conv_asks_only_for_needed_gradients_and_takes_any_layout(handle, refs):
    (feat, w, b, g), _ = refs[IDS.index("odd")]
    base = run(handle, feat, w, b, g)
    # weight [C, 64], feat without grad: grad_feat is not computed, the parameters' gradients are the same bits
    wa, ba = dev(w).requires_grad_(), dev(b).requires_grad_()
    out = head_conv(dev(feat), wa, ba, handle=handle)
    out.backward(dev(g))
    assert bits(out) == bits(base[0]) and bits(wa.grad) == bits(base[1]) and bits(ba.grad) == bits(base[2])
    # non-contiguous fp64 features: made contiguous fp32 first; the gradient comes back in the input's dtype
    fa = dev(feat).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).double().requires_grad_()
    assert not fa.is_contiguous()
    out = head_conv(fa, dev(w), dev(b))
    out.backward(dev(g))
    assert bits(out) == bits(base[0]) and fa.grad.dtype == torch.float64
    assert bits(fa.grad.float().contiguous()) == bits(base[3])
    with torch.no_grad():
        assert head_conv(dev(feat), wa, ba).grad_fn is None


# ---------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("name", ["odd", "spans"])
def test_bitwise_reproducible_and_independent_of_alignment(name, handle, refs):
    (feat, w, b, g), _ = refs[IDS.index(name)]
    a = run(handle, feat, w, b, g)
    again = run(handle, feat, w, b, g)
    fo, wo, bo, go = (offset_copy(dev(t)) for t in (feat, w, b, g))
    n, c, h, wd = g.shape
    outs = [torch.empty(numel + 1, device=DEV)[1:].view(shape)
            for numel, shape in ((g.size, g.shape), (c * 64, (c, 64)), (c, (c,)), (feat.size, feat.shape))]
    handle.head_forward(fo, wo, bo, stream(), logits=outs[0])
    handle.head_backward(fo, go, wo, stream(), want_feat=True, grad_w=outs[1], grad_b=outs[2], grad_feat=outs[3])
    for k, x, y, z in zip(head_ref.OUTPUTS, a, again, outs):
        assert bits(x) == bits(y), k
        assert bits(x) == bits(z), k


def test_logits_do_not_depend_on_the_batch(handle, refs):
    (feat, w, b, _), _ = refs[IDS.index("spans")]
    one = handle.head_forward(dev(feat[1:2]), dev(w), dev(b), stream())
    three = handle.head_forward(dev(np.concatenate([feat[0:1], feat[1:2], feat[0:1]])), dev(w), dev(b), stream())
    assert bits(three[1]) == bits(one[0])


# ---------------------------------------------------------------- 3. IEEE propagation
def test_nan_rules(handle, refs):
    (feat, w, b, g), clean_ref = refs[IDS.index("dead")]
    clean = [t.cpu().numpy() for t in run(handle, feat, w, b, g)]
    # a NaN feature: the logits of its pixel and grad_w[:, k] of its channel, nothing else
    f2 = feat.copy()
    f2[1, 7, 3, 5] = np.nan
    want = head_ref.head(f2, w, b, g)
    got = [t.cpu().numpy() for t in run(handle, f2, w, b, g)]
    for k, a, r, c in zip(head_ref.OUTPUTS, got, want, clean):
        assert np.array_equal(np.isnan(a), np.isnan(r)), k
        keep = ~np.isnan(r)
        assert a[keep].tobytes() == c[keep].tobytes(), k
    assert np.isnan(got[0]).sum() == 3 and np.isnan(got[1]).sum() == 3
    assert not np.isnan(got[2]).any() and not np.isnan(got[3]).any()
    # a NaN gradient: grad_w[c][:], grad_b[c] and grad_feat[n][:, p], nothing else
    g2 = g.copy()
    g2[0, 1, 2, 9] = np.nan
    want = head_ref.head(feat, w, b, g2)
    got = [t.cpu().numpy() for t in run(handle, feat, w, b, g2)]
    for k, a, r, c in zip(head_ref.OUTPUTS, got, want, clean):
        assert np.array_equal(np.isnan(a), np.isnan(r)), k
        keep = ~np.isnan(r)
        assert a[keep].tobytes() == c[keep].tobytes(), k
    assert np.isnan(got[1]).sum() == 64 and np.isnan(got[2]).sum() == 1 and np.isnan(got[3]).sum() == 64
    # a zero weight does not hide a NaN feature (0 x NaN), a zero feature not a NaN gradient
    w0 = w.copy()
    w0[:, 7] = 0.0
    assert np.isnan(run(handle, f2, w0, b, g, want_feat=False)[0].cpu().numpy()[1, :, 3, 5]).all()


# ---------------------------------------------------------------- 4. null outputs, scratch, capture
def test_null_outputs_leave_the_others_unchanged(handle, refs):
    (feat, w, b, g), _ = refs[IDS.index("spans")]
    full = run(handle, feat, w, b, g)
    _, gw, gb, gf = run(handle, feat, w, b, g, want_feat=False)
    assert gf is None and bits(gw) == bits(full[1]) and bits(gb) == bits(full[2])
    _, gw, gb, gf = run(handle, feat, w, b, g, want_params=False)
    assert gw is None and gb is None and bits(gf) == bits(full[3])
    with pytest.raises(ValueError):
        run(handle, feat, w, b, g, want_params=False, want_feat=False)


def test_scratch_grows_and_leaves_the_forward_workspace_alone(refs):
    (feat, w, b, g), _ = refs[IDS.index("spans")]
    h = native.Handle(3, 3, "fp32", 0)
    before = h.workspace_bytes(2, 64, 64)
    h.head_reserve(1, 16, 16)   # smaller: the call below must grow it
    a = run(h, feat, w, b, g)
    h.head_reserve(4, 128, 96)
    c = run(h, feat, w, b, g)
    assert all(bits(x) == bits(y) for x, y in zip(a, c))
    assert h.workspace_bytes(2, 64, 64) == before
    h.close()


def test_capture_replays_to_the_eager_result(refs):
    """One torch.cuda.graph capture (a single stream, no parallel branches) of a forward and a backward after
    head_reserve: the replay equals the eager calls bitwise, also on new contents of the captured buffers.  A
    backward whose scratch would have to grow under capture is refused (UNET_ESTATE) before it launches."""
    (feat, w, b, g), _ = refs[IDS.index("spans")]
    h, small = native.Handle(3, 3, "fp32", 0), native.Handle(3, 3, "fp32", 0)
    fd, wd, bd, gd = dev(feat), dev(w), dev(b), dev(g)
    n, c = g.shape[:2]
    outs = (torch.zeros(g.shape, device=DEV), torch.zeros((c, 64), device=DEV), torch.zeros((c,), device=DEV),
            torch.zeros(feat.shape, device=DEV))
    h.head_reserve(2, 48, 96)
    eager = run(h, feat, w, b, g)
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
    e2 = (h.head_forward(fd, wd, bd, stream()),) + h.head_backward(fd, gd, wd, stream(), want_feat=True)
    graph.replay()
    torch.cuda.synchronize()
    assert all(bits(x) == bits(y) for x, y in zip(outs, e2)) and bits(e2[1]) != bits(eager[1])
    del graph
    h.close()
    small.close()


# ---------------------------------------------------------------- 5. indices past 2^31
def test_elements_past_2_31(handle):
    """Features of 129 x 64 x 512 x 512 = 2^31 + 2^24 elements.  The last image's logits equal the one-image call
    on its slice bitwise; grad_w / grad_b from a gradient that is zero on every other image agree with that call
    within the bar of the fixture's `big` case (the two sums run over different trees: 8256 slabs against 64)."""
    n, c, s = 129, 3, 512
    gen = torch.Generator(device=DEV).manual_seed(5)
    base = torch.relu(torch.randn((1, 64, s, s), device=DEV, generator=gen)) * 2.5
    feat = torch.empty((n, 64, s, s), device=DEV)
    torch.mul(base, torch.linspace(0.5, 1.5, n, device=DEV).view(n, 1, 1, 1), out=feat)
    assert feat.numel() > 2 ** 31 and feat.is_contiguous()
    w, b = dev(head_ref.generate((1, c, 1, 1), 99)[1]), torch.full((c,), -4.0, device=DEV)
    g = torch.zeros((n, c, s, s), device=DEV)
    g[-1] = torch.randn((c, s, s), device=DEV, generator=gen) * 1e-3
    logits = handle.head_forward(feat, w, b, stream())
    gw, gb, _ = handle.head_backward(feat, g, w, stream())
    last = feat[-1:].contiguous()
    one = handle.head_forward(last, w, b, stream())
    gw1, gb1, gf1 = handle.head_backward(last, g[-1:].contiguous(), w, stream(), want_feat=True)
    assert torch.isfinite(logits[-1]).all() and float(one.abs().max()) > 0
    assert torch.equal(logits[-1], one[0])
    assert not torch.equal(logits[0], one[0])
    bar = SPREAD_FACTOR * CASES[IDS.index("big")]["spread_grad_w"]
    dw = head_ref.distance(gw.cpu().numpy(), gw1.cpu().numpy())
    db = head_ref.distance(gb.cpu().numpy(), gb1.cpu().numpy())
    print(f"past 2^31: grad_w {dw:.3e}, grad_b {db:.3e} (bar {bar:.3e})")
    assert float(gw1.abs().max()) > 0 and dw <= bar and db <= bar
    del logits, one
    # grad_feat at the far end of the tensor: written in place of a sentinel, equal to the one-image call
    gf = torch.full((n, 64, s, s), 7.0, device=DEV)
    handle.head_backward(feat, g, w, stream(), want_params=False, want_feat=True, grad_feat=gf)
    assert torch.equal(gf[-1], gf1[0]) and not gf[n // 2].any()
    del feat, g, gf, base
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 6. the features feed the head
@pytest.fixture(scope="module")
def structured():
    from oracle import unet_oracle as orc
    sd_np = syn.make_state_dict(11, 3, 3, profile="structured")
    x = torch.from_numpy(syn.invoice_pages(11, 2, 64, 64, 3))
    ref = orc.unet_forward(sd_np, x).numpy()
    return sd_np, x, ref


@pytest.mark.parametrize("plan, tol", [("fp32", 2e-5), ("mixed", 3e-2)])
def test_features_feed_the_head_consistently(plan, tol, structured):
    """model.head(model.features(x)) meets the bar smoke() and test_forward_gpu.py apply to model(x)."""
    sd_np, x, ref = structured
    m = UNet(3, 3, compute_dtype=plan)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()})
    m = m.to(DEV).eval()
    xd = x.to(DEV)
    with torch.no_grad():
        fused = m(xd)
        feat = m.features(xd)
        out = m.head(feat)
    assert feat.shape == (2, 64, 64, 64) and feat.dtype == torch.float32 and float(feat.min()) >= 0.0
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(out.cpu().numpy() - ref).max()) / scale
    print(f"{plan}: head(features(x)) against the oracle {err:.3e} (bar {tol:.0e}), against model(x) "
          f"{float((out - fused).abs().max()) / scale:.3e}")
    assert err <= tol
    m.train()   # the backbone runs with eval BatchNorm whatever the mode, and the mode is left as found
    assert torch.equal(m.features(xd), feat) and m.training
    m.close()


# ---------------------------------------------------------------- 7. trajectory
@pytest.mark.parametrize("lr", head_ref.TRAJ_LRS)
def test_trajectory(lr):
    """train.py's loop on the head alone (head_conv + InvoiceLoss + AdamW + CosineAnnealingWarmRestarts on the
    device): every step's loss within 8 x max(spread, 2^-23) of the reference's fp32 loop."""
    traj = head_ref.trajectory_fixture()[lr]
    feat, target, w0, b0 = head_ref.trajectory_tensors()
    f, t = dev(feat), dev(target)
    w = torch.nn.Parameter(dev(w0).view(3, 64, 1, 1))
    b = torch.nn.Parameter(dev(b0))
    crit = InvoiceLoss()
    opt = torch.optim.AdamW([w, b], lr=lr, weight_decay=head_ref.TRAJ_WD)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2)
    losses = []
    for _ in range(head_ref.TRAJ_EPOCHS):
        for lo in range(0, f.shape[0], head_ref.TRAJ_BATCH):
            loss = crit(head_conv(f[lo:lo + head_ref.TRAJ_BATCH], w, b), t[lo:lo + head_ref.TRAJ_BATCH])
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        sched.step()
    crit.close()
    got, ref = np.array(losses, np.float64), traj["losses"].astype(np.float64)
    rel = np.abs(got - ref) / np.abs(ref)
    bar = SPREAD_FACTOR * max(traj["spread"], 2.0 ** -23)
    print(f"lr {lr}: loss {got[0]:.4f} -> {got[-1]:.4f}, largest distance {rel.max():.3e} at step "
          f"{int(rel.argmax())} (bar {bar:.3e})")
    assert len(got) == len(ref) and rel.max() <= bar


# ---------------------------------------------------------------- 8. end to end
def probe_setup():
    """(pretrained state_dict with the head re-initialised, pages fp32 [4, 3, 64, 64], targets fp32 0/1)."""
    sd = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in syn.make_state_dict(0, 3, 3, "pretrained").items()}
    rs = np.random.RandomState(8)
    sd["out_conv.weight"] = torch.from_numpy(rs.uniform(-0.125, 0.125, size=(3, 64, 1, 1)).astype(np.float32))
    sd["out_conv.bias"] = torch.full((3,), -4.0)
    x = syn.invoice_pages(5, 4, 64, 64, 3)
    t = (syn.invoice_fields(5, 4, 64, 64) > 0).astype(np.float32)
    return sd, x, t


def test_fit_head_end_to_end():
    sd, x, t = probe_setup()
    m = UNet(3, 3, compute_dtype="fp32")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    xd, td = dev(x), dev(t)
    losses = m.fit_head(xd, td, epochs=20, batch=2, lr=1e-2)
    after_fit = m.score(xd, td).loss(batch=2)   # the fused forward: the new head reached the handle
    print(f"fit_head: epoch losses {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[-1] / losses[0]:.3f} of the first), "
          f"fused forward afterwards {after_fit:.4f}")
    assert len(losses) == 20 and not m.training
    assert losses[-1] < 0.5 * losses[0]
    assert after_fit < 0.5 * losses[0]
    changed = sorted(k for k, v in m.state_dict().items() if not torch.equal(v, before[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"]
    # shuffled batches and a short last batch run too, and fit further
    more = m.fit_head(xd[:3], td[:3], epochs=2, batch=2, lr=1e-3, shuffle_seed=1)
    assert len(more) == 2 and all(np.isfinite(more))
    m.close()


# ---------------------------------------------------------------- 9. the directory front end
def test_finetune_head_on_a_directory(tmp_path):
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
                                     compute_dtype="fp32")
    assert len(losses) == 20 and losses[-1] < 0.5 * losses[0]
    saved = torch.load(out, map_location="cpu", weights_only=True)
    assert len(saved) == 136
    fresh = UNet(3, 3, compute_dtype="fp32")
    fresh.load_state_dict(saved, strict=True)
    changed = sorted(k for k in saved if not torch.equal(saved[k], sd[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"]
    after = inference.evaluate(str(img_dir), str(mask_dir), out, batch=2, compute_dtype="fp32").loss(batch=2)
    print(f"finetune_head: epoch losses {losses[0]:.4f} -> {losses[-1]:.4f}, evaluate afterwards {after:.4f}")
    assert after < 0.5 * losses[0]
    assert os.path.getsize(out) > 100 << 20   # the full checkpoint, not the head alone
