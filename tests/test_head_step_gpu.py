"""The fused head training step on the device (unet_head_step, include/unet_mi355x.h): one pass
over the stored features gives the loss, the gradient at the head's parameters and the AdamW update.  Against the
reference's autograd (tests/golden/head_step_cases.npz), against the three native calls it replaces, and the
properties the header states: bitwise independence of feature type and alignment, page indices, capture, scratch,
NaN reach, 64-bit offsets, and ``fit_head(fused=True)`` end to end."""
import numpy as np
import pytest
import torch

import head_ref
import head_step_ref as ref
import loss_ref
from unet_mi355x import native
from unet_mi355x.head import HeadFit, head_conv
from unet_mi355x.metrics import InvoiceLoss
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ref.fixture()
IDS = [c["name"] for c in CASES]
OPT = (1e-2, 0.9, 0.999, 1e-8, 1e-4)   # lr, betas, eps, weight decay (fit_head's)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.uint32 if t.element_size() == 4 else np.uint16).tolist()


def offset_copy(t, off):
    """t's values in a fresh buffer whose base lies ``off`` bytes past a 16-byte boundary"""
    es = t.element_size()
    buf = torch.empty(t.numel() + 16, device=t.device, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0 and off % es == 0
    v = buf[off // es: off // es + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off % 16 and v.is_contiguous()
    return v


@pytest.fixture(scope="module")
def handle():
    h = native.Handle(3, 4, "fp32", 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def refs():
    """per fixture case: the generated host tensors, made once"""
    return [ref.case_tensors(c) for c in CASES]


def grads(h, feat, target, w, b, pages=None):
    """(loss, grad_w, grad_b) without an update"""
    return h.head_step(feat, target, w, b, stream(), pages=pages)


def update(h, feat, target, w, b, pages=None, step_no=1, lr=OPT[0]):
    """one AdamW step from zero moments on copies of (w, b): (loss, grad_w, grad_b, w', b', state')"""
    w, b = w.clone(), b.clone()
    state = torch.zeros(2 * (w.numel() + b.numel()), device=DEV)
    loss, gw, gb = h.head_step(feat, target, w, b, stream(), pages=pages, opt=(lr,) + OPT[1:] + (step_no,),
                               state=state, want_grads=True)
    return loss, gw, gb, w, b, state


def same_bits(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. the reference's autograd
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixture_cases(i, handle, refs):
    """loss, grad_w and grad_b within 8 x max(spread, 2^-23) of the reference's fp32 autograd, for the uint8 NHWC
    target and for the same target as fp32 NCHW."""
    case = CASES[i]
    feat, w, b, tu8 = refs[i]
    for target in (dev(tu8), dev(ref.target_f32(tu8))):
        got = dict(zip(ref.OUTPUTS, (t.cpu().numpy() for t in grads(handle, dev(feat), target, dev(w), dev(b)))))
        for k in ref.OUTPUTS:
            d = ref.distance(got[k], case[k])
            print(f"{case['name']} {target.dtype} {k}: {d:.3e} (bar {ref.bar(case, k):.3e})")
            assert np.isfinite(got[k]).all() and d <= ref.bar(case, k)


# ---------------------------------------------------------------- 2. the three calls it replaces
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_three_native_calls(i, handle, refs):
    """head_forward, loss_grad, head_backward on the same tensors: the loss within 1 fp32 ulp (the plane sums run
    over another tree), the gradients within the fixture's bars."""
    case = CASES[i]
    feat, w, b, tu8 = (dev(a) for a in refs[i])
    logits = handle.head_forward(feat, w, b, stream())
    l3, g = handle.loss_grad(logits, tu8, stream())
    gw3, gb3, _ = handle.head_backward(feat, g, w, stream())
    loss, gw, gb = grads(handle, feat, tu8, w, b)
    u = loss_ref.ulps(loss.item(), l3.item())
    dw, db = ref.distance(gw.cpu().numpy(), gw3.cpu().numpy()), ref.distance(gb.cpu().numpy(), gb3.cpu().numpy())
    print(f"{case['name']}: loss {u} ulp, grad_w {dw:.3e} (bar {ref.bar(case, 'grad_w'):.3e}), grad_b {db:.3e} "
          f"(bar {ref.bar(case, 'grad_b'):.3e})")
    assert u <= 1 and dw <= ref.bar(case, "grad_w") and db <= ref.bar(case, "grad_b")


# ---------------------------------------------------------------- 3. feature type and alignment
EDGES = [(1, 1, 1, 1), (1, 3, 5, 7), (2, 2, 2, 6), (1, 4, 3, 8), (2, 3, 48, 96)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", EDGES, ids=["x".join(map(str, s)) for s in EDGES])
def test_16_bit_features_and_any_alignment_give_the_fp32_bits(shape, dtype, handle):
    """Every output -- loss, gradients, updated w, b, m, v -- of a call on fp16 / bf16 features, at bases 0, 2, 4
    and 8 bytes past a 16-byte boundary, is bitwise that of the fp32 call on the widened tensor (itself at 0, 4 and
    8 bytes)."""
    feat, w, b, tu8 = ref.generate(shape, 500 + sum(shape), 0.3, True)
    f16 = dev(feat).to(dtype)
    wide = f16.float()
    w, b, t = dev(w), dev(b), dev(tu8)
    want = update(handle, wide, t, w, b)
    assert all(torch.isfinite(x).all() for x in want) and float(want[5].abs().max()) > 0
    assert not same_bits(want[3:5], (w, b))
    for off in (4, 8):
        assert same_bits(update(handle, offset_copy(wide, off), t, w, b), want), f"fp32 base + {off}"
    for off in (0, 2, 4, 8):
        assert same_bits(update(handle, offset_copy(f16, off), t, w, b), want), f"{dtype} base + {off}"
    tf = dev(ref.target_f32(tu8))   # the fp32 target at an unaligned base too
    assert same_bits(update(handle, f16, offset_copy(tf, 4), w, b), update(handle, wide, tf, w, b))


# ---------------------------------------------------------------- 4. pages
def test_pages_select_the_batch(handle, refs):
    """A permutation and a repeated index equal the call on the gathered cache bitwise; two runs are bitwise equal;
    a host list with a bad index raises; a device index equal to P gives NaN, and nothing is read there."""
    feat, w, b, tu8 = ref.generate((4, 3, 48, 96), 450, 0.2, False)
    p = 4
    cache = torch.empty((p + 1,) + feat.shape[1:], device=DEV)   # one page more than the call is told of
    cache[:p] = dev(feat)
    cache[p] = float("inf")
    masks = torch.zeros((p + 1,) + tu8.shape[1:], device=DEV, dtype=torch.uint8)
    masks[:p] = dev(tu8)
    f, t, w, b = cache[:p], masks[:p], dev(w), dev(b)
    for idx in ([2, 0, 3, 1], [1, 1, 3]):
        pages = torch.tensor(idx, device=DEV, dtype=torch.int32)
        got = update(handle, f, t, w, b, pages=pages)
        want = update(handle, f[idx].contiguous(), t[idx].contiguous(), w, b)
        assert same_bits(got, want), idx
        assert same_bits(update(handle, f, t, w, b, pages=pages), got)
    assert not same_bits(update(handle, f, t, w, b, pages=torch.tensor([0, 1], device=DEV, dtype=torch.int32))[:1],
                         update(handle, f, t, w, b, pages=torch.tensor([2, 3], device=DEV, dtype=torch.int32))[:1])
    fit = HeadFit(w.clone(), b.clone(), 1e-2, handle=handle)
    for bad in ([0, p], [-1], []):
        with pytest.raises(IndexError):
            fit.loss_and_grads(f, t, pages=bad)
    out = update(handle, f, t, w, b, pages=torch.tensor([0, p], device=DEV, dtype=torch.int32))
    assert all(bool(torch.isnan(x).all()) for x in out)
    out = update(handle, f, t, w, b, pages=torch.tensor([-1, 1], device=DEV, dtype=torch.int32))
    assert all(bool(torch.isnan(x).all()) for x in out)


# ---------------------------------------------------------------- 5. AdamW
def test_adamw_first_step_matches_the_float64_restatement(handle):
    """m, v, w and b after step 1: torch.optim.AdamW's formulas on the fp32 gradient in float64, rounded once
    (head_step_ref.adamw).  m and v are products and sums only: bitwise; the parameter goes through a square root and
    a quotient as well, so one fp32 ulp is allowed for a tie broken the other way."""
    feat, target, w0, b0 = head_ref.trajectory_tensors()
    f, t, w, b = dev(feat), dev(target), dev(w0), dev(b0)
    _, gw, gb, w1, b1, state = update(handle, f, t, w, b)
    _, gw_only, gb_only = grads(handle, f, t, w, b)
    assert same_bits((gw, gb), (gw_only, gb_only))
    g = np.concatenate([gw.cpu().numpy().ravel(), gb.cpu().numpy()])
    theta = np.concatenate([w0.ravel(), b0])
    th, m, v = ref.adamw(theta, np.zeros_like(theta), np.zeros_like(theta), g, OPT[0], 1)
    st = state.cpu().numpy()
    assert st[:195].view(np.uint32).tolist() == m.view(np.uint32).tolist()
    assert st[195:].view(np.uint32).tolist() == v.view(np.uint32).tolist()
    got = np.concatenate([w1.cpu().numpy().ravel(), b1.cpu().numpy()])
    assert np.abs(got.view(np.int32).astype(np.int64) - th.view(np.int32).astype(np.int64)).max() <= 1
    assert np.abs(got - theta).max() > 1e-3   # a step of about lr


@pytest.mark.parametrize("lr", head_ref.TRAJ_LRS)
def test_trajectory(lr, handle):
    """train.py's loop on the head alone, 40 steps, every step one unet_head_step: every step's loss within
    8 x max(spread, 2^-23) of the reference's fp32 loop (the fixture of tests/test_head_gpu.py) and of the same loop
    on head_conv + InvoiceLoss + torch.optim.AdamW on the device."""
    traj = head_ref.trajectory_fixture()[lr]
    feat, target, w0, b0 = head_ref.trajectory_tensors()
    f, t = dev(feat), dev(target)
    n, nb = f.shape[0], head_ref.TRAJ_BATCH

    def schedule(opt):
        return torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=10, T_mult=2)

    w = torch.nn.Parameter(dev(w0).view(3, 64, 1, 1))
    b = torch.nn.Parameter(dev(b0))
    crit = InvoiceLoss()
    opt = torch.optim.AdamW([w, b], lr=lr, weight_decay=head_ref.TRAJ_WD)
    sched = schedule(opt)
    torch_losses = []
    for _ in range(head_ref.TRAJ_EPOCHS):
        for lo in range(0, n, nb):
            loss = crit(head_conv(f[lo:lo + nb], w, b), t[lo:lo + nb])
            opt.zero_grad()
            loss.backward()
            opt.step()
            torch_losses.append(loss.detach())
        sched.step()
    crit.close()

    fit = HeadFit(dev(w0), dev(b0), lr, weight_decay=head_ref.TRAJ_WD, handle=handle)
    stand_in = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    sched = schedule(stand_in)
    losses = []
    for _ in range(head_ref.TRAJ_EPOCHS):
        for lo in range(0, n, nb):
            losses.append(fit.step(f, t, list(range(lo, lo + nb)), lr=stand_in.param_groups[0]["lr"]))
        stand_in.step()
        sched.step()
    got = torch.stack(losses).cpu().numpy().astype(np.float64)
    bar = ref.SPREAD_FACTOR * max(traj["spread"], ref.FLOOR)
    assert fit.steps == len(got) == len(traj["losses"]) == 40
    for name, other in (("the reference's fp32 loop", traj["losses"].astype(np.float64)),
                        ("torch.optim.AdamW on the device", torch.stack(torch_losses).cpu().numpy().astype(np.float64))):
        rel = np.abs(got - other) / np.abs(other)
        print(f"lr {lr}: loss {got[0]:.4f} -> {got[-1]:.4f}, against {name} {rel.max():.3e} at step "
              f"{int(rel.argmax())} (bar {bar:.3e})")
        assert rel.max() <= bar


# ---------------------------------------------------------------- 6. capture
def test_capture_replays_to_the_eager_result(refs):
    """A captured step (after the reserve) replays to the eager result, on the buffers it captured; a step whose
    scratch would have to grow under capture is refused (UNET_ESTATE) before it launches."""
    feat, w, b, tu8 = (dev(a) for a in refs[IDS.index("spans")])
    h, small = native.Handle(3, 4, "fp32", 0), native.Handle(3, 4, "fp32", 0)
    eager = update(h, feat, tu8, w, b)
    h.head_step_reserve(2, 48, 96)
    wc, bc, state = w.clone(), b.clone(), torch.zeros(2 * 195, device=DEV)
    outs = (torch.zeros((), device=DEV), torch.zeros((3, 64), device=DEV), torch.zeros((3,), device=DEV))
    opt = OPT + (1,)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="unet_head_step_reserve"):
            small.head_step(feat, tu8, wc, bc, stream(), opt=opt, state=state)
        h.head_step(feat, tu8, wc, bc, stream(), opt=opt, state=state, want_grads=True, loss=outs[0], grad_w=outs[1],
                    grad_b=outs[2])
    assert same_bits((wc, bc), (w, b))   # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(outs + (wc, bc, state), eager)
    feat.copy_(feat.flip(0))   # the graph reads the buffers it captured: new features, the head where it was
    wc.copy_(w)
    bc.copy_(b)
    state.zero_()
    e2 = update(h, feat, tu8, w, b)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(outs + (wc, bc, state), e2) and not same_bits(e2[1:2], eager[1:2])
    del graph
    h.close()
    small.close()


# ---------------------------------------------------------------- 7. scratch
def test_no_output_depends_on_the_scratch_found(refs):
    """Scratch filled with 0xFF, or left over from a call of another shape, changes no output bit; the forward
    workspace's size does not move."""
    feat, w, b, tu8 = (dev(a) for a in refs[IDS.index("spans")])
    h = native.Handle(3, 4, "fp32", 0)
    before = h.workspace_bytes(2, 64, 64)
    clean = update(h, feat, tu8, w, b)
    h.debug_fill(0xFF, stream())
    assert same_bits(update(h, feat, tu8, w, b), clean)
    other = [dev(a) for a in refs[IDS.index("c4")]]
    update(h, other[0], other[3], other[1], other[2])
    h.head_step_reserve(4, 128, 96)   # a larger allocation, uninitialised
    assert same_bits(update(h, feat, tu8, w, b), clean)
    h.debug_fill(0x7F, stream())
    assert same_bits(update(h, feat, tu8, w, b), clean)
    assert h.workspace_bytes(2, 64, 64) == before
    h.close()


# ---------------------------------------------------------------- 8. NaN
def test_nan_reach(handle, refs):
    """a NaN feature reaches every logit of its pixel, so every plane of its page, so the loss
    and every gradient and updated value; a NaN target of class c reaches the loss and row c only, and leaves the
    other rows' bits."""
    feat, w, b, tu8 = (dev(a) for a in refs[IDS.index("spans")])
    clean = update(handle, feat, dev(ref.target_f32(refs[IDS.index("spans")][3])), w, b)
    f = feat.clone()
    f[1, 17, 40, 3] = float("nan")
    out = update(handle, f, tu8, w, b)
    assert all(bool(torch.isnan(x).all()) for x in out)
    t = dev(ref.target_f32(refs[IDS.index("spans")][3]))
    t[0, 1, 5, 9] = float("nan")
    loss, gw, gb, w1, b1, state = update(handle, feat, t, w, b)
    st, st0 = state.view(2, 195), clean[5].view(2, 195)
    assert bool(torch.isnan(loss)) and bool(torch.isnan(gw[1]).all()) and bool(torch.isnan(gb[1]))
    assert bool(torch.isnan(w1[1]).all()) and bool(torch.isnan(b1[1]))
    assert bool(torch.isnan(st[:, 64:128]).all()) and bool(torch.isnan(st[:, 193]).all())
    for c in (0, 2):
        got = (gw[c], gb[c], w1[c], b1[c], st[:, 64 * c:64 * c + 64], st[:, 192 + c])
        want = (clean[1][c], clean[2][c], clean[3][c], clean[4][c], st0[:, 64 * c:64 * c + 64], st0[:, 192 + c])
        assert same_bits(got, want), c


# ---------------------------------------------------------------- 9. offsets past 2^31 elements
def test_offsets_past_2_31(handle):
    """A 129-page 512 x 512 fp16 cache (2^31 + 2^24 elements), uninitialised except pages 0 and 128: pages [0, 128]
    equals the call on the two pages alone bitwise."""
    p, c, s = 129, 3, 512
    gen = torch.Generator(device=DEV).manual_seed(9)
    two = (torch.relu(torch.randn((2, 64, s, s), device=DEV, generator=gen)) * 2.5).to(torch.float16)
    masks2 = (torch.rand((2, s, s, c), device=DEV, generator=gen) < 0.2).to(torch.uint8) * 255
    cache = torch.empty((p, 64, s, s), device=DEV, dtype=torch.float16)
    masks = torch.empty((p, s, s, c), device=DEV, dtype=torch.uint8)
    assert cache.numel() > 2 ** 31
    cache[0], cache[128], masks[0], masks[128] = two[0], two[1], masks2[0], masks2[1]
    w, b = dev(head_ref.generate((1, c, 1, 1), 99)[1]), torch.full((c,), -4.0, device=DEV)
    got = update(handle, cache, masks, w, b, pages=torch.tensor([0, 128], device=DEV, dtype=torch.int32))
    want = update(handle, two, masks2, w, b)
    assert all(torch.isfinite(x).all() for x in want) and float(want[1].abs().max()) > 0
    assert same_bits(got, want)
    del cache, masks
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 10. fit_head(fused=True)
def test_fit_head_fused():
    """The four-page 64 x 64 probe of tests/test_head_gpu.py: the fused loop's epoch losses within the trajectory
    bar of the unfused loop's; only out_conv moves; and the fused forward afterwards scores what the head scores on
    the features -- the native update moved the parameters' version counters, so the handle re-packed the head."""
    from test_head_gpu import probe_setup
    sd, x, t = probe_setup()
    xd, td = dev(x), dev(t)
    runs = {}
    for fused in (False, True):
        m = UNet(3, 3, compute_dtype="fp32")
        m.load_state_dict(sd)
        m = m.to(DEV).eval()
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m(xd[:1])   # the handle packs the old head: the fit has to replace it
        versions = (m.out_conv.weight._version, m.out_conv.bias._version)
        losses = m.fit_head(xd, td, epochs=20, batch=2, lr=1e-2, fused=fused)
        changed = sorted(k for k, v in m.state_dict().items() if not torch.equal(v, before[k]))
        assert changed == ["out_conv.bias", "out_conv.weight"] and not m.training
        assert m.out_conv.weight._version > versions[0] and m.out_conv.bias._version > versions[1]
        runs[fused] = (np.array(losses, np.float64), m)
    got, want = runs[True][0], runs[False][0]
    rel = np.abs(got - want) / np.abs(want)
    bar = ref.SPREAD_FACTOR * max(head_ref.trajectory_fixture()[1e-2]["spread"], ref.FLOOR)
    print(f"fit_head fused: epoch losses {got[0]:.4f} -> {got[-1]:.4f}, against the unfused loop {rel.max():.3e} at "
          f"epoch {int(rel.argmax())} (bar {bar:.3e})")
    assert len(got) == 20 and got[-1] < 0.5 * got[0] and rel.max() <= bar
    m = runs[True][1]
    through_fused = m.score(xd, td).loss(batch=2)
    fit = HeadFit(m.out_conv.weight.detach().clone(), m.out_conv.bias.detach().clone(), 1e-2)
    feats = m.features(xd)
    through_head = float(sum(fit.loss_and_grads(feats, td, pages=[lo, lo + 1])[0] for lo in (0, 2)).item()) / 2
    print(f"after the fused fit: fused forward {through_fused:.6f}, head on the features {through_head:.6f}")
    # the two paths differ by the fp32 plan's forward error (2e-5 of the logits' scale: test_forward_gpu.py)
    assert abs(through_fused - through_head) <= 1e-3 * through_head and through_fused < 0.5 * got[0]
    # shuffled batches and a short last batch run too
    more = m.fit_head(xd[:3], td[:3], epochs=2, batch=2, lr=1e-3, shuffle_seed=1, fused=True, feature_dtype="fp16")
    assert len(more) == 2 and all(np.isfinite(more))
    for _, mm in runs.values():
        mm.close()
