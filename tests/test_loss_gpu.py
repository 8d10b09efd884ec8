"""unet_loss_grad on the device: against the reference's fp32 loss and autograd gradient (tests/golden/
loss_cases.npz), the numpy restatement (tests/loss_ref.py) and unet_score's entries, through native.Handle,
metrics.InvoiceLoss (autograd) and UNet.loss_grad.  Needs a GPU: run with -m gpu.

Bars: the gradient within 8 x the case's own spread (the reference's fp32 autograd against its fp64 autograd) of
the reference's, as max |g - g_ref| / max |g_ref|; the loss within 1 fp32 ulp of metrics.Score.loss() of
unet_score's entries for the same tensors.  Logits of the accuracy cases avoid 14 < |x| < 20, where the clamp of
train.py:41 makes correct fp32 implementations disagree element by element; that band has a property test.

Largest distances observed on MI355X: see test_fixture_cases' docstring.
"""
import numpy as np
import pytest
import torch

import loss_ref
from loss_ref import SPREAD_FACTOR
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.metrics import InvoiceLoss, Score
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = loss_ref.fixture()
IDS = [c["name"] for c in CASES]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ulp_distance(a, b):
    """Largest distance of two fp32 arrays in units in the last place (sign-magnitude order)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


@pytest.fixture(scope="module")
def handle():
    h = native.Handle(3, 4, "fp32", 0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def crit():
    c = InvoiceLoss()
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """Per case, once: (logits, target uint8 NHWC, target fp32 NCHW, restatement's loss, restatement's gradient)."""
    out = []
    for case in CASES:
        x, tu8 = loss_ref.case_tensors(case)
        tf = loss_ref.target_f32(tu8)
        out.append((x, tu8, tf) + loss_ref.loss_grad(x, tf))
    return out


def run(h, x, t, **kw):
    loss, grad = h.loss_grad(dev(x), dev(t), stream(), **kw)
    return loss.cpu().numpy(), None if grad is None else grad.cpu().numpy()


@pytest.mark.parametrize("form", ["f32_nchw", "u8_nhwc"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixture_cases(i, form, handle, refs):
    """Every fixture case in both target forms: the gradient within 8 x spread of the reference's, the NaN pattern
    the fixture's, the loss within 1 ulp of Score.loss() of unet_score's entries and within 8 x spread of the
    reference's, and the loss-only call the same loss bitwise.

    Largest distances observed on MI355X: see DESIGN.md section 10."""
    case = CASES[i]
    x, tu8, tf, _, g_np = refs[i]
    t = tf if form == "f32_nchw" else tu8
    loss, g = run(handle, x, t)
    bar = SPREAD_FACTOR * case["spread"]
    d = loss_ref.grad_distance(g, case["grad"])
    entries, _ = handle.score(dev(x), dev(t), stream())
    want = np.float32(Score(entries.cpu().numpy()).loss())
    print(f"{IDS[i]} {form}: gradient {d:.3e} from the reference (bar {bar:.3e}), "
          f"{loss_ref.grad_distance(g, g_np):.3e} from the restatement; loss {loss!r}, Score.loss {want!r}, "
          f"reference {case['loss']!r}")
    assert g.dtype == np.float32 and g.shape == case["shape"]
    assert np.array_equal(np.isnan(g), np.isnan(case["grad"]))
    assert np.isfinite(g[~np.isnan(g)]).all()
    assert d <= bar
    if case["nan_at"] is None:
        assert loss_ref.ulps(loss, want) <= 1, (loss, want)
        assert abs(float(loss) - float(case["loss"])) <= bar * abs(float(case["loss"]))
    else:
        assert np.isnan(loss) and np.isnan(want)
    only, none = run(handle, x, t, want_grad=False)
    assert none is None and only.tobytes() == loss.tobytes()


def test_both_target_forms_agree_bitwise(handle, refs):
    x, tu8, tf, _, _ = refs[IDS.index("c4")]
    la, ga = run(handle, x, tf)
    lb, gb = run(handle, x, tu8)
    assert la.tobytes() == lb.tobytes() and ga.tobytes() == gb.tobytes()


def test_clamp_band(handle):
    """Logits swept over +-[14, 20], both target values: every gradient finite, >= 0 where t = 0 and <= 0 where
    t = 1 (2 I + s <= U + s), and no larger than the restatement's largest on the page.  No element-wise comparison:
    one ulp of expf decides on which side of the clamp an element of this band falls."""
    sweep = np.linspace(14.0, 20.0, 768, dtype=np.float32)
    x = np.concatenate([sweep, -sweep]).reshape(1, 3, 8, 64)
    t = (np.arange(x.size) % 2).astype(np.float32).reshape(x.shape)
    for sign in (1, -1):
        for tv in (0, 1):
            assert ((np.sign(x) == sign) & (t == tv)).sum() >= 256
    _, g_np = loss_ref.loss_grad(x, t)
    for tgt in (t, np.ascontiguousarray((t * 255).astype(np.uint8).transpose(0, 2, 3, 1))):
        loss, g = run(handle, x, tgt)
        print(f"clamp band: max |g| device {np.abs(g).max():.6e} restatement {np.abs(g_np).max():.6e}; "
              f"elements differing by > 1e-3 max: {(np.abs(g - g_np) > 1e-3 * np.abs(g_np).max()).sum()} of {g.size}")
        assert np.isfinite(loss) and np.isfinite(g).all()
        assert (g[t == 0] >= 0).all() and (g[t == 1] <= 0).all()
        assert np.abs(g).max() <= (1 + 1e-3) * np.abs(g_np).max()


def test_nan_logit(handle, refs):
    """The NaN pattern of loss and gradient is the restatement's: the loss and the NaN logit's whole (n, c) plane,
    nothing else; the other planes are bitwise those of the same call with the NaN replaced."""
    i = IDS.index("nan")
    x, tu8, _, l_np, g_np = refs[i]
    n, c = CASES[i]["nan_at"][:2]
    loss, g = run(handle, x, tu8)
    assert np.isnan(loss) and np.isnan(l_np)
    assert np.array_equal(np.isnan(g), np.isnan(g_np))
    assert np.isnan(g[n, c]).all() and np.isnan(g).sum() == g[n, c].size
    _, g0 = run(handle, np.where(np.isnan(x), np.float32(0), x), tu8)
    keep = np.ones(x.shape[:2], bool)
    keep[n, c] = False
    assert g[keep].tobytes() == g0[keep].tobytes()


# ---------------------------------------------------------------- autograd
def test_backward_scales_by_the_upstream_gradient(crit, handle, refs):
    x, tu8, tf, _, _ = refs[IDS.index("odd")]
    _, direct = run(handle, x, tf)
    for tgt in (tf, tu8):
        xd = dev(x).requires_grad_()
        loss = crit(xd, dev(tgt))
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
        (3 * loss).backward()
        assert ulp_distance(xd.grad.cpu().numpy(), np.float32(3) * direct) <= 1
    xd = dev(x).requires_grad_()
    crit(xd, dev(tf)).backward()
    assert xd.grad.cpu().numpy().tobytes() == direct.tobytes()
    crit(xd, dev(tf)).backward()   # a second backward accumulates
    assert xd.grad.cpu().numpy().tobytes() == (direct + direct).tobytes()


def test_device_upstream_argument(handle, refs):
    """grad_out on the device scales inside the kernels: a power of two exactly."""
    x, _, tf, _, _ = refs[IDS.index("c4")]
    l1, g1 = run(handle, x, tf)
    l2, g2 = run(handle, x, tf, grad_out=torch.tensor([0.5], device=DEV))
    assert l1.tobytes() == l2.tobytes() and g2.tobytes() == (np.float32(0.5) * g1).tobytes()


def test_non_contiguous_pred_and_no_grad(crit, refs):
    x, tu8, tf, _, _ = refs[IDS.index("far")]
    xd = dev(x).requires_grad_()
    loss = crit(xd, dev(tu8))
    loss.backward()
    base = dev(x.transpose(0, 2, 3, 1)).requires_grad_()   # NHWC storage
    pred = base.permute(0, 3, 1, 2)
    assert not pred.is_contiguous()
    loss2 = crit(pred, dev(tu8))
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(base.grad.permute(0, 3, 1, 2), xd.grad)

    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    t = dev(tu8)
    with torch.no_grad():
        quiet = crit(xd, t)
    grown = torch.cuda.memory_allocated(DEV) - before - t.numel()
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, loss)
    assert grown < x.size * 4 // 2, "no gradient buffer under no_grad"
    plain = crit(dev(x), t)   # nothing requires a gradient
    assert plain.grad_fn is None and torch.equal(plain, loss)


def test_criterion_weights(refs):
    x, _, tf, _, _ = refs[IDS.index("c1")]
    c = InvoiceLoss(dice_weight=0.5, focal_weight=0.5, focal_alpha=0.25)
    xd = dev(x).requires_grad_()
    loss = c(xd, dev(tf))
    loss.backward()
    l_np, g_np = loss_ref.loss_grad(x, tf, weights=(0.5, 0.5, 0.25, 1.0))
    assert loss_ref.ulps(loss.item(), l_np) <= 1
    assert loss_ref.grad_distance(xd.grad.cpu().numpy(), g_np) <= SPREAD_FACTOR * CASES[IDS.index("c1")]["spread"]
    c.close()


def test_criterion_refuses_bad_tensors(crit):
    x = torch.zeros(1, 3, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        crit(x.double(), torch.zeros(1, 3, 4, 4, device=DEV))
    with pytest.raises(ValueError, match="target must be"):
        crit(x, torch.zeros(1, 3, 4, 4, device=DEV, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        crit(x, torch.zeros(1, 3, 4, 5, device=DEV))
    with pytest.raises(ValueError, match="shape"):
        crit(x, torch.zeros(1, 3, 4, 4, device=DEV, dtype=torch.uint8))   # uint8 is NHWC: [1, 4, 4, 3]
    with pytest.raises(ValueError, match="on cuda"):
        crit(x, torch.zeros(1, 3, 4, 4))


def test_unet_loss_grad_is_forward_then_criterion(crit):
    sd = syn.make_state_dict(7, 3, 3, profile="structured")
    m = UNet(3, 3, compute_dtype="fp32")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(DEV).eval()
    x = dev(syn.invoice_pages(7, 1, 32, 32, 3))
    t = dev(np.where(np.random.RandomState(7).rand(1, 32, 32, 3) < 0.3, 255, 0).astype(np.uint8))
    loss, grad = m.loss_grad(x, t)
    assert loss.dim() == 0 and grad.shape == (1, 3, 32, 32) and loss.grad_fn is None
    logits = m(x).requires_grad_()
    l2 = crit(logits, t)
    l2.backward()
    assert torch.equal(loss, l2.detach()) and torch.equal(grad, logits.grad)
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    l3, g3 = m.loss_grad(x, t, criterion=InvoiceLoss(0.5, 0.5, 0.25))
    assert not torch.equal(l3, loss) and not torch.equal(g3, grad)
    with pytest.raises(TypeError):
        m.loss_grad(x, t, criterion=torch.nn.MSELoss())
    m.close()


# ---------------------------------------------------------------- reproducibility, capture
@pytest.mark.parametrize("name", ["odd", "spans"])
def test_bitwise_reproducible_and_independent_of_alignment(name, handle, refs):
    x, tu8, tf, _, _ = refs[IDS.index(name)]
    for tgt in (tf, tu8):
        la, ga = run(handle, x, tgt)
        lb, gb = run(handle, x, tgt)
        assert la.tobytes() == lb.tobytes() and ga.tobytes() == gb.tobytes()
        # the same tensors one element into larger buffers: every plane's alignment moves by 4 bytes (target: 4 or 1)
        xo = torch.empty(x.size + 1, device=DEV)[1:].view(x.shape).copy_(dev(x))
        to = torch.empty(tgt.size + 1, device=DEV, dtype=dev(tgt).dtype)[1:].view(tgt.shape).copy_(dev(tgt))
        go = torch.empty(x.size + 1, device=DEV)[1:].view(x.shape)
        assert xo.data_ptr() % 16 == 4 and go.data_ptr() % 16 == 4 and xo.is_contiguous()
        lo, _ = handle.loss_grad(xo, to, stream(), grad=go)
        assert lo.cpu().numpy().tobytes() == la.tobytes() and go.cpu().numpy().tobytes() == ga.tobytes()


def test_elements_past_2_31(handle):
    """129 x 4 x 2048 x 2048 = 2^31 + 2^24 elements, every image a copy of the first: element offsets past 2^31 are
    the only thing that can go wrong here and not at the small shapes.  Each image's gradient must then be bitwise
    the first image's (same plane sums, same coefficients), the last one included."""
    n, c, s = 129, 4, 2048
    g = torch.Generator(device=DEV).manual_seed(3)
    x1 = torch.randn((1, c, s, s), device=DEV, generator=g) * 3.0 - 2.0
    t1 = torch.where(torch.rand((1, s, s, c), device=DEV, generator=g) < 0.2, 255, 0).to(torch.uint8)
    x = x1.expand(n, c, s, s).contiguous()
    t = t1.expand(n, s, s, c).contiguous()
    assert x.numel() > 2 ** 31
    loss, grad = handle.loss_grad(x, t, stream())
    _, one = handle.loss_grad(x1, t1, stream())
    assert torch.isfinite(loss) and torch.isfinite(grad[-1]).all() and float(grad[-1].abs().max()) > 0
    assert torch.equal(grad[-1], grad[0]) and torch.equal(grad[n // 2], grad[0])
    # against the one-image call: the same Dice coefficients up to the 1 / N of the mean, g0 likewise
    assert torch.allclose(grad[-1] * n, one[0], rtol=1e-5, atol=0)
    del x, t, grad, one
    torch.cuda.empty_cache()


def test_scratch_grows_and_leaves_the_forward_workspace_alone(refs):
    x, tu8, _, _, _ = refs[IDS.index("spans")]
    h = native.Handle(3, 3, "fp32", 0)
    before = h.workspace_bytes(2, 64, 64)
    h.loss_reserve(1, 16, 16)   # smaller: the call below must grow it
    la, ga = run(h, x, tu8)
    h.loss_reserve(4, 64, 96)
    lb, gb = run(h, x, tu8)
    assert la.tobytes() == lb.tobytes() and ga.tobytes() == gb.tobytes()
    assert h.workspace_bytes(2, 64, 64) == before
    h.close()


def test_capture_replays_to_the_eager_result(refs):
    """One torch.cuda.graph capture of a loss_grad call (a single stream, no parallel branches) after
    loss_reserve: the replay equals the eager call bitwise, also on new contents of the captured buffers."""
    x, tu8, _, _, _ = refs[IDS.index("spans")]
    h = native.Handle(3, 3, "fp32", 0)
    xd, td = dev(x), dev(tu8)
    loss = torch.zeros((), device=DEV)
    grad = torch.zeros(x.shape, device=DEV)
    h.loss_reserve(2, 48, 96)
    le, ge = h.loss_grad(xd, td, stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.loss_grad(xd, td, stream(), loss=loss, grad=grad)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, le) and torch.equal(grad, ge)
    xd.copy_(-xd)   # the graph reads the buffers it captured
    l2, g2 = h.loss_grad(xd, td, stream())
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, l2) and torch.equal(grad, g2) and not torch.equal(l2, le)
    del g
    h.close()
