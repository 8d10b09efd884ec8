"""The head score on the device (unet_head_score, include/unet_mi355x.h): out_conv's logits
scored from the feature cache in one pass.  Against the two native calls it replaces, against the reference's loss
(tests/golden/head_step_cases.npz), and the properties the header states: bitwise independence of feature type,
alignment, N and slot, page indices, NaN reach, thresholds, capture, scratch, 64-bit offsets; then ``fit_head`` with
held-out pages and ``finetune_head(val_fraction=)`` end to end."""
import ctypes

import numpy as np
import pytest
import torch

import head_ref
import head_score_ref as ref
import head_step_ref
from unet_mi355x import head, native
from unet_mi355x import synthetic as syn
from unet_mi355x.metrics import ENTRY_DTYPE, Score
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = ref.fixture()
IDS = [c["name"] for c in CASES]
SUMS = ("sum_p", "sum_t", "sum_pt", "sum_focal")
COUNTS = ("n_pred", "n_tgt", "n_both", "n_px")
SWEEPS = {"K0": None, "K1": ref.SWEEP_1, "K19": ref.SWEEP, "K64": ref.SWEEP_64}


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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
    """per case (the fixture's, then the 33 x 130 tail): the generated host tensors, made once"""
    out = {c["name"]: ref.case_tensors(c) for c in CASES}
    out[ref.TAIL[0]] = head_step_ref.generate(*ref.TAIL[1:])
    return out


def host(entries, hist):
    e = entries.cpu().numpy().view(ENTRY_DTYPE)[..., 0]
    return e, None if hist is None else hist.cpu().numpy()


def fused(h, feat, target, w, b, **kw):
    """(entries [N, C], hist or None) on the host, from one unet_head_score"""
    return host(*h.head_score(feat, target, w, b, stream(), **kw))


def two_calls(h, feat, target, w, b, thresholds=None, sweep=None):
    """the same from unet_head_forward(_typed) followed by unet_score"""
    return host(*h.score(h.head_forward(feat, w, b, stream()), target, stream(), thresholds=thresholds, sweep=sweep))


def same(a, b):
    """two (entries, hist) results, bit for bit"""
    return a[0].tobytes() == b[0].tobytes() and (a[1] is None) == (b[1] is None) and \
        (a[1] is None or np.array_equal(a[1], b[1]))


# ---------------------------------------------------------------- 1. the two native calls it replaces
@pytest.mark.parametrize("sweep", list(SWEEPS), ids=list(SWEEPS))
@pytest.mark.parametrize("name", IDS + [ref.TAIL[0]])
def test_against_the_two_native_calls(name, sweep, handle, refs):
    """unet_score(unet_head_forward_typed(feat)) on the same tensors, both target forms: counts and every bin equal,
    the four sums within 2 H W 2^-53 of the value (fp64 sums of non-negative fp32 terms over two trees)."""
    feat, w, b, tu8 = refs[name]
    f, wd, bd = dev(feat), dev(w), dev(b)
    hw = feat.shape[2] * feat.shape[3]
    for target in (dev(tu8), dev(ref.target_f32(tu8))):
        got = fused(handle, f, target, wd, bd, sweep=SWEEPS[sweep])
        want = two_calls(handle, f, target, wd, bd, sweep=SWEEPS[sweep])
        for k in COUNTS:
            assert np.array_equal(got[0][k], want[0][k]), k
        assert (got[0]["n_px"] == hw).all()
        assert (got[1] is None) == (SWEEPS[sweep] is None)
        if got[1] is not None:
            assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1])
            assert (got[1].sum((-1, -2)) == hw).all()
        for k in SUMS:
            err = np.abs(got[0][k] - want[0][k])
            worst = float((err / np.maximum(np.abs(want[0][k]), 1e-300)).max())
            print(f"{name} {sweep} {target.dtype} {k}: {worst:.3e} relative (bar {2.0 * hw * 2.0 ** -53:.3e})")
            assert np.isfinite(got[0][k]).all()
            assert (err <= np.vectorize(ref.sum_bar)(hw, want[0][k])).all(), k


# ---------------------------------------------------------------- 2. the reference
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_reference_loss(i, handle, refs):
    """Score.loss() of the entries within 8 x max(spread, 2^-23) of the reference's fp32 loss; the entries beside
    the float64 restatement's."""
    case = CASES[i]
    feat, w, b, tu8 = refs[case["name"]]
    for target in (dev(tu8), dev(ref.target_f32(tu8))):
        e, _ = fused(handle, dev(feat), target, dev(w), dev(b))
        got = np.float32(Score(e).loss())
        d = head_step_ref.distance(got, case["loss"])
        print(f"{case['name']} {target.dtype} loss {got:.7f}: {d:.3e} (bar {ref.bar(case, 'loss'):.3e})")
        assert np.isfinite(got) and d <= ref.bar(case, "loss")
        assert abs(ref.loss(e) - Score(e).loss()) == 0.0


# ---------------------------------------------------------------- 3. feature type and alignment
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["one", "odd", "spans", ref.TAIL[0]])
def test_16_bit_features_and_any_alignment_give_the_fp32_bits(name, dtype, handle, refs):
    """fp16 / bf16 caches give the bits of the fp32 call on the widened tensor; a base one element past a 16-byte
    boundary (features, and the fp32 target) gives the same bits; two runs give the same bits."""
    feat, w, b, tu8 = refs[name]
    f16 = dev(feat).to(dtype)
    wide = f16.float()
    wd, bd, t = dev(w), dev(b), dev(tu8)
    want = fused(handle, wide, t, wd, bd, sweep=ref.SWEEP)
    assert np.isfinite(want[0]["sum_focal"]).all() and want[0]["sum_p"].min() > 0
    assert same(fused(handle, wide, t, wd, bd, sweep=ref.SWEEP), want)
    assert same(fused(handle, offset_copy(wide, 4), t, wd, bd, sweep=ref.SWEEP), want)
    for off in (0, 2):
        assert same(fused(handle, offset_copy(f16, off), t, wd, bd, sweep=ref.SWEEP), want), f"{dtype} base + {off}"
    tf = dev(ref.target_f32(tu8))
    assert same(fused(handle, f16, offset_copy(tf, 4), wd, bd, sweep=ref.SWEEP),
                fused(handle, wide, tf, wd, bd, sweep=ref.SWEEP))
    assert same(fused(handle, offset_copy(f16, 2), offset_copy(t, 1), wd, bd), fused(handle, wide, t, wd, bd))


# ---------------------------------------------------------------- 4. pages
def test_pages_select_the_slots(handle):
    """Permuted and repeated indices give the in-order entries rearranged by slot; a slot's entry does not depend on
    N or on the other slots; no pages means in order; a host list with a bad index raises; device indices -1 and P
    give that slot NaN sums, zero counts and bins and n_px = H W, and leave the other slots' bits.

    The guard (head_score_pass_kernel, csrc/unet_hscore.hip): ``page`` is pages[n] with n = blockIdx.x / spans < N,
    and ``if (page < 0 || page >= P)`` stores the NaN partial and returns before fbase, the target address or any
    barrier is formed from it.  The cache here keeps a spare page on either side of the P pages the call is told
    of, so -1 and P name memory of this test whatever the kernel did with them."""
    feat, w, b, tu8 = head_step_ref.generate((4, 3, 48, 96), 450, 0.2, False)
    p, hw = 4, 48 * 96
    cache = torch.full((p + 2,) + feat.shape[1:], float("inf"), device=DEV)
    cache[1:p + 1] = dev(feat)
    masks = torch.zeros((p + 2,) + tu8.shape[1:], device=DEV, dtype=torch.uint8)
    masks[1:p + 1] = dev(tu8)
    f, t, w, b = cache[1:p + 1], masks[1:p + 1], dev(w), dev(b)

    def at(idx, **kw):
        return fused(handle, f, t, w, b, pages=torch.tensor(idx, device=DEV, dtype=torch.int32), sweep=ref.SWEEP, **kw)

    base = fused(handle, f, t, w, b, sweep=ref.SWEEP)
    assert base[0].shape == (p, 3) and np.isfinite(base[0]["sum_focal"]).all()
    assert len({base[0][i].tobytes() for i in range(p)}) == p   # the pages differ
    assert same(at([0, 1, 2, 3]), base)
    for idx in ([2, 0, 3, 1], [1, 1, 3], [2], [3, 3, 3, 3, 3, 0]):
        got = at(idx)
        assert same(got, (base[0][idx], base[1][idx])), idx
    assert same(host(*handle.head_score(f[:2], t[:2], w, b, stream(), sweep=ref.SWEEP)), (base[0][:2], base[1][:2]))
    for bad in ([0, p], [-1], []):
        with pytest.raises(IndexError):
            head.head_score(f, w, b, t, pages=bad, handle=handle)
    ok = head.head_score(f, w, b, t, pages=[3, 1], sweep=ref.SWEEP, handle=handle)
    assert ok.entries.tobytes() == base[0][[3, 1]].tobytes() and np.array_equal(ok.hist, base[1][[3, 1]])
    for idx, out in (([0, p, 2], 1), ([-1, 1], 0), ([3, -1, p], 1)):
        e, hist = at(idx)
        for slot, page in enumerate(idx):
            if 0 <= page < p:
                assert e[slot].tobytes() == base[0][page].tobytes() and np.array_equal(hist[slot], base[1][page])
            else:
                assert all(np.isnan(e[slot][k]).all() for k in SUMS)
                assert all((e[slot][k] == 0).all() for k in COUNTS[:3]) and (e[slot]["n_px"] == hw).all()
                assert (hist[slot] == 0).all()


# ---------------------------------------------------------------- 5. NaN
def test_nan_reach(handle, refs):
    """A NaN feature makes the four sums of every class of its page NaN, counts as not predicted and lands in bin 0
    of its target row; other pages keep their bits.  A NaN fp32 target of class c reaches class c's sums only."""
    feat, w, b, tu8 = (dev(a) for a in refs["spans"])
    tf = dev(ref.target_f32(refs["spans"][3]))
    clean = fused(handle, feat, tf, w, b, sweep=ref.SWEEP)
    lib = native.load_library()
    y, x = 40, 3
    logits = handle.head_forward(feat, w, b, stream())[1, :, y, x].cpu().numpy()
    f = feat.clone()
    f[1, 17, y, x] = float("nan")
    e, hist = fused(handle, f, tf, w, b, sweep=ref.SWEEP)
    assert e[0].tobytes() == clean[0][0].tobytes() and np.array_equal(hist[0], clean[1][0])
    want_hist = clean[1][1].copy()
    for c in range(3):
        assert all(np.isnan(e[1, c][k]) for k in SUMS)
        tv = int(float(tf[1, c, y, x]) > 0.5)
        was_pred = bool(logits[c] > lib.unet_logit_cut(ctypes.c_float(handle_threshold(c))))
        was_bin = sum(bool(logits[c] > lib.unet_logit_cut(ctypes.c_float(q))) for q in ref.SWEEP)
        assert e[1, c]["n_pred"] == clean[0][1, c]["n_pred"] - int(was_pred)
        assert e[1, c]["n_both"] == clean[0][1, c]["n_both"] - int(was_pred and tv == 1)
        assert e[1, c]["n_tgt"] == clean[0][1, c]["n_tgt"]
        want_hist[c, tv, was_bin] -= 1
        want_hist[c, tv, 0] += 1
    assert np.array_equal(hist[1], want_hist)
    e2, hist2 = two_calls(handle, f, tf, w, b, sweep=ref.SWEEP)
    assert np.array_equal(hist, hist2) and all(np.array_equal(e[k], e2[k]) for k in COUNTS)
    t = tf.clone()
    t[0, 1, 5, 9] = float("nan")
    e, hist = fused(handle, feat, t, w, b, sweep=ref.SWEEP)
    assert all(np.isnan(e[0, 1][k]) for k in ("sum_t", "sum_pt", "sum_focal"))
    assert e[0, 1]["sum_p"] == clean[0][0, 1]["sum_p"]
    for n, c in ((0, 0), (0, 2), (1, 0), (1, 1), (1, 2)):
        assert e[n, c].tobytes() == clean[0][n, c].tobytes() and np.array_equal(hist[n, c], clean[1][n, c]), (n, c)


def handle_threshold(c):
    """native.Handle's default thresholds"""
    return (0.25, 0.40, 0.30, 0.5)[c]


# ---------------------------------------------------------------- 6. thresholds
def test_thresholds(handle, refs):
    """The thresholds argument overrides the handle's; UNet.score_features scores at the model's."""
    feat, w, b, tu8 = (dev(a) for a in refs["big"])
    default = fused(handle, feat, tu8, w, b)
    assert same(fused(handle, feat, tu8, w, b, thresholds=[handle_threshold(c) for c in range(3)]), default)
    thr = (0.02, 0.6, 0.011)
    moved = fused(handle, feat, tu8, w, b, thresholds=thr)
    want = two_calls(handle, feat, tu8, w, b, thresholds=thr)
    assert np.array_equal(moved[0]["n_pred"], want[0]["n_pred"]) and np.array_equal(moved[0]["n_both"], want[0]["n_both"])
    assert not np.array_equal(moved[0]["n_pred"], default[0]["n_pred"])
    for k in SUMS + ("n_tgt",):
        assert moved[0][k].tobytes() == default[0][k].tobytes()
    m = UNet(3, 3, compute_dtype="fp32", thresholds=thr).to(DEV).eval()
    with torch.no_grad():
        m.out_conv.weight.copy_(w.view(3, 64, 1, 1))
        m.out_conv.bias.copy_(b)
    got = m.score_features(feat, tu8, sweep=ref.SWEEP)
    assert got.entries.tobytes() == moved[0].tobytes()
    assert np.array_equal(got.hist, fused(handle, feat, tu8, w, b, sweep=ref.SWEEP)[1])
    part = m.score_features(feat, tu8, pages=[1])
    assert part.entries.tobytes() == moved[0][[1]].tobytes()
    m.close()


# ---------------------------------------------------------------- 7. capture
def test_capture_replays_to_the_eager_result(refs):
    """A captured score (after the reserve) replays to the eager bits, on the buffers it captured; a score whose
    scratch would have to grow under capture is refused (UNET_ESTATE) before it launches."""
    feat, w, b, tu8 = (dev(a) for a in refs["spans"])
    h, small = native.Handle(3, 4, "fp32", 0), native.Handle(3, 4, "fp32", 0)
    eager = fused(h, feat, tu8, w, b, sweep=ref.SWEEP)
    h.head_score_reserve(2, 48, 96, len(ref.SWEEP))
    entries = torch.zeros((2, 3, 64), device=DEV, dtype=torch.uint8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="unet_head_score_reserve"):
            small.head_score(feat, tu8, w, b, stream(), sweep=ref.SWEEP)
        _, hist = h.head_score(feat, tu8, w, b, stream(), sweep=ref.SWEEP, entries=entries)
    assert not entries.any()   # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert same(host(entries, hist), eager)
    feat.copy_(feat.flip(0))   # the graph reads the buffers it captured: the two pages change places
    tu8.copy_(tu8.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert same(host(entries, hist), (eager[0][::-1], eager[1][::-1]))
    del graph
    h.close()
    small.close()


# ---------------------------------------------------------------- 8. scratch
def test_no_output_depends_on_the_scratch_found(refs):
    """Scratch filled with 0xFF, or left over from a call of another shape, changes no output bit; the forward
    workspace's size does not move."""
    feat, w, b, tu8 = (dev(a) for a in refs["spans"])
    h = native.Handle(3, 4, "fp32", 0)
    before = h.workspace_bytes(2, 64, 64)
    clean = fused(h, feat, tu8, w, b, sweep=ref.SWEEP)
    plain = fused(h, feat, tu8, w, b)
    h.debug_fill(0xFF, stream())
    assert same(fused(h, feat, tu8, w, b, sweep=ref.SWEEP), clean)
    h.debug_fill(0xFF, stream())
    assert same(fused(h, feat, tu8, w, b), plain)
    other = [dev(a) for a in refs["c4"]]
    fused(h, other[0], other[3], other[1], other[2], sweep=ref.SWEEP_64)
    h.head_score_reserve(4, 128, 96, 64)   # a larger allocation, uninitialised
    assert same(fused(h, feat, tu8, w, b, sweep=ref.SWEEP), clean)
    h.debug_fill(0x7F, stream())
    assert same(fused(h, feat, tu8, w, b, sweep=ref.SWEEP), clean)
    bad = torch.tensor([0, 7], device=DEV, dtype=torch.int32)   # the NaN slot's partials are stored, not found
    first = fused(h, feat, tu8, w, b, pages=bad, sweep=ref.SWEEP)
    h.debug_fill(0xFF, stream())
    again = fused(h, feat, tu8, w, b, pages=bad, sweep=ref.SWEEP)
    assert same(again, first) and (again[1][1] == 0).all() and (again[0][1]["n_pred"] == 0).all()
    assert h.workspace_bytes(2, 64, 64) == before
    h.close()


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
    got = fused(handle, cache, masks, w, b, pages=torch.tensor([0, 128], device=DEV, dtype=torch.int32),
                sweep=ref.SWEEP)
    want = fused(handle, two, masks2, w, b, sweep=ref.SWEEP)
    assert np.isfinite(want[0]["sum_focal"]).all() and want[0]["n_tgt"].min() > 0
    assert want[0][0].tobytes() != want[0][1].tobytes()
    assert same(got, want)
    del cache, masks
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 10. fit_head with held-out pages
def six_pages():
    """(pretrained state_dict with the head re-initialised as tests/test_head_gpu.py's probe, six 64 x 64 pages,
    their targets fp32 0/1)."""
    from test_head_gpu import probe_setup
    sd, _, _ = probe_setup()
    x = syn.invoice_pages(5, 6, 64, 64, 3)
    t = (syn.invoice_fields(5, 6, 64, 64) > 0).astype(np.float32)
    return sd, x, t


def probe_model(sd):
    m = UNet(3, 3, compute_dtype="fp32")
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def f32_bits(values):
    return np.asarray(values, np.float64).tobytes()


@pytest.mark.parametrize("fused_steps", [False, True], ids=["unfused", "fused"])
def test_fit_head_with_validation(fused_steps):
    """Six pages, batch 2 (the forward's plan depends on N: the four training pages get the same feature bits
    whether two more follow or not), 12 epochs, a seeded shuffle."""
    sd, x, t = six_pages()
    xd, td = dev(x), dev(t)
    kw = dict(epochs=12, batch=2, lr=1e-2, shuffle_seed=3, fused=fused_steps)
    m4 = probe_model(sd)
    want = m4.fit_head(xd[:4], td[:4], **kw)
    m4.close()

    # the last epoch kept
    m = probe_model(sd)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    report = {}
    losses = m.fit_head(xd, td, val_pages=[4, 5], report=report, **kw)
    assert f32_bits(losses) == f32_bits(want)   # training saw pages 0..3 only, in the same order
    changed = sorted(k for k, v in m.state_dict().items() if not torch.equal(v, before[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"] and not m.training
    assert sorted(report) == ["best_epoch", "heads", "val_iou", "val_loss"]
    assert len(report["val_loss"]) == 12 and all(np.isfinite(report["val_loss"]))
    assert report["val_iou"].shape == (12, 3) and report["heads"].shape == (12, 195)
    assert report["heads"].dtype == np.float32 and len({h.tobytes() for h in report["heads"]}) == 12
    cache = m.feature_cache(xd, batch=2)
    again = m.score_features(cache, td, pages=[4, 5])
    assert report["val_loss"][-1] == again.loss()
    assert np.array_equal(report["val_iou"][-1], again.pooled_iou())
    head_now = np.concatenate([m.out_conv.weight.detach().cpu().numpy().ravel(), m.out_conv.bias.detach().cpu().numpy()])
    assert head_now.tobytes() == report["heads"][-1].tobytes()
    print(f"fit_head(fused={fused_steps}) validation loss per epoch: "
          + " ".join(f"{v:.4f}" for v in report["val_loss"]))
    m.close()

    # the best epoch kept, and thresholds from a sweep
    m = probe_model(sd)
    m(xd[:1])   # the handle packs the old head: the kept one has to replace it
    best = {}
    losses = m.fit_head(xd, td, val_pages=[4, 5], keep_best=True, sweep=ref.SWEEP, report=best, **kw)
    assert f32_bits(losses) == f32_bits(want)
    assert f32_bits(best["val_loss"]) == f32_bits(report["val_loss"])
    assert best["heads"].tobytes() == report["heads"].tobytes()
    k = best["best_epoch"]
    assert k == int(np.argmin(np.asarray(best["val_loss"]))) == report["best_epoch"]
    head_now = np.concatenate([m.out_conv.weight.detach().cpu().numpy().ravel(), m.out_conv.bias.detach().cpu().numpy()])
    assert head_now.tobytes() == best["heads"][k].tobytes()
    kept = m.score_features(cache, td, pages=[4, 5])
    assert kept.loss() == best["val_loss"][k]
    separate = m.score_features(cache, td, pages=[4, 5], sweep=ref.SWEEP)
    assert np.array_equal(best["thresholds"], separate.best_thresholds()) and best["thresholds"].shape == (3,)
    # a fused forward afterwards runs the kept head: its loss on the held-out pages is the head's on the features,
    # up to the fp32 plan's forward error (2e-5 of the logits' scale: tests/test_forward_gpu.py)
    through_forward = m.score(xd[4:6], td[4:6]).loss()
    print(f"kept epoch {k}: validation loss {best['val_loss'][k]:.6f}, through the fused forward {through_forward:.6f}")
    assert abs(through_forward - best["val_loss"][k]) <= 1e-3 * best["val_loss"][k]
    m.close()

    # held-out pages scored against the complement of their masks: the better the head finds the fields, the further
    # it is from that target, so the loss rises with the fit and an early epoch wins -- the head kept is not the last
    # one, and the fused forward has to pick it up
    anti = td.clone()
    anti[4:6] = 1.0 - td[4:6]
    m = probe_model(sd)
    m(xd[:1])
    early = {}
    losses = m.fit_head(xd, anti, val_pages=[4, 5], keep_best=True, report=early, **kw)
    assert f32_bits(losses) == f32_bits(want) and early["heads"].tobytes() == report["heads"].tobytes()
    k = early["best_epoch"]
    print("complemented held-out masks: validation loss per epoch " + " ".join(f"{v:.4f}" for v in early["val_loss"])
          + f", kept epoch {k}")
    assert k == int(np.argmin(np.asarray(early["val_loss"]))) and k < 11
    head_now = np.concatenate([m.out_conv.weight.detach().cpu().numpy().ravel(), m.out_conv.bias.detach().cpu().numpy()])
    assert head_now.tobytes() == early["heads"][k].tobytes() != early["heads"][-1].tobytes()
    assert m.score_features(cache, anti, pages=[4, 5]).loss() == early["val_loss"][k]
    through_forward = m.score(xd[4:6], anti[4:6]).loss()
    assert abs(through_forward - early["val_loss"][k]) <= 1e-3 * early["val_loss"][k]
    assert abs(through_forward - early["val_loss"][-1]) > 2e-3 * early["val_loss"][k]
    m.close()


# ---------------------------------------------------------------- 11. the directory front end
def test_finetune_head_with_held_out_pages(tmp_path):
    from PIL import Image
    from unet_mi355x import inference
    sd, x, t = six_pages()
    img_dir, mask_dir = tmp_path / "images", tmp_path / "masks"
    img_dir.mkdir()
    mask_dir.mkdir()
    for i in range(6):
        page = np.round(x[i].transpose(1, 2, 0) * 255.0).astype(np.uint8)
        Image.fromarray(page).save(img_dir / f"page{i}.png")
        np.save(mask_dir / f"page{i}.npy", (t[i].transpose(1, 2, 0) * 255).astype(np.uint8))
    ckpt, out = str(tmp_path / "start.pth"), str(tmp_path / "probed.pth")
    torch.save(sd, ckpt)
    report = {}
    losses = inference.finetune_head(str(img_dir), str(mask_dir), ckpt, out, epochs=12, batch=2, lr=1e-2,
                                     compute_dtype="fp32", fused=True, val_fraction=1 / 3, val_seed=1, keep_best=True,
                                     sweep=ref.SWEEP, report=report)
    assert len(losses) == 12 and losses[-1] < losses[0]
    assert sorted(report) == ["best_epoch", "heads", "thresholds", "val_iou", "val_loss", "val_pages"]
    assert len(report["val_pages"]) == 2 and len(set(report["val_pages"])) == 2
    assert all(0 <= i < 6 for i in report["val_pages"])
    assert len(report["val_loss"]) == 12 and report["best_epoch"] == int(np.argmin(report["val_loss"]))
    saved = torch.load(out, map_location="cpu", weights_only=True)
    assert len(saved) == 136
    changed = sorted(k for k in saved if not torch.equal(saved[k], sd[k]))
    assert changed == ["out_conv.bias", "out_conv.weight"]
    head_saved = np.concatenate([saved["out_conv.weight"].numpy().ravel(), saved["out_conv.bias"].numpy()])
    assert head_saved.tobytes() == report["heads"][report["best_epoch"]].tobytes()
    other = {}
    inference.finetune_head(str(img_dir), str(mask_dir), ckpt, out, epochs=1, batch=2, lr=1e-2, compute_dtype="fp32",
                            val_fraction=1 / 3, val_seed=2, report=other)
    assert len(other["val_pages"]) == 2 and "thresholds" not in other
    with pytest.raises(ValueError, match="val_fraction"):
        inference.finetune_head(str(img_dir), str(mask_dir), ckpt, out, epochs=1, val_fraction=1.0)
