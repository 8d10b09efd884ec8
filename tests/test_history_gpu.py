"""Every output of every entry point is a function of its arguments and the loaded weights only, never of what an
earlier call left in the handle's scratch memory.  Needs a GPU: run with -m gpu (premises: tests/test_history_cpu.py).

The other GPU tests run on fresh handles, whose scratch the platform normally hands out zeroed, or reuse a handle at
one shape, whose stale data is finite and plausible: a kernel that reads scratch no earlier launch of the same call
wrote sees 0 x 0 or + 0 there and passes.  Here one handle is reserved once, for the largest shape it will see, and
every call under test runs after unet_debug_fill(0xFF) -- a NaN in every float format, all-ones mask bits, -1 as a
count -- or after a forward of another shape, or after a real all-NaN forward.  The fill always comes BEFORE a call,
never between a forward and UNet.intermediate, which reads the workspace.  References are the existing ones (the CPU
oracle, the exact-arithmetic expectations, the float64 restatements, Pillow); the forward, graph, block and preprocess
comparisons are bitwise, the score / loss / head ones keep the bars of their own test files and add bitwise equality
with a handle that was never filled."""
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
import head_ref
import loss_ref
import score_ref
import test_head_gpu as thg
import test_loss_gpu as tlg
import test_score_gpu as tsg
from test_exact_gpu import FORCED, assert_forced_labels
from test_rounding_gpu import SPLIT_LAUNCH
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.metrics import Score
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANS = ["fp32", "fp32_exact", "fp16", "bf16", "mixed"]
FILL = en.HISTORY_FILL


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _routing_model(seed, c_in, dtype):
    m = UNet(c_in, 3, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in en.routing_state_dict(seed, c_in).items()})
    return m.to(DEV).eval()


def _reserve(m, probes):
    """Reserve once at HISTORY_RESERVE; no probe may need more (it would re-allocate: fresh memory)."""
    m.reserve(*en.HISTORY_RESERVE)
    h = m.native_handle(torch.device(DEV))
    room = h.workspace_bytes(*en.HISTORY_RESERVE)
    for p in probes:
        assert 0 < h.workspace_bytes(*p) <= room, (p, h.workspace_bytes(*p), room)


# ------------------------------------------------------------------------------------ the hook itself
def test_debug_fill_semantics():
    """With nothing allocated the fill is a no-op that succeeds; a byte outside 0..255 is refused; after a forward the
    fill reaches the workspace (the one use between a forward and UNet.intermediate: every fetched value is then the
    fill pattern, a NaN) and leaves the weights alone (the next forward is right again)."""
    h = native.Handle(3, 3, "fp32", 0)
    try:
        h.debug_fill(FILL, _stream())
        for byte in (-1, 256):
            with pytest.raises(ValueError, match="0..255"):
                h.debug_fill(byte, _stream())
    finally:
        h.close()
    seed, c_in = en.HISTORY_NETS[0]
    case = (seed, c_in) + en.HISTORY_GRAPHS[0]
    for dtype in ("fp32", "mixed"):
        m = _routing_model(seed, c_in, dtype)
        try:
            _reserve(m, [case[2:]])
            en.check_routing_model(m, case, dtype, "before the fill")
            with torch.no_grad():
                m(torch.from_numpy(np.array(en.routing_reference(*case)[0])).to(DEV))
            m.debug_fill(FILL)
            for name in ("c1", "p4", "bn", "u1", "c8a"):
                assert bool(torch.isnan(m.intermediate(name)).all()), (dtype, name)
            en.check_routing_model(m, case, dtype, "after the fill")
        finally:
            m.close()


# ------------------------------------------------------------------------------------ a. forward, one handle across shapes
_MODELS = {}


@pytest.fixture(scope="module")
def shared_model():
    """One model per (plan, network) for the "fill" and "nan_forward" histories: the handle's past is what these
    tests are about."""
    def get(dtype, net):
        if (dtype, net) not in _MODELS:
            m = _MODELS[(dtype, net)] = _routing_model(*net, dtype)
            _reserve(m, en.HISTORY_STEPS)
        return _MODELS[(dtype, net)]
    yield get
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _nan_flood(m, c_in):
    """A real forward of an all-NaN batch at the reserved shape: all-NaN logits, all-zero masks (a NaN logit is a
    False mask), and every buffer a forward stores left NaN."""
    n, h, w = en.HISTORY_RESERVE
    x = torch.full((n, c_in, h, w), float("nan"), device=DEV)
    with torch.no_grad():
        masks, logits = m.forward_masks(x, with_logits=True)
    assert bool(torch.isnan(logits).all()), "the all-NaN forward's logits are not all NaN"
    assert not bool(masks.any()), "the all-NaN forward set mask bits"


@pytest.mark.parametrize("history", ["fill", "stale", "nan_forward"])
@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("net", en.HISTORY_NETS, ids=str)
def test_forward_after_other_shapes(net, dtype, history, shared_model):
    """HISTORY_STEPS in order on one handle reserved at HISTORY_RESERVE -- the large- and the small-batch (split-K)
    plan alternating, N = 4 | 5 across the small-batch limit, a 1-pixel bottleneck, ragged tiles at every level,
    W % 32 both ways -- with the whole routing check at every step (logits, every stored intermediate, u8 and packed
    masks, boxes with u8, packed and workspace masks), bitwise.  In front of every forward-type call: "fill", the
    scratch set to 0xFF; "stale", nothing, so each step sees the finite remains of the previous shape; "nan_forward",
    a real all-NaN forward at the reserved shape (needs no hook)."""
    seed, c_in = net
    if history == "stale":   # a handle of its own that is never filled: what it finds is what its own forwards left
        m = _routing_model(seed, c_in, dtype)
        _reserve(m, en.HISTORY_STEPS)
    else:
        m = shared_model(dtype, net)
    before = {"fill": lambda: m.debug_fill(FILL), "stale": None, "nan_forward": lambda: _nan_flood(m, c_in)}[history]
    try:
        for n, h, w in en.HISTORY_STEPS:
            en.check_routing_model(m, (seed, c_in, n, h, w), dtype, f"history {history}", before=before,
                                   every_box_path=True)
    finally:
        if history == "stale":
            m.close()


# ------------------------------------------------------------------------------------ b. captured graphs
@pytest.mark.parametrize("dtype", ["mixed", "fp32"])
def test_graph_replay_after_fill_and_after_another_shape(dtype):
    """Graphs captured at (1, 16, 16) and (3, 48, 80) with logits, packed masks and boxes: fill, replay, check; an
    eager forward of (6, 16, 112) on the same handle; fill, replay, check again.  The fill neither allocates nor
    stales a graph."""
    seed, c_in = en.HISTORY_NETS[0]
    m = _routing_model(seed, c_in, dtype)
    try:
        _reserve(m, en.HISTORY_GRAPHS + en.HISTORY_STEPS[:1])
        hd = m.native_handle(torch.device(DEV))
        graphs = []
        for n, h, w in en.HISTORY_GRAPHS:
            x, ref = en.routing_reference(seed, c_in, n, h, w)
            bufs = (torch.from_numpy(np.array(x)).to(DEV), torch.empty((n, 3, h, w), device=DEV),
                    torch.empty((n, 3, h, w // 8), dtype=torch.uint8, device=DEV),
                    torch.empty((n, 3, 4), dtype=torch.int32, device=DEV))
            # an eager run first, as test_graph_replay_equals_eager does
            hd.forward_boxes(bufs[0], bufs[1], bufs[2], native.MASK_BITS, bufs[3], _stream())
            graphs.append((hd.graph(bufs[0], bufs[1], bufs[2], native.MASK_BITS, boxes=bufs[3]), bufs, ref, (n, h, w)))

        def replay_all(when):
            for g, (_, lg, mk, bx), ref, shape in graphs:
                for t in (lg, mk, bx):
                    t.fill_(77)
                m.debug_fill(FILL)
                g.launch(_stream())
                torch.cuda.synchronize()
                got = lg.cpu().numpy()
                if not np.array_equal(got, ref["logits"]):
                    pytest.fail(f"{dtype} graph {shape} {when}: " + en.describe_mismatch("logits", got, ref["logits"], "graph"))
                ref_masks = en.reference_masks(ref["logits"], en.DEFAULT_THRESHOLDS)
                assert np.array_equal(np.unpackbits(mk.cpu().numpy(), axis=-1, bitorder="little").astype(bool),
                                      ref_masks), (shape, when)
                assert np.array_equal(bx.cpu().numpy(), en.np_boxes(ref_masks)), (shape, when)

        replay_all("after the fill")
        en.check_routing_model(m, (seed, c_in) + en.HISTORY_STEPS[0], dtype, "eager between replays")
        replay_all("after an eager forward of another shape and the fill")
        for g, *_ in graphs:
            g.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------ c. forced configurations
def _forced(case, dtype, tag):
    m = _routing_model(case[0], case[1], dtype)   # a fresh handle: unet_create reads the environment
    try:
        _reserve(m, [case[2:]])
        return en.check_routing_model(m, case, dtype, f"{tag}, filled", before=lambda: m.debug_fill(FILL),
                                      every_box_path=True)
    finally:
        m.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp32_exact"])
@pytest.mark.parametrize("var,value,tag", FORCED, ids=[f[2] for f in FORCED])
def test_forced_configurations_after_fill(var, value, tag, dtype, monkeypatch):
    """tests/test_exact_gpu.py's forced configurations (every 3x3 and ConvTranspose kernel family, split-K off, up1
    fused and not) at N = 2, 64 x 64 on a handle reserved at HISTORY_RESERVE and filled before each call; the same
    label assertions."""
    monkeypatch.setenv(var, value)
    if var == "UNET_MI355X_UPCFG":
        monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    assert_forced_labels(var, value, tag, dtype, _forced(en.ROUTING_FORCED, dtype, tag))


@pytest.mark.parametrize("dtype", ["bf16", "fp32_exact"])
def test_forced_split_k_after_fill(dtype, monkeypatch):
    """Two K slices forced on every layer that can split (tests/test_rounding_gpu.py's setting) at N = 1, 16 x 16:
    splitk_reduce_kernel reads exactly the slice rows the partial kernels stored, in a partial buffer full of NaN.
    Every layer of SPLIT_LAUNCH is eligible in both plans (the 8-wave 128-row ring and the LDS-halo family with a
    store or pool epilogue, Cin a multiple of 64), so every one of them must run split."""
    monkeypatch.setenv("UNET_MI355X_KSPLIT_FORCE", ",".join(f"{i}:2" for i in SPLIT_LAUNCH))
    monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    labels = _forced(en.HISTORY_SPLIT, dtype, "two K slices forced")
    print(f"{dtype} forced split: " + " | ".join(f"{i}: {s}" for i, s in enumerate(labels)))
    unsplit = [(i, labels[i]) for i in SPLIT_LAUNCH.values() if "splitk_reduce_kernel" not in labels[i]]
    assert not unsplit, unsplit


# ------------------------------------------------------------------------------------ d. stand-alone blocks
@functools.lru_cache(maxsize=None)
def _unet(dtype):
    """One module tree per plan; the blocks under test get their weights loaded into it."""
    return UNet(3, 3, compute_dtype=dtype).to(DEV).eval()


@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("name", list(en.BLOCKS))
def test_block_after_fill(name, dtype):
    """Every block shape through the stand-alone DoubleConv on a workspace reserved for more images of more than
    twice the size and filled: bitwise the dense block's expectation ("mixed": fp16 up to 128 output channels, bf16
    beyond, as unet_block_create documents)."""
    blk = en.dense_block(name)
    stored = dtype if dtype != "mixed" else ("fp16" if blk.cout <= 128 else "bf16")
    dc = getattr(_unet(dtype), blk.name)
    dc.close()                                   # a fresh native block
    dc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in blk.sd.items()})
    try:
        dc.reserve(*en.history_block_reserve(name))
        dc.debug_fill(FILL)
        with torch.no_grad():
            got = dc(torch.from_numpy(np.array(blk.x)).to(DEV)).cpu().numpy()
    finally:
        dc.close()
    want = blk.expected(stored)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        pytest.fail(f"{dtype} filled: " + en.describe_mismatch(
            f"{blk.name} output", got, want, f"unet_block_forward DoubleConv({blk.cin}, {blk.cout})"))


# ------------------------------------------------------------------------------------ e. score, loss, head scratch
def _reserve_shape(cases):
    """The element-wise maximum of the fixture shapes (N, C, H, W), H doubled: (N, H, W)."""
    n, _, h, w = (max(c["shape"][i] for c in cases) for i in range(4))
    return n, 2 * h, w


@pytest.fixture(scope="module")
def score_handles():
    hs = {c: native.Handle(3, c, "fp32", 0, tsg.THR) for c in (1, 3, 4)}
    for h in hs.values():
        h.score_reserve(*_reserve_shape(tsg.CASES), native.SCORE_MAX_K)
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def score_refs():
    out = []
    for case in tsg.CASES:
        logits, tu8 = score_ref.case_tensors(case)
        tf = score_ref.target_f32(tu8)
        out.append((logits, tu8, tf) + score_ref.score(logits, tf, tsg.logit_cuts(tsg.THR[:case["shape"][1]]),
                                                        tsg.logit_cuts(score_ref.SWEEP)))
    return out


def _fresh_score(c, *args, **kw):
    h = native.Handle(3, c, "fp32", 0, tsg.THR)   # never filled, sees only this call
    try:
        return tsg.run_score(h, *args, **kw)
    finally:
        h.close()


@pytest.mark.parametrize("form", ["f32_nchw", "u8_nhwc"])
@pytest.mark.parametrize("i", range(len(tsg.CASES)), ids=tsg.IDS)
def test_score_after_fill(i, form, score_handles, score_refs):
    """Every score fixture case in both target forms on a filled scratch reserved for a larger call with the full
    sweep: tests/test_score_gpu.py's bars (counts and histogram bitwise, sums and losses within BAR), and the entries
    and histogram bitwise those of a handle that was never filled."""
    case = tsg.CASES[i]
    logits, tu8, tf, e, hist = score_refs[i]
    t = tf if form == "f32_nchw" else tu8
    h = score_handles[case["shape"][1]]
    h.debug_fill(FILL, _stream())
    s = tsg.run_score(h, logits, t, sweep=score_ref.SWEEP)
    for k in tsg.COUNTS:
        assert np.array_equal(s.entries[k], e[k]), k
    assert np.array_equal(s.hist, hist)
    worst = max(score_ref.rel(got, want) for k in tsg.SUMS for got, want in zip(s.entries[k].ravel(), e[k].ravel()))
    got = dict(dice=s.dice(), focal=s.focal(), loss=s.loss(), loss_b1=s.loss(batch=1), loss_b2=s.loss(batch=2))
    worst_loss = max(score_ref.rel(v, case[k]) for k, v in got.items())
    print(f"{tsg.IDS[i]} {form}: sums rel {worst:.3e}, losses rel {worst_loss:.3e} (bar {tsg.BAR:.3e})")
    assert worst <= tsg.BAR
    assert worst_loss <= tsg.BAR
    clean = _fresh_score(case["shape"][1], logits, t, sweep=score_ref.SWEEP)
    assert s.entries.tobytes() == clean.entries.tobytes() and np.array_equal(s.hist, clean.hist)
    h.debug_fill(FILL, _stream())
    s0 = tsg.run_score(h, logits, t)             # without the sweep: the same entries
    assert s0.hist is None and s0.entries.tobytes() == s.entries.tobytes()


def test_score_nan_logit_after_fill(score_handles, score_refs):
    """tests/test_score_gpu.py's NaN case on a filled scratch: the NaN logit's entry has NaN sums, no other entry
    gains one, and all of it is bitwise what a never-filled handle gives."""
    logits, tu8, _, e, _ = score_refs[4]
    x = logits.copy()
    x[1, 2, 17, 5] = np.nan
    h = score_handles[3]
    h.debug_fill(FILL, _stream())
    s = tsg.run_score(h, x, tu8, sweep=score_ref.SWEEP)
    keep = np.ones((2, 3), bool)
    keep[1, 2] = False
    for k in tsg.SUMS:
        assert np.isnan(s.entries[k][1, 2]) and np.isfinite(s.entries[k][keep]).all(), k
    assert s.entries["n_pred"][1, 2] == e["n_pred"][1, 2] - int(logits[1, 2, 17, 5] > tsg.logit_cuts(tsg.THR)[2])
    for k in ("n_tgt", "n_px"):
        assert s.entries[k][1, 2] == e[k][1, 2]
    for k in tsg.COUNTS:
        assert np.array_equal(s.entries[k][keep], e[k][keep]), k
    clean = _fresh_score(3, x, tu8, sweep=score_ref.SWEEP)
    assert s.entries.tobytes() == clean.entries.tobytes() and np.array_equal(s.hist, clean.hist)


@pytest.fixture(scope="module")
def loss_handle():
    h = native.Handle(3, 4, "fp32", 0)
    shape = _reserve_shape(tlg.CASES)
    h.loss_reserve(*shape)
    h.score_reserve(*shape, native.SCORE_MAX_K)   # the loss is also compared with unet_score's entries
    yield h
    h.close()


@pytest.fixture(scope="module")
def loss_refs():
    out = []
    for case in tlg.CASES:
        x, tu8 = loss_ref.case_tensors(case)
        tf = loss_ref.target_f32(tu8)
        out.append((x, tu8, tf) + loss_ref.loss_grad(x, tf))
    return out


@pytest.mark.parametrize("form", ["f32_nchw", "u8_nhwc"])
@pytest.mark.parametrize("i", range(len(tlg.CASES)), ids=tlg.IDS)
def test_loss_after_fill(i, form, loss_handle, loss_refs):
    """Every loss fixture case in both target forms on a filled scratch reserved for a larger call:
    tests/test_loss_gpu.py's bars (gradient within 8 x spread of the reference's, the fixture's NaN pattern and no
    NaN more, loss within 1 ulp of Score.loss() and within the bar of the reference's), and loss and gradient
    bitwise those of a handle that was never filled."""
    case = tlg.CASES[i]
    x, tu8, tf, _, _ = loss_refs[i]
    t = tf if form == "f32_nchw" else tu8
    h = loss_handle
    h.debug_fill(FILL, _stream())
    loss, g = tlg.run(h, x, t)
    bar = loss_ref.SPREAD_FACTOR * case["spread"]
    d = loss_ref.grad_distance(g, case["grad"])
    h.debug_fill(FILL, _stream())
    entries, _ = h.score(tlg.dev(x), tlg.dev(t), _stream())
    want = np.float32(Score(entries.cpu().numpy()).loss())
    print(f"{tlg.IDS[i]} {form}: gradient {d:.3e} from the reference (bar {bar:.3e}); loss {loss!r}, "
          f"Score.loss {want!r}, reference {case['loss']!r}")
    assert g.dtype == np.float32 and g.shape == case["shape"]
    assert np.array_equal(np.isnan(g), np.isnan(case["grad"]))
    assert np.isfinite(g[~np.isnan(g)]).all()
    assert d <= bar
    if case["nan_at"] is None:
        assert loss_ref.ulps(loss, want) <= 1, (loss, want)
        assert abs(float(loss) - float(case["loss"])) <= bar * abs(float(case["loss"]))
    else:
        assert np.isnan(loss) and np.isnan(want)
    h.debug_fill(FILL, _stream())
    only, none = tlg.run(h, x, t, want_grad=False)
    assert none is None and only.tobytes() == loss.tobytes()
    fresh = native.Handle(3, 4, "fp32", 0)        # never filled, sees only this case
    try:
        loss0, g0 = tlg.run(fresh, x, t)
    finally:
        fresh.close()
    assert loss.tobytes() == loss0.tobytes() and g.tobytes() == g0.tobytes()


@pytest.fixture(scope="module")
def head_handle():
    h = native.Handle(3, 4, "fp32", 0)
    h.head_reserve(*_reserve_shape(thg.CASES))
    yield h
    h.close()


@pytest.mark.parametrize("i", range(len(thg.CASES)), ids=thg.IDS)
def test_head_after_fill(i, head_handle):
    """Every head fixture case on a filled scratch reserved for a larger call: tests/test_head_gpu.py's bars (each
    output within 8 x its own spread of the reference's, grad_w of a dead channel exactly 0), and all four outputs
    bitwise those of a handle that was never filled."""
    case = thg.CASES[i]
    feat, w, b, g = head_ref.case_tensors(case)
    restated = head_ref.head(feat, w, b, g)
    h = head_handle
    f, wd = thg.dev(feat), thg.dev(w)
    h.debug_fill(FILL, _stream())
    logits = h.head_forward(f, wd, thg.dev(b), _stream())
    h.debug_fill(FILL, _stream())
    outs = (logits,) + h.head_backward(f, thg.dev(g), wd, _stream(), want_params=True, want_feat=True)
    for k, out, ours in zip(head_ref.OUTPUTS, outs, restated):
        got = out.cpu().numpy()
        assert got.dtype == np.float32 and np.isfinite(got).all(), k
        if k == "grad_feat":
            got, ours = got.reshape(-1)[case["positions"]], ours.reshape(-1)[case["positions"]]
        d, bar = head_ref.distance(got, case[k]), head_ref.SPREAD_FACTOR * case[f"spread_{k}"]
        print(f"{thg.IDS[i]} {k}: reference {d:.3e} (bar {bar:.3e}), restatement {head_ref.distance(got, ours):.3e}")
        assert d <= bar, (k, d, bar)
    gw = outs[1].cpu().numpy()
    for k in case["dead"]:
        assert (gw[:, k] == 0.0).all()
    fresh = native.Handle(3, 4, "fp32", 0)        # never filled, sees only this case
    try:
        clean = thg.run(fresh, feat, w, b, g)
        for k, a, c in zip(head_ref.OUTPUTS, outs, clean):
            assert thg.bits(a) == thg.bits(c), k
    finally:
        fresh.close()


def _tiny_call(what):
    """(reserve, call) of `what` on tiny operands -- logits [1, 1, 8, 8] with a uint8 target; feat [1, 64, 8, 8] with
    C = 1 and want_params -- call(handle) -> the outputs' bytes."""
    gen = torch.Generator(device=DEV).manual_seed(8)
    if what == "head":
        feat = torch.randn((1, 64, 8, 8), device=DEV, generator=gen)
        g = torch.randn((1, 1, 8, 8), device=DEV, generator=gen)
        w = torch.randn((1, 64), device=DEV, generator=gen)
        return "head_reserve", lambda h: b"".join(thg.bits(t) for t in h.head_backward(feat, g, w, _stream(),
                                                                                       want_params=True)[:2])
    logits = torch.randn((1, 1, 8, 8), device=DEV, generator=gen)
    target = (torch.rand((1, 8, 8, 1), device=DEV, generator=gen) > 0.5).to(torch.uint8)
    if what == "score":
        return "score_reserve", lambda h: thg.bits(h.score(logits, target, _stream())[0])
    return "loss_reserve", lambda h: b"".join(thg.bits(t) for t in h.loss_grad(logits, target, _stream()))


@pytest.mark.parametrize("what", ["score", "loss", "head"])
def test_too_small_scratch_is_refused_during_capture(what):
    """A call whose scratch was never reserved, made on a capturing stream, is refused (UNET_ESTATE, naming its
    unet_<what>_reserve) before any device work; the handle then reserves, runs the same call eagerly and gives
    bitwise what a second fresh handle gives."""
    reserve, call = _tiny_call(what)
    h, fresh = native.Handle(3, 3, "fp32", 0), native.Handle(3, 3, "fp32", 0)
    try:
        buf = torch.ones(16, device=DEV)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            buf.zero_()   # the capture is not empty
            with pytest.raises(RuntimeError, match="capturing stream") as err:
                call(h)
        assert f"unet_{what}_reserve" in str(err.value)
        del graph
        getattr(h, reserve)(1, 8, 8)
        got, want = call(h), call(fresh)   # the fresh handle grows its scratch in the call: no capture, no refusal
        assert len(got) > 0 and got == want
    finally:
        h.close()
        fresh.close()


# ------------------------------------------------------------------------------------ f. preprocess row buffer
def test_preprocess_after_fill():
    """A 1400 x 1100 photo sizes the row buffer of the two-pass resize; then, with the buffer filled in front of every
    photo, smaller geometries -- up- and down-scaling, gray, one with no vertical pass (512 x 900) and one with no
    horizontal pass (700 x 512) -- each bit for bit Pillow's resize."""
    from PIL import Image
    m = UNet(3, 3, compute_dtype="bf16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in syn.make_state_dict(0, 3, 3).items()})
    m = m.to(DEV).eval()
    try:
        for h, w, c in [(1400, 1100, 3), (37, 23, 3), (390, 517, 1), (400, 600, 3), (512, 900, 3), (700, 512, 3)]:
            rng = np.random.default_rng(h + 3 * w)
            arr = rng.integers(0, 256, (h, w, 3) if c == 3 else (h, w), dtype=np.uint8)
            ref = np.array(Image.fromarray(arr).resize((512, 512)).convert("RGB")).astype(np.float32) / 255.0
            m.debug_fill(FILL)
            got = m.preprocess(torch.from_numpy(arr).to(DEV)).cpu().numpy()[0]
            assert got.shape == (3, 512, 512)
            assert np.array_equal(got, ref.transpose(2, 0, 1)), (h, w, c)
    finally:
        m.close()
