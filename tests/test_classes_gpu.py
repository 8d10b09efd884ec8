"""The fused head at 1, 2 and 4 classes and at thresholds of the caller's (csrc/unet_kernels.hip head_epilogue:
the fp32 FMA chains, the 16-bit MFMA head and the dword-packed masks, in the four kernels that include it), and
what depends on the class count around it: plane addresses, the mask-box grid and its sync entries, the
workspace masks of a boxes-only call, the copy sizes of the photo graph.  Needs a GPU: run with -m gpu.

Every output here goes through native.Handle with caller tensors that are views into a larger allocation, a
sentinel on either side (``Guarded``): logits in NaN, masks and boxes in 0xA5 bytes.  After a call the guards
must be untouched -- a store for a dead class lands past the last image -- and no sentinel may be left inside --
a plane nobody wrote.  (A packed mask byte may legitimately be 0xA5; those are compared with their reference.)

  a  bitwise, every plan: the dense-head routing networks of tests/exact_nets.py (premises on the CPU, in
     tests/test_exact_cpu.py) against the oracle -- logits, stored intermediates, masks, boxes
  b  the same, with one configuration per kernel family that includes the head forced, and the family asserted
  c  real-valued dense heads (tests/class_cases.py) to the tolerance of tests/test_forward_gpu.py, their masks
     and boxes bitwise against their own logits
  d  thresholds 0 and 1, and the padding of a short thresholds tuple
  e  the captured forward and the photo graph at 1 and 4 classes"""
import numpy as np
import pytest
import torch

import class_cases as cc
import exact_nets as en
from test_forward_gpu import TOL, rel_err
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANS = ["fp32", "fp32_exact", "fp16", "bf16", "mixed"]
CLASS_COUNTS = [1, 2, 4]
THR = en.CLASS_THRESHOLDS
GUARD_BYTES = 2048     # at least 256 elements of every output type on either side
HEAD_LAUNCH = 21       # conv1.3 + out_conv (include/unet_mi355x.h order)
HEAD_FAMILIES = ("conv3x3_halo_kernel<", "conv3x3_ring_kernel<", "conv3x3_ring8_kernel<", "conv3x3_x3w_kernel")


class Guarded:
    """Output tensors carved back to back out of one allocation (device, or pinned host memory) with GUARD_BYTES
    of sentinel before the first and after the last: ``parts`` = [(shape, dtype), ...].  float32 (alone): NaN
    everywhere; integer types: 0xA5 in every byte.  ``t``: the views."""

    def __init__(self, parts, pinned=False):
        self.parts = [(tuple(s), d) for s, d in parts]
        self.nan = self.parts[0][1] == torch.float32
        assert all((d == torch.float32) == self.nan for _, d in self.parts) and (not self.nan or len(parts) == 1)
        sizes = [int(np.prod(s)) * torch.empty((), dtype=d).element_size() for s, d in self.parts]
        assert all(b % 8 == 0 for b in sizes[:-1]), "parts must keep their successors aligned"
        self.inner = sum(sizes)
        total = -(-(2 * GUARD_BYTES + self.inner) // 4) * 4
        self.raw = torch.empty(total, dtype=torch.uint8, pin_memory=True) if pinned else \
            torch.empty(total, dtype=torch.uint8, device=DEV)
        self.t, off = [], GUARD_BYTES
        for (shape, dtype), b in zip(self.parts, sizes):
            self.t.append(self.raw[off:off + b].view(dtype).view(shape))
            off += b
        self.fill()

    def fill(self, inside=None):
        """Sentinel everywhere; ``inside`` = 0: the outputs zeroed between untouched guards."""
        if self.nan:
            self.raw.view(torch.float32).fill_(float("nan"))
        else:
            self.raw.fill_(0xA5)
        if inside is not None:
            self.raw[GUARD_BYTES:GUARD_BYTES + self.inner].fill_(inside)

    def check(self, what, packed=False):
        """Guards untouched, no sentinel inside; returns the parts as numpy arrays (after a synchronising copy)."""
        if self.raw.is_cuda:
            torch.cuda.synchronize()
        raw = self.raw.cpu().numpy()
        for name, g in (("before", raw[:GUARD_BYTES]), ("after", raw[GUARD_BYTES + self.inner:])):
            ok = np.isnan(g[:g.size // 4 * 4].view(np.float32)).all() if self.nan else (g == 0xA5).all()
            assert ok, f"{what}: the guard {name} the buffer was written"
        out = [t.cpu().numpy().copy() for t in self.t]
        for a in out:
            if self.nan:
                assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} of {a.size} elements never written"
            elif a.dtype == np.uint8:
                assert packed or a.max() <= 1, f"{what}: {int((a > 1).sum())} of {a.size} mask bytes never written"
            else:   # boxes, crop rectangles (>= -1) and crop sums (>= 0): the sentinel is a large negative number
                assert a.min() >= -1, f"{what}: {int((a < -1).sum())} of {a.size} elements never written"
        return out


def _model(sd, c_in, n_classes, dtype, thresholds):
    m = UNet(c_in, n_classes, compute_dtype=dtype, thresholds=thresholds)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def _run_guarded(h, xd, n_classes):
    """Every way the head is asked for outputs, each into guarded buffers: logits + u8 masks, logits + packed
    masks, logits alone, and forward_boxes without masks (bit masks in the workspace), with u8 and with packed
    masks.  Returns {name: numpy array}."""
    n, _, hh, ww = xd.shape
    stream = torch.cuda.current_stream().cuda_stream
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    full, bits, box = (n, n_classes, hh, ww), (n, n_classes, hh, ww // 8), (n, n_classes, 4)
    h.reserve(n, hh, ww)
    out = {}

    def call(tag, logits, masks, kind, boxes):
        bufs = [Guarded([(s, d)]) for s, d in ((full, f32),) * logits + (((full if kind == native.MASK_U8 else bits, u8),)
                                                                       if masks else ()) + ((box, i32),) * boxes]
        it = iter(bufs)
        lg = next(it).t[0] if logits else None
        mk = next(it).t[0] if masks else None
        if boxes:
            h.forward_boxes(xd, lg, mk, kind, next(it).t[0], stream)
        else:
            h.forward(xd, lg, mk, kind, stream)
        names = ["logits"] * logits + ["masks"] * masks + ["boxes"] * boxes
        for name, g in zip(names, bufs):
            out[f"{tag} {name}"] = g.check(f"{tag}: {name}", packed=kind == native.MASK_BITS)[0]

    call("forward u8", 1, 1, native.MASK_U8, 0)
    call("forward bits", 1, 1, native.MASK_BITS, 0)
    call("forward plain", 1, 0, native.MASK_NONE, 0)
    call("boxes only", 0, 0, native.MASK_NONE, 1)
    call("boxes u8", 0, 1, native.MASK_U8, 1)
    call("boxes bits", 1, 1, native.MASK_BITS, 1)
    return out


def _compare_outputs(got, logits, masks, label, what):
    """``got`` (_run_guarded) against reference logits (or None: not compared) and bool masks, bitwise."""
    packed = np.packbits(masks, axis=-1, bitorder="little")
    boxes = en.np_boxes(masks)
    for name, a in got.items():
        if name.endswith("logits"):
            want = logits
        elif name.endswith("masks"):
            want = packed if "bits" in name else masks.astype(np.uint8)
        else:
            want = boxes
        if want is not None and not np.array_equal(a, want):
            pytest.fail(f"{what}: " + en.describe_mismatch(name, a, want, label))


def _check_dense_routing(n_classes, case, dtype, tag=""):
    """One dense-head routing model, three forwards on one handle (page, mirrored page, page again: the mask-box
    sync entries must be idle again after each launch, or the next boxes are wrong): everything bitwise against
    the oracle.  Returns the launch labels."""
    seed, c_in, n, hh, ww = case
    thr = THR[:n_classes]
    m = _model(en.routing_state_dict(seed, c_in, n_classes, "dense", thr), c_in, n_classes, dtype, thr)
    try:
        h = m.native_handle(torch.device(DEV))
        labels = h.launch_labels_at(n, hh, ww)
        for mirror in (False, True, False):
            x, ref = en.routing_reference(seed, c_in, n, hh, ww, n_classes=n_classes, head="dense", thresholds=thr,
                                          mirror=mirror)
            what = f"{dtype} {n_classes} classes {case}{' mirrored' if mirror else ''} {tag}"
            got = _run_guarded(h, torch.from_numpy(np.array(x)).to(DEV), n_classes)
            bad = en.first_stored_mismatch(m, got["forward u8 logits"], ref, labels)
            if bad:
                pytest.fail(f"{what}: {bad}")
            _compare_outputs(got, ref["logits"], en.reference_masks(ref["logits"], thr), labels[HEAD_LAUNCH], what)
        return labels
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("case", en.ROUTING_CLASSES, ids=str)
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_dense_head_bitwise(n_classes, case, dtype):
    """1, 2 and 4 classes at thresholds (0.35, 0.5, 0.1, 0.9), dense {-1, 0, +1} head (every K slot of the head's
    dot carries a term), in every plan, at a size of the small-batch plan with partial tiles, a ragged size, a
    size whose packed masks leave as dwords and one above the small-batch limit."""
    labels = _check_dense_routing(n_classes, case, dtype)
    print(f"{dtype} {n_classes} classes {case}: {labels[HEAD_LAUNCH]}")


@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("case", [en.ROUTING_CLASSES[1], en.ROUTING_CLASSES[3]], ids=str)
def test_dense_head_bitwise_three_classes(case, dtype):
    """The product's class count with the dense head and the non-default thresholds."""
    _check_dense_routing(3, case, dtype)


# ------------------------------------------------------------------------------------------------ b
FORCED_HEAD = [(0, "conv3x3_halo_kernel<"), (3, "conv3x3_ring_kernel<"), (8, "conv3x3_ring8_kernel<"), (None, None)]


@pytest.mark.parametrize("dtype", ["bf16", "fp32_exact"])
@pytest.mark.parametrize("cfg,family", FORCED_HEAD, ids=["cfg0", "cfg3", "cfg8", "default"])
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_dense_head_in_every_kernel_family(n_classes, cfg, family, dtype, monkeypatch):
    """N = 2 at 64 x 64 with one configuration of each kernel family that includes head_epilogue forced on all
    layers (and the plan's own choice): the same integers, and launch 21 really ran that family."""
    if cfg is not None:
        monkeypatch.setenv("UNET_MI355X_CFG", ",".join(f"{i}:{cfg}" for i in range(17)))
    labels = _check_dense_routing(n_classes, en.ROUTING_CLASSES[2], dtype, f"cfg {cfg}")
    print(f"{dtype} {n_classes} classes cfg {cfg}: {labels[HEAD_LAUNCH]}")
    if family is None:
        assert labels[HEAD_LAUNCH].startswith(HEAD_FAMILIES[:3]), labels[HEAD_LAUNCH]
    else:
        assert labels[HEAD_LAUNCH].startswith(family), labels[HEAD_LAUNCH]


@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_dense_head_in_the_three_term_kernel(n_classes):
    """The "fp32" plan's own head site: conv3x3_x3w_kernel."""
    labels = _check_dense_routing(n_classes, en.ROUTING_CLASSES[2], "fp32")
    assert labels[HEAD_LAUNCH].startswith("conv3x3_x3w_kernel"), labels[HEAD_LAUNCH]


# ------------------------------------------------------------------------------------------------ c
def _cuts(thresholds):
    lib = native.load_library()
    return [np.float32(lib.unet_logit_cut(np.float32(t))) for t in thresholds]


def _check_self_consistent(got, thresholds, label, what):
    """Masks and boxes of every call against the logits of the same handle and input, bitwise: masks ==
    (logits > unet_logit_cut(thr)) per class, boxes == numpy's min / max over those masks.  The logits of all
    calls are the same bits."""
    logits = got["forward u8 logits"]
    masks = np.stack([logits[:, c] > cut for c, cut in enumerate(_cuts(thresholds))], axis=1)
    _compare_outputs(got, logits, masks, label, what)
    return logits, masks


@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("index", range(len(cc.SHAPES)), ids=[str(s) for s in cc.SHAPES])
@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
def test_real_dense_head_to_tolerance(n_classes, index, dtype):
    """Real-valued dense heads: logits within TOL of the oracle; masks (u8, packed, those of forward_boxes) and
    boxes bitwise what the call's own logits say; on the fp32 plans the masks equal the oracle's outside the
    band of TOL around the cut (at most 8 pixels per class, asserted on the oracle before the GPU is used)."""
    assert cc.FP32_TOL == TOL["fp32"] == TOL["fp32_exact"]
    case = cc.dense_case(n_classes, index)
    case.check_oracle()
    m = _model(case.sd, 3, n_classes, dtype, case.thresholds)
    try:
        h = m.native_handle(torch.device(DEV))
        n, hh, ww = cc.SHAPES[index]
        label = h.launch_labels_at(n, hh, ww)[HEAD_LAUNCH]
        what = f"{dtype} {n_classes} classes {cc.SHAPES[index]}"
        got = _run_guarded(h, torch.from_numpy(np.array(case.x)).to(DEV), n_classes)
        logits, masks = _check_self_consistent(got, case.thresholds, label, what)
        err = rel_err(logits, case.ref)
        print(f"{what}: logits rel err {err:.3e} (TOL {TOL[dtype]:.1e}); {label}")
        assert err <= TOL[dtype]
        if dtype in ("fp32", "fp32_exact"):
            differ = (masks != case.masks) & ~case.near
            assert not differ.any(), en.describe_mismatch("masks vs the oracle's", masks & ~case.near,
                                                          case.masks & ~case.near, label)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("dtype", ["mixed", "fp32"])
@pytest.mark.parametrize("index", [2, 1], ids=[str(cc.SHAPES[2]), str(cc.SHAPES[1])])
def test_threshold_extremes(index, dtype):
    """thresholds (0, 1) on two classes: every pixel of class 0 is on (u8 1, packed 0xFF, the box the whole
    image), none of class 1 (zeros, the box -1s), whatever the logits (|logit| < 50, asserted on the oracle)."""
    case = cc.dense_case(2, index)
    assert np.abs(case.ref).max() < 50
    n, hh, ww = cc.SHAPES[index]
    m = _model(case.sd, 3, 2, dtype, (0.0, 1.0))
    try:
        h = m.native_handle(torch.device(DEV))
        got = _run_guarded(h, torch.from_numpy(np.array(case.x)).to(DEV), 2)
        assert rel_err(got["forward u8 logits"], case.ref) <= TOL[dtype]
        masks = np.zeros((n, 2, hh, ww), bool)
        masks[:, 0] = True
        _compare_outputs(got, None, masks, h.launch_labels_at(n, hh, ww)[HEAD_LAUNCH], f"{dtype} thresholds (0, 1)")
        for name in ("boxes only boxes", "boxes u8 boxes", "boxes bits boxes"):
            assert (got[name][:, 0] == (0, 0, ww - 1, hh - 1)).all() and (got[name][:, 1] == -1).all(), name
        assert (got["forward bits masks"][:, 0] == 0xFF).all() and (got["forward u8 masks"][:, 0] == 1).all()
        assert not got["forward bits masks"][:, 1].any() and not got["forward u8 masks"][:, 1].any()
    finally:
        m.close()


def test_fourth_class_of_a_short_thresholds_tuple_cuts_at_one_half():
    """UNet(3, 4) with the default three thresholds: native.Handle pads the tuple, the fourth class is cut at
    0.5 -- and at no other slot's threshold (the case's fourth class straddles all of them differently)."""
    defaults = (0.25, 0.40, 0.30)
    case = cc.dense_case(4, 2, defaults + (0.5,))
    case.check_oracle()
    m = UNet(3, 4, compute_dtype="mixed")
    assert m.thresholds == defaults
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in case.sd.items()})
    m = m.to(DEV).eval()
    try:
        h = m.native_handle(torch.device(DEV))
        got = _run_guarded(h, torch.from_numpy(np.array(case.x)).to(DEV), 4)
        logits, masks = _check_self_consistent(got, defaults + (0.5,), h.launch_labels_at(*cc.SHAPES[2])[HEAD_LAUNCH],
                                               "mixed, padded thresholds")
        for cut in _cuts(defaults):
            assert not np.array_equal(masks[:, 3], logits[:, 3] > cut)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("n_classes", [1, 4])
def test_graph_replay_equals_eager(n_classes):
    """unet_graph_create at 1 and 4 classes, N = 2 at 64 x 64: three replays into zeroed (guarded) buffers give
    the eager call's logits, packed masks and boxes bit for bit -- the oracle's."""
    seed, c_in, n, hh, ww = case = en.ROUTING_CLASSES[2]
    thr = THR[:n_classes]
    x, ref = en.routing_reference(seed, c_in, n, hh, ww, n_classes=n_classes, head="dense", thresholds=thr)
    m = _model(en.routing_state_dict(seed, c_in, n_classes, "dense", thr), c_in, n_classes, "mixed", thr)
    try:
        h = m.native_handle(torch.device(DEV))
        stream = torch.cuda.current_stream().cuda_stream
        xd = torch.from_numpy(np.array(x)).to(DEV)
        shapes = [((n, n_classes, hh, ww), torch.float32), ((n, n_classes, hh, ww // 8), torch.uint8),
                  ((n, n_classes, 4), torch.int32)]
        h.reserve(n, hh, ww)
        eager = [Guarded([p]) for p in shapes]
        h.forward_boxes(xd, eager[0].t[0], eager[1].t[0], native.MASK_BITS, eager[2].t[0], stream)
        want = [g.check(f"eager {i}", packed=True)[0] for i, g in enumerate(eager)]
        bufs = [Guarded([p]) for p in shapes]
        g = h.graph(xd, bufs[0].t[0], bufs[1].t[0], native.MASK_BITS, boxes=bufs[2].t[0])
        for b in bufs:
            b.fill(inside=0)
        for _ in range(3):
            g.launch(stream)
        got = [b.check(f"replayed {i}", packed=True)[0] for i, b in enumerate(bufs)]
        g.close()
        masks = en.reference_masks(ref["logits"], thr)
        oracle = [ref["logits"], np.packbits(masks, axis=-1, bitorder="little"), en.np_boxes(masks)]
        for name, a, b, c in zip(("logits", "packed masks", "boxes"), got, want, oracle):
            assert np.array_equal(a, b), f"{case} {n_classes} classes: replayed {name} differ from the eager call's"
            assert np.array_equal(b, c), f"{case} {n_classes} classes: eager {name} differ from the oracle's"
    finally:
        m.close()


@pytest.mark.parametrize("adjacent", [True, False], ids=["adjacent", "separate"])
@pytest.mark.parametrize("n_classes", [1, 4])
def test_photo_graph_equals_eager_steps(n_classes, adjacent):
    """unet_photo_graph_create at 1 and 4 classes on a 100 x 140 RGB photo and a 64 x 64 network input: the
    pinned masks, boxes, crop rectangles and crop sums of two replays equal preprocess + forward_boxes +
    crop_stats run eagerly.  ``adjacent``: boxes | rectangles | sums back to back on the device and on the
    host, which the graph copies back as one node of n_classes * 40 bytes; else three copies."""
    from unet_mi355x import inference as inf
    size, ih, iw = 64, 100, 140
    case = cc.dense_case(n_classes, 2)
    photo = np.ascontiguousarray((syn.invoice_pages(77, 1, ih, iw, 3)[0].transpose(1, 2, 0) * 255).astype(np.uint8))
    m = _model(case.sd, 3, n_classes, "mixed", case.thresholds)
    try:
        h = m.native_handle(torch.device(DEV))
        stream = torch.cuda.current_stream().cuda_stream
        u8, i32, i64 = torch.uint8, torch.int32, torch.int64
        small = [((1, n_classes, 4), i32), ((n_classes, 4), i32), ((n_classes,), i64)]
        mshape = ((1, n_classes, size, size), u8)

        def outputs(pinned):
            mk = Guarded([mshape], pinned)
            rest = [Guarded(small, pinned)] if adjacent else [Guarded([p], pinned) for p in small]
            return mk, rest, [mk.t[0]] + [t for g in rest for t in g.t]

        def read(mk, rest, what):
            return mk.check(f"{what} masks") + [a for g in rest for a in g.check(f"{what} boxes / rects / sums")]

        img = torch.from_numpy(photo).to(DEV)
        # the same steps, eagerly
        e_mk, e_rest, (e_m, e_b, e_r, e_s) = outputs(False)
        with torch.no_grad():
            xe = m.preprocess(img, size)
        h.reserve(1, size, size)
        h.forward_boxes(xe, None, e_m, native.MASK_U8, e_b, stream)
        native.crop_stats(img, e_b, size, size, inf.CROP_PAD, e_r, e_s, stream)
        want = read(e_mk, e_rest, "eager")
        assert (want[1][..., 2] >= 0).any(), "no class found anything on the photo"
        # as one graph, uploaded from and copied back to pinned memory
        h_img = torch.from_numpy(photo.reshape(-1).copy()).pin_memory()
        d_img = torch.empty((ih, iw, 3), dtype=u8, device=DEV)
        xg = torch.empty((1, 3, size, size), dtype=torch.float32, device=DEV)
        d_mk, d_rest, (d_m, d_b, d_r, d_s) = outputs(False)
        p_mk, p_rest, (p_m, p_b, p_r, p_s) = outputs(True)
        g = h.photo_graph(h_img, d_img, xg, d_m, native.MASK_U8, d_b, inf.CROP_PAD, d_r, d_s, p_m, p_b, p_r, p_s)
        for replay in range(2):
            for buf in [p_mk] + p_rest:
                buf.fill()
            g.launch(stream)
            torch.cuda.synchronize()
            got = read(p_mk, p_rest, f"replay {replay}")
            for name, a, b in zip(("masks", "boxes", "rects", "sums"), got, want):
                assert np.array_equal(a, b), f"{n_classes} classes, replay {replay}: pinned {name} differ from eager"
        read(d_mk, d_rest, "device side")
        g.close()
    finally:
        m.close()
