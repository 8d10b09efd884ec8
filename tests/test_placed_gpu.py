"""Placed masks: the stage after the head -- the masks themselves, mask_boxes_kernel and crop_stats_kernel -- on masks
the TEST chooses bit by bit (tests/placed_nets.py: a pass-through network whose masks are its input bits; premises in
tests/test_placed_cpu.py).  Needs a GPU: run with -m gpu.

  a  masks are the placed bits: every plan, both sides of the small-batch limit, u8 / packed / the three box paths,
     a uint8 NHWC input, 1 and 4 classes, every kernel family that includes the head
  b  boxes at every edge: single pixels in the corners, on bits 15 | 16 of a column word, in the last row of a strip,
     on either side of a chunk border, in a ragged last chunk
  c  more strips than blocks (65 chunks: block 0 loops)
  d  rows wider than 256 column words (a thread flushes the word it collected when the word changes)
  e  caller masks that are not 16-byte aligned (mask_boxes_kernel<MASK_U8, false>)
  f  the box sync entries are idle after every launch: full -> corner -> empty -> opposite corner -> full, eagerly,
     as one captured graph whose input is rewritten in place, and with another shape's forward in between
  g  the photo graph with changing photos: crop_stats_kernel's count-and-sum word under replay

References: the placed bits, exact_nets.np_boxes, numpy's packbits and sums, inference.crop_rect, Pillow's resize.

What the library let through: 16 x 4112 and 1040 x 1024 are accepted as they are, and a caller mask buffer at any byte
offset is accepted, so the scalar path of the box kernel is reachable from the API.  Two shapes are this file's own:
32 x 48 holds only 96 column words, fewer than the block's 256 threads, so no thread there meets a second word -- 96
x 48 (288 words) does; and words 256 of row 0 and 0 of row 1 of a 257-word row belong to neighbouring threads, so
wide_patterns adds pairs in words i and i + 256, which one thread loads one after the other.

Value-only mutations of the kernels, each caught on an MI355X (tests that then fail):
  31 - clz -> 32 - clz                          all 99, e.g. test_boxes_at_every_edge[16-16-none]
  16 i + ctz -> 16 i                            all 99, e.g. test_boxes_at_every_edge[16-16-none]
  no reset of e[0..3] in mask_boxes_kernel      all 99 (a shared handle), test_box_entries_are_idle_after_every_launch
  no flush of cacc when the column word changes test_boxes_at_every_edge[96-48-*], test_rows_wider_than_256_column_words
  c += gridDim.y -> one pass                    test_more_strips_than_blocks
  no atomicExch(e, 0) in crop_stats_kernel      all 45 cases of test_photo_graph_with_changing_photos
The whole file takes about 7.5 s on an MI355X; no test more than 1.1 s (the first one, which creates the HIP context)."""
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
import placed_nets as pn
from test_classes_gpu import FORCED_HEAD, HEAD_LAUNCH, Guarded
from unet_mi355x import inference as inf
from unet_mi355x import native
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANS = ["fp32", "fp32_exact", "fp16", "bf16", "mixed"]
BOX_PATHS = [None, "u8", "bits"]
BOX_SHAPES = [(16, 16), (32, 48), (48, 32), (96, 48), (512, 512), (528, 512)]   # (96, 48): 288 words, a thread meets two


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the shared references are read-only


def _make(dtype, n_classes=3, thresholds=en.DEFAULT_THRESHOLDS):
    m = UNet(3, n_classes, compute_dtype=dtype, thresholds=tuple(thresholds)[:n_classes])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in pn.passthrough_state_dict(3, n_classes).items()})
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def models():
    """One pass-through model per (plan, class count), made when first asked for, closed at the end."""
    made = {}

    def get(dtype, n_classes=3):
        if (dtype, n_classes) not in made:
            thr = en.DEFAULT_THRESHOLDS if n_classes == 3 else en.CLASS_THRESHOLDS
            made[(dtype, n_classes)] = _make(dtype, n_classes, thr)
        return made[(dtype, n_classes)]

    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def _packed(h, w, n_classes=3):
    """(x, planes, bits, boxes) of pack_planes of every pattern: computed once, shared, read-only."""
    x, planes = pn.pack_planes(list(pn.placed_patterns(h, w)), h, w, n_classes)
    bits = pn.placed_bits(x, n_classes)
    boxes = en.np_boxes(bits)
    for a in (x, bits, boxes):
        a.setflags(write=False)
    return x, planes, bits, boxes


def _unpack(packed):
    return np.unpackbits(packed, axis=-1, bitorder="little").astype(bool)


def _assert_masks(got, bits, planes, what):
    if not np.array_equal(got, bits):
        n, k = (int(v) for v in np.argwhere((got != bits).any(axis=(2, 3)))[0])
        pytest.fail(f"{what}: plane (n {n}, k {k}) = '{planes[n][k]}': " +
                    en.describe_mismatch("masks", got, bits, "head"))


def _assert_boxes(got, want, planes, what):
    got = np.asarray(got)
    if not np.array_equal(got, want):
        bad = [(int(n), int(k), planes[n][k], got[n, k].tolist(), want[n, k].tolist())
               for n, k in np.argwhere((got != want).any(axis=-1))]
        pytest.fail(f"{what}: {len(bad)} boxes wrong; (n, k, pattern, got, want): {bad[:8]}")


def _check_placed(m, x, planes, what, n_classes=3):
    """Every way masks leave the library, on one input: all of them the placed bits, the logits exactly -8 / +8, the
    boxes np_boxes of the bits; and the same from the uint8 NHWC form of the input."""
    xd = _dev(x)
    bits, want_lg = pn.placed_bits(x, n_classes), pn.placed_logits(x, n_classes)
    boxes = en.np_boxes(bits)
    with torch.no_grad():
        u8, lg = m.forward_masks(xd, with_logits=True)
        pk, lg2 = m.forward_masks(xd, packed=True, with_logits=True)
        only = m.forward_boxes(xd, masks=None)
        bu8, b1 = m.forward_boxes(xd, masks="u8")
        bpk, b2 = m.forward_boxes(xd, masks="bits")
    for name, a in (("forward_masks", lg), ("forward_masks(packed)", lg2)):
        a = a.cpu().numpy()
        assert np.array_equal(a, want_lg), f"{what}: " + en.describe_mismatch(f"logits of {name}", a, want_lg, "head")
    u8 = u8.cpu().numpy()
    assert u8.max() <= 1, f"{what}: u8 masks hold values other than 0 / 1"
    _assert_masks(u8.astype(bool), bits, planes, f"{what}: forward_masks u8")
    pk = pk.cpu().numpy()
    assert np.array_equal(pk, np.packbits(bits, axis=-1, bitorder="little")), f"{what}: packed masks (bit order?)"
    _assert_masks(_unpack(pk), bits, planes, f"{what}: forward_masks packed")
    _assert_masks(bu8.cpu().numpy().astype(bool), bits, planes, f"{what}: forward_boxes u8 masks")
    _assert_masks(_unpack(bpk.cpu().numpy()), bits, planes, f"{what}: forward_boxes packed masks")
    for name, b in (("masks=None", only), ("masks='u8'", b1), ("masks='bits'", b2)):
        _assert_boxes(b.cpu().numpy(), boxes, planes, f"{what}: forward_boxes {name}")
    # the uint8 NHWC form of the same input, through the handle
    n, _, hh, ww = x.shape
    h = m.native_handle(torch.device(DEV))
    xu = _dev((x * 255).astype(np.uint8).transpose(0, 2, 3, 1))
    lg = torch.empty((n, n_classes, hh, ww), device=DEV)
    mk = torch.empty((n, n_classes, hh, ww // 8), dtype=torch.uint8, device=DEV)
    bx = torch.empty((n, n_classes, 4), dtype=torch.int32, device=DEV)
    h.forward_boxes(xu, lg, mk, native.MASK_BITS, bx, _stream(), layout=native.LAYOUT_NHWC)
    assert np.array_equal(lg.cpu().numpy(), want_lg), f"{what}: logits of the uint8 NHWC input"
    _assert_masks(_unpack(mk.cpu().numpy()), bits, planes, f"{what}: uint8 NHWC input, packed masks")
    _assert_boxes(bx.cpu().numpy(), boxes, planes, f"{what}: uint8 NHWC input")


def _batches(x, planes, n):
    """Every image of a pack in batches of n (the last batch overlaps the one before)."""
    starts = list(range(0, len(x) - n + 1, n))
    if starts[-1] + n < len(x):
        starts.append(len(x) - n)
    return [(np.ascontiguousarray(x[s:s + n]), planes[s:s + n]) for s in starts]


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("h,w", [(32, 48), (64, 64)])
@pytest.mark.parametrize("dtype", PLANS)
def test_masks_are_the_placed_bits(dtype, h, w, n, models):
    """Every pattern of placed_patterns (and the full | empty | full images) in batches of N = 1 and N = 5, on either
    side of the small-batch limit."""
    m = models(dtype)
    limit = m.native_handle(torch.device(DEV)).small_batch_limit()
    assert limit < 5, limit
    x, planes, _, _ = _packed(h, w)
    for xb, pb in _batches(x, planes, n):
        _check_placed(m, xb, pb, f"{dtype} N={n} {h}x{w} {pb}")


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("n_classes", [1, 4])
def test_masks_are_the_placed_bits_at_1_and_4_classes(n_classes, n, models):
    """"mixed" at 1 and 4 classes and the class tests' thresholds, 32 x 48: with one class the two channels nobody
    reads carry decoys, with four the last plane repeats channel 0."""
    m = models("mixed", n_classes)
    x, planes, _, _ = _packed(32, 48, n_classes)
    for xb, pb in _batches(x, planes, n):
        _check_placed(m, xb, pb, f"mixed {n_classes} classes N={n} {pb}", n_classes)


@pytest.mark.parametrize("cfg,family", FORCED_HEAD, ids=["cfg0", "cfg3", "cfg8", "default"])
def test_masks_are_the_placed_bits_in_every_kernel_family(cfg, family, monkeypatch):
    """N = 2 at 64 x 64 in "mixed" with one configuration of each kernel family that includes the head forced on all
    layers (tests/test_classes_gpu.py's list), and launch 21 really ran that family."""
    if cfg is not None:
        monkeypatch.setenv("UNET_MI355X_CFG", ",".join(f"{i}:{cfg}" for i in range(17)))
    m = _make("mixed")
    try:
        label = m.native_handle(torch.device(DEV)).launch_labels_at(2, 64, 64)[HEAD_LAUNCH]
        if family is not None:
            assert label.startswith(family), label
        x, planes, _, _ = _packed(64, 64)
        for s in (0, len(x) - 3):   # [pixel, full, pixel] + [pixel, empty, pixel]; empty + full images
            _check_placed(m, np.ascontiguousarray(x[s:s + 2]), planes[s:s + 2], f"mixed cfg {cfg} ({label})")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("path", BOX_PATHS, ids=["none", "u8", "bits"])
@pytest.mark.parametrize("h,w", BOX_SHAPES)
def test_boxes_at_every_edge(h, w, path, models):
    """Every pattern's box through each of the three box paths (masks in the workspace, caller u8, caller bits), one
    forward per shape and path."""
    m = models("mixed")
    x, planes, bits, boxes = _packed(h, w)
    with torch.no_grad():
        out = m.forward_boxes(_dev(x), masks=path)
    if path is None:
        got = out
    else:
        mk, got = out
        mk = mk.cpu().numpy()
        _assert_masks(mk.astype(bool) if path == "u8" else _unpack(mk), bits, planes, f"{h}x{w} masks={path}")
    _assert_boxes(got.cpu().numpy(), boxes, planes, f"{h}x{w} masks={path}")


def _check_planes(m, named, h, w, what):
    """Named bool planes, three per image, through the three box paths."""
    names = list(named)
    x = pn.planes_input(np.stack([named[k] for k in names]))
    planes = [[(names + ["empty"] * 2)[3 * n + k] for k in range(3)] for n in range(len(x))]
    bits = pn.placed_bits(x, 3)
    boxes = en.np_boxes(bits)
    xd = _dev(x)
    for path in BOX_PATHS:
        with torch.no_grad():
            out = m.forward_boxes(xd, masks=path)
        if path is not None:
            mk = out[0].cpu().numpy()
            _assert_masks(mk.astype(bool) if path == "u8" else _unpack(mk), bits, planes, f"{what} masks={path}")
        _assert_boxes((out if path is None else out[1]).cpu().numpy(), boxes, planes, f"{what} masks={path}")


# ------------------------------------------------------------------------------------------------ c
def test_more_strips_than_blocks(models):
    """1040 x 1024, N = 1: 65 chunks against 64 blocks per plane, so block 0 takes chunk 64 on its second pass."""
    h, w = 1040, 1024
    named = {k: pn.pixels_plane(v, h, w) for k, v in pn.strip_patterns(h, w).items()}
    _check_planes(models("mixed"), named, h, w, f"{h}x{w}")


# ------------------------------------------------------------------------------------------------ d
def test_rows_wider_than_256_column_words(models):
    """16 x 4112: 257 words per row, so a thread meets a new column word with every load."""
    h, w = 16, 4112
    _check_planes(models("mixed"), pn.wide_patterns(h, w), h, w, f"{h}x{w}")


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("offset", [0, 1, 4, 8])
def test_unaligned_caller_masks(offset, models):
    """native.Handle.forward_boxes with MASK_U8 into a view at byte offset 1, 4 and 8 (and 0, the vector path) of a
    larger buffer: masks, boxes and the guard bytes on either side."""
    guard, (h, w), n = 2048, (32, 48), 5
    x, planes, bits, boxes = _packed(h, w)
    x, planes, bits, boxes = np.ascontiguousarray(x[:n]), planes[:n], bits[:n], boxes[:n]
    hd = models("mixed").native_handle(torch.device(DEV))
    size = bits.size
    raw = torch.full((2 * guard + size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 16 == 0
    mk = raw[guard + offset:guard + offset + size].view(n, 3, h, w)
    assert mk.data_ptr() % 16 == offset and mk.is_contiguous()
    bx = Guarded([((n, 3, 4), torch.int32)])
    hd.reserve(n, h, w)
    hd.forward_boxes(_dev(x), None, mk, native.MASK_U8, bx.t[0], _stream())
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    assert (got[:guard + offset] == 0xA5).all() and (got[guard + offset + size:] == 0xA5).all(), "guard bytes written"
    inner = got[guard + offset:guard + offset + size].reshape(n, 3, h, w)
    assert inner.max() <= 1
    _assert_masks(inner.astype(bool), bits, planes, f"masks at byte offset {offset}")
    _assert_boxes(bx.check(f"boxes, masks at byte offset {offset}")[0], boxes, planes, f"masks at byte offset {offset}")


# ------------------------------------------------------------------------------------------------ f
@functools.lru_cache(maxsize=None)
def _sequence(h, w):
    """The inputs [2, 3, h, w] of the five steps.  Image 0: full, one corner per plane, empty, the opposite corners,
    full; image 1 runs the same steps two ahead, so that the two images' entries never change alike."""
    p = pn.placed_patterns(h, w)
    first = [p["corner_tl"], p["corner_tr"], p["corner_bl"]]
    opposite = [p["corner_br"], p["corner_bl"], p["corner_tr"]]
    steps = [[p["full"]] * 3, first, [p["empty"]] * 3, opposite, [p["full"]] * 3]
    out = []
    for i in range(5):
        x = np.stack([np.stack(steps[i]), np.stack(steps[(i + 2) % 5])]).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return out


SEQ_PLANES = [["step"] * 3, ["two steps ahead"] * 3]


@pytest.mark.parametrize("h,w", [(64, 64), (512, 512)])
def test_box_entries_are_idle_after_every_launch(h, w, models):
    """One handle, five inputs whose boxes shrink, vanish and grow: every box is that step's np_boxes, never the union
    with an earlier step's -- eagerly on the three box paths, as one captured graph whose input tensor is rewritten
    in place between replays, and with another shape's forward between the replays."""
    m = models("mixed")
    hd = m.native_handle(torch.device(DEV))
    seq = _sequence(h, w)
    want = [en.np_boxes(pn.placed_bits(x, 3)) for x in seq]
    assert not np.array_equal(want[0], want[1]) and (want[2][0] == -1).all()
    for path in BOX_PATHS:
        for i, x in enumerate(seq):
            with torch.no_grad():
                out = m.forward_boxes(_dev(x), masks=path)
            got = (out if path is None else out[1]).cpu().numpy()
            _assert_boxes(got, want[i], SEQ_PLANES, f"{h}x{w} eager masks={path} step {i}")
    # another shape for in between, and room for both before the capture (a growing reserve would stale the graph)
    ox, oplanes, _, oboxes = _packed(32, 48)
    ox, oplanes, oboxes = _dev(ox[:3]), oplanes[:3], oboxes[:3]
    hd.reserve(2, h, w)
    hd.reserve(3, 32, 48)
    xd = _dev(seq[0])
    lg = torch.empty((2, 3, h, w), device=DEV)
    mk = torch.empty((2, 3, h, w // 8), dtype=torch.uint8, device=DEV)
    bx = torch.empty((2, 3, 4), dtype=torch.int32, device=DEV)
    g = hd.graph(xd, lg, mk, native.MASK_BITS, boxes=bx)
    try:
        for interleave in (False, True):
            for i, x in enumerate(seq):
                xd.copy_(torch.from_numpy(np.array(x)))
                bx.fill_(-7)
                g.launch(_stream())
                torch.cuda.synchronize()
                what = f"{h}x{w} replay {i}{' after another shape' if interleave else ''}"
                _assert_boxes(bx.cpu().numpy(), want[i], SEQ_PLANES, what)
                _assert_masks(_unpack(mk.cpu().numpy()), pn.placed_bits(x, 3), SEQ_PLANES, what)
                assert np.array_equal(lg.cpu().numpy(), pn.placed_logits(x, 3)), what
                if interleave:
                    ob = torch.empty((3, 3, 4), dtype=torch.int32, device=DEV)
                    hd.forward_boxes(ox, None, None, native.MASK_NONE, ob, _stream())
                    _assert_boxes(ob.cpu().numpy(), oboxes, oplanes, f"32x48 between replays {i} and {i + 1}")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ g
@functools.lru_cache(maxsize=None)
def _photo_case(ih, iw, size, mode):
    """(photos, resized bytes per photo): shared between the plans."""
    photos = pn.photo_sequence(ih, iw, mode)
    return photos, [pn.pillow_resized(p, size) for p in photos]


@pytest.mark.parametrize("dtype", ["fp32", "mixed", "bf16"])
@pytest.mark.parametrize("mode", pn.PHOTO_MODES)
@pytest.mark.parametrize("ih,iw,size", pn.PHOTO_SIZES, ids=[f"{a}x{b}to{s}" for a, b, s in pn.PHOTO_SIZES])
def test_photo_graph_with_changing_photos(ih, iw, size, mode, dtype, models, monkeypatch):
    """One photo graph, one pinned photo buffer rewritten between six replays (all 255, a block at the top left, all
    0, a block at the bottom right, an interior block, all 255).  Every replay: masks against Pillow's resized bytes
    (fp32: the oracle's masks of fl32(16 fl32(v / 255) - 8), no exclusions; 16-bit plans: where v <= 64 or v >=
    192), boxes = np_boxes of the replay's own masks, rectangles = inference.crop_rect, sums = numpy's.  The all-0
    photo gives -1 rectangles and 0 sums straight after full-frame crops; the last replay equals the first bitwise."""
    monkeypatch.setattr(inf, "IMG_SIZE", size)   # crop_rect's mask size: the network size of this case
    photos, resized = _photo_case(ih, iw, size, mode)
    c = photos[0].shape[2]
    m = models(dtype)
    hd = m.native_handle(torch.device(DEV))
    hd.reserve(1, size, size)
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    small = [((1, 3, 4), i32), ((3, 4), i32), ((3,), i64)]
    h_img = torch.empty(ih * iw * c, dtype=u8).pin_memory()
    d_img = torch.empty((ih, iw, c), dtype=u8, device=DEV)
    xg = torch.empty((1, 3, size, size), dtype=torch.float32, device=DEV)
    d_mk, d_rest = Guarded([((1, 3, size, size), u8)]), Guarded(small)
    p_mk, p_rest = Guarded([((1, 3, size, size), u8)], pinned=True), Guarded(small, pinned=True)
    g = hd.photo_graph(h_img, d_img, xg, d_mk.t[0], native.MASK_U8, d_rest.t[0], inf.CROP_PAD, d_rest.t[1], d_rest.t[2],
                       p_mk.t[0], p_rest.t[0], p_rest.t[1], p_rest.t[2])
    try:
        first = None
        for step, photo, v in zip(pn.PHOTO_STEPS, photos, resized):
            what = f"{dtype} {mode} {ih}x{iw}->{size} '{step}'"
            h_img.copy_(torch.from_numpy(photo.reshape(-1)))
            p_mk.fill()
            p_rest.fill()
            g.launch(_stream())
            torch.cuda.synchronize()
            masks = p_mk.check(f"{what}: masks")[0]
            boxes, rects, sums = p_rest.check(f"{what}: boxes / rects / sums")
            got = masks.astype(bool)
            if dtype in ("fp32", "fp32_exact"):
                ref = en.reference_masks(pn.photo_logits(v)[None], en.DEFAULT_THRESHOLDS[:3])
                assert np.array_equal(got, ref), f"{what}: " + en.describe_mismatch("masks", got, ref, "head")
            else:
                far = ~pn.near_cut(v)[None]
                assert far.mean() >= 1 - pn.NEAR_CAP
                ref = (v >= pn.NEAR_HI)[None]
                assert np.array_equal(got & far, ref & far), f"{what}: " + en.describe_mismatch(
                    "masks away from the cut", got & far, ref & far, "head")
            assert np.array_equal(boxes, en.np_boxes(got)), (what, boxes.tolist(), en.np_boxes(got).tolist())
            for k in range(3):
                if boxes[0, k, 2] < 0:
                    want_r, want_s = (-1, -1, -1, -1), 0
                else:
                    x1, y1, x2, y2 = want_r = inf.crop_rect(boxes[0, k], iw, ih)
                    crop = photo[y1:y2, x1:x2, :3] if (x2 > x1 and y2 > y1) else photo[:0]
                    want_s = int(crop.astype(np.int64).sum())
                assert tuple(int(t) for t in rects[k]) == tuple(want_r), (what, k, rects[k].tolist(), want_r)
                assert int(sums[k]) == want_s, (what, k, int(sums[k]), want_s)
            if step == "all255":
                assert got.all() and (boxes[0] == (0, 0, size - 1, size - 1)).all(), what
                assert (sums > 0).all(), what
            if step == "all0":
                assert not got.any() and (boxes == -1).all() and (rects == -1).all() and (sums == 0).all(), what
            out = (masks.tobytes(), boxes.tobytes(), rects.tobytes(), sums.tobytes())
            if first is None:
                first = out
        assert out == first, f"{dtype} {mode} {ih}x{iw}: the last all-255 replay differs from the first"
        d_mk.check("device masks")
        d_rest.check("device boxes / rects / sums")
    finally:
        g.close()
