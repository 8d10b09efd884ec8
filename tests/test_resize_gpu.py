"""The device resize (csrc/unet_preprocess.hip: resample_h_kernel, resample_v_kernel, to_planar_f32_kernel) and the
crop statistics at every geometry edge (tests/resize_cases.py; premises in tests/test_resize_cpu.py).  Needs a GPU: run
with -m gpu.

  a  the eager resize, bit for bit against Pillow itself: output sizes 1 .. 1024, square and not, ow below, at and one
     past a block of 256 threads; tap counts 1, 8, 9, 16, 17 and up to 300; RGB, RGBX and L crossed with both passes,
     one pass and none; random bytes and, where an axis grows, saturated bytes (clip8 at both ends); the output carved
     out of a buffer of NaNs that must stay NaN on either side
  b  the photo graph's resized pixels at adjacent byte levels, in every plan: a pass-through network whose class k
     answers "resized byte > a_k", so that the pre-cast 16-bit input the vertical pass writes into the workspace is
     read back through the head with no pixel left out -- and the eager preprocess + forward gives the same masks
  c  crop statistics in mask spaces other than 512 x 512 and at pads 0, 0.15 and 0.5
  d  photos taller than 100 times their width take run_unet's host path; one at the limit still takes the graph

References: Pillow's Image.resize, numpy's sums, the reference's crop lines restated (resize_cases.crop_rect).  Every
comparison is np.array_equal; nothing here looks for reads or writes out of bounds other than by value.

Value-only mutations of the kernels, each caught on an MI355X (tests that then fail):
  resample_v_kernel's 16-bit store writes byte 128 as 127      exactly the 27 cases of b on fp16 / bf16 / mixed with a
                                                                vertical pass; the fp32 and 64 x 90 cases, all of a and
                                                                every older photo-graph and resize test still pass
  to_planar_f32_kernel halves plane 2 of a gray photo          a [512x512to512x512] L (older tests: none)
  resample_h_kernel counts the last tap twice in a ragged      a [512x1to512x512] and every row with a horizontal pass
  group (weight kept for x0 + j == n)
The whole file takes about 7 s on an MI355X; no test more than 0.9 s (the first one, which creates the HIP context)."""
import os
import tempfile

import numpy as np
import pytest
import torch

import exact_nets as en
import placed_nets as pn
import resize_cases as rc
from test_classes_gpu import GUARD_BYTES, Guarded
from unet_mi355x import inference as inf
from unet_mi355x import native
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)   # a copy: the shared photos are read-only


def _model(sd, n_classes, dtype, thresholds):
    m = UNet(3, n_classes, compute_dtype=dtype, thresholds=thresholds)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def _describe(got, want):
    """The first bytes that differ, as bytes: '(c, y, x) got / want'."""
    bad = np.argwhere(got != want)
    head = "; ".join(f"{tuple(int(i) for i in p)} got {float(got[tuple(p)]) * 255:.4f} want "
                     f"{float(want[tuple(p)]) * 255:.0f}" for p in bad[:6])
    return f"{len(bad)} of {got.size} samples differ; first (c, y, x), as bytes: {head}"


# ------------------------------------------------------------------------------------------------ a
@pytest.fixture(scope="module")
def handle():
    """Any handle resizes: one small fp32 model for the whole file."""
    m = _model(pn.passthrough_state_dict(3, 3), 3, "fp32", en.DEFAULT_THRESHOLDS[:3])
    yield m.native_handle(torch.device(DEV))
    m.close()


@pytest.mark.parametrize("c", rc.CASES, ids=[rc.case_id(c) for c in rc.CASES])
def test_eager_resize_equals_pillow_bit_for_bit(c, handle):
    """Handle.preprocess into [3, oh, ow] in the middle of a buffer of NaNs, every form of the row, random bytes and
    (an axis grows) saturated bytes: Pillow's bytes / 255 exactly, no NaN left inside, every NaN left outside, and
    the RGBX result equal to the RGB result."""
    for content in (rc.CONTENTS if rc.upscales(c) else rc.CONTENTS[:1]):
        got = {}
        for form in c.forms:
            what = f"{rc.case_id(c)} {form} {content} ({c.why})"
            p = rc.photo(c, form, content)
            out = Guarded([((3, c.oh, c.ow), torch.float32)])
            handle.preprocess(_dev(p), out.t[0], _stream())
            got[form] = out.check(what)[0]
            want = rc.pillow_input(p, c.oh, c.ow)
            assert np.array_equal(got[form], want), f"{what}: " + _describe(got[form], want)
        if "RGB" in got and "RGBX" in got:
            assert np.array_equal(got["RGBX"], got["RGB"]), f"{rc.case_id(c)} {content}: RGBX differs from RGB"


# ------------------------------------------------------------------------------------------------ b
@pytest.fixture(scope="module")
def level_models():
    """One level network per (plan, level set), made when first asked for, closed at the end."""
    made = {}

    def get(plan, levels):
        if (plan, levels) not in made:
            made[(plan, levels)] = _model(rc.level_state_dict(plan, levels), rc.LEVEL_CLASSES, plan, rc.LEVEL_THRESHOLDS)
        return made[(plan, levels)]

    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("plan", rc.LEVEL_PLANS)
@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("ih,iw,size", rc.LEVEL_SIZES, ids=[f"{a}x{b}to{s}" for a, b, s in rc.LEVEL_SIZES])
def test_photo_graph_resized_pixels_at_every_level(ih, iw, size, form, plan, level_models):
    """Per level set one photo graph, replayed with two photos: mask k == (Pillow's resized byte of channel k % 3 >
    a_k) at every pixel, on bytes that hold a_k and a_k + 1.  The network input the graph was given is either never
    written (the 16-bit plans' vertical pass writes the first conv's pre-cast input instead) or Pillow's bytes / 255
    exactly; the fp32 plan, and a photo without a vertical pass, must write it.  The eager preprocess + forward_boxes
    gives the same masks."""
    photos = rc.level_photos(ih, iw, form)
    resized = [rc.pillow_bytes(p, size, size) for p in photos]
    c = photos[0].shape[2]
    u8, i32, i64 = torch.uint8, torch.int32, torch.int64
    nk = rc.LEVEL_CLASSES
    small = [((1, nk, 4), i32), ((nk, 4), i32), ((nk,), i64)]
    for levels in rc.LEVEL_SETS:
        m = level_models(plan, levels)
        hd = m.native_handle(torch.device(DEV))
        hd.reserve(1, size, size)
        h_img = torch.empty(ih * iw * c, dtype=u8).pin_memory()
        d_img = torch.empty((ih, iw, c), dtype=u8, device=DEV)
        xg = Guarded([((1, 3, size, size), torch.float32)])
        d_mk, d_rest = Guarded([((1, nk, size, size), u8)]), Guarded(small)
        p_mk = Guarded([((1, nk, size, size), u8)], pinned=True)
        g = hd.photo_graph(h_img, d_img, xg.t[0], d_mk.t[0], native.MASK_U8, d_rest.t[0], inf.CROP_PAD, d_rest.t[1],
                           d_rest.t[2], p_mk.t[0])
        try:
            for i, (photo, v) in enumerate(zip(photos, resized)):
                what = f"{plan} {form} {ih}x{iw}->{size} levels {levels} photo {i}"
                want = rc.level_masks(v, levels)
                h_img.copy_(torch.from_numpy(np.array(photo).reshape(-1)))   # a copy: the photos are read-only
                p_mk.fill()
                xg.fill()
                g.launch(_stream())
                torch.cuda.synchronize()
                got = p_mk.check(f"{what}: masks")[0].astype(bool)
                assert np.array_equal(got, want), f"{what}: " + en.describe_mismatch("masks", got, want, "photo graph")
                raw = xg.raw.cpu().numpy().view(np.float32)
                lo, hi = GUARD_BYTES // 4, GUARD_BYTES // 4 + 3 * size * size
                assert np.isnan(raw[:lo]).all() and np.isnan(raw[hi:]).all(), f"{what}: written around the input"
                x = raw[lo:hi].reshape(3, size, size)
                written = not np.isnan(x).all()
                if plan == "fp32" or ih == size:
                    assert written, f"{what}: the graph did not write its network input"
                if written:
                    xw = v.astype(np.float32) / np.float32(255.0)
                    assert np.array_equal(x, xw), f"{what}: network input: " + _describe(x, xw)
                # the eager path
                with torch.no_grad():
                    mk, _ = m.forward_boxes(m.preprocess(_dev(photo), size), masks="u8")
                eager = mk.cpu().numpy().astype(bool)
                assert np.array_equal(eager, want), f"{what}: " + en.describe_mismatch("eager masks", eager, want, "head")
            d_mk.check("device masks")
            d_rest.check("device boxes / rects / sums")
        finally:
            g.close()


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("form", rc.FORMS)
@pytest.mark.parametrize("ih,iw", rc.CROP_PHOTOS, ids=[f"{a}x{b}" for a, b in rc.CROP_PHOTOS])
def test_crop_statistics_in_other_mask_spaces(ih, iw, form):
    """native.crop_stats with boxes of four mask spaces at three pads: the rectangles are the reference's lines in
    float64 with the mask size as a parameter, the sums numpy's over the rectangle's RGB (or L) bytes; the empty
    box gives four -1s and 0."""
    photo = rc.crop_photo(ih, iw, form)
    img = _dev(photo)
    for bh, bw in rc.CROP_SPACES:
        boxes = rc.crop_boxes(bh, bw)
        n = len(boxes)
        d_boxes = _dev(boxes)
        for pad in rc.CROP_PADS:
            what = f"{ih}x{iw} {form}, boxes of {bh}x{bw}, pad {pad}"
            out = Guarded([((n, 4), torch.int32), ((n,), torch.int64)])
            native.crop_stats(img, d_boxes, bh, bw, pad, out.t[0], out.t[1], _stream())
            rects, sums = out.check(what)
            want_r = np.array([rc.crop_rect(b, iw, ih, bw, bh, pad) for b in boxes], np.int32)
            want_s = np.array([rc.crop_sum(photo, tuple(int(t) for t in r)) for r in want_r], np.int64)
            bad = np.argwhere((rects != want_r).any(axis=1))[:, 0]
            assert bad.size == 0, (what, [(boxes[i].tolist(), rects[i].tolist(), want_r[i].tolist()) for i in bad[:6]])
            bad = np.argwhere(sums != want_s)[:, 0]
            assert bad.size == 0, (what, [(boxes[i].tolist(), want_r[i].tolist(), int(sums[i]), int(want_s[i]))
                                          for i in bad[:6]])
            assert (rects[0] == -1).all() and sums[0] == 0 and (sums[1:] >= 0).all()


# ------------------------------------------------------------------------------------------------ d
def _host_path(model, pil):
    """run_unet's host path: Pillow's resize, the host preprocess, forward_boxes, boxes_to_crops."""
    x = inf.preprocess(pil.resize((inf.IMG_SIZE, inf.IMG_SIZE)))
    with torch.no_grad():
        mk, bx = model.forward_boxes(x, masks="u8")
    m = mk.cpu().numpy()[0].astype(bool)
    return {k: m[i] for i, k in enumerate(inf.FIELDS)}, inf.boxes_to_crops(pil, bx.cpu().numpy()[0])


def _same(a, b, what):
    (m1, c1), (m2, c2) = a, b
    for k in inf.FIELDS:
        assert np.array_equal(m1[k], m2[k]), f"{what}: mask {k}: {int((m1[k] != m2[k]).sum())} pixels differ"
        assert (c1[k] is None) == (c2[k] is None), f"{what}: crop {k}"
        if c1[k] is not None:
            assert c1[k].size == c2[k].size and np.array_equal(np.asarray(c1[k]), np.asarray(c2[k])), f"{what}: crop {k}"


def test_photos_taller_than_100_widths_take_the_host_path(monkeypatch):
    """run_unet and run_unet_batch on a 1001 x 10 RGB and a 606 x 6 L photo return exactly the host path's masks and
    crops -- the masks of the pass-through network, resized byte above the cut, so a resize in the other pass order
    shows at thousands of pixels -- and no graph is captured for them; a 1000 x 10 photo still takes the photo graph,
    and its masks are Pillow's bytes above the cut too."""
    from PIL import Image
    monkeypatch.setattr(inf, "DEVICE", DEV)
    rng = np.random.default_rng(5)
    tall = [Image.fromarray(rng.integers(0, 256, (1001, 10, 3), dtype=np.uint8)),
            Image.fromarray(rng.integers(0, 256, (606, 6), dtype=np.uint8))]
    limit = Image.fromarray(rng.integers(0, 256, (1000, 10, 3), dtype=np.uint8))
    assert [p.mode for p in tall] == ["RGB", "L"] and all(inf.resizes_on_host(p) for p in tall)
    assert not inf.resizes_on_host(limit)
    sd = pn.passthrough_state_dict(3, 3)
    with tempfile.TemporaryDirectory() as td:
        ck = os.path.join(td, "best_unet_model.pth")
        torch.save({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, ck)
        model = inf._cached_model(ck, "fp32")
        st = inf._staging.get(DEV)
        if st is not None:
            with st.lock:
                st.drop_graphs()
        want = [_host_path(model, p) for p in tall]
        for p, w in zip(tall, want):
            v = pn.pillow_resized(np.asarray(p).reshape(p.size[1], p.size[0], -1), inf.IMG_SIZE)
            ref = en.reference_masks(pn.photo_logits(v)[None], inf.THRESHOLDS)[0]
            for i, k in enumerate(inf.FIELDS):   # the host path itself: Pillow's bytes above the cut
                assert np.array_equal(w[0][k], ref[i]) and 0.2 < ref[i].mean() < 0.8, k
            for rep in range(2):
                _same(inf.run_unet(p, ck, compute_dtype="fp32"), w, f"run_unet {p.size[1]} x {p.size[0]} {p.mode}")
        st = inf._staging[DEV]
        assert not any(key[:2] in ((1001, 10), (606, 6)) for key in st.graphs), list(st.graphs)
        at_limit = inf.run_unet(limit, ck, compute_dtype="fp32")
        assert [key[:2] for key in st.graphs] == [(1000, 10)], list(st.graphs)
        v = pn.pillow_resized(np.asarray(limit), inf.IMG_SIZE)
        ref = en.reference_masks(pn.photo_logits(v)[None], inf.THRESHOLDS)[0]
        for i, k in enumerate(inf.FIELDS):
            assert np.array_equal(at_limit[0][k], ref[i]), k
        batch = inf.run_unet_batch(tall + [limit], ck, compute_dtype="fp32")
        for p, got, w in zip(tall + [limit], batch, want + [at_limit]):
            _same(got, w, f"run_unet_batch {p.size[1]} x {p.size[0]} {p.mode}")
        with st.lock:
            st.drop_graphs()
