"""The premises of the placed-mask tests (tests/placed_nets.py, tests/test_placed_gpu.py), checked without a GPU:
the pass-through network's logits are exactly -8 / +8 and its masks the placed bits, every named pattern has the
box its name promises and lies where the box kernel's chunks and words make it interesting, and the photos of the
photo-graph test survive Pillow's resize as the test assumes."""
import numpy as np
import pytest
import torch

import exact_nets as en
import placed_nets as pn
from oracle import unet_oracle as orc

BOX_SHAPES = [(16, 16), (32, 48), (48, 32), (64, 64), (512, 512), (528, 512)]


# ------------------------------------------------------------------------------------------------ the network
@pytest.mark.parametrize("c_in,n_classes", [(3, 1), (3, 3), (3, 4), (1, 3)])
def test_passthrough_logits_are_exact_and_masks_are_the_placed_bits(c_in, n_classes):
    """2 x c_in x 32 x 48: the oracle's logits are exactly -8 or +8 and equal placed_logits, routing_forward_f64
    (float64, BatchNorm taken as + beta) gives the same values, and the oracle's masks at the default and at the
    class tests' thresholds are the placed bits."""
    sd = pn.passthrough_state_dict(c_in, n_classes)
    x, planes = pn.pack_planes(list(pn.placed_patterns(32, 48)), 32, 48, n_classes)
    x = np.ascontiguousarray(x[:2, :c_in])
    assert set(np.unique(x)) == {0.0, 1.0}
    logits = orc.unet_forward({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, torch.from_numpy(x)).numpy()
    assert logits.dtype == np.float32 and set(np.unique(logits)) == {-8.0, 8.0}
    assert np.array_equal(logits, pn.placed_logits(x, n_classes))
    f64 = en.routing_forward_f64(sd, x)["logits"]
    assert np.array_equal(f64, logits.astype(np.float64))
    bits = pn.placed_bits(x, n_classes)
    assert bits.any(axis=(2, 3)).any() and not bits.all()
    for thr in (en.DEFAULT_THRESHOLDS, en.CLASS_THRESHOLDS):
        assert all(-8 < en.logit_cut64(t) < 8 for t in thr)
        assert np.array_equal(en.reference_masks(logits, thr[:n_classes]), bits), thr
    # a uint8 input in {0, 255} is the same input: 255 / 255 == 1 in fp32
    assert np.array_equal((x * 255).astype(np.uint8).astype(np.float32) / np.float32(255.0), x)


def test_passthrough_weights_are_what_the_module_says():
    sd = pn.passthrough_state_dict(3, 4)
    nz = {k: np.argwhere(v != 0) for k, v in sd.items() if k.endswith(".weight") and v.ndim == 4}
    assert [tuple(p) for p in nz["down1.net.0.weight"]] == [(0, 0, 1, 1), (1, 1, 1, 1), (2, 2, 1, 1), (3, 0, 1, 1)]
    assert [tuple(p) for p in nz["conv1.net.0.weight"]] == [(k, 64 + k, 1, 1) for k in range(4)]
    for key in ("down1.net.3.weight", "conv1.net.3.weight"):
        assert [tuple(p) for p in nz[key]] == [(k, k, 1, 1) for k in range(4)]
    assert [tuple(p) for p in nz["out_conv.weight"]] == [(k, k, 0, 0) for k in range(4)]
    assert set(sd["out_conv.weight"][sd["out_conv.weight"] != 0]) == {16.0} and set(sd["out_conv.bias"]) == {-8.0}
    others = [k for k in nz if k not in ("down1.net.0.weight", "down1.net.3.weight", "conv1.net.0.weight",
                                         "conv1.net.3.weight", "out_conv.weight")]
    assert len(others) == 14 + 4 and all(len(nz[k]) == 0 for k in others)
    for v in (0.0, 1.0, 8.0, 16.0, -8.0):
        assert en.representable(np.array([v], np.float64))


# ------------------------------------------------------------------------------------------------ the patterns
@pytest.mark.parametrize("h,w", BOX_SHAPES)
def test_every_pattern_has_the_box_its_name_promises(h, w):
    pats = pn.placed_patterns(h, w)
    names = list(pats)
    boxes = en.np_boxes(np.stack(list(pats.values()))[None])[0]
    for name, box in zip(names, boxes):
        want = pn.promised_box(name, h, w)
        if want is not None:
            assert tuple(int(v) for v in box) == want, (name, box, want)
    for name in ("empty", "full", "corner_tl", "corner_tr", "corner_bl", "corner_br", "diag", "row", "col", "half"):
        assert name in pats
    singles = {tuple(int(v) for v in n.split("_")[1:]) for n in names if n.startswith("px_")}
    singles |= {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    for y in (0, h - 1):
        for x in (15, 16, 31, w - 17, w - 16):
            assert not 0 <= x < w or (y, x) in singles, (y, x)
    assert (h - 1, w - 8) in singles                      # the last row, inside the last word
    assert not pats["empty"].any() and pats["full"].all()
    for name in names:
        if name.startswith(("px_", "corner_")):
            assert pats[name].sum() == 1
    assert pats["diag"].sum() == pats["row"].sum() == pats["col"].sum() == 2
    assert 0.4 < pats["half"].mean() < 0.6
    assert len({a.tobytes() for a in pats.values()}) == len(pats), "two names, one pattern"
    if w >= 32:
        ys, xs = np.where(pats["row"])
        assert ys[0] == ys[1] and xs[0] // 16 != xs[1] // 16
    if h * w // 16 > pn.BOX_CHUNK:
        last0 = [p for p in singles if pn.chunk_of(*p, w) == 0 and (p[0] * (w // 16) + p[1] // 16) == pn.BOX_CHUNK - 1]
        first1 = [p for p in singles if (p[0] * (w // 16) + p[1] // 16) == pn.BOX_CHUNK]
        assert last0 and first1, (last0, first1)
    if (h, w) == (512, 512):
        assert "px_31_511" in pats and "px_32_0" in pats
    if (h, w) == (528, 512):   # 16.5 chunks: the last one is ragged and holds the last row
        assert h * (w // 16) == 16 * pn.BOX_CHUNK + pn.BOX_CHUNK // 2 and pn.chunk_of(h - 1, w - 1, w) == 16


@pytest.mark.parametrize("n_classes", [1, 3, 4])
@pytest.mark.parametrize("h,w", [(16, 16), (32, 48), (512, 512)])
def test_pack_planes_gives_every_name_a_plane_of_its_own(h, w, n_classes):
    pats = pn.placed_patterns(h, w)
    x, planes = pn.pack_planes(list(pats), h, w, n_classes)
    assert x.shape == (len(planes), 3, h, w) and x.dtype == np.float32 and set(np.unique(x)) <= {0.0, 1.0}
    used = min(n_classes, 3)
    named = [p[:used] for p in planes[:-3]]
    flat = [n for img in named for n in img]
    for name in pats:
        assert flat.count(name) >= 1, name
        if name not in ("empty", "full"):
            assert flat.count(name) == 1, name
    assert [p[:used] for p in planes[-3:]] == [["full"] * used, ["empty"] * used, ["full"] * used]
    bits = pn.placed_bits(x, n_classes)
    for n, img in enumerate(planes):
        assert len(img) == n_classes
        for k, name in enumerate(img):
            assert np.array_equal(bits[n, k], pats[name]), (n, k, name)
    if used == 3:   # full and empty sit between single pixels of the same image
        for special in ("full", "empty"):
            img = next(p for p in planes if p[1] == special and p[0] != special)
            assert pats[img[0]].sum() <= 2 and pats[img[2]].sum() <= 2, img
    if n_classes < 3:   # channels nobody reads are not empty: reading the wrong one shows
        assert all(x[n, c].any() for n in range(len(planes)) for c in range(used, 3))


def test_wide_and_strip_patterns_lie_where_their_names_say():
    h, w = 16, 4112
    words = w // 16
    assert words == 257 and words & (words - 1) and w <= 16384
    pats = pn.wide_patterns(h, w)
    for x in (0, 4095, 4096, 4111):
        assert pats[f"px_0_{x}"].sum() == 1 and pats[f"px_0_{x}"][0, x]
        assert pats[f"px_{h - 1}_{x}"][h - 1, x]
    word = lambda y, x: y * words + x // 16   # noqa: E731
    (a, b) = np.argwhere(pats["words_0_256_one_row"])
    assert a[0] == b[0] and (a[1] // 16, b[1] // 16) == (0, 256)
    (a, b) = np.argwhere(pats["word_256_then_word_0"])
    assert (a[0], a[1] // 16, b[0], b[1] // 16) == (0, 256, 1, 0) and word(*b) == word(*a) + 1
    for name in ("same_thread", "same_thread_late"):
        (a, b) = np.argwhere(pats[name])
        assert word(*b) == word(*a) + pn.BOX_THREADS and a[1] // 16 != b[1] // 16   # one thread, two column words
        assert word(*a) // pn.BOX_CHUNK == word(*b) // pn.BOX_CHUNK                # in one loop pass
    h, w = 1040, 1024
    assert h * (w // 16) == 65 * pn.BOX_CHUNK and 65 == pn.BOX_MAX_STRIPS + 1
    sp = pn.strip_patterns(h, w)
    assert [pn.chunk_of(y, x, w) for y, x in sp["second_pass"]] == [64] and sp["second_pass"][0][0] >= 1024
    assert [pn.chunk_of(y, x, w) for y, x in sp["chunk_63"]] == [63]
    assert [pn.chunk_of(y, x, w) for y, x in sp["far_corners"]] == [0, 64]


# ------------------------------------------------------------------------------------------------ the photos
@pytest.mark.parametrize("ih,iw,size", pn.PHOTO_SIZES)
def test_photos_survive_the_resize_as_the_gpu_test_assumes(ih, iw, size):
    """Pillow's own resize: an all-0 photo stays all 0 and an all-255 photo all 255; block photos leave at most
    NEAR_CAP of the network's pixels between NEAR_LO and NEAR_HI (the pixels the 16-bit plans are not compared at),
    per photo and per plane; and every block photo's masks are neither empty nor full."""
    worst = 0.0
    for mode in pn.PHOTO_MODES:
        photos = pn.photo_sequence(ih, iw, mode)
        assert len(photos) == len(pn.PHOTO_STEPS)
        for step, photo in zip(pn.PHOTO_STEPS, photos):
            assert photo.shape == (ih, iw, {"RGB": 3, "RGBX": 4, "L": 1}[mode]) and photo.dtype == np.uint8
            v = pn.pillow_resized(photo, size)
            assert v.shape == (3, size, size)
            if step == "all255":
                assert (v == 255).all()
            elif step == "all0":
                assert (v == 0).all()
            else:
                on = v >= pn.NEAR_HI
                assert on.any(axis=(1, 2)).all() and not on.all(axis=(1, 2)).any(), (mode, step)
            near = pn.near_cut(v)
            share = max(float(near.mean()), float(near.mean(axis=(1, 2)).max()))
            worst = max(worst, share)
            assert share <= pn.NEAR_CAP, (mode, step, share)
        if mode == "RGB":   # a different block per channel
            v = pn.pillow_resized(photos[1], size)
            assert not np.array_equal(v[0], v[1]) and not np.array_equal(v[1], v[2])
    print(f"{ih} x {iw} -> {size}: largest near-cut share {worst:.4f} (cap {pn.NEAR_CAP})")
    # the logits the fp32 plans must give at the extremes, and the 16-bit plans' margins
    assert np.array_equal(pn.photo_logits(np.array([0, 255], np.uint8)), np.array([-8.0, 8.0], np.float32))
    lo, hi = pn.photo_logits(np.array([pn.NEAR_LO, pn.NEAR_HI], np.uint8))
    assert lo < -3.98 and hi > 4.04
    assert all(lo + 0.5 < en.logit_cut64(t) < hi - 0.5 for t in en.DEFAULT_THRESHOLDS + en.CLASS_THRESHOLDS)
