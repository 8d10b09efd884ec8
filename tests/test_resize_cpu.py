"""The premises of the resize tests (tests/resize_cases.py, tests/test_resize_gpu.py), checked without a GPU: the
table lies outside Pillow's tall-photo branch and covers the pixel forms and passes it claims, the restatement
(oracle/pil_resample.py) equals the installed Pillow on every row, the tap counts are the ones the rows are there for,
saturated content makes clip8 act at both ends, Pillow's pass order changes where the library's routing says it
does, and the level network's biases separate adjacent byte levels in every plan on photos that hold those levels."""
import numpy as np
import pytest
import torch
from PIL import Image

import exact_nets as en
import resize_cases as rc
from oracle import pil_resample as pr
from oracle import unet_oracle as orc

CASE_IDS = [rc.case_id(c) for c in rc.CASES]


# ------------------------------------------------------------------------------------------------ the table
def test_table_lies_outside_the_tall_photo_branch_and_covers_forms_and_passes():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    for c in rc.CASES:
        assert c.ih <= rc.TALL * c.iw or c.oh >= c.ih, rc.case_id(c)
        assert 1 <= c.oh <= 16384 and 1 <= c.ow <= 16384
        if c.ih * c.iw < rc.LARGE:
            assert c.forms == rc.FORMS, rc.case_id(c)
        else:
            assert len(c.forms) == 1, rc.case_id(c)
    for form in ("L", "RGBX", "RGB"):
        ran = {rc.passes(c) for c in rc.CASES if form in c.forms}
        assert ran == {(True, True), (True, False), (False, True), (False, False)}, (form, ran)
    ows = {c.ow for c in rc.CASES}
    assert 1 in ows and any(o < rc.BLOCK for o in ows) and any(o % rc.BLOCK == 1 for o in ows if o > rc.BLOCK)
    assert any(o % rc.BLOCK == rc.BLOCK - 1 for o in ows) and any(o > 512 for o in ows)
    assert any(c.oh != c.ow for c in rc.CASES) and any(c.oh == 1 for c in rc.CASES)
    # a photo of an RGBX case is the RGB photo plus a fourth byte that is not a copy of anything
    c = rc.CASES[2]
    rgb, rgbx, gray = (rc.photo(c, f) for f in rc.FORMS)
    assert rgb.shape == (3, 5, 3) and rgbx.shape == (3, 5, 4) and gray.shape == (3, 5, 1)
    assert np.array_equal(rgbx[..., :3], rgb) and not any(np.array_equal(rgbx[..., 3], rgb[..., k]) for k in range(3))


def test_tap_counts_are_the_ones_the_rows_are_there_for():
    seen = set()
    for c in rc.CASES:
        th, tv = rc.tap_counts(c)
        seen |= set(int(t) for t in th) | set(int(t) for t in tv)
        if c.taps is not None:
            got = (int(th.max()) if th.size else 0, int(tv.max()) if tv.size else 0)
            assert got == c.taps, (rc.case_id(c), got, c.taps)
    by_id = {rc.case_id(c): c for c in rc.CASES}
    assert by_id["1024x1024to512x512"].taps == (8, 8) and by_id["1100x1030to512x512"].taps == (9, 9)
    assert by_id["2048x2050to512x512"].taps == (17, 16)
    assert by_id["7x4000to512x512"].taps[0] == 32 and by_id["9000x600to512x512"].taps[1] == 71
    assert by_id["400x600to16x16"].taps == (150, 100) and by_id["300x200to1x1"].taps == (200, 300)
    for n in rc.TAP_COUNTS_WANTED + (2, 3, 32):
        assert n in seen, n
    assert max(seen) >= 300
    # the last group of a loop is padded in every way: all residues of the tap count modulo the group occur
    assert {n % rc.TAP_GROUP for n in seen} == set(range(rc.TAP_GROUP))


@pytest.mark.parametrize("c", rc.CASES, ids=CASE_IDS)
def test_restatement_equals_pillow_on_every_row_and_form(c):
    contents = rc.CONTENTS if rc.upscales(c) else rc.CONTENTS[:1]
    for content in contents:
        for form in c.forms:
            p = rc.photo(c, form, content)
            assert p.dtype == np.uint8 and p.shape == (c.ih, c.iw, {"RGB": 3, "RGBX": 4, "L": 1}[form])
            if form == "RGBX":   # the image of an RGBX photo is its first three bytes: the RGB case
                if "RGB" in c.forms:
                    assert np.array_equal(p[..., :3], rc.photo(c, "RGB", content))
                continue
            ref = np.asarray(rc.pillow_image(p).resize((c.ow, c.oh)))
            got = pr.resize(p if form == "RGB" else p[..., 0], c.ow, c.oh)
            assert np.array_equal(got, ref), (rc.case_id(c), form, content)
            want = rc.pillow_input(p, c.oh, c.ow)
            assert want.shape == (3, c.oh, c.ow) and want.dtype == np.float32
            rgb = ref if form == "RGB" else np.repeat(ref[..., None], 3, axis=2)
            assert np.array_equal(rc.pillow_bytes(p, c.oh, c.ow), rgb.transpose(2, 0, 1))


UPSCALING = [c for c in rc.CASES if rc.upscales(c)]


@pytest.mark.parametrize("c", UPSCALING, ids=[rc.case_id(c) for c in UPSCALING])
def test_saturated_content_makes_clip8_act_at_both_ends(c):
    """This file's own copy of the passes (rc.unclipped_resize) gives Pillow's bytes, and its sums before clip8 fall
    below 0 somewhere and above 255 somewhere -- except in the rows of NEVER_CLIPS, where they provably cannot."""
    for form in c.forms:
        if form == "RGBX":
            continue
        p = rc.photo(c, form, "saturated")
        assert set(np.unique(p)) <= {0, 255} and (len(np.unique(p)) == 2 or p.size < 4)
        got, sums = rc.unclipped_resize(p, c.oh, c.ow)
        assert np.array_equal(np.broadcast_to(got.transpose(2, 0, 1), (3, c.oh, c.ow)), rc.pillow_bytes(p, c.oh, c.ow))
        lo, hi = min(int(s.min()) for s in sums.values()), max(int(s.max()) for s in sums.values())
        print(rc.case_id(c), form, {k: (int(s.min()), int(s.max())) for k, s in sums.items()})
        if rc.case_id(c) in rc.NEVER_CLIPS:
            assert 0 <= lo and hi <= 255, (rc.case_id(c), form, lo, hi)
        else:
            assert lo < 0 and hi > 255, (rc.case_id(c), form, lo, hi)
    assert set(rc.NEVER_CLIPS) <= set(CASE_IDS)


# ------------------------------------------------------------------------------------------------ tall photos
@pytest.mark.parametrize("h,w,mode", [(1000, 10, "RGB"), (1001, 10, "RGB"), (606, 6, "L"), (300, 2, "L")])
def test_pillows_pass_order_changes_where_the_routing_says(h, w, mode):
    """Up to H = 100 W, and when the photo is not made less tall, the horizontal-first restatement alone equals the
    installed Pillow.  Above, Pillow 12 runs the vertical pass first and Pillow 10 does not: exactly one order
    matches, whichever, and run_unet sends exactly these photos down the host path."""
    from unet_mi355x import inference as inf
    rng = np.random.default_rng([h, w])
    arr = rng.integers(0, 256, (h, w, 3) if mode == "RGB" else (h, w), dtype=np.uint8)
    pil = Image.fromarray(arr)
    ref = np.asarray(pil.resize((512, 512)))
    hv = bool(np.array_equal(pr.resize(arr, 512, 512), ref))
    vh = bool(np.array_equal(pr.resize(arr, 512, 512, order="vh"), ref))
    print(f"{h} x {w} {mode}: Pillow {Image.__version__} equals order " + ", ".join(
        o for o, ok in (("hv", hv), ("vh", vh)) if ok))
    tall = h > 100 * w and h > inf.IMG_SIZE
    assert tall == ((h, w) in ((1001, 10), (606, 6)))
    assert inf.resizes_on_host(pil) == tall
    if tall:
        assert hv != vh, "exactly one pass order must equal the installed Pillow"
    else:
        assert hv and not vh
    assert not inf.resizes_on_host(Image.new(mode, (5, inf.IMG_SIZE)))         # tall, but not made less tall
    assert inf.resizes_on_host(Image.new(mode, (5, inf.IMG_SIZE + 1)))
    assert inf.resizes_on_host(Image.new("RGBA", (8, 8))) and inf.resizes_on_host(Image.new("P", (8, 8)))
    with pytest.raises(ValueError):
        pr.resize(arr, 512, 512, order="xy")


# ------------------------------------------------------------------------------------------------ the levels
@pytest.mark.parametrize("plan", rc.LEVEL_PLANS)
def test_level_biases_separate_adjacent_bytes(plan):
    t = rc.level_values(plan)
    assert len(set(t)) == 256 and (np.diff(t) > 0).all() and np.diff(t).min() >= 2.0 ** -8
    assert t[0] == 0.0 and t[255] == 1.0
    x32 = np.arange(256).astype(np.float32) / np.float32(255.0)
    if plan == "fp32":
        assert np.array_equal(t, x32.astype(np.float64))
    else:   # the plan's level-0 type holds t, and t is not what fp32 holds: the cast is visible
        assert np.array_equal(rc.level_type(plan)(t.astype(np.float32)).astype(np.float64), t)
        assert not np.array_equal(t, x32.astype(np.float64))
    assert abs(en.logit_cut64(0.5)) <= rc.LEVEL_MARGIN * 2.0 ** -10   # the cut of threshold 0.5 is 0
    for levels in rc.LEVEL_SETS:
        assert len(levels) == rc.LEVEL_CLASSES and all(0 <= a < 255 for a in levels)
        b = rc.level_bias(plan, levels)
        assert b.dtype == np.float32
        for k, a in enumerate(levels):
            mid = -(t[a] + t[a + 1]) / 2
            if plan != "fp32":   # the midpoint of two 16-bit values is an fp32 value
                assert float(b[k]) == mid, (plan, a)
            else:                # of two fp32 values it may need a 25th bit: the stored value is its rounding
                assert abs(float(b[k]) - mid) <= 2.0 ** -25
            s = t + float(b[k])
            assert (s[:a + 1] < 0).all() and (s[a + 1:] > 0).all(), (plan, a)
            assert np.abs(s).min() >= rc.LEVEL_MARGIN, (plan, a, np.abs(s).min())
            # the head's fp32 sum has the same sign (and is exact on the 16-bit plans)
            s32 = t.astype(np.float32) + b[k]
            assert np.array_equal(s32 > 0, s > 0) and (plan == "fp32" or np.array_equal(s32.astype(np.float64), s))
    assert len({a for levels in rc.LEVEL_SETS for a in levels}) == 8


@pytest.mark.parametrize("plan", rc.LEVEL_PLANS)
def test_level_network_gives_the_level_masks(plan):
    """The oracle's fp32 forward of the level network on all 256 bytes (a 16 x 16 image per channel, rounded to
    the plan's level-0 type as the device rounds its input): masks at threshold 0.5 == level_masks."""
    v = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16), np.arange(256, dtype=np.uint8).reshape(16, 16).T,
                  np.arange(255, -1, -1, dtype=np.uint8).reshape(16, 16)])
    x = rc.level_type(plan)(v.astype(np.float32) / np.float32(255.0)).astype(np.float32)[None]
    for levels in rc.LEVEL_SETS:
        sd = rc.level_state_dict(plan, levels)
        logits = orc.unet_forward({k: torch.from_numpy(np.array(a)) for k, a in sd.items()}, torch.from_numpy(x)).numpy()
        want = rc.level_masks(v, levels)
        assert np.array_equal(en.reference_masks(logits, rc.LEVEL_THRESHOLDS), want), (plan, levels)
        assert np.array_equal(logits > 0, want) and np.abs(logits).min() >= rc.LEVEL_MARGIN
        assert want.any(axis=(2, 3)).all() and not want.all(axis=(2, 3)).any()


@pytest.mark.parametrize("ih,iw,size", rc.LEVEL_SIZES)
def test_level_photos_hold_every_probed_level_and_its_successor(ih, iw, size):
    for form in rc.FORMS:
        photos = rc.level_photos(ih, iw, form)
        assert len(photos) == 2 and not np.array_equal(photos[0], photos[1])
        for p in photos:
            assert p.shape == (ih, iw, {"RGB": 3, "RGBX": 4, "L": 1}[form]) and p.dtype == np.uint8
            v = rc.pillow_bytes(p, size, size)
            for levels in rc.LEVEL_SETS:
                for k, a in enumerate(levels):
                    assert (v[k % 3] == a).any() and (v[k % 3] == a + 1).any(), (form, a)
    assert not np.array_equal(rc.pillow_bytes(photos[0], size, size), rc.pillow_bytes(photos[1], size, size))
    need_h, need_v = iw != size, ih != size
    assert need_h and need_v == ((ih, iw) != (64, 90))   # 64 x 90 alone has no vertical pass


# ------------------------------------------------------------------------------------------------ the crops
@pytest.mark.parametrize("bh,bw", rc.CROP_SPACES)
def test_crop_boxes_and_rectangle_reference(bh, bw):
    from unet_mi355x import inference as inf
    b = rc.crop_boxes(bh, bw)
    assert b.shape == (6 + rc.CROP_RANDOM, 4) and b.dtype == np.int32 and (b[0] == -1).all()
    assert (b[1:, 0] <= b[1:, 2]).all() and (b[1:, 1] <= b[1:, 3]).all() and b[1:].min() >= 0
    assert b[1:, 2].max() == bw - 1 and b[1:, 3].max() == bh - 1
    assert tuple(b[5]) == (0, 0, bw - 1, bh - 1)
    if (bh, bw) == (64, 64):   # at the drop-in's own mask size and pad, the reference is inference.crop_rect
        for box in rc.crop_boxes(inf.IMG_SIZE, inf.IMG_SIZE)[1:]:
            assert rc.crop_rect(box, 600, 400, inf.IMG_SIZE, inf.IMG_SIZE, inf.CROP_PAD) == inf.crop_rect(box, 600, 400)
    kinds = set()
    for ih, iw in rc.CROP_PHOTOS:
        p = rc.crop_photo(ih, iw, "RGB")
        assert p.shape == (ih, iw, 3)
        for pad in rc.CROP_PADS:
            for box in b:
                x1, y1, x2, y2 = r = rc.crop_rect(box, iw, ih, bw, bh, pad)
                if r == (-1, -1, -1, -1):
                    kinds.add("empty")
                    continue
                assert 0 <= x1 and x2 <= iw and 0 <= y1 and y2 <= ih
                kinds.add("degenerate" if x2 <= x1 or y2 <= y1 else "crop")
                if x2 > x1 and y2 > y1:
                    assert rc.crop_sum(p, r) == int(p[y1:y2, x1:x2].sum(dtype=np.int64))
    assert kinds == {"empty", "degenerate", "crop"}
