"""Resize cases (tests/test_resize_cpu.py, tests/test_resize_gpu.py): the geometries, pixel forms and contents at
which the device resize (csrc/unet_preprocess.hip: resample_h_kernel, resample_v_kernel, to_planar_f32_kernel)
changes behaviour, the level network that makes the photo graph's resized pixels readable through the head, and the
boxes of the crop-statistics cases.

  CASES              (ih, iw) -> (oh, ow) geometries, each with the property it is there for, the pixel forms it runs
                     in and, where the property is a tap count, the largest tap count per pass it claims
  photo              the seeded content of a case in one form: random bytes, or saturated (random 0 / 255)
  pillow_bytes       Pillow's own resize of a photo, gray replicated: uint8 [3, oh, ow] -- THE reference
  unclipped_resize   this module's own numpy copy of the two passes, returning the sums before clip8 per pass
  level_*            the pass-through network with one bias per class between two adjacent byte levels, so that
                     mask[k] == (resized[k % 3] > a_k) exactly in every plan, and photos that hold every probed level
  crop_*             mask-space boxes and the reference's crop rectangle with the mask size as a parameter

References are Pillow itself, numpy's sums and the reference's crop lines restated; nothing here is taken from the
code under test.  A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import exact_nets as en
import placed_nets as pn
from oracle import pil_resample as pr

FORMS = ("RGB", "RGBX", "L")
LARGE = 4_000_000          # photos of more pixels run in the one form their row names
TALL = 100                 # Pillow's Image.resize runs the vertical pass first when ih > TALL * iw and oh < ih
TAP_GROUP = 8              # csrc/unet_preprocess.hip kTapGroup
BLOCK = 256                # threads per block of every resize kernel: the guard is xx >= ow

Case = namedtuple("Case", "ih iw oh ow why forms taps")


def _case(ih, iw, oh, ow, why, taps=None, forms=FORMS):
    """taps = (largest horizontal tap count, largest vertical tap count) where the row claims one (None: no claim;
    a pass that does not run has no taps: 0)."""
    return Case(ih, iw, oh, ow, why, tuple(forms), taps)


CASES = [
    # one-pixel axes and tiny photos
    _case(1, 1, 512, 512, "a 1-pixel photo: one tap, weight 1, in both passes", (1, 1)),
    _case(2, 2, 512, 512, "two taps in both passes, one weight negative", (2, 2)),
    _case(3, 5, 512, 512, "three vertical taps, four horizontal", (4, 3)),
    _case(1, 700, 512, 512, "a 1-pixel column: one vertical tap after a down-scaling horizontal pass", (6, 1)),
    _case(512, 1, 512, 512, "a 1-pixel row, horizontal pass only: one tap", (1, 0)),
    _case(1, 512, 512, 512, "a 1-pixel column, vertical pass only: one tap", (0, 1)),
    _case(300, 3, 512, 512, "three pixels wide", (3, 4)),
    # near-identity
    _case(511, 513, 512, 512, "near-identity: up by one row, down by one column"),
    _case(513, 511, 512, 512, "near-identity: down by one row, up by one column"),
    _case(512, 512, 512, 512, "no resize: to_planar_f32_kernel alone, C = 1 and 3, S = 1, 3 and 4", (0, 0)),
    # tap counts at the 8-tap group's borders
    _case(1024, 1024, 512, 512, "exactly one full tap group in both passes", (8, 8)),
    _case(1100, 1030, 512, 512, "one tap into the second group in both passes", (9, 9)),
    _case(2048, 2050, 512, 512, "two full groups vertically, one tap into the third horizontally", (17, 16),
          forms=("RGB",)),
    # long tap loops
    _case(7, 4000, 512, 512, "four full groups horizontally", (32, 4)),
    _case(9000, 600, 512, 512, "71 vertical taps, 9 groups", (5, 71), forms=("L",)),
    _case(400, 600, 16, 16, "150 and 100 taps, an output far below one block", (150, 100)),
    _case(300, 200, 1, 1, "every pixel of the photo in one output sample", (200, 300)),
    _case(300, 200, 1, 700, "one output row, 300 vertical taps", (4, 300)),
    _case(300, 200, 700, 1, "one output column, 200 horizontal taps: one live thread", (200, 4)),
    # outputs that are not 512
    _case(400, 600, 1024, 1024, "1024 out, up-scaling: four full blocks per row"),
    _case(1500, 1100, 1024, 1024, "1024 out, down-scaling"),
    _case(1024, 700, 1024, 1024, "1024 out, horizontal pass only", (4, 0)),
    _case(400, 600, 48, 80, "a small non-square output: ow below one block", (30, 34)),
    _case(300, 200, 257, 255, "ow = 255: the last thread of the only block is idle"),
    _case(300, 200, 255, 257, "ow = 257: the second block has one live thread"),
    _case(64, 64, 100, 300, "a wide non-square output: ow = 256 + 44"),
]
TAP_COUNTS_WANTED = (1, 8, 9, 16, 17)   # each occurs as some output sample's tap count somewhere in the table


def case_id(c: Case) -> str:
    return f"{c.ih}x{c.iw}to{c.oh}x{c.ow}"


def passes(c: Case):
    """(horizontal pass runs, vertical pass runs), as the library decides it."""
    return c.ow != c.iw, c.oh != c.ih


def upscales(c: Case) -> bool:
    """The rows that also run with saturated content: some axis grows."""
    return c.ow > c.iw or c.oh > c.ih


# Up-scaling rows in which no sum can leave 0..255, so that clip8 cannot act (asserted on the CPU, both ways: these
# rows' sums stay inside, every other up-scaling row's sums leave at both ends).  They still run saturated on the
# device.
NEVER_CLIPS = {
    "1x1to512x512": "one tap of weight 1 in both passes",
    "512x1to512x512": "one tap of weight 1, no vertical pass",
    "1x512to512x512": "one tap of weight 1, no horizontal pass",
    "300x200to700x1": "the horizontal pass averages 200 samples to mid-gray before the vertical pass up-scales",
}


def tap_counts(c: Case):
    """Per pass that runs, the tap count of every output sample (pr.coeffs' bounds): (horizontal, vertical), an
    empty array for a pass that does not run."""
    need_h, need_v = passes(c)
    none = np.zeros(0, np.int64)
    return (pr.coeffs(c.iw, c.ow)[0][:, 1] if need_h else none, pr.coeffs(c.ih, c.oh)[0][:, 1] if need_v else none)


# ------------------------------------------------------------------------------------------------ contents
CONTENTS = ("random", "saturated")


@functools.lru_cache(maxsize=8)
def _bytes4(ih: int, iw: int, content: str) -> np.ndarray:
    rng = np.random.default_rng([ih, iw, CONTENTS.index(content), 41])
    if content == "saturated":
        a = rng.integers(0, 2, (ih, iw, 4), dtype=np.uint8) * np.uint8(255)
        a[..., 3] = rng.integers(0, 256, (ih, iw), dtype=np.uint8)
    else:
        a = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    a.setflags(write=False)
    return a


def photo(c: Case, form: str, content: str = "random") -> np.ndarray:
    """uint8 [ih, iw, C]: C = 3 (RGB), 4 (RGBX: the same RGB bytes and a random fourth byte) or 1 (L: the bytes of
    the RGB photo's second channel).  Seeded by the geometry and the content; read-only."""
    assert form in FORMS and content in CONTENTS
    a = _bytes4(c.ih, c.iw, content)
    out = np.ascontiguousarray({"RGB": a[..., :3], "RGBX": a, "L": a[..., 1:2]}[form])
    out.setflags(write=False)
    return out


def pillow_image(photo_: np.ndarray):
    """The PIL image of a photo array: mode L for one channel, else RGB of the first three bytes (an RGBX photo's
    fourth byte is not part of the image)."""
    from PIL import Image
    if photo_.shape[2] == 1:
        return Image.fromarray(np.ascontiguousarray(photo_[..., 0]))
    return Image.fromarray(np.ascontiguousarray(photo_[..., :3]))


def pillow_bytes(photo_: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """Pillow's own Image.resize((ow, oh)) + convert("RGB") of a photo, as bytes [3, oh, ow]."""
    arr = np.asarray(pillow_image(photo_).resize((ow, oh)).convert("RGB"))
    return np.ascontiguousarray(arr.transpose(2, 0, 1))


def pillow_input(photo_: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """What unet_preprocess must write, bit for bit: Pillow's bytes as float32, divided by 255, in CHW order."""
    return pillow_bytes(photo_, oh, ow).astype(np.float32) / np.float32(255.0)


# ------------------------------------------------------------------------------------------------ the pass, again
def unclipped_pass(a: np.ndarray, in_size: int, out_size: int, axis: int) -> np.ndarray:
    """One pass of Pillow's resampler along ``axis`` of an integer array, BEFORE clip8: (2^21 + sum in * w) >> 22 per
    output sample, with pr.coeffs' windows and weights.  This module's own copy of the arithmetic (one gather and
    one weighted sum per output sample), so that a test can see which sums leave 0..255."""
    bounds, kk = pr.coeffs(in_size, out_size)
    a = np.moveaxis(np.asarray(a, np.int64), axis, 0)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    for i, (lo, n) in enumerate(bounds):
        w = kk[i, :n].reshape((n,) + (1,) * (a.ndim - 1))
        out[i] = ((a[lo:lo + n] * w).sum(axis=0) + (1 << (pr.PRECISION_BITS - 1))) >> pr.PRECISION_BITS
    return np.moveaxis(out, 0, axis)


def unclipped_resize(arr: np.ndarray, oh: int, ow: int):
    """(bytes [oh, ow, C], {"h": sums before clip8 of the horizontal pass, "v": ... of the vertical pass}), the
    horizontal pass first and over all rows, each only if it runs."""
    ih, iw = arr.shape[:2]
    a, sums = np.asarray(arr, np.int64), {}
    if ow != iw:
        sums["h"] = unclipped_pass(a, iw, ow, 1)
        a = np.clip(sums["h"], 0, 255)
    if oh != ih:
        sums["v"] = unclipped_pass(a, ih, oh, 0)
        a = np.clip(sums["v"], 0, 255)
    return a.astype(np.uint8), sums


# ------------------------------------------------------------------------------------------------ the level network
LEVEL_PLANS = ("fp32", "fp16", "bf16", "mixed")
LEVEL_SETS = ((0, 63, 127, 254), (1, 128, 191, 253))       # a_k of class k, one model per set and plan
LEVEL_CLASSES = 4
LEVEL_THRESHOLDS = (0.5,) * LEVEL_CLASSES
LEVEL_MARGIN = 2.0 ** -10                                   # |T(a / 255) + b_k| of every byte a, at least
LEVEL_SIZES = [(100, 140, 64), (23, 37, 64), (64, 90, 64), (400, 600, 512)]   # (ih, iw, network size)


def level_type(plan: str):
    """The rounding of a plan's level-0 activations: the type the network input is cast to before the first conv."""
    return {"fp32": lambda a: np.asarray(a, np.float32), "fp16": en.f16_rne, "mixed": en.f16_rne,
            "bf16": en.bf16_rne}[plan]


def level_values(plan: str) -> np.ndarray:
    """float64 [256]: T(fl32(a / 255)) of every byte a -- what the pass-through network carries to the head."""
    x = np.arange(256).astype(np.float32) / np.float32(255.0)
    return level_type(plan)(x).astype(np.float64)


def level_bias(plan: str, levels) -> np.ndarray:
    """float32 [4]: b_k = -(T(a_k / 255) + T((a_k + 1) / 255)) / 2.  The midpoint of two 16-bit values is an fp32
    value (asserted on the CPU); the midpoint of two adjacent fp32 values may need a 25th bit, so for the fp32 plan
    b_k is the fp32 rounding of the midpoint and the premises are asserted on that stored value."""
    t = level_values(plan)
    return np.array([-(t[a] + t[a + 1]) / 2 for a in levels], np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def level_state_dict(plan: str, levels: tuple):
    """passthrough_state_dict(3, 4, gain 1) with class k's out_conv.bias = level_bias(plan, levels)[k]: logit k =
    T(v[k % 3] / 255) + b_k, negative up to v = a_k and positive from a_k + 1.  Shared (cached): read-only."""
    sd = {k: v for k, v in pn.passthrough_state_dict(3, LEVEL_CLASSES, gain=1.0, bias=0.0).items()}
    b = level_bias(plan, levels)
    b.setflags(write=False)
    sd["out_conv.bias"] = b
    return sd


def level_masks(v: np.ndarray, levels) -> np.ndarray:
    """The masks the level network must give on resized bytes v [3, S, S]: bool [1, 4, S, S], plane k =
    v[k % 3] > a_k."""
    return np.stack([v[k % 3] > a for k, a in enumerate(levels)])[None]


@functools.lru_cache(maxsize=None)
def level_photos(ih: int, iw: int, form: str):
    """Two photos uint8 [ih, iw, C] whose resized bytes hold every probed level and its successor (asserted on the
    CPU): per channel a ramp that overshoots 0..255 at both ends (flat saturated zones survive the filter as 0 and
    255) in another direction per channel, plus uniform noise of a few levels; the second photo runs the ramps the
    other way with other noise."""
    assert form in FORMS
    rng = np.random.default_rng([ih, iw, 43])
    yy, xx = np.mgrid[0:ih, 0:iw]
    ramps = [xx / max(iw - 1, 1), yy / max(ih - 1, 1), (xx + yy) / max(iw + ih - 2, 1)]
    out = []
    for flip in (False, True):
        chans = []
        for r in ramps:
            r = 1.0 - r if flip else r
            chans.append(np.clip(np.rint(-48 + 351 * r + rng.integers(-6, 7, (ih, iw))), 0, 255).astype(np.uint8))
        chans.append(rng.integers(0, 256, (ih, iw), dtype=np.uint8))
        a = np.stack(chans, axis=-1)
        p = np.ascontiguousarray({"RGB": a[..., :3], "RGBX": a, "L": a[..., 2:3]}[form])
        p.setflags(write=False)
        out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ crop statistics
CROP_SPACES = [(1024, 1024), (48, 80), (64, 64), (16, 16)]      # (box_h, box_w): the mask space of the boxes
CROP_PADS = (0.0, 0.15, 0.5)
CROP_PHOTOS = [(1, 1), (3, 2), (1, 700), (23, 37), (400, 600)]   # (ih, iw)
CROP_RANDOM = 40


def crop_photo(ih: int, iw: int, form: str) -> np.ndarray:
    return photo(_case(ih, iw, ih, iw, "crop statistics"), form)


@functools.lru_cache(maxsize=None)
def crop_boxes(bh: int, bw: int) -> np.ndarray:
    """int32 [46, 4] mask-space boxes (x_min, y_min, x_max, y_max) as the box kernel writes them: the empty box, the
    four corner pixels, the full frame and CROP_RANDOM seeded boxes with x_min <= x_max, y_min <= y_max."""
    rng = np.random.default_rng([bh, bw, 47])
    out = [(-1, -1, -1, -1), (0, 0, 0, 0), (bw - 1, 0, bw - 1, 0), (0, bh - 1, 0, bh - 1),
           (bw - 1, bh - 1, bw - 1, bh - 1), (0, 0, bw - 1, bh - 1)]
    for _ in range(CROP_RANDOM):
        x = np.sort(rng.integers(0, bw, 2))
        y = np.sort(rng.integers(0, bh, 2))
        out.append((x[0], y[0], x[1], y[1]))
    b = np.array(out, np.int32)
    b.setflags(write=False)
    return b


def crop_rect(box, iw: int, ih: int, bw: int, bh: int, pad: float):
    """The reference's crop lines with the mask size as a parameter: float64 true division, int() truncation, pad,
    clamp.  The four -1s for the empty box."""
    mx1, my1, mx2, my2 = (int(v) for v in box)
    if mx2 < 0:
        return (-1, -1, -1, -1)
    scale_x, scale_y = iw / bw, ih / bh
    x1, x2 = int(mx1 * scale_x), int(mx2 * scale_x)
    y1, y2 = int(my1 * scale_y), int(my2 * scale_y)
    pad_x, pad_y = int((x2 - x1) * pad), int((y2 - y1) * pad)
    return max(0, x1 - pad_x), max(0, y1 - pad_y), min(iw, x2 + pad_x), min(ih, y2 + pad_y)


def crop_sum(photo_: np.ndarray, rect) -> int:
    """numpy's sum over the RGB (or L) bytes of the rectangle; 0 for an empty or degenerate one."""
    x1, y1, x2, y2 = rect
    if x2 <= x1 or y2 <= y1:
        return 0
    return int(photo_[y1:y2, x1:x2, :3].astype(np.int64).sum())
