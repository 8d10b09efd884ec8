"""Placed masks (tests/test_placed_cpu.py, tests/test_placed_gpu.py): a pass-through network whose masks ARE its
input bits, so that a test chooses every mask bit and the real fused head still writes it, in every plan.

  passthrough_state_dict  every weight zero but one centre tap per class in down1.0, down1.3, conv1.0 (on the
                          skip half of cat([u1, c1])) and conv1.3, and out_conv = gain * c8[k] + bias.  On an input
                          in {0, 1} every sum has one nonzero term and logit k is bias or gain + bias (-8 / +8):
                          exact in fp32, bf16 and fp16, so mask[n, k, y, x] == (x[n, k % c_in, y, x] != 0) at any
                          threshold whose cut lies inside (-8, 8)
  placed_patterns         named bool [h, w] planes: the pixels at which a box or packing kernel goes wrong
  pack_planes             patterns stacked into an input batch, every checked (n, k) plane a different pattern
  wide_patterns           rows wider than 256 column words (mask_boxes_kernel's cached-word flush)
  photo_sequence          photos of 255-blocks on 0 for the photo graph, and what survives Pillow's resize

References are exact_nets.np_boxes, numpy's packbits and sums and inference.crop_rect; nothing here is taken from
the code under test.  A helper module, not a conftest: it holds no fixtures and changes nothing about how the
suite runs.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np

import exact_nets as en

GAIN, BIAS = 16.0, -8.0
BOX_CHUNK = 1024       # csrc/unet_kernels.hip kBoxChunk: column words a block takes per loop pass
BOX_MAX_STRIPS = 64    # kBoxMaxStrips: blocks per (image, field)
BOX_THREADS = 256      # kBoxThreads


# ------------------------------------------------------------------------------------------------ the network
def _centre_taps(cout: int, cin: int, pairs) -> np.ndarray:
    w = np.zeros((cout, cin, 3, 3), np.float32)
    for o, i in pairs:
        w[o, i, 1, 1] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def passthrough_state_dict(c_in: int, n_classes: int, gain: float = GAIN, bias: float = BIAS):
    """Module docstring.  BatchNorm is exact_fold's identity (scale 1, beta 0, the fold asserted exact);
    ConvTranspose weights and biases are zero, so the up-sampled halves of every concat are zero and the deep
    levels carry nothing.  Shared (cached): read-only."""
    assert 1 <= n_classes <= 4 and c_in >= 1
    taps = {("down1", 0): [(k, k % c_in) for k in range(n_classes)],
            ("down1", 3): [(k, k) for k in range(n_classes)],
            ("conv1", 0): [(k, 64 + k) for k in range(n_classes)],   # the skip half of cat([u1, c1])
            ("conv1", 3): [(k, k) for k in range(n_classes)]}
    sd = {}
    for name, (ci, co) in en.BLOCKS.items():
        ci = c_in if name == "down1" else ci
        for idx, cin in ((0, ci), (3, co)):
            w = _centre_taps(co, cin, taps.get((name, idx), ()))
            en._put_conv_bn(sd, name, idx, en.exact_fold(w, 1.0, np.zeros(co)))
    for name, ci in (("up4", 1024), ("up3", 512), ("up2", 256), ("up1", 128)):
        sd[f"{name}.weight"] = np.zeros((ci, ci // 2, 2, 2), np.float32)
        sd[f"{name}.bias"] = np.zeros(ci // 2, np.float32)
    w = np.zeros((n_classes, 64, 1, 1), np.float32)
    w[np.arange(n_classes), np.arange(n_classes), 0, 0] = gain
    sd["out_conv.weight"] = w
    sd["out_conv.bias"] = np.full(n_classes, bias, np.float32)
    out = en._ordered(sd, c_in, n_classes)
    for v in out.values():
        v.setflags(write=False)
    return out


def placed_bits(x: np.ndarray, n_classes: int) -> np.ndarray:
    """The masks the pass-through network must give: bool [N, n_classes, H, W], plane k = channel k % c_in != 0."""
    c_in = x.shape[1]
    return np.ascontiguousarray(np.asarray(x)[:, [k % c_in for k in range(n_classes)]] != 0)


def placed_logits(x: np.ndarray, n_classes: int, gain: float = GAIN, bias: float = BIAS) -> np.ndarray:
    """The logits it must give, exactly: gain + bias where the bit is set, bias elsewhere."""
    return np.where(placed_bits(x, n_classes), np.float32(gain + bias), np.float32(bias)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the patterns
def pattern_pixels(h: int, w: int) -> "OrderedDict[str, list]":
    """name -> the (y, x) pixels of every pattern that is a handful of pixels (placed_patterns adds empty, full and
    half).  Single pixels are named px_<y>_<x>; a position that a corner already takes is not repeated."""
    out = OrderedDict()
    out["corner_tl"], out["corner_tr"] = [(0, 0)], [(0, w - 1)]
    out["corner_bl"], out["corner_br"] = [(h - 1, 0)], [(h - 1, w - 1)]
    taken = {p[0] for p in out.values()}

    def single(y, x):
        if 0 <= x < w and 0 <= y < h and (y, x) not in taken:
            taken.add((y, x))
            out[f"px_{y}_{x}"] = [(y, x)]

    # bits 15 | 16: the last bit of one 16-pixel column word and the first of the next; 31, w - 17: the last bit
    # of the second and of the last but one word; w - 16: the first bit of the last word
    for y in (0, h - 1):
        for x in (15, 16, 31, w - 17, w - 16):
            single(y, x)
    words = w // 16
    if h * words > BOX_CHUNK:   # the last word of chunk 0 (its last bit) and the first word of chunk 1 (its first)
        single((BOX_CHUNK - 1) // words, 16 * ((BOX_CHUNK - 1) % words) + 15)
        single(BOX_CHUNK // words, 16 * (BOX_CHUNK % words))
    single(h - 1, w - 8)        # the last row, inside the last word
    out["diag"] = [(0, 0), (h - 1, w - 1)]
    out["row"] = [(h // 2, 3), (h // 2, w - 4)]   # the first and the last column word (one word at w = 16)
    out["col"] = [(0, w // 2), (h - 1, w // 2)]
    return out


def placed_patterns(h: int, w: int, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """name -> bool [h, w], in a fixed order: empty, full, the pixel patterns of pattern_pixels, and half (density
    0.5 from a seeded generator: the packing and the bit order)."""
    assert h % 16 == 0 and w % 16 == 0
    out = OrderedDict()
    out["empty"] = np.zeros((h, w), bool)
    out["full"] = np.ones((h, w), bool)
    for name, pix in pattern_pixels(h, w).items():
        a = np.zeros((h, w), bool)
        for y, x in pix:
            a[y, x] = True
        out[name] = a
    out["half"] = np.random.default_rng([seed, h, w, 23]).random((h, w)) < 0.5
    for v in out.values():
        v.setflags(write=False)
    return out


def promised_box(name: str, h: int, w: int):
    """The box (x_min, y_min, x_max, y_max) a pattern's NAME promises, worked out from the name alone (None for
    half, which promises none)."""
    corners = {"corner_tl": (0, 0), "corner_tr": (0, w - 1), "corner_bl": (h - 1, 0), "corner_br": (h - 1, w - 1)}
    if name == "empty":
        return (-1, -1, -1, -1)
    if name in ("full", "diag"):
        return (0, 0, w - 1, h - 1)
    if name in corners:
        y, x = corners[name]
        return (x, y, x, y)
    if name.startswith("px_"):
        y, x = (int(v) for v in name.split("_")[1:])
        return (x, y, x, y)
    if name == "row":
        return (3, h // 2, w - 4, h // 2)
    if name == "col":
        return (w // 2, 0, w // 2, h - 1)
    assert name == "half", name
    return None


def pack_planes(names, h: int, w: int, n_classes: int, patterns=None):
    """(x, planes): an input fp32 [N, 3, h, w] in {0, 1} and, per image, the names of its n_classes mask planes.

    Every name takes one checked plane (n, k), k < min(n_classes, 3); the order puts ``full`` and ``empty`` in the
    middle field of images whose other fields are single pixels (a leak between the fields of one image), and after
    the named planes come three whole images full | empty | full (a leak between images, a plane-index mix-up).
    Channels that no class reads (n_classes < 3) carry decoy patterns, so that the wrong input plane shows too; with
    4 classes plane 3 repeats channel 0, as the network does."""
    pats = patterns if patterns is not None else placed_patterns(h, w)
    names = [n for n in names if n in pats]
    used = min(n_classes, 3)
    rest = [n for n in names if n not in ("full", "empty")]
    order = []
    for special in ("full", "empty"):   # [pixel, special, pixel] with three fields, [special] / [pixel, special] else
        if special in names:
            lead = [rest.pop(0)] if used >= 2 and rest else []
            tail = [rest.pop(0)] if used >= 3 and rest else []
            order += lead + [special] + tail
            while len(order) % used:
                order.append(rest.pop(0) if rest else "empty")
    order += rest
    while len(order) % used:
        order.append("empty")
    images = [order[i:i + used] for i in range(0, len(order), used)]
    images += [["full"] * used, ["empty"] * used, ["full"] * used]
    decoys = [n for n in pats if n not in ("empty",)]
    x = np.zeros((len(images), 3, h, w), np.float32)
    planes = []
    for n, img in enumerate(images):
        chans = list(img) + [decoys[(n + j) % len(decoys)] for j in range(3 - used)]
        for c, name in enumerate(chans):
            x[n, c] = pats[name]
        planes.append([chans[k % 3] for k in range(n_classes)])
    return x, planes


def wide_patterns(h: int, w: int) -> "OrderedDict[str, np.ndarray]":
    """Rows of more than 256 column words: a thread of mask_boxes_kernel then meets several column words and must
    flush the word it has been collecting whenever the word changes.  Single pixels at x = 0, 4095, 4096 and w - 1;
    pairs in words 0 and 256 of one row, in word 256 of row 0 and word 0 of row 1 (consecutive words, neighbouring
    threads), and in words i and i + 256 of the plane (the SAME thread's consecutive loads, different columns)."""
    words = w // 16
    assert words > BOX_THREADS and h >= 2
    out = OrderedDict()

    def put(name, pix):
        a = np.zeros((h, w), bool)
        for y, x in pix:
            a[y, x] = True
        a.setflags(write=False)
        out[name] = a

    for x in (0, 4095, 4096, w - 1):
        put(f"px_0_{x}", [(0, x)])
        put(f"px_{h - 1}_{x}", [(h - 1, x)])
    put("words_0_256_one_row", [(1, 5), (1, 16 * 256 + 9)])
    put("word_256_then_word_0", [(0, 16 * 256 + 15), (1, 0)])
    i = 256                                           # word i and word i + 256 of the plane: one thread, k and k + 1
    put("same_thread", [(i // words, 16 * (i % words) + 7), ((i + 256) // words, 16 * ((i + 256) % words) + 2)])
    j = 2 * BOX_CHUNK + 10                            # the same in a later chunk, both pixels inside their words
    put("same_thread_late", [(j // words, 16 * (j % words) + 1), ((j + 256) // words, 16 * ((j + 256) % words) + 14)])
    put("empty", [])
    out["full"] = np.ones((h, w), bool)
    return out


def chunk_of(y: int, x: int, w: int) -> int:
    """The chunk of BOX_CHUNK column words that pixel (y, x) of a plane of width w lies in."""
    return (y * (w // 16) + x // 16) // BOX_CHUNK


def strip_patterns(h: int, w: int) -> "OrderedDict[str, list]":
    """More chunks than blocks (h * w / 16 / BOX_CHUNK > BOX_MAX_STRIPS): name -> pixels.  One pixel only in the
    chunk that block 0 reaches on its second loop pass, one only in the last chunk of the first pass, and the two
    far corners together (first chunk of the first pass, last chunk of the second)."""
    words = w // 16
    chunks = -(-h * words // BOX_CHUNK)
    assert chunks > BOX_MAX_STRIPS
    second = BOX_MAX_STRIPS * BOX_CHUNK + 5 * words + 3          # a word of chunk 64, not on its first row
    last_first = (BOX_MAX_STRIPS - 1) * BOX_CHUNK + 2 * words + 7
    return OrderedDict([("second_pass", [(second // words, 16 * (second % words) + 6)]),
                        ("chunk_63", [(last_first // words, 16 * (last_first % words) + 11)]),
                        ("far_corners", [(0, 0), (h - 1, w - 1)])])


def pixels_plane(pix, h: int, w: int) -> np.ndarray:
    a = np.zeros((h, w), bool)
    for y, x in pix:
        a[y, x] = True
    return a


def planes_input(planes) -> np.ndarray:
    """bool planes [P, h, w] -> input fp32 [ceil(P / 3), 3, h, w], plane p = (image p // 3, channel p % 3), the
    tail empty."""
    planes = np.asarray(planes)
    p, h, w = planes.shape
    x = np.zeros((-(-p // 3) * 3, h, w), np.float32)
    x[:p] = planes
    return x.reshape(-1, 3, h, w)


# ------------------------------------------------------------------------------------------------ photos
PHOTO_SIZES = [(64, 64, 64), (100, 64, 64), (100, 140, 64), (23, 37, 64), (400, 600, 512)]   # (ih, iw, network size)
PHOTO_MODES = ("RGB", "RGBX", "L")
PHOTO_STEPS = ("all255", "top_left", "all0", "bottom_right", "interior", "all255")
NEAR_LO, NEAR_HI = 64, 192     # 16-bit plans: only resized bytes <= 64 or >= 192 are compared
NEAR_CAP = 0.02                # ... and at most this share of any photo's network pixels may lie between


def _block(ih, iw, y0, y1, x0, x1):
    a = np.zeros((ih, iw), np.uint8)
    a[max(0, y0):min(ih, y1), max(0, x0):min(iw, x1)] = 255
    return a


def photo_sequence(ih: int, iw: int, mode: str, seed: int = 0):
    """The photos of PHOTO_STEPS as uint8 [ih, iw, C] (C = 3: RGB, 4: RGBX with a random 4th byte, 1: L): blocks of
    255 on 0, a different block per channel of an RGB photo."""
    assert mode in PHOTO_MODES
    c = 1 if mode == "L" else 3
    rng = np.random.default_rng([seed, ih, iw, 31])
    out = []
    for step in PHOTO_STEPS:
        chans = []
        for k in range(c):
            bh, bw = max(2, ih // 3 + k * (ih // 16)), max(2, iw // 3 + k * (iw // 12))
            if step == "all255":
                a = np.full((ih, iw), 255, np.uint8)
            elif step == "all0":
                a = np.zeros((ih, iw), np.uint8)
            elif step == "top_left":
                a = _block(ih, iw, 0, bh, 0, bw)
            elif step == "bottom_right":
                a = _block(ih, iw, ih - bh, ih, iw - bw, iw)
            else:
                y0, x0 = ih // 4 + k * (ih // 12), iw // 5 + k * (iw // 9)
                a = _block(ih, iw, y0, y0 + bh, x0, x0 + bw)
            chans.append(a)
        if mode == "RGBX":
            chans.append(rng.integers(0, 256, (ih, iw), dtype=np.uint8))
        out.append(np.ascontiguousarray(np.stack(chans, axis=-1)))
    return out


def pillow_resized(photo: np.ndarray, size: int) -> np.ndarray:
    """What the network sees of a photo, as bytes [3, size, size]: Pillow's own resize((size, size)) of the RGB or L
    image (an RGBX photo's 4th byte is not part of the image), gray replicated (convert("RGB"))."""
    from PIL import Image
    c = photo.shape[2]
    img = Image.fromarray(photo[..., 0]) if c == 1 else Image.fromarray(np.ascontiguousarray(photo[..., :3]))
    arr = np.asarray(img.resize((size, size)).convert("RGB"))
    return np.ascontiguousarray(arr.transpose(2, 0, 1))


def photo_logits(v: np.ndarray, gain: float = GAIN, bias: float = BIAS) -> np.ndarray:
    """The fp32 plans' logits of resized bytes v: fl32(16 * fl32(v / 255) - 8), one rounding of an exact value
    (16 * x is exact), whichever way the head adds the bias."""
    x = v.astype(np.float32) / np.float32(255.0)
    return (x.astype(np.float64) * gain + bias).astype(np.float32)


def near_cut(v: np.ndarray) -> np.ndarray:
    """Resized bytes the 16-bit plans are not compared at: NEAR_LO < v < NEAR_HI.  Outside, the logit is at most
    16 * 64 / 255 - 8 = -3.98 or at least 16 * 192 / 255 - 8 = +4.05, hundreds of 16-bit ulps from any cut of
    thresholds in (0.03, 0.97)."""
    return (v > NEAR_LO) & (v < NEAR_HI)
