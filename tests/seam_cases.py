"""Ragged tiles beside full ones at every U-Net level (tests/test_seam_cpu.py, tests/test_seam_gpu.py).

H and W are multiples of 16, so the level-l map is a multiple of 16 / 2^l and the smallest remainder beside a full
16-wide tile is 8, 4, 2, 1 pixels at levels 1..4 (16, 8, 4, 2, 1 beside a 32-wide tile at levels 0..4).  The older exact
shapes (W in 16, 64, 80, 96, 112, 512; H in 16, 32, 48, 64, 512) give levels 3 and 4 -- and level 2 under 32-wide
tiles, and every level below 1 vertically -- one partial tile per tile row, or at 512 x 512 full tiles only: never a
full tile followed in the same row or column by a ragged one.  The shapes here do, at every level at once:

  W = 272: 272, 136, 68, 34, 17   full 16-wide tiles + 8, 4, 2, 1 at levels 1..4; full 32-wide + 16, 8, 4, 2 at 0..3
  W = 528: 528, 264, 132, 66, 33  full 32-wide tiles + 16, 8, 4, 2, 1 at levels 0..4
  H = 272                         the same vertically (every kernel's tile is 16 high)
  144:     144, 72, 36, 18, 9     a corner tile ragged both ways, with full neighbours on both sides, at N = 5

This module holds the case lists, the plain restatement of a launch's pixel tile from its label and (ks, rows), what
that tile covers of a map, and the seam set of a stored tensor (where the premises look for liveliness).

A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.
"""
from __future__ import annotations

import re

import numpy as np

import split_cases as sc

# ------------------------------------------------------------------------------------------------ the case lists
# (seed, c_in, n, h, w) like exact_nets.ROUTING_*, on seeds of their own (none of ROUTING_CHECKSUMS' 0..8, the class
# cases' 9..12 or split_cases.NETS' 16) and kept out of en.ROUTING_*.  Each shape at an N inside the small-batch plan
# (<= unet_small_batch_limit, 4) and at one above it.
SEAM_X16 = [(20, 3, 1, 16, 272), (21, 3, 5, 16, 272)]     # the seam in x at every level, 16-wide tiles
SEAM_X32 = [(22, 1, 2, 16, 528), (23, 1, 5, 16, 528)]     # the seam in x for 32-wide tiles down to level 4
SEAM_Y = [(24, 3, 1, 272, 16), (25, 3, 5, 272, 16)]       # the seam in y at every level
SEAM_CORNER = [(26, 3, 1, 272, 272), (27, 3, 5, 144, 144)]   # a corner tile ragged both ways, full neighbours
SEAM_MANY = [(28, 3, 37, 16, 16)]                         # many one-tile images: every item crosses an image border
WHOLE_CASES = SEAM_X16 + SEAM_X32 + SEAM_Y + SEAM_CORNER + SEAM_MANY
WIDE_CASES = list(SEAM_X16)                               # the fp32 plans on 23-bit inputs (en.WIDE_BITS)
FORCED_CASES = [(29, 3, 2, 16, 272), (30, 3, 2, 272, 16)]    # every kernel family (test_exact_gpu.FORCED)
SPLIT_CASES = [(31, 3, 1, 16, 272), (32, 3, 1, 272, 16)]     # every forced split-K plan (split_cases.FORCED_RUNS)
WALK_CASE, WALK_CAPS = FORCED_CASES[0], [1, 3]               # capped walkers (walk_cases)
ALL_CASES = WHOLE_CASES + FORCED_CASES + SPLIT_CASES
SMALL_BATCH_LIMIT = 4
LEVELS = range(5)

# launch slot (1..21) -> resolution level of the map the launch's kernel tiles (its input; include/unet_mi355x.h order)
LEVEL = {sc.LAUNCH_OF_ID[i]: sc.LAYER[i][1] for i in sc.LAUNCH_OF_ID}


# ------------------------------------------------------------------------------------------------ a launch's tile
def tile_of_launch(label: str, ks: int = 1, rows: int = 0):
    """(tile height, tile width) in pixels of the launch whose label (unet_launch_label_at) is ``label`` and whose
    split (unet_launch_split_at) is (``ks``, ``rows``); None for a slot that launches nothing (the fused up1) and for
    the first conv and the pre-cast, which are not tiled this way.  The pixel tile is the kernel family's: a K split
    runs the same tiles on ks slices ("partial + reduce": the partial kernel's) and a row tile (64-row halves of the
    8-wave ring, 128-row halves of the ConvTranspose ring) divides the GEMM rows, not the pixels.  Restated from
    csrc/unet_kernels.hip's launchers (launch_halo, launch_x3w, launch_ring, launch_ring8, launch_tring); a label of
    a family unknown here raises, so a new kernel cannot pass the coverage assertion unseen."""
    assert ks >= 1 and rows in (0, 64, 128), (ks, rows)
    if not label:
        return None
    first = label.split(" + ")[0]
    assert (ks > 1) == (" + splitk_reduce_kernel<" in label), (label, ks)
    m = re.match(r"(\w+)<(.*)>$", first)
    assert m, label
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    if name in ("first_conv_kernel", "first_conv_mfma_kernel", "x_to_px4_kernel"):
        return None
    if name == "conv3x3_ring8_kernel":      # 8 waves, 16 x 32 pixels; <T, TCW, ...>: rows = 16 TCW
        assert rows in (0, 16 * int(args[1])), (label, rows)
        return 16, 32
    if name == "conv3x3_ring_kernel":       # <T, WR, WPX, TCW, NS, EPI, TPS, HS, TO, TQ, TH, TW>
        return int(args[10]), int(args[11])
    if name == "convT_ring_kernel":         # 16 x 16 input pixels, scattered to 32 x 32
        return 16, 16
    if name in ("conv3x3_halo_kernel", "conv3x3_x3s_kernel"):
        return 16, 16
    if name == "conv3x3_x3w_kernel":        # the three-term plan's conv1.3: 16 x 32, whole 32-pixel rows for the head
        return 16, 32
    raise AssertionError(f"seam_cases.tile_of_launch: unknown kernel family in {label!r}")


def axis_cover(extent: int, tile: int):
    """(tiles, pixels of the last tile) of ``extent`` pixels under ``tile``-pixel tiles."""
    n = -(-extent // tile)
    return n, extent - (n - 1) * tile


def seam_on_axis(extent: int, tile: int) -> bool:
    """At least two tiles, the last one ragged: a full tile followed by a partial one."""
    n, last = axis_cover(extent, tile)
    return n >= 2 and last < tile


def never_ragged(level: int, tile: int) -> bool:
    """No legal input gives the launch a ragged tile on this axis: H and W are multiples of 16, the level-l extent of
    16 >> l, and the tile divides nothing finer -- level 0 under 16-pixel tiles (32 does not divide every multiple of
    16, so a 32-wide tile can be ragged there)."""
    return (16 >> level) % tile == 0


def launch_seams(labels, splits, h: int, w: int):
    """slot -> (level, tile height, tile width, seam in y, seam in x) of every slot of a forward at h x w that issues
    a tiled kernel; ``labels`` launch_labels_at, ``splits`` launch_split_at of the same (n, h, w)."""
    out = {}
    for slot in range(1, sc.NUM_LAUNCHES):
        t = tile_of_launch(labels[slot], *splits[slot])
        if t is None:
            continue
        lv = LEVEL[slot]
        out[slot] = (lv, t[0], t[1], seam_on_axis(h >> lv, t[0]), seam_on_axis(w >> lv, t[1]))
    return out


# Launches that get no seam at any shape of the module although some legal shape would give them one: (plan, regime,
# axis) -> {slot: reason}, regime "small" (N <= 4) or "large".  At most 2 slots per plan (asserted).  Empty: every
# launch that can have a ragged tile beside a full one has it here.  (Level-0 launches under 16-pixel tiles cannot, at
# any legal shape -- never_ragged, computed, not listed: for them the test asks for two tiles on the axis.)
EXCEPTIONS = {}


# ------------------------------------------------------------------------------------------------ the seam set
def seam_lines(extent: int):
    """Indices along one axis within one pixel of a 16-pixel tile border (32-pixel borders are among them) or of the
    far edge: 16 k - 1 and 16 k for every border inside the map, and extent - 1."""
    idx = {extent - 1}
    for b in range(16, extent, 16):
        idx |= {b - 1, b}
    return sorted(idx)


def seam_mask(h: int, w: int) -> np.ndarray:
    """bool [h, w]: the pixel lies in a seam row or a seam column."""
    m = np.zeros((h, w), bool)
    m[seam_lines(h), :] = True
    m[:, seam_lines(w)] = True
    return m


def seam_values(a: np.ndarray) -> np.ndarray:
    """The seam set of a stored tensor [N, C, H, W], flat."""
    return a[:, :, seam_mask(*a.shape[2:])].reshape(-1)
