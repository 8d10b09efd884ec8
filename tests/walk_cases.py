"""Persistent walkers that take several tiles each (tests/test_walk_cpu.py, tests/test_walk_gpu.py).

The ring kernels (conv3x3_ring_kernel, conv3x3_ring8_kernel, convT_ring_kernel) are persistent: every row tile of a
launch has ``slots`` walkers and walker s takes the items s, s + slots, ... -- pixel tiles in (image, tile row, tile
column) order, or (tile, K slice) pairs of a split launch with the slice fastest.  A walker carries its weight ring's
slot phase, its halo buffer parity, its input window or stationary weights and its accumulators from one item into the
next.  The launchers give every tile its own walker whenever the chip has room, which at every small test shape it has,
so the hand-over never runs there; UNET_MI355X_WALKERS=k (read by unet_create and unet_block_create) caps the walkers
and unet_launch_walk_at reports what a launch got.

This module restates the walk in plain Python -- the launcher's walker count, the item assignment and what it hands
over -- from a launch's label and its (ks, rows) alone, and holds the case lists of the GPU module.

A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.
"""
from __future__ import annotations

import math
import re

import exact_nets as en
import split_cases as sc

NUM_CUS = 256
LDS_PER_CU = 160 * 1024
ENV = "UNET_MI355X_WALKERS"
WALKER_PLANS = ["bf16", "fp16", "mixed", "fp32_exact"]   # "fp32", the three-term plan, runs no ring kernel

# ------------------------------------------------------------------------------------------------ the case lists
WHOLE_CASES = list(en.ROUTING_RAGGED) + [c for c in en.ROUTING_SMALL if c[2:] == (6, 16, 112)]
WHOLE_CAPS = [1, 2, 3, 5]
FORCED_CASE, FORCED_CAPS, FORCED_PLANS = en.ROUTING_FORCED, [1, 3], ["bf16", "fp32_exact"]
ROUNDING_CASE, ROUNDING_CAPS, ROUNDING_PLANS = en.ROUNDING_LARGER[1], [1, 3], ["bf16", "fp16", "mixed"]
ROUNDING_R12_LAYER = "down4.net.3"
SPLIT_ENTRIES = ["ks2_own", "ks4_own", "ks8_own", "ks2_r64", "ks4_r64", "ks8_r64"]   # names of split_cases.FORCED
SPLIT_SHAPE, SPLIT_PLANS = (3, 48, 80), ["bf16", "mixed"]
BLOCK_NAMES, BLOCK_CAPS, BLOCK_PLANS = ["down1", "down3", "down4", "conv1"], [1, 2], ["bf16", "fp16"]
REAL_SHAPES, REAL_CAPS = [(2, 64, 64), (3, 48, 80)], [1, 2, 3, 7]
# every (N, H, W) a capped whole-network forward runs at, for the premises of tests/test_walk_cpu.py
CAPPED_SHAPES = [((3, 48, 80), WHOLE_CAPS), ((6, 16, 112), WHOLE_CAPS), ((2, 64, 64), FORCED_CAPS)]

# launch slot (1..21) -> (Cin, GEMM rows, resolution level), from split_cases' per-id tables
GEOM = {sc.LAUNCH_OF_ID[i]: (sc.CIN[i], sc.ROWS[i], sc.LAYER[i][1]) for i in sc.LAUNCH_OF_ID}


# ------------------------------------------------------------------------------------------------ a launch's kernel
class Kernel:
    """What a launch label says about its walk: ``kind`` ring8 / ring / tring; ``rows`` x ``th`` x ``tw`` the block
    tile; ``resident`` blocks the chip holds at once; ``ns`` weight-ring slots (0: weight-stationary, no ring);
    ``spc`` ring steps per K chunk; ``su`` extra ring steps per tile (the fused up1); ``bke`` K elements per chunk;
    ``part``: a split-K partial kernel."""

    def __init__(self, kind, rows, th, tw, resident, ns, spc, su, bke, part):
        self.kind, self.rows, self.th, self.tw, self.resident = kind, rows, th, tw, resident
        self.ns, self.spc, self.su, self.bke, self.part = ns, spc, su, bke, part

    def steps(self, cin: int, ks: int = 1):
        """(ST, nch): ring steps and halo chunks of one item."""
        nch = cin // self.bke // ks
        return self.spc * nch + self.su, nch


def _ring_lds(rows, ns, tps, hs, th, tw, esize):
    """RingGeom::LDS_BYTES of the 4-wave ring (csrc/unet_kernels.hip)."""
    hp = (th + 2) * (tw + 2)
    hi = -(-hp // (16 * 3))
    halo = hp * 64 if hs else hi * 3 * 16 * 64
    params = (rows if hs else rows + 4 * 64 + 4) * 4
    return 2 * halo + ns * tps * rows * 64 + params + (20 * 20 * 4 * esize if hs else 0)


def parse_label(label: str):
    """The Kernel of a launch label (its first kernel: a split launch is "partial + reduce"); None for a launch that
    is no walker kernel or launches nothing."""
    first = label.split(" + ")[0]
    m = re.match(r"(\w+)<(.*)>$", first)
    if not m:
        return None
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    esize = 4 if args[0] == "float" else 2
    bke = 64 // esize
    if name == "conv3x3_ring8_kernel":    # <T, TCW, NS, EPI, TPS, WST, TO, TQ, HS, ABL>
        tcw, ns, epi, tps, wst = (int(a) for a in args[1:6])
        return Kernel("ring8", 16 * tcw, 16, 32, NUM_CUS, 0 if wst else ns, 9 // tps, 4 if epi == 4 else 0, bke, epi == 5)
    if name == "conv3x3_ring_kernel":     # <T, WR, WPX, TCW, NS, EPI, TPS, HS, TO, TQ, TH, TW>
        tcw, ns, epi, tps, hs = (int(a) for a in args[3:8])
        th, tw = int(args[10]), int(args[11])
        per_cu = LDS_PER_CU // _ring_lds(16 * tcw, ns, tps, hs, th, tw, esize)
        return Kernel("ring", 16 * tcw, th, tw, NUM_CUS * per_cu, ns, 9 // tps, 8 if epi == 4 else 0, bke, False)
    if name == "convT_ring_kernel":       # <T, TCW, NS, WRW, TO>
        tcw, ns, wrw = (int(a) for a in args[1:4])
        rows = 16 * tcw * wrw
        return Kernel("tring", rows, 16, 16, NUM_CUS * (LDS_PER_CU // (ns * (rows * 64 + 256 * 64))), ns, 1, 0, bke, False)
    return None


# ------------------------------------------------------------------------------------------------ the walk
def walk_of(resident: int, n_ct: int, n_mt: int, ks: int = 1, cap: int = 0):
    """(slots, items) of a launch of ``n_mt`` items on ``n_ct`` row tiles: as many walkers as the chip holds, a
    multiple of ``ks`` and at least ``ks`` (a walker keeps one K slice), at most one per item, and under a cap k at
    most max(ks, k - k % ks)."""
    n = resident // n_ct
    n = max(ks, n - n % ks)
    n = min(n, n_mt)
    if cap > 0:
        n = min(n, max(ks, cap - cap % ks))
    return (n, -(-n_mt // n)) if n > 0 else (0, 0)


def tiles(k: Kernel, n: int, h: int, w: int):
    """(tiles_y, tiles_x) of an h x w map under the kernel's pixel tile."""
    return -(-h // k.th), -(-w // k.tw)


def predict(label: str, ks: int, rows_ctot: int, n: int, h: int, w: int, cap: int = 0):
    """(slots, items) of one launch: ``label`` its label, ``ks`` its K slices, ``rows_ctot`` its GEMM rows, (n, h, w)
    its input map.  (0, 0) for a launch that is no walker."""
    k = parse_label(label)
    if k is None or n <= 0:
        return 0, 0
    ty, tx = tiles(k, n, h, w)
    return walk_of(k.resident, rows_ctot // k.rows, n * ty * tx * (ks if k.part else 1), ks if k.part else 1, cap)


def predict_all(labels, splits, n: int, h: int, w: int, cap: int = 0):
    """predict() for every launch slot of a forward of (n, h, w): ``labels`` launch_labels_at, ``splits``
    launch_split_at."""
    out = [(0, 0)]
    for slot in range(1, sc.NUM_LAUNCHES):
        _, ctot, lv = GEOM[slot]
        out.append(predict(labels[slot], splits[slot][0], ctot, n, h >> lv, w >> lv, cap))
    return out


def assignment(n_mt: int, slots: int):
    """walker -> its items, in the order it takes them: s, s + slots, ..."""
    return [list(range(s, n_mt, slots)) for s in range(slots)]


def tile_of(item: int, ks: int, ty: int, tx: int):
    """(image, tile row, tile column, K slice) of an item."""
    m, kslice = divmod(item, ks)
    m, x = divmod(m, tx)
    n, y = divmod(m, ty)
    return n, y, x, kslice


def is_partial(y: int, x: int, h: int, w: int, th: int, tw: int) -> bool:
    """The tile reaches past the map's bottom or right edge."""
    return (y + 1) * th > h or (x + 1) * tw > w


def handovers(n: int, h: int, w: int, th: int, tw: int, slots: int, ks: int = 1):
    """Every (previous tile, next tile) pair handed over inside one walker, as ((n, y, x, slice), partial?) pairs."""
    ty, tx = -(-h // th), -(-w // tw)
    out = []
    for items in assignment(n * ty * tx * ks, slots):
        t = [tile_of(i, ks, ty, tx) for i in items]
        t = [(v, is_partial(v[1], v[2], h, w, th, tw)) for v in t]
        out += list(zip(t, t[1:]))
    return out


def summary(n, h, w, th, tw, slots, ks=1):
    """What the walk of one launch exercises: the premises tests/test_walk_cpu.py asserts over the cases."""
    ty, tx = -(-h // th), -(-w // tw)
    asg = assignment(n * ty * tx * ks, slots)
    ho = handovers(n, h, w, th, tw, slots, ks)
    last = [tile_of(a[-1], ks, ty, tx) for a in asg if a]
    return {
        "items": max(len(a) for a in asg),
        "uneven": len({len(a) for a in asg}) > 1,
        "partial_to_full": any(p[1] and not q[1] for p, q in ho),
        "full_to_partial": any(not p[1] and q[1] for p, q in ho),
        "next_image": any(q[0][0] == p[0][0] + 1 and p[0][1:3] == (ty - 1, tx - 1) and q[0][1:3] == (0, 0) for p, q in ho),
        "last_partial": any(is_partial(v[1], v[2], h, w, th, tw) for v in last),
    }


def phases(k: Kernel, cin: int, ks: int, items: int):
    """(ring slot phases, halo parities) a walker of ``items`` tiles starts a tile in, and the same over any number of
    tiles: the weight ring's slot is (i * ST) mod NS at tile i, the halo buffer (i * nch) mod 2."""
    st, nch = k.steps(cin, ks)
    ns = k.ns or 1
    got = ({(i * st) % ns for i in range(items)}, {(i * nch) % 2 for i in range(items)})
    every = ({(i * st) % ns for i in range(ns)}, {(i * nch) % 2 for i in range(2)})
    return got, every


# ------------------------------------------------------------------------------------------------ the product plan
# The 16-bit plans' kernels above the small-batch limit, launch slot -> label of a bf16 forward (unet_launch_label):
# what the CPU premises are computed from.  tests/test_walk_gpu.py asserts the library still reports exactly these.
_R8 = "conv3x3_ring8_kernel<__bf16, 8, 3, {epi}, 3, 0, __bf16, __bf16, 0, 0>"
PRODUCT_LABELS = {
    1: "conv3x3_ring8_kernel<__bf16, 4, 3, 1, 3, 1, __bf16, __bf16, 1, 0>",
    2: _R8.format(epi=0), 3: _R8.format(epi=1), 4: _R8.format(epi=0), 5: _R8.format(epi=1), 6: _R8.format(epi=0),
    7: _R8.format(epi=1), 8: _R8.format(epi=0), 9: _R8.format(epi=0),
    10: "convT_ring_kernel<__bf16, 8, 4, 2, __bf16>",
    11: _R8.format(epi=0), 12: _R8.format(epi=0),
    13: "convT_ring_kernel<__bf16, 8, 4, 2, __bf16>",
    14: _R8.format(epi=0), 15: _R8.format(epi=0),
    16: "convT_ring_kernel<__bf16, 8, 4, 2, __bf16>",
    17: _R8.format(epi=0), 18: _R8.format(epi=4), 19: "",
    20: "conv3x3_ring8_kernel<__bf16, 4, 2, 0, 9, 0, __bf16, __bf16, 0, 0>",
    21: "conv3x3_ring8_kernel<__bf16, 4, 3, 2, 3, 1, __bf16, __bf16, 0, 0>",
}
LEVELS = range(5)


def product_walks(n: int, h: int, w: int, cap: int):
    """slot -> (Kernel, summary) of every walker launch of the unsplit product plan at (n, h, w) under ``cap``.  A
    launch the small-batch plan splits over K or runs on finer row tiles has the same pixel tiles and at least as many
    items per walker: with ks slices the walkers number max(ks, cap - cap % ks) <= max(ks, cap), over ks times the
    items."""
    out = {}
    for slot, label in PRODUCT_LABELS.items():
        k = parse_label(label)
        if k is None:
            continue
        cin, ctot, lv = GEOM[slot]
        hl, wl = h >> lv, w >> lv
        ty, tx = tiles(k, n, hl, wl)
        slots, items = walk_of(k.resident, ctot // k.rows, n * ty * tx, 1, cap)
        s = summary(n, hl, wl, k.th, k.tw, slots)
        assert s["items"] == items
        out[slot] = (k, s)
    return out


def parent_grid(label: str, ks: int, rows_ctot: int, n: int, h: int, w: int):
    """(slots, items) by the three launchers' own formulas as they stood before the cap existed, one by one:
    launch_ring8 256 / n_ct rounded down to a multiple of ks and at least ks; launch_ring (256 x blocks per CU) /
    n_ct and at least 1; launch_tring the same with its own LDS size; each clamped to the item count."""
    k = parse_label(label)
    if k is None:
        return 0, 0
    n_ct = rows_ctot // k.rows
    ty, tx = tiles(k, n, h, w)
    if k.kind == "ring8":
        ks = ks if k.part else 1
        n_mt = n * ty * tx * ks
        n_slots = 256 // n_ct
        n_slots -= n_slots % ks
        if n_slots < ks:
            n_slots = ks
    else:
        n_mt = n * ty * tx
        n_slots = max(1, k.resident // n_ct)
    n_slots = min(n_slots, n_mt)
    return n_slots, math.ceil(n_mt / n_slots)
