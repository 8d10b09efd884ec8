"""The small-batch split-K plan space under test (tests/test_split_cpu.py, tests/test_split_gpu.py).

csrc/unet_capi.cpp layer_split chooses, per launch of a forward of N <= 4 images, a slice count ks in {1, 2, 4, 8, 16,
32} and -- on the 8-wave ring of the 16-bit plans -- the layer's own 128-row tiles or 64-row halves of them.  The small
test shapes never split on their own, so the tests FORCE every pair the plan could choose (UNET_MI355X_KSPLIT_FORCE,
"id:ks" on the layer's own rows, "id:ks+100" on 64-row halves) and run the bitwise routing check on each.  This module
restates which values are legal -- exactly what layer_split's own loop can emit, never more: the forced path does not
check the ring's two-chunk minimum, and a kernel run outside its premises is not a test -- and holds the one table of
forced plans, FORCED.

A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import exact_nets as en

PLANS = ["fp32", "fp32_exact", "fp16", "bf16", "mixed"]
PLANS32, PLANS16 = ("fp32", "fp32_exact"), ("fp16", "bf16", "mixed")
NUM_LAUNCHES = 22
EPI_STORE, EPI_POOL, EPI_HEAD, EPI_UPSCATTER = 0, 1, 2, 3          # csrc/unet_internal.h Epi
CHUNK = 32                                                         # the K slice granule: one 32-channel chunk

# split-plan ids (UNET_MI355X_KSPLIT_FORCE's index; csrc/unet_capi.cpp kLaunches): 0..16 the 3x3 layers down1.3 ..
# conv1.3, 17..20 the ConvTranspose layers up4..up1
CIN = [64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 1024, 512, 256, 128]
ROWS = [64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64, 2048, 1024, 512, 256]
# id -> (state_dict weight key, resolution level of the launch's input)
LAYER = OrderedDict((i, (f"{b}.net.{c}.weight", lv)) for i, (b, c, lv) in enumerate(
    [("down1", 3, 0), ("down2", 0, 1), ("down2", 3, 1), ("down3", 0, 2), ("down3", 3, 2), ("down4", 0, 3),
     ("down4", 3, 3), ("bottleneck", 0, 4), ("bottleneck", 3, 4), ("conv4", 0, 3), ("conv4", 3, 3), ("conv3", 0, 2),
     ("conv3", 3, 2), ("conv2", 0, 1), ("conv2", 3, 1), ("conv1", 0, 0), ("conv1", 3, 0)]))
LAYER.update({17: ("up4.weight", 4), 18: ("up3.weight", 3), 19: ("up2.weight", 2), 20: ("up1.weight", 1)})
# launch slot (include/unet_mi355x.h order; slot 0 is the first conv or the input pre-cast) of every id
LAUNCH_IDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 17, 9, 10, 18, 11, 12, 19, 13, 14, 20, 15, 16]
LAUNCH_OF_ID = {i: slot + 1 for slot, i in enumerate(LAUNCH_IDS)}
EPI = {i: EPI_STORE for i in range(16)}
EPI.update({0: EPI_POOL, 2: EPI_POOL, 4: EPI_POOL, 6: EPI_POOL, 16: EPI_HEAD,
            17: EPI_UPSCATTER, 18: EPI_UPSCATTER, 19: EPI_UPSCATTER, 20: EPI_UPSCATTER})
UP_LAUNCHES_16 = (10, 13, 16)   # the 16-bit ConvTranspose launches that exist (up1 runs inside conv2.3)


def eligible_ids(plan: str) -> list:
    """The ids a K split or a finer row tile may touch.  16-bit plans: the layers on the 8-wave 128-row ring with a
    plain or pooled store, down2.0 .. conv2.0 -- not the fused first conv (id 0), not conv2.3 (id 14: it carries the
    fused up1, EPI_UPFUSE), not the 64-row conv1.0, not the head, and never the ConvTranspose ring.  fp32 plans: every
    LDS-halo launch but the head, the ConvTranspose layers (ids 17-20) included."""
    return list(range(1, 14)) if plan in PLANS16 else list(range(16)) + [17, 18, 19, 20]


def legal_ks(plan: str, i: int) -> list:
    """Every ks > 1 layer_split's loop can emit for id ``i``: a power of two <= 32 that divides the layer's chunk
    count, leaving at least two chunks per slice on the 8-wave ring and one on the LDS-halo family."""
    if i not in eligible_ids(plan) or CIN[i] % CHUNK:
        return []
    nch, least = CIN[i] // CHUNK, 2 if plan in PLANS16 else 1
    return [ks for ks in (2, 4, 8, 16, 32) if nch % ks == 0 and nch // ks >= least]


def largest_legal(plan: str, i: int, t: int) -> int:
    """The largest legal slice count <= t; 1 (unsplit) when none is."""
    return max([ks for ks in legal_ks(plan, i) if ks <= t], default=1)


class Entry:
    """One forced plan: target ``t`` slices on the layers' own rows, or (``halves``) on 64-row halves of the 8-wave
    ring's 128-row tiles.  ``force[plan]``: the UNET_MI355X_KSPLIT_FORCE string that puts the largest legal value <= t
    on every eligible id -- 1 where no split is legal, so that no launch is left to the cost model.  ``want[plan]``:
    id -> (ks, rows) as unet_launch_split_at reports it (rows 0 = the layer's own tile)."""

    def __init__(self, t: int, halves: bool):
        self.t, self.halves = t, halves
        self.name = f"ks{t}_{'r64' if halves else 'own'}"
        self.force, self.want = {}, {}
        for plan in (PLANS16 if halves else PLANS):
            ks = OrderedDict((i, largest_legal(plan, i, t)) for i in eligible_ids(plan))
            self.force[plan] = ",".join(f"{i}:{k + 100 if halves else k}" for i, k in ks.items())
            self.want[plan] = {i: (k, 64 if halves else 0) for i, k in ks.items()}

    def __repr__(self):
        return self.name


def _table():
    """t in {2, 4, 8, 16, 32} on own rows in every plan and on 64-row halves in the 16-bit plans, plus the halves alone
    (t = 1: the plan's "finer row tiles, no K split").  A (plan, entry) whose string equals that of a smaller target of
    the same kind is the same run and is dropped: no ring layer has the 64 chunks that 32 slices need."""
    entries = [Entry(t, False) for t in (2, 4, 8, 16, 32)] + [Entry(t, True) for t in (1, 2, 4, 8, 16, 32)]
    runs, seen = [], set()
    for e in entries:
        for plan in e.force:
            key = (plan, e.halves, e.force[plan])
            if key not in seen:
                seen.add(key)
                runs.append((plan, e))
    return OrderedDict((e.name, e) for e in entries), runs


FORCED, FORCED_RUNS = _table()          # name -> Entry; the distinct (plan, Entry) runs
RUN_IDS = [f"{plan}-{e.name}" for plan, e in FORCED_RUNS]


def expected_splits(plan: str, entry, n: int, h: int, w: int) -> list:
    """(ks, rows) of every launch slot under ``entry`` (None: nothing is expected of the forced ids) for a forward of
    n x h x w, n <= 4: the forced value on every forced id, (1, 0) elsewhere -- except the 16-bit ConvTranspose ring,
    which no variable forces: it runs 128-row halves of its 256-row packing whenever one image's 256-row grid has
    fewer than 128 blocks (layer_split), reported as (1, 128)."""
    out = [(1, 0)] * NUM_LAUNCHES
    if plan in PLANS16:
        for i, slot in zip((17, 18, 19), UP_LAUNCHES_16):
            lv = LAYER[i][1]
            blocks = ROWS[i] // 256 * (((h >> lv) + 15) // 16) * (((w >> lv) + 15) // 16)
            out[slot] = (1, 128) if blocks < 128 else (1, 0)
    for i, v in (entry.want[plan] if entry is not None else {}).items():
        out[LAUNCH_OF_ID[i]] = v
    return out


def covered_pairs() -> dict:
    """plan -> {(launch slot, ks, rows)}: every choice other than (1, 0) that some FORCED entry forces, plus the
    16-bit ConvTranspose halves -- what tests/test_split_gpu.py verifies bitwise, and what the auto plan must stay in."""
    out = {plan: set() for plan in PLANS}
    for plan, e in FORCED_RUNS:
        out[plan] |= {(LAUNCH_OF_ID[i], ks, rows) for i, (ks, rows) in e.want[plan].items() if (ks, rows) != (1, 0)}
    for plan in PLANS16:
        out[plan] |= {(slot, 1, 128) for slot in UP_LAUNCHES_16}
    return out


# ------------------------------------------------------------------------------------------------ the networks
# (seed, c_in) of the routing networks every forced plan runs on, and the two shapes: ragged tiles at every level, and
# a 1-pixel bottleneck.  One +-1 or two per output channel is sparse: the seeds are chosen (tests/test_split_cpu.py
# asserts it) so that over the networks every (64-row group, K slice) of every forced layer holds a nonzero weight.
NETS = [(4, 3), (16, 3), (5, 1)]
SHAPES = [(3, 48, 80), (1, 16, 16)]
WIDE_NET, WIDE_SHAPE = NETS[0], SHAPES[0]   # the fp32 plans' run on 23-bit inputs (en.WIDE_BITS), once per target


def weight_rows(sd, i: int) -> np.ndarray:
    """bool [rows, cin]: output row r of id ``i`` has a nonzero weight on input channel c (any tap), with the input
    channels in the layer's input (concat) order and a ConvTranspose's 4 cout rows in the kernels' (dy, dx, cout) order."""
    w = np.asarray(sd[LAYER[i][0]]) != 0
    if i >= 17:   # [cin, cout, 2, 2] -> [(dy, dx, cout), cin]
        return w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0])
    return w.any(axis=(2, 3))


def slice_coverage(sds, i: int, ks: int) -> np.ndarray:
    """bool [rows / 64, ks]: over the state dicts ``sds``, the 64-row group and K slice hold a nonzero weight."""
    hit = np.zeros((ROWS[i] // 64, ks), bool)
    for sd in sds:
        m = weight_rows(sd, i)
        assert m.shape == (ROWS[i], CIN[i]), (i, m.shape)
        hit |= m.reshape(ROWS[i] // 64, 64, ks, CIN[i] // ks).any(axis=(1, 3))
    return hit


def nets_state_dicts():
    return [en.routing_state_dict(seed, c_in) for seed, c_in in NETS]
