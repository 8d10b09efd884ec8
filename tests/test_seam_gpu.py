"""Bitwise tests of ragged tiles beside full ones at every U-Net level.  Needs a GPU: run with -m gpu (premises:
tests/test_seam_cpu.py; shapes, case lists and the restatement of tile coverage: tests/seam_cases.py).

The older exact shapes give the deep levels one partial tile per tile row or (512 x 512) full tiles only; a full tile
followed in the same row or column by a ragged one -- shared halo columns, the ragged tile's staging, the `inside`
store predicate, pool anchors, the pixel-shuffle scatter, partial stores and the split-K reduce all next to live data
-- ran bitwise nowhere below level 2.  W = 272 (272, 136, 68, 34, 17), W = 528 (528, 264, 132, 66, 33), H = 272 and
144 (144, 72, 36, 18, 9) put it at every level at once.  Every comparison is en.check_routing_model's np.array_equal
on logits, every stored intermediate, u8 and packed masks and boxes, and every forward starts from a workspace filled
with 0xFF (unet_debug_fill), so a read past a ragged edge into scratch is a NaN.

  1. the whole network in all five plans at (1 | 5, 16, 272), (2 | 5, 16, 528), (1 | 5, 272, 16), (1, 272, 272),
     (5, 144, 144) and (37, 16, 16); the fp32 plans also (1 | 5, 16, 272) on 23-bit inputs;
  2. coverage asserted from the library's own labels and splits: per plan and batch regime every launch that issues a
     tiled kernel has, in some case, a full tile followed by a ragged one in x, and in y (level-0 launches under
     16-pixel tiles cannot at any legal shape: two full tiles); seam_cases.EXCEPTIONS (empty) would name the rest;
  3. every kernel family of test_exact_gpu.FORCED at (2, 16, 272) and (2, 272, 16) in bf16 and fp32_exact, with that
     module's label assertions;
  4. every forced split-K plan of split_cases.FORCED_RUNS at (1, 16, 272) and (1, 272, 16), the forced (ks, rows)
     asserted through unet_launch_split_at (no entry is refused by the launcher at these shapes);
  5. capped walkers (UNET_MI355X_WALKERS 1 and 3) at (2, 16, 272): a walker hands a full tile to a ragged one and on
     to the next image's first tile; (slots, items) asserted against walk_cases' restatement.

No defect was found in the kernels: all 200 tests pass on an MI355X, in 41 s (the slowest, 1. on fp32 at (1, 16, 272),
0.9 s).

Value-only mutations -- a halo load pointed at the zero page the kernels already read for pixels outside the image, or
a store suppressed; no address, loop bound or wait changed -- each applied to a scratch copy of csrc/unet_kernels.hip
and run once on an MI355X against the 67 older routing tests of test_exact_gpu (test_routing_minimum_sizes,
test_routing_ragged, test_routing_forced_configurations) and against this module.  "Such a tile": ragged in x (in y
for 2.) with a left (upper) neighbour.  None slips through the older tests -- (3, 48, 80) and (6, 16, 112) have such
tiles at levels 0-2 -- but they reach them in the default kernels only: the 32 forced-configuration runs at 64 x 64 pass
under every mutation, while here every forced configuration fails under 1.-3. at the shape on the mutated axis (32 of
the 64 runs of 3.), 24 fail under 4. and 16 under 5.

  1. the left halo column of such a tile zeroed (conv3x3_halo_kernel, conv3x3_x3s_kernel, conv3x3_x3w_kernel,
     conv3x3_ring_kernel, conv3x3_ring8_kernel)
       older 25 of 67 (minimum sizes 10, ragged 15); here 111 of 200: 1. 30 + 4, 3. 32 of 64, 4. 37 of 74, 5. 8 of 8
  2. the top halo row of such a tile zeroed (the same five kernels)
       older 15 (ragged); here 89: 1. 20, 3. 32, 4. 37
  3. conv_epilogue's `inside` store predicate false on such a tile
       older 22 (minimum sizes 10, ragged 12); here 101: 1. 30 + 4, 3. 32, 4. 27, 5. 8
  4. conv_epilogue's pool anchor predicate false on such a tile (the pooled map of the tile is not stored)
       older 19 (minimum sizes 10, ragged 9); here 85: 1. 24 + 2, 3. 24, 4. 27, 5. 8
  5. partial_store's predicate false on such a tile (its fp32 partials stay 0xFF)
       older 15 (ragged); here 73: 1. 15 + 2, 3. 16, 4. 34, 5. 6
"""
import numpy as np
import pytest
import torch

import exact_nets as en
import seam_cases as sm
import split_cases as sc
import walk_cases as wc
from test_exact_gpu import FORCED, assert_forced_labels
from test_forward_gpu import make_model
from test_split_gpu import _assert_splits
from test_walk_gpu import _assert_walk, _plan_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = en.HISTORY_FILL
_ENV = ("UNET_MI355X_KSPLIT", "UNET_MI355X_KSPLIT_FORCE", "UNET_MI355X_FUSE_UP1", "UNET_MI355X_CFG",
        "UNET_MI355X_UPCFG", "UNET_MI355X_F32X3", wc.ENV)


def _set_env(monkeypatch, **extra):
    """A clean plan environment (unet_create reads it), then the overrides."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _model(case, plan):
    return make_model(en.routing_state_dict(case[0], case[1]), case[1], plan)


def _handle(m):
    return m.native_handle(torch.device(DEV))


def _check_filled(m, case, plan, tag, bits=4):
    """en.check_routing_model on a workspace reserved for the case and filled with 0xFF before every forward."""
    m.reserve(*case[2:])
    return en.check_routing_model(m, case, plan, f"{tag}, filled", bits, before=lambda: m.debug_fill(FILL))


def _seams(m, shape):
    h = _handle(m)
    return sm.launch_seams(h.launch_labels_at(*shape), h.launch_split_at(*shape), *shape[1:])


# ------------------------------------------------------------------------------------------------ 1.
@pytest.mark.parametrize("plan", sc.PLANS)
@pytest.mark.parametrize("case", sm.WHOLE_CASES, ids=str)
def test_whole_network_at_the_seams(case, plan, monkeypatch):
    """The default plan of every precision plan at every shape of the module, inside the small-batch plan and above
    it.  The shape must really put a seam somewhere (37 one-tile images: none, that case is about image borders)."""
    _set_env(monkeypatch)
    m = _model(case, plan)
    try:
        seams = _seams(m, case[2:])
        assert len(seams) >= 19, sorted(seams)
        assert any(sy or sx for _, _, _, sy, sx in seams.values()) == (case not in sm.SEAM_MANY), seams
        _check_filled(m, case, plan, "seams")
    finally:
        m.close()


@pytest.mark.parametrize("plan", sc.PLANS32)
@pytest.mark.parametrize("case", sm.WIDE_CASES, ids=str)
def test_wide_inputs_at_the_seams(case, plan, monkeypatch):
    """The fp32 plans on 23-bit inputs (as test_exact_gpu.test_routing_wide_inputs_fp32_plans): the three-term plan's
    hi, mid and lo planes of a ragged tile's halo beside a full tile's."""
    _set_env(monkeypatch)
    m = _model(case, plan)
    try:
        _check_filled(m, case, plan, "seams, 23-bit inputs", en.WIDE_BITS)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 2.
@pytest.mark.parametrize("plan", sc.PLANS)
def test_every_launch_has_a_seam(plan, monkeypatch):
    """Host arithmetic on the library's own plan (unet_launch_label_at, unet_launch_split_at; a handle needs a
    device).  In both batch regimes, for every launch slot that issues a tiled kernel: some whole-network case gives it
    at least two tiles in x with a ragged last one, and some case the same in y.  Where no legal shape can (H, W
    multiples of 16: level 0 under 16-pixel tiles, seam_cases.never_ragged) some case gives it two tiles on the axis.
    Every other launch without a seam must be named in seam_cases.EXCEPTIONS, at most 2 slots per plan.  Prints the
    coverage table and what the auto split-K plan picks at the small-batch cases."""
    _set_env(monkeypatch)
    m = _model(sm.WHOLE_CASES[0], plan)
    try:
        h = _handle(m)
        assert h.small_batch_limit() == sm.SMALL_BATCH_LIMIT
        excused_all = set()
        for regime in ("small", "large"):
            cases = [c for c in sm.WHOLE_CASES if (c[2] <= sm.SMALL_BATCH_LIMIT) == (regime == "small")]
            assert len(cases) >= 3, regime
            got = {}    # slot -> {"tile": set, "x": [shapes], "y": [shapes], "x2": any, "y2": any}
            for case in cases:
                shape = case[2:]
                labels, splits = h.launch_labels_at(*shape), h.launch_split_at(*shape)
                seams = sm.launch_seams(labels, splits, *shape[1:])
                assert set(seams) == {s for s in range(1, sc.NUM_LAUNCHES) if labels[s]}, (shape, sorted(seams))
                if regime == "small":
                    picks = {s: v for s, v in enumerate(splits) if v != (1, 0)}
                    print(f"{plan} {shape}: the auto plan picks (ks, rows) per launch {picks}")
                else:
                    assert splits == [(1, 0)] * sc.NUM_LAUNCHES, (shape, splits)
                for slot, (lv, th, tw, sy, sx) in seams.items():
                    g = got.setdefault(slot, {"tile": set(), "x": [], "y": [], "x2": False, "y2": False})
                    g["tile"].add((lv, th, tw))
                    g["x"] += [shape] if sx else []
                    g["y"] += [shape] if sy else []
                    g["x2"] |= sm.axis_cover(shape[2] >> lv, tw)[0] >= 2
                    g["y2"] |= sm.axis_cover(shape[1] >> lv, th)[0] >= 2
            assert len(got) >= 19, sorted(got)     # 17 3x3 launches and 3 or 4 ConvTranspose launches, less nothing
            for axis in ("x", "y"):
                excused = sm.EXCEPTIONS.get((plan, regime, axis), {})
                excused_all |= set(excused)
                for slot, g in sorted(got.items()):
                    assert len(g["tile"]) == 1, (slot, g["tile"])      # one tile shape per launch and regime
                    lv, th, tw = next(iter(g["tile"]))
                    t = tw if axis == "x" else th
                    if sm.never_ragged(lv, t):
                        assert not g[axis] and g[axis + "2"], (plan, regime, axis, slot, g)
                    elif slot in excused:
                        assert not g[axis], f"{plan} {regime} {axis}: launch {slot} has a seam, drop it from EXCEPTIONS"
                    else:
                        assert g[axis], (f"{plan} {regime}: launch {slot} (level {lv}, {th} x {tw} tiles) has no full "
                                         f"tile followed by a ragged one in {axis} at any of {[c[2:] for c in cases]}")
                assert set(excused) <= set(got), (plan, regime, axis, excused)
            for slot, g in sorted(got.items()):
                lv, th, tw = next(iter(g["tile"]))
                print(f"{plan} {regime} launch {slot:2d} level {lv} tile {th} x {tw}: seam in x at {g['x'] or 'never (two full tiles)'}, "
                      f"in y at {g['y'] or 'never (two full tiles)'}")
        assert len(excused_all) <= 2, (plan, sorted(excused_all))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 3.
@pytest.mark.parametrize("plan", ["bf16", "fp32_exact"])
@pytest.mark.parametrize("case", sm.FORCED_CASES, ids=str)
@pytest.mark.parametrize("var,value,tag", FORCED, ids=[f[2] for f in FORCED])
def test_forced_configurations_at_the_seams(var, value, tag, case, plan, monkeypatch):
    """test_exact_gpu.test_routing_forced_configurations at N = 2, 16 x 272 and 272 x 16: the three LDS-halo
    configurations, every 3x3 ring configuration (3, 4, 5, 8-11), the three ConvTranspose configurations with up1 as its
    own launch, the split-K plan off and up1 fused and not -- with the label assertions that prove the force."""
    extra = {var: value}
    if var == "UNET_MI355X_UPCFG":
        extra["UNET_MI355X_FUSE_UP1"] = "0"
    _set_env(monkeypatch, **extra)
    m = _model(case, plan)
    try:
        seams = _seams(m, case[2:])
        axis = 4 if case[4] > case[3] else 3       # the seam in x at 16 x 272, in y at 272 x 16
        assert sum(1 for v in seams.values() if v[axis]) >= 16, (tag, seams)
        labels = _check_filled(m, case, plan, tag)
        assert_forced_labels(var, value, tag, plan, labels)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 4.
@pytest.mark.parametrize("case", sm.SPLIT_CASES, ids=str)
@pytest.mark.parametrize("plan,entry", sc.FORCED_RUNS, ids=sc.RUN_IDS)
def test_forced_split_at_the_seams(plan, entry, case, monkeypatch):
    """Every forced split-K plan at N = 1, 16 x 272 and 272 x 16: partial_store and splitk_reduce_kernel with its
    store, pool and scatter epilogues on ragged tiles beside full ones.  unet_launch_split_at must report the forced
    (ks, rows) on every forced launch (test_split_gpu._assert_splits): the launcher refuses none at these shapes."""
    _set_env(monkeypatch, UNET_MI355X_KSPLIT_FORCE=entry.force[plan])
    m = _model(case, plan)
    try:
        _assert_splits(m, plan, entry, case[2:])
        seams = _seams(m, case[2:])
        axis = 4 if case[4] > case[3] else 3
        split = [sc.LAUNCH_OF_ID[i] for i, (ks, _) in entry.want[plan].items() if ks > 1]
        assert all(s in seams for s in split)
        if entry.t > 1:    # some split launch has the seam (every one below level 0 under 16-pixel tiles)
            assert any(seams[s][axis] for s in split), (plan, entry, [seams[s] for s in split])
        _check_filled(m, case, plan, f"forced {entry}")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ 5.
@pytest.mark.parametrize("cap", sm.WALK_CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("plan", wc.WALKER_PLANS)
def test_walkers_at_the_seams(plan, cap, monkeypatch):
    """Capped walkers at N = 2, 16 x 272 (fp32_exact on forced rings, test_walk_gpu.RINGS32): under cap 1 one walker
    takes every tile of a launch -- full tiles, then the ragged one, then the next image's first tile."""
    extra = dict(_plan_env(plan))
    extra[wc.ENV] = str(cap)
    _set_env(monkeypatch, **extra)
    case = sm.WALK_CASE
    m = _model(case, plan)
    try:
        walk = _assert_walk(m, case[2:], cap)
        assert sum(1 for s, _ in walk if s) >= 20, walk
        if cap == 1:   # one walker per row tile (per K slice of a launch the small-batch plan splits): all the tiles
            labels, splits = _handle(m).launch_labels_at(*case[2:]), _handle(m).launch_split_at(*case[2:])
            for slot, (slots, items) in enumerate(walk):
                if slots and splits[slot][0] == 1:
                    k, lv = wc.parse_label(labels[slot]), sm.LEVEL[slot]
                    ty, tx = wc.tiles(k, case[2], case[3] >> lv, case[4] >> lv)
                    assert (slots, items) == (1, case[2] * ty * tx), (slot, slots, items)
        _check_filled(m, case, plan, f"cap {cap}")
    finally:
        m.close()
