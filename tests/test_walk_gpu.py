"""Bitwise tests of persistent walkers that take several tiles each.  Needs a GPU: run with -m gpu (premises:
tests/test_walk_cpu.py; the restatement of the walk and the case lists: tests/walk_cases.py).

The ring kernels (conv3x3_ring_kernel, conv3x3_ring8_kernel, convT_ring_kernel) carry their weight ring's phase, their
halo buffer parity, the fused first conv's input window, the stationary weights, the fused up1's extra ring steps and
the accumulator re-initialisation from one tile into the next -- but the launchers give every tile its own walker at
every small shape, so the older bitwise suites run that hand-over at 512 x 512 only.  UNET_MI355X_WALKERS=k caps the
walkers per row tile; every run here first proves through unet_launch_walk_at that each walker launch has the (slots,
items) the plain restatement predicts and that every other launch reports (0, 0), then runs an existing checker
unchanged.  Every comparison of outputs is np.array_equal.

  a. the default grids: with the variable unset the query gives the launchers' former formulas at 512 x 512, all plans;
  b. the whole network on exact operands (en.check_routing_model) under caps 1, 2, 3, 5, four plans;
  c. every forced configuration of test_exact_gpu.FORCED under caps 1 and 3, with its label assertions;
  d. the rounding network (test_rounding_gpu._check) under caps 1 and 3, one r12 case, the three 16-bit plans;
  e. split-K walkers: ks = 2, 4, 8 on own rows and 64-row halves under caps ks and 2 ks, scratch filled with 0xFF;
  f. the stand-alone blocks (test_exact_gpu._check_block) under caps 1 and 2;
  g. real weights: the capped forwards are bit for bit the uncapped one, which is within TOL of the oracle;
  h. "fp32" (the three-term plan) runs no walker kernel: the variable is inert.

Value-only mutations of the walk (no address changes, no wait or barrier removed), each applied to a scratch copy of
csrc/unet_kernels.hip and run once on an MI355X against this module and against the gap it closes --
test_exact_gpu's test_routing_minimum_sizes, test_routing_ragged and test_routing_forced_configurations (67 tests).
Every one of them passes all 67 of those and fails here (of 220):

  1. convT_ring_kernel: no init_acc_bias() after an item's epilogue
       141 failed: b. 80 of 80, c. 21, d. 12 of 12, e. 12, g. 16 of 16; f. (no ConvTranspose) passes
  2. conv3x3_ring8_kernel, streamed-weight loop: no init_acc_bias(0, TC) after an item's epilogue (kept for EPI_HEAD,
     whose fp32 instantiation would otherwise spill and fail the build's resource gate)
       172 failed: b. 80, c. 28, d. 12, e. 24 of 24, f. 12, g. 16
  3. conv3x3_ring8_kernel issue_halo: the halo buffer from (hq_c + hq_i) & 1 -- chunk and ITEM index -- where the
     chunk sequence hq_seq & 1 belongs (the same buffer on a walker's first item)
       172 failed: the runs of 2.
  4. conv3x3_ring8_kernel, fused-first-conv loop (weights stationary): no init_acc_bias(0, TC) after an item
       122 failed: b. 60 (the three 16-bit plans), c. 14, d. 12, e. 24, g. 12; "fp32_exact" has no fused first conv
  5. conv3x3_ring8_kernel compute_halo: every item's first-conv halo from input window 0, not window i & 1
       122 failed: the runs of 4.
  6. conv3x3_ring_kernel (4-wave), 64-row tiles with a store or pool epilogue: accumulators not zeroed after an item
       12 failed: c. [cfg{3,4,5}-{bf16,fp32_exact}-cap{1,3}], the only runs on that family

The module's 220 tests take 64 s on one MI355X (the slowest, g. on bf16, 1.7 s).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
import split_cases as sc
import walk_cases as wc
from test_exact_gpu import FORCED, _check_block, assert_forced_labels
from test_forward_gpu import TOL, _forward_state, make_model, rel_err
from test_rounding_gpu import _check as rounding_check
from test_split_gpu import _assert_splits
from unet_mi355x import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = en.HISTORY_FILL
_ENV = ("UNET_MI355X_KSPLIT", "UNET_MI355X_KSPLIT_FORCE", "UNET_MI355X_FUSE_UP1", "UNET_MI355X_CFG",
        "UNET_MI355X_UPCFG", "UNET_MI355X_F32X3", wc.ENV)


def _set_env(monkeypatch, cap=None, **extra):
    """A clean plan environment (unet_create reads it), then the cap and the other overrides."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    if cap is not None:
        monkeypatch.setenv(wc.ENV, str(cap))
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


# "fp32_exact" runs the LDS-halo family, which does not walk, unless a ring is forced: b. and g. run it on the 8-wave
# ring (configuration 8; its 64-channel and fp32 layers fall back to 9 within the family) and the 256-row ConvTranspose
# ring -- the fp32 instantiations of the walkers
RINGS32 = {"UNET_MI355X_CFG": ",".join(f"{i}:8" for i in range(17)), "UNET_MI355X_UPCFG": ",".join(f"{i}:7" for i in range(4))}


def _plan_env(plan):
    return RINGS32 if plan == "fp32_exact" else {}


def _handle(m):
    return m.native_handle(torch.device(DEV))


def _assert_walk(m, shape, cap, need_items=2):
    """unet_launch_walk_at against the restatement: every walker launch has the predicted (slots, items), every other
    launch (0, 0); under a cap no launch has more walkers than the cap allows and some walker takes ``need_items``
    tiles or more.  Returns the (slots, items) list."""
    h = _handle(m)
    labels, splits = h.launch_labels_at(*shape), h.launch_split_at(*shape)
    got, want = h.launch_walk_at(*shape), wc.predict_all(labels, splits, *shape, cap)
    assert got == want, (shape, cap, [(i, labels[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])
    for i, ((slots, items), label) in enumerate(zip(got, labels)):
        walker = wc.parse_label(label) is not None
        assert (slots > 0 and items > 0) == walker, (i, label, slots, items)
        if walker and cap:
            assert slots <= max(cap, splits[i][0]), (i, label, slots, cap)
    if cap and any(s for s, _ in got):
        assert max(it for _, it in got) >= need_items, (shape, cap, got)
    return got


# ------------------------------------------------------------------------------------------------ a.
@pytest.mark.parametrize("plan", sc.PLANS)
def test_default_grids_are_the_former_ones(plan, monkeypatch):
    """With the variable unset (and set to 0) unet_launch_walk_at reports, for every launch of a forward of N = 1, 2
    and 256 at 512 x 512 and at the small shapes, the walker count of the launchers' former formulas (wc.parent_grid
    restates the three of them one by one): the default launch grids are what they were."""
    for value in (None, 0):
        _set_env(monkeypatch, value)
        m = make_model(en.routing_state_dict(4, 3), 3, plan)
        try:
            h = _handle(m)
            for shape in [(1, 512, 512), (2, 512, 512), (256, 512, 512), (3, 48, 80), (6, 16, 112), (1, 16, 16)]:
                labels, splits, got = h.launch_labels_at(*shape), h.launch_split_at(*shape), h.launch_walk_at(*shape)
                n, hh, ww = shape
                want = [(0, 0)] + [wc.parent_grid(labels[s], splits[s][0], wc.GEOM[s][1], n, hh >> wc.GEOM[s][2],
                                                  ww >> wc.GEOM[s][2]) for s in range(1, sc.NUM_LAUNCHES)]
                assert got == want, (plan, shape, [(i, labels[i], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])
                assert _assert_walk(m, shape, 0) == got
            if plan == "mixed" and value is None:
                print("mixed, (2, 512, 512): (slots, items) per launch", h.launch_walk_at(2, 512, 512))
            assert h.launch_walk_at(0, 512, 512) == [(0, 0)] * sc.NUM_LAUNCHES
        finally:
            m.close()


def test_product_labels_are_the_table_of_the_premises():
    """tests/walk_cases.py PRODUCT_LABELS, from which the CPU premises are computed, is what a bf16 model runs above
    the small-batch limit."""
    m = make_model(en.routing_state_dict(4, 3), 3, "bf16")
    try:
        labels = _handle(m).launch_labels()
    finally:
        m.close()
    assert {i: s for i, s in enumerate(labels) if i > 0} == wc.PRODUCT_LABELS


def test_launch_walk_at_arguments(monkeypatch):
    """UNET_EINVAL (a ValueError) for a bad index, a negative shape and null pointers; the outputs are written."""
    _set_env(monkeypatch, 2)
    m = make_model(en.routing_state_dict(4, 3), 3, "mixed")
    try:
        h = _handle(m)
        slots, items = ctypes.c_int(-7), ctypes.c_int(-7)
        for args in ((-1, 1, 16, 16), (sc.NUM_LAUNCHES, 1, 16, 16), (3, -1, 16, 16), (3, 1, -16, 16), (3, 1, 16, -16)):
            assert h.lib.unet_launch_walk_at(h._h, *args, ctypes.byref(slots), ctypes.byref(items)) == -1, args
        assert h.lib.unet_launch_walk_at(h._h, 3, 1, 16, 16, None, ctypes.byref(items)) == -1
        assert h.lib.unet_launch_walk_at(h._h, 3, 1, 16, 16, ctypes.byref(slots), None) == -1
        assert h.lib.unet_launch_walk_at(None, 3, 1, 16, 16, ctypes.byref(slots), ctypes.byref(items)) == -1
        assert h.lib.unet_launch_walk_at(h._h, 3, 3, 48, 80, ctypes.byref(slots), ctypes.byref(items)) == 0
        assert slots.value in (1, 2) and items.value >= 6
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ b.
@pytest.mark.parametrize("cap", wc.WHOLE_CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("plan", wc.WALKER_PLANS)
@pytest.mark.parametrize("case", wc.WHOLE_CASES, ids=str)
def test_whole_network_walked(case, plan, cap, monkeypatch):
    """The routing networks under a cap: logits, every stored intermediate, u8 and packed masks and boxes bitwise, at
    N = 3, 48 x 80 (cap 1: one walker takes the 3 to 27 tiles of a launch) and N = 6, 16 x 112 ("fp32_exact": RINGS32)."""
    _set_env(monkeypatch, cap, **_plan_env(plan))
    m = make_model(en.routing_state_dict(case[0], case[1]), case[1], plan)
    try:
        walk = _assert_walk(m, case[2:], cap)
        assert sum(1 for s, _ in walk if s) >= 20, walk   # every 3x3 and ConvTranspose launch walks
        en.check_routing_model(m, case, plan, f"cap {cap}")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ c.
@pytest.mark.parametrize("cap", wc.FORCED_CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("plan", wc.FORCED_PLANS)
@pytest.mark.parametrize("var,value,tag", FORCED, ids=[f[2] for f in FORCED])
def test_forced_configurations_walked(var, value, tag, plan, cap, monkeypatch):
    """test_exact_gpu.test_routing_forced_configurations under a cap: every 3x3 ring configuration (3, 4, 5, 8-11) on
    all layers, both ConvTranspose rings with up1 as its own launch, up1 fused and not, the split-K plan off -- with
    the label assertions.  The LDS-halo configurations 0-2 are no walkers: their 3x3 launches report no walk and no
    forward runs; neither does one when no launch of the configuration walks at all ("fp32_exact" off the rings)."""
    extra = {var: value}
    if var == "UNET_MI355X_UPCFG":
        extra["UNET_MI355X_FUSE_UP1"] = "0"
    _set_env(monkeypatch, cap, **extra)
    case = wc.FORCED_CASE
    m = make_model(en.routing_state_dict(case[0], case[1]), case[1], plan)
    try:
        walk = _assert_walk(m, case[2:], cap)
        labels = _handle(m).launch_labels_at(*case[2:])
        assert_forced_labels(var, value, tag, plan, labels)
        if var == "UNET_MI355X_CFG" and int(tag[3:]) in (0, 1, 2):
            assert all(walk[sc.LAUNCH_OF_ID[i]] == (0, 0) for i in range(17)), walk
            return
        if not any(s for s, _ in walk):
            assert plan == "fp32_exact"
            return
        assert en.check_routing_model(m, case, plan, f"{tag}, cap {cap}") == labels
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ d.
@pytest.mark.parametrize("cap", wc.ROUNDING_CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("plan", wc.ROUNDING_PLANS)
@pytest.mark.parametrize("r12", [None, wc.ROUNDING_R12_LAYER], ids=["rounding", "r12"])
def test_rounding_points_walked(r12, plan, cap, monkeypatch):
    """The rounding network at N = 3, 48 x 80 (and once with 12-bit weights on down4.3): the 16-bit epilogue stores of
    the second, third, ... tile of a walker round like the first one's."""
    _set_env(monkeypatch, cap)
    rounding_check(wc.ROUNDING_CASE, plan, f"cap {cap}", r12=r12, pre=lambda m: _assert_walk(m, wc.ROUNDING_CASE[2:], cap))


# ------------------------------------------------------------------------------------------------ e.
@pytest.mark.parametrize("mult", [1, 2], ids=["cap_ks", "cap_2ks"])
@pytest.mark.parametrize("plan", wc.SPLIT_PLANS)
@pytest.mark.parametrize("name", wc.SPLIT_ENTRIES)
def test_split_walkers_keep_their_slice(name, plan, mult, monkeypatch):
    """split_cases.FORCED's ks = 2, 4, 8 on the 8-wave ring's own rows and on its 64-row halves at N = 3, 48 x 80,
    capped at the entry's slice count -- one walker per slice of the layers that take it, which then walks every tile
    on that slice -- and at twice that; the scratch (partials included) filled with 0xFF before every forward."""
    entry = sc.FORCED[name]
    cap = mult * entry.t
    _set_env(monkeypatch, cap, UNET_MI355X_KSPLIT_FORCE=entry.force[plan])
    seed, c_in = sc.NETS[0]
    m = make_model(en.routing_state_dict(seed, c_in), c_in, plan)
    try:
        shape = wc.SPLIT_SHAPE
        m.reserve(*shape)
        _assert_splits(m, plan, entry, shape)
        walk = _assert_walk(m, shape, cap, need_items=3)
        if mult == 1:   # a layer on the entry's full slice count: ks walkers, every tile on each
            full = [i for i, (ks, _) in entry.want[plan].items() if ks == entry.t]
            assert full, entry
            for i in full:
                k = wc.parse_label(_handle(m).launch_labels_at(*shape)[sc.LAUNCH_OF_ID[i]])
                lv = sc.LAYER[i][1]
                ty, tx = wc.tiles(k, shape[0], shape[1] >> lv, shape[2] >> lv)
                assert walk[sc.LAUNCH_OF_ID[i]] == (entry.t, shape[0] * ty * tx), (i, walk[sc.LAUNCH_OF_ID[i]])
        en.check_routing_model(m, (seed, c_in) + shape, plan, f"forced {entry}, cap {cap}, filled",
                               before=lambda: m.debug_fill(FILL))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ f.
@pytest.mark.parametrize("cap", wc.BLOCK_CAPS, ids=lambda c: f"cap{c}")
@pytest.mark.parametrize("plan", wc.BLOCK_PLANS)
@pytest.mark.parametrize("name", wc.BLOCK_NAMES)
def test_dense_blocks_walked(name, plan, cap, monkeypatch):
    """The stand-alone DoubleConv on dense {-1, 0, 1} weights at its ragged size, N = 2: every (cin, tap) position of
    both convs carries a weight in every tile a walker takes (unet_block_create honours the cap)."""
    _set_env(monkeypatch, cap)
    blk = en.dense_block(name)
    n, (hh, ww) = en.BLOCK_N, en.BLOCK_SIZE[name]

    def pre(dc):
        got = dc.native_block(torch.device(DEV)).launch_walk_at(n, hh, ww)
        first = blk.cin in (1, 3)
        rows = 64 if blk.cout == 64 else 128
        n_mt = n * -(-hh // 16) * -(-ww // 32)        # the 8-wave rings' 16 x 32 tiles
        want = wc.walk_of(256, blk.cout // rows, n_mt, 1, cap)
        assert got == [(0, 0) if first else want, want], (name, got, want)
        assert want[0] == min(cap, n_mt) and (want[1] >= 2 or n_mt <= cap)   # (9 x 21 is one tile per image)

    _check_block(blk, plan, f"dense, cap {cap}", pre=pre)


# ------------------------------------------------------------------------------------------------ g.
@functools.lru_cache(maxsize=None)
def _real_case(profile, shape):
    n, hh, ww = shape
    sd = syn.make_state_dict(0, 3, 3, profile)
    x = syn.invoice_pages(3, n, hh, ww, 3)
    return sd, x, en.oracle_stored(sd, x)


@pytest.mark.parametrize("plan", wc.WALKER_PLANS)
@pytest.mark.parametrize("shape", wc.REAL_SHAPES, ids=str)
@pytest.mark.parametrize("profile", ["structured", "pretrained"])
def test_real_weights_do_not_depend_on_the_walk(profile, shape, plan, monkeypatch):
    """Real-valued weights on invoice pages: which walker computes a tile must not change the tile's arithmetic.  The
    uncapped forward is within test_forward_gpu's TOL of the oracle (logits and every stored intermediate); under caps
    1, 2, 3 and 7 the logits, every stored intermediate and the packed masks are bit for bit the uncapped ones."""
    sd, x, ref = _real_case(profile, shape)
    xd = torch.from_numpy(x).to(DEV)

    def run(cap):
        _set_env(monkeypatch, cap, **_plan_env(plan))
        m = make_model(sd, 3, plan)
        try:
            walk = _assert_walk(m, shape, cap or 0)
            st = _forward_state(m, xd)
            with torch.no_grad():
                st["packed"] = m.forward_masks(xd, packed=True).clone()
            return walk, st
        finally:
            m.close()

    walk0, base = run(None)
    errs = {k: rel_err(v.cpu().numpy().reshape(ref[k].shape), ref[k]) for k, v in base.items() if k in ref}
    print(f"{plan} {profile} {shape}: rel err " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert len(errs) >= 14 and "logits" in errs, sorted(errs)
    bad = {k: v for k, v in errs.items() if not v <= TOL[plan]}
    assert not bad, (plan, bad, TOL[plan])
    assert sum(1 for s, _ in walk0 if s) >= 20, walk0
    for cap in wc.REAL_CAPS:
        _, got = run(cap)
        assert got.keys() == base.keys()
        for k, v in base.items():
            assert torch.equal(got[k], v), f"{plan} {profile} {shape}: {k} under cap {cap} differs from the uncapped forward"


# ------------------------------------------------------------------------------------------------ h.
def test_fp32_plan_has_no_walkers(monkeypatch):
    """The three-term plan runs conv3x3_halo_kernel, conv3x3_x3s_kernel and conv3x3_x3w_kernel, one tile per block:
    with the variable set every launch reports no walk, the labels are those without it, and the routing check holds."""
    def labels(cap):
        _set_env(monkeypatch, cap)
        m = make_model(en.routing_state_dict(4, 3), 3, "fp32")
        try:
            h = _handle(m)
            for shape in [(3, 48, 80), (6, 16, 112), (1, 512, 512)]:
                assert h.launch_walk_at(*shape) == [(0, 0)] * sc.NUM_LAUNCHES, shape
            if cap:
                en.check_routing_model(m, en.ROUTING_RAGGED[0], "fp32", f"cap {cap}")
            return h.launch_labels(), h.launch_labels_at(3, 48, 80), h.launch_labels_at(1, 512, 512)
        finally:
            m.close()
    assert labels(1) == labels(None)
