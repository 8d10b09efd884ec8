"""Premises of tests/test_seam_gpu.py, checked without a GPU: the routing networks of tests/seam_cases.py are exact
and lively WHERE THE TEST LOOKS -- along the tile borders and the ragged edges -- and the plain restatement of tile
coverage says what the module claims of its shapes.  (What the library's own plan gives each launch is host
arithmetic too, but a handle needs a device: that assertion, and the print of what the auto split-K plan picks at the
small-batch cases, are test_seam_gpu.test_every_launch_has_a_seam.)"""
import time

import numpy as np
import pytest

import exact_nets as en
import seam_cases as sm
import split_cases as sc
import walk_cases as wc


@pytest.mark.parametrize("case", sm.ALL_CASES, ids=str)
def test_seam_net_is_exact_and_lively_at_the_seams(case):
    """test_exact_cpu.test_routing_net_is_exact_and_lively's assertions -- the fp32 oracle equals the float64 run
    element for element, every activation is an integer and its own bf16 and fp16 rounding -- and liveliness of the
    seam set of every stored tensor (seam_cases.seam_values: within one pixel of a 16- or 32-pixel tile border or of
    the right or bottom edge): with 256 elements or more at least half nonzero and 16 distinct values, the bars that
    test sets for whole layers; at least one nonzero in a smaller set."""
    seed, c_in, n, h, w = case
    t0 = time.perf_counter()
    x, ref = en.routing_reference(seed, c_in, n, h, w)
    t1 = time.perf_counter()
    f64 = en.routing_forward_f64(en.routing_state_dict(seed, c_in), x)
    print(f"{case}: fp32 oracle {t1 - t0:.2f} s, float64 reference {time.perf_counter() - t1:.2f} s")
    assert x.min() >= 0 and x.max() <= 15 and np.array_equal(x, np.round(x))
    for k in en.FORWARD_ORDER:
        a = ref[k]
        assert np.array_equal(a.astype(np.float64), f64[k]), k
        assert np.array_equal(a, np.round(a)), k
        assert np.array_equal(en.bf16_rne(a), a) and np.array_equal(en.f16_rne(a), a), k
        s = sm.seam_values(a)
        nz, distinct = float((s != 0).mean()), len(np.unique(s))
        print(f"{case} {k} {a.shape[2]} x {a.shape[3]}: seam set {s.size} of {a.size}, {100 * nz:.0f} % nonzero, "
              f"{distinct} distinct values")
        if s.size >= 256:
            assert nz >= 0.5 and distinct >= 16, (k, s.size, nz, distinct)
        else:
            assert s.size > 0 and nz > 0, (k, s.size)


@pytest.mark.parametrize("case", sm.WIDE_CASES, ids=str)
def test_seam_net_on_wide_inputs(case):
    """The fp32 plans' runs on 23-bit inputs: oracle == float64, every value below 2^24, and the seam set of every
    stored tensor carries nonzero mid and lo terms of the three-term split."""
    seed, c_in, n, h, w = case
    x, ref = en.routing_reference(seed, c_in, n, h, w, en.WIDE_BITS)
    f64 = en.routing_forward_f64(en.routing_state_dict(seed, c_in), x)
    for k in en.FORWARD_ORDER:
        assert np.array_equal(ref[k].astype(np.float64), f64[k]), k
        assert ref[k].max() < 2.0 ** 24
        _, mid, lo = en.split3(sm.seam_values(ref[k]))
        print(f"{case} {k}: seam set mid != 0 on {int((mid != 0).sum())}, lo != 0 on {int((lo != 0).sum())} of {mid.size}")
        assert (mid != 0).any() and (lo != 0).any(), k


def test_cases_take_seeds_and_shapes_of_their_own():
    """Seeds of their own, outside en.ROUTING_*; both batch regimes; H and W multiples of 16."""
    old = en.ROUTING_SMALL + en.ROUTING_RAGGED + [en.ROUTING_FORCED] + en.ROUTING_LARGE + en.ROUTING_CLASSES
    taken = {s for s, *_ in old} | {s for s, _ in sc.NETS}
    seeds = [c[0] for c in sm.ALL_CASES]
    assert len(set(seeds)) == len(seeds) and not set(seeds) & taken
    assert not set(sm.ALL_CASES) & set(old)
    for _, c_in, n, h, w in sm.ALL_CASES:
        assert c_in in (1, 3) and h % 16 == 0 and w % 16 == 0 and n >= 1
    for group in (sm.SEAM_X16, sm.SEAM_X32, sm.SEAM_Y, sm.SEAM_CORNER):
        assert [c[2] <= sm.SMALL_BATCH_LIMIT for c in group] == [True, False], group
    assert all(c[2] <= sm.SMALL_BATCH_LIMIT for c in sm.SPLIT_CASES)
    assert sm.SEAM_MANY[0][2] > 6          # the older exact cases stop at N = 6


def test_seam_arithmetic():
    """axis_cover, seam_on_axis and never_ragged on the numbers of the module docstring."""
    assert [272 >> lv for lv in sm.LEVELS] == [272, 136, 68, 34, 17]
    assert [528 >> lv for lv in sm.LEVELS] == [528, 264, 132, 66, 33]
    assert [144 >> lv for lv in sm.LEVELS] == [144, 72, 36, 18, 9]
    assert [sm.axis_cover(272 >> lv, 16) for lv in sm.LEVELS] == [(17, 16), (9, 8), (5, 4), (3, 2), (2, 1)]
    assert [sm.axis_cover(272 >> lv, 32) for lv in sm.LEVELS] == [(9, 16), (5, 8), (3, 4), (2, 2), (1, 17)]
    assert [sm.axis_cover(528 >> lv, 32) for lv in sm.LEVELS] == [(17, 16), (9, 8), (5, 4), (3, 2), (2, 1)]
    assert [sm.axis_cover(144 >> lv, 16) for lv in sm.LEVELS] == [(9, 16), (5, 8), (3, 4), (2, 2), (1, 9)]
    assert [sm.seam_on_axis(272 >> lv, 16) for lv in sm.LEVELS] == [False, True, True, True, True]
    assert [sm.seam_on_axis(272 >> lv, 32) for lv in sm.LEVELS] == [True, True, True, True, False]
    assert all(sm.seam_on_axis(528 >> lv, 32) for lv in sm.LEVELS)
    # the gap: no older exact shape has a seam at levels 3 and 4, nor at level 2 under 32-wide tiles, nor vertically
    # below level 1 -- except 512, whose tiles are all full
    for w in (16, 64, 80, 96, 112, 512):
        assert not any(sm.seam_on_axis(w >> lv, 16) for lv in (3, 4)), w
        assert not any(sm.seam_on_axis(w >> lv, 32) for lv in (2, 3, 4)), w
    for h in (16, 32, 48, 64, 512):
        assert not any(sm.seam_on_axis(h >> lv, 16) for lv in (2, 3, 4)), h
    # a ragged tile is impossible only at level 0 under 16-pixel tiles
    assert [(lv, t) for lv in sm.LEVELS for t in (16, 32) if sm.never_ragged(lv, t)] == [(0, 16)]
    for lv in sm.LEVELS:
        for t in (16, 32):
            possible = any(sm.seam_on_axis(e >> lv, t) for e in range(16, 2049, 16))
            assert possible != sm.never_ragged(lv, t), (lv, t)
    assert sm.seam_lines(16) == [15] and sm.seam_lines(17) == [15, 16] and sm.seam_lines(34) == [15, 16, 31, 32, 33]
    assert sm.seam_mask(1, 1).all() and sm.seam_mask(16, 272).sum() == 272 + 15 * (2 * 16 + 1)


def test_tile_of_launch_knows_every_family():
    """The pixel tile of every kernel family from its label; nothing for an empty slot, the first conv and the
    pre-cast; an unknown family raises; a split label must come with ks > 1 and the reverse."""
    r8 = "conv3x3_ring8_kernel<__bf16, 8, 3, 0, 3, 0, __bf16, __bf16, 0, 0>"
    assert sm.tile_of_launch(r8) == (16, 32) and sm.tile_of_launch(r8, 1, 128) == (16, 32)
    part = "conv3x3_ring8_kernel<__bf16, 4, 3, 5, 3, 0, __bf16, __bf16, 0, 0> + splitk_reduce_kernel<__bf16, __bf16, 0>"
    assert sm.tile_of_launch(part, 4, 64) == (16, 32)
    assert sm.tile_of_launch("conv3x3_ring_kernel<__bf16, 1, 4, 4, 3, 0, 3, 0, __bf16, __bf16, 16, 16>") == (16, 16)
    assert sm.tile_of_launch("conv3x3_ring_kernel<__bf16, 1, 4, 4, 4, 0, 1, 0, __bf16, __bf16, 12, 32>") == (12, 32)
    assert sm.tile_of_launch("convT_ring_kernel<__bf16, 8, 3, 1, _Float16>", 1, 128) == (16, 16)
    assert sm.tile_of_launch("conv3x3_halo_kernel<float, 1, 4, 8, 2, 3, 0, 0>") == (16, 16)
    assert sm.tile_of_launch("conv3x3_halo_kernel<float, 1, 4, 4, 2, 1, 5, 2> + splitk_reduce_kernel<float, float, 3>", 2) == (16, 16)
    assert sm.tile_of_launch("conv3x3_x3s_kernel<1>") == (16, 16) and sm.tile_of_launch("conv3x3_x3w_kernel<2>") == (16, 32)
    for label in ("", "x_to_px4_kernel<__bf16>", "first_conv_kernel<float, 3>", "first_conv_mfma_kernel<__bf16, 1>"):
        assert sm.tile_of_launch(label) is None, label
    with pytest.raises(AssertionError, match="unknown kernel family"):
        sm.tile_of_launch("conv3x3_new_kernel<float>")
    with pytest.raises(AssertionError):
        sm.tile_of_launch(part, 1, 64)
    with pytest.raises(AssertionError):
        sm.tile_of_launch(r8, 2, 0)
    # the walkers' restatement (walk_cases.parse_label) reads the same tiles off the ring labels
    for label in list(wc.PRODUCT_LABELS.values()) + [part]:
        k = wc.parse_label(label)
        if k is not None:
            assert sm.tile_of_launch(label, 4 if " + " in label else 1) == (k.th, k.tw), label


def test_capped_walkers_cross_the_seam():
    """The product plan's walkers at (2, 16, 272) under cap 1 (walk_cases' restatement): at every level some launch
    has a walker that is handed a ragged tile by a full one and the next image's first tile by the last tile of an
    image; under cap 3 the walkers of a launch still take several tiles each at every level but the last."""
    _, _, n, h, w = sm.WALK_CASE
    assert sm.WALK_CAPS == [1, 3]
    by_level = {lv: set() for lv in sm.LEVELS}
    for slot, (k, s) in wc.product_walks(n, h, w, 1).items():
        lv = wc.GEOM[slot][2]
        wl = w >> lv               # (16 rows: below level 0 every tile is partial in y, so "full" is meant in x)
        ho = wc.handovers(n, h >> lv, wl, k.th, k.tw, 1)
        to_ragged = any((p[0][2] + 1) * k.tw <= wl < (q[0][2] + 1) * k.tw and q[0][2] == p[0][2] + 1 for p, q in ho)
        if to_ragged and s["next_image"] and s["last_partial"]:
            by_level[lv].add(slot)
    print("cap 1, launches with full -> ragged -> next image per level:", by_level)
    assert all(by_level.values()), by_level
    items = {lv: 0 for lv in sm.LEVELS}
    for slot, (k, s) in wc.product_walks(n, h, w, 3).items():
        items[wc.GEOM[slot][2]] = max(items[wc.GEOM[slot][2]], s["items"])
    print("cap 3, most items of one walker per level:", items)
    assert all(items[lv] >= 2 for lv in range(4)), items


def test_product_plan_has_a_seam_at_every_launch():
    """On the 16-bit product plan's labels (walk_cases.PRODUCT_LABELS; test_walk_gpu asserts the library reports
    them): over the whole-network cases above the small-batch limit every launch has a full tile followed by a ragged
    one in x, and in y every launch below level 0 -- the three level-0 launches, 16 high, can never have a ragged
    row of tiles and have 17 full ones.  (test_seam_gpu asserts this on the library's own labels, all five plans,
    both regimes.)"""
    labels = [""] + [wc.PRODUCT_LABELS[s] for s in range(1, sc.NUM_LAUNCHES)]
    splits = [(1, 0)] * sc.NUM_LAUNCHES
    in_x, in_y, tall = set(), set(), set()
    for _, _, n, h, w in sm.WHOLE_CASES:
        if n <= sm.SMALL_BATCH_LIMIT:
            continue
        for slot, (lv, th, tw, sy, sx) in sm.launch_seams(labels, splits, h, w).items():
            in_x |= {slot} if sx else set()
            in_y |= {slot} if sy else set()
            if sm.never_ragged(lv, th) and sm.axis_cover(h >> lv, th)[0] >= 2:
                tall.add(slot)
    issuing = {s for s in range(1, sc.NUM_LAUNCHES) if labels[s]}
    assert in_x == issuing, sorted(issuing - in_x)
    assert issuing - in_y == {1, 20, 21} == tall, (sorted(issuing - in_y), sorted(tall))
