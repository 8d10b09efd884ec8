"""Premises of tests/test_walk_gpu.py, asserted without a GPU on the plain restatement of tests/walk_cases.py: under
the chosen (shape, cap) pairs the walkers of the product plan really take several tiles each, at every level, with
every hand-over the kernels treat differently."""
import pytest

import walk_cases as wc


def test_item_assignment_is_a_partition():
    """Walker s of W takes s, s + W, ...: every item exactly once, counts differing by at most one, and walk_of's
    items is the largest count."""
    for n_mt in (1, 2, 3, 7, 45, 135):
        for cap in (1, 2, 3, 5, 7, 200):
            slots, items = wc.walk_of(256, 4, n_mt, 1, cap)
            asg = wc.assignment(n_mt, slots)
            assert sorted(i for a in asg for i in a) == list(range(n_mt))
            assert max(map(len, asg)) == items and max(map(len, asg)) - min(map(len, asg)) <= 1
            assert slots == min(n_mt, cap, 64)


@pytest.mark.parametrize("ks", [2, 4, 8])
def test_a_split_walker_keeps_one_slice(ks):
    """The walker count is a multiple of ks and never below it, so item % ks -- the K slice -- is the same for every
    item of a walker; cap ks gives one walker per slice, which takes every tile."""
    for n_tiles in (1, 3, 9, 18):
        for cap in (1, 2, 3, 5, 7, ks, 2 * ks, 0):
            slots, items = wc.walk_of(256, 8, n_tiles * ks, ks, cap)
            assert slots % ks == 0 and slots >= ks
            for a in wc.assignment(n_tiles * ks, slots):
                assert len({i % ks for i in a}) == 1
            if cap == ks:
                assert (slots, items) == (ks, n_tiles)
            if cap == 0:
                assert slots == min(256 // 8, n_tiles * ks) and items == -(-n_tiles * ks // slots)


def test_uncapped_walks_take_one_tile_at_the_small_shapes():
    """The gap: at every small shape of the bitwise suites the launchers give each tile its own walker."""
    for (n, h, w), _ in wc.CAPPED_SHAPES:
        for slot, (k, s) in wc.product_walks(n, h, w, 0).items():
            assert s["items"] == 1, (n, h, w, slot)


def test_capped_walks_reach_every_hand_over():
    """Over the (shape, cap) pairs of the whole-network runs: at every level a walker with at least 4 items (more than
    any ring depth, so every ring phase and halo parity a layer can start a tile in is reached -- printed per layer),
    walkers of unequal item counts in one launch, a partial tile handed to a full one and the reverse, the last tile
    of image n handed to the first of image n + 1, and a walk that ends on a partial tile."""
    deepest = {lv: 0 for lv in wc.LEVELS}
    seen = {key: set() for key in ("uneven", "partial_to_full", "full_to_partial", "next_image", "last_partial")}
    reached = {}
    for (n, h, w), caps in wc.CAPPED_SHAPES:
        for cap in caps:
            for slot, (k, s) in wc.product_walks(n, h, w, cap).items():
                cin, _, lv = wc.GEOM[slot]
                deepest[lv] = max(deepest[lv], s["items"])
                for key in seen:
                    if s[key]:
                        seen[key].add((slot, (n, h, w), cap))
                got, every = wc.phases(k, cin, 1, s["items"])
                r = reached.setdefault(slot, (set(), set(), every, k, cin))
                r[0].update(got[0])
                r[1].update(got[1])
    print("most items of one walker per level:", deepest)
    assert all(v >= 4 for v in deepest.values()), deepest
    assert max(k.ns for _, _, _, k, _ in reached.values()) <= 4   # so 4 items start a tile in every phase there is
    for key, where in seen.items():
        print(f"{key}: {len(where)} (launch, shape, cap) triples, e.g. {sorted(where)[:2]}")
        print(f"  levels: {sorted({wc.GEOM[slot][2] for slot, _, _ in where})}")
        assert where, key
    for slot, (ring, parity, every, k, cin) in sorted(reached.items()):
        st, nch = k.steps(cin)
        print(f"launch {slot:2d} {k.kind:5s} rows {k.rows:3d}: ST = {st:3d}, NS = {k.ns}, ST mod NS = {st % k.ns if k.ns else '-'}, "
              f"nch = {nch:2d}: ring phases {sorted(ring)} of {sorted(every[0])}, halo parities {sorted(parity)} of {sorted(every[1])}")
        assert ring == every[0] and parity == every[1], slot


def test_cap_one_item_counts_at_the_ragged_shape():
    """Cap 1 at (3, 48, 80): one walker takes every tile of a launch.  The maps are 48 x 80, 24 x 40, 12 x 20, 6 x 10
    and 3 x 5; the 8-wave ring's 16 x 32 tiles give 3 x (3 x 3, 2 x 2, 1 x 1, 1, 1) = 27, 12, 3, 3, 3 items and the
    16 x 16 tiles of the ConvTranspose ring and of the 4-wave ring 3 x (3 x 5, 2 x 3, 1 x 2, 1, 1) = 45, 18, 6, 3, 3."""
    walks = wc.product_walks(3, 48, 80, 1)
    by_level = {}
    for slot, (k, s) in walks.items():
        by_level.setdefault(wc.GEOM[slot][2], set()).add(s["items"])
    print("items per walker under cap 1:", by_level)
    assert by_level == {0: {27}, 1: {12}, 2: {3, 6}, 3: {3}, 4: {3}}
    ring4 = "conv3x3_ring_kernel<__bf16, 1, 4, 4, 3, 0, 3, 0, __bf16, __bf16, 16, 16>"
    assert [wc.predict(ring4, 1, 64, 3, 48 >> lv, 80 >> lv, 1) for lv in wc.LEVELS] == [(1, 45), (1, 18), (1, 6), (1, 3), (1, 3)]


def test_label_parser_knows_every_walker_kernel():
    """Geometry of the three families from their labels, and None for everything that does not walk."""
    k = wc.parse_label("conv3x3_ring8_kernel<__bf16, 4, 3, 5, 3, 0, __bf16, __bf16, 0, 0> + splitk_reduce_kernel<__bf16, __bf16, 0>")
    assert (k.kind, k.rows, k.th, k.tw, k.resident, k.part, k.ns) == ("ring8", 64, 16, 32, 256, True, 3)
    k = wc.parse_label("conv3x3_ring_kernel<__bf16, 1, 4, 8, 3, 4, 1, 0, __bf16, __bf16, 16, 16>")
    assert (k.kind, k.rows, k.resident, k.su, k.spc) == ("ring", 128, 512, 8, 9)
    k = wc.parse_label("conv3x3_ring_kernel<float, 1, 4, 4, 3, 0, 3, 0, float, float, 16, 16>")
    assert (k.rows, k.resident, k.bke, k.spc) == (64, 512, 16, 3)
    k = wc.parse_label("convT_ring_kernel<_Float16, 8, 4, 2, _Float16>")
    assert (k.kind, k.rows, k.resident, k.ns) == ("tring", 256, 256, 4)
    k = wc.parse_label("convT_ring_kernel<__bf16, 8, 3, 1, _Float16>")
    assert (k.rows, k.resident, k.ns) == (128, 512, 3)
    for label in ("", "x_to_px4_kernel<__bf16>", "conv3x3_halo_kernel<float, 1, 4, 8, 2, 3, 0, 0>", "conv3x3_x3s_kernel<0>",
                  "first_conv_mfma_kernel<__bf16, 3>"):
        assert wc.parse_label(label) is None, label
