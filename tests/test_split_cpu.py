"""Premises of the split-K plan-space tests (tests/split_cases.py, tests/test_split_gpu.py), checked without a GPU."""
import numpy as np

import exact_nets as en
import split_cases as sc


def test_forced_values_are_legal():
    """Every value FORCED puts on a layer is one the plan's own loop could emit: a power of two <= 32 dividing the
    chunk count, two chunks per slice on the ring and one on the LDS-halo family, ConvTranspose ids on the fp32 plans
    only, halves on the 16-bit plans only; and every legal (id, ks) is forced by some entry, on both row tiles."""
    forced = {plan: set() for plan in sc.PLANS}
    for plan, e in sc.FORCED_RUNS:
        assert not (e.halves and plan in sc.PLANS32)
        items = [s.split(":") for s in e.force[plan].split(",")]
        assert [int(i) for i, _ in items] == sc.eligible_ids(plan)
        for i, v in ((int(a), int(b)) for a, b in items):
            ks, rows = v % 100, 64 if v >= 100 else 0
            assert (v >= 100) == e.halves and ks <= e.t and e.want[plan][i] == (ks, rows)
            assert ks & (ks - 1) == 0 and 1 <= ks <= 32
            nch = sc.CIN[i] // sc.CHUNK
            assert sc.CIN[i] % sc.CHUNK == 0 and nch % ks == 0
            if ks > 1:
                assert nch // ks >= (2 if plan in sc.PLANS16 else 1), (plan, i, ks)
                assert ks == max(k for k in sc.legal_ks(plan, i) if k <= e.t)
            assert i < 17 or plan in sc.PLANS32
            assert sc.EPI[i] in (sc.EPI_STORE, sc.EPI_POOL, sc.EPI_UPSCATTER)
            forced[plan].add((i, ks, rows))
    for plan in sc.PLANS:
        for i in sc.eligible_ids(plan):
            for ks in sc.legal_ks(plan, i):
                for rows in ((0, 64) if plan in sc.PLANS16 else (0,)):
                    assert (i, ks, rows) in forced[plan], (plan, i, ks, rows)
            if plan in sc.PLANS16:
                assert (i, 1, 64) in forced[plan], (plan, i)
    pairs = sc.covered_pairs()
    print(f"{len(sc.FORCED)} entries, {len(sc.FORCED_RUNS)} distinct (plan, entry) runs; (launch, ks, rows) covered: "
          + ", ".join(f"{p} {len(v)}" for p, v in pairs.items()))
    assert sorted(sc.LAUNCH_OF_ID.values()) == list(range(1, sc.NUM_LAUNCHES))


def test_every_row_group_and_slice_carries_a_weight():
    """Over the networks of sc.NETS every (64-row group of output rows, K slice) of every forced layer, at every
    forced slice count, holds at least one nonzero weight (the ConvTranspose over its 4 cout rows): a slice that is
    dropped, doubled or handed to the wrong row tile changes an integer somewhere, however sparse one network is."""
    sds = sc.nets_state_dicts()
    for plan in ("fp32", "bf16"):   # the two eligibility rules: the fp32 plans share one, the 16-bit plans the other
        for i in sc.eligible_ids(plan):
            for ks in sc.legal_ks(plan, i):
                hit = sc.slice_coverage(sds, i, ks)
                per_net = [sc.slice_coverage([sd], i, ks).mean() for sd in sds]
                print(f"{plan} id {i} ({sc.LAYER[i][0]}) ks {ks}: {hit.size} (row group, slice) pairs, covered "
                      f"{100 * hit.mean():.1f} % over {len(sds)} networks (" +
                      ", ".join(f"{100 * p:.1f}" for p in per_net) + " % each)")
                assert hit.all(), (plan, i, ks, np.argwhere(~hit)[:4].tolist())


def test_wide_inputs_stay_exact():
    """The fp32 plans' run on 23-bit inputs: the oracle's fp32 forward of WIDE_NET at WIDE_SHAPE equals the float64
    forward, every value below 2^24, and activations with nonzero mid and lo terms reach the deepest layer -- so the
    three-term activation planes inside a K slice are exercised and an exact result is the only right one."""
    (seed, c_in), (n, h, w) = sc.WIDE_NET, sc.WIDE_SHAPE
    x, ref = en.routing_reference(seed, c_in, n, h, w, en.WIDE_BITS)
    f64 = en.routing_forward_f64(en.routing_state_dict(seed, c_in), x)
    for k in en.FORWARD_ORDER:
        assert np.array_equal(ref[k].astype(np.float64), f64[k]), k
        assert ref[k].max() < 2.0 ** 24
    _, mid, lo = en.split3(ref["bn"])
    print(f"bn: max {ref['bn'].max():.0f}, mid != 0 on {100 * (mid != 0).mean():.0f} %, lo != 0 on {100 * (lo != 0).mean():.0f} %")
    assert (mid != 0).sum() >= 1000 and (lo != 0).sum() >= 1000   # test_exact_cpu's bar for the wide routing runs


def test_expected_splits_restates_the_small_shapes():
    """Under a forced entry nothing is left to the cost model at the test shapes: every slot is the forced value,
    (1, 0), or the 16-bit ConvTranspose halves."""
    for plan, e in sc.FORCED_RUNS:
        for shape in sc.SHAPES + [(2, 64, 64)]:
            want = sc.expected_splits(plan, e, *shape)
            assert len(want) == sc.NUM_LAUNCHES and want[0] == (1, 0) and want[21] == (1, 0)
            assert want[19] == ((1, 0) if plan in sc.PLANS16 else (min(e.t, 4), 0))
            if plan in sc.PLANS16:
                assert [want[s] for s in sc.UP_LAUNCHES_16] == [(1, 128)] * 3
