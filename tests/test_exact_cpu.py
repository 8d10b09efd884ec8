"""The premises of the bitwise GPU tests (tests/test_exact_gpu.py), checked on the CPU: the operands of
tests/exact_nets.py really are exact -- the BatchNorm fold, every activation of the routing networks in fp32,
bf16 and fp16, the accumulation bound and the stored intermediate of every dense block, the three-term split of
the wide-operand cases -- and the networks are lively enough to notice an error (not mostly zeros)."""
import numpy as np
import pytest

import exact_nets as en

CUTS = (-1.10, -0.41, -0.85)   # logit(0.25), logit(0.40), logit(0.30): the sigmoid cuts of the three fields


def test_batchnorm_fold_is_exact():
    """fold() (csrc/unet_capi.cpp) with running_var = float32(1 - 1e-5), gamma = 2^-k, mean 0, conv bias 0:
    the scale is within 1e-8 of gamma and float32(w * s) == w * gamma for integer |w| < 2^24, beta exact."""
    rng = np.random.default_rng(0)
    s = 1.0 / np.sqrt(np.float64(en.RUNNING_VAR) + 1e-5)
    print(f"fold scale - 1 = {s - 1:.3e}")
    assert abs(s - 1) < 1e-8
    edge = np.array([1, -1, 3, 255, 257, 65535, 2 ** 23 + 1, 2 ** 24 - 1, -(2 ** 24 - 1)])
    w = np.concatenate([edge, rng.integers(-(2 ** 24) + 1, 2 ** 24, 64 * 27 * 9 - len(edge))]).reshape(64, 27, 3, 3)
    for k in range(0, 9):
        ent = en.exact_fold(w, 2.0 ** -k, rng.integers(-4, 5, 64))   # asserts
        wf, bf = en.fold_f64(ent["weight"], ent["bias"], ent["g"], ent["beta"], ent["mean"], ent["var"])
        assert np.array_equal(wf.astype(np.float32), (w * 2.0 ** -k).astype(np.float32))
        assert np.array_equal(bf, ent["beta"].astype(np.float64))
    with pytest.raises(AssertionError):   # the helper does notice an inexact fold
        en.exact_fold(np.full((1, 1, 3, 3), 2 ** 24 + 1), 1.0, np.zeros(1))


@pytest.mark.parametrize("case", en.ROUTING_SMALL + en.ROUTING_RAGGED + [en.ROUTING_FORCED], ids=str)
def test_routing_net_is_exact_and_lively(case):
    """The fp32 oracle equals the float64 run of the intended operands element for element; every activation
    equals its own bf16 and fp16 rounding; and (above the minimum size, whose deep layers hold a handful of
    pixels) each stored layer is at least half nonzero with at least 16 distinct values, and 5 .. 95 % of
    each class's logits lie above its cut."""
    seed, c_in, n, h, w = case
    x, ref = en.routing_reference(seed, c_in, n, h, w)
    f64 = en.routing_forward_f64(en.routing_state_dict(seed, c_in), x)
    assert x.min() >= 0 and x.max() <= 15 and np.array_equal(x, np.round(x))
    for k in en.FORWARD_ORDER:
        a = ref[k]
        assert np.array_equal(a.astype(np.float64), f64[k]), k
        assert np.array_equal(a, np.round(a)), k
        assert np.array_equal(en.bf16_rne(a), a) and np.array_equal(en.f16_rne(a), a), k
        nz, distinct = float((a != 0).mean()), len(np.unique(a))
        print(f"{case} {k}: max {a.max():.0f}, {100 * nz:.0f} % nonzero, {distinct} distinct values")
        if h >= 48 and k != "logits":
            assert nz >= 0.5 and distinct >= 16, (k, nz, distinct)
    for c, cut in enumerate(CUTS):
        share = float((ref["logits"][:, c] > cut).mean())
        print(f"{case} class {c}: {100 * share:.0f} % of logits above the cut")
        assert np.abs(ref["logits"][:, c] - cut).min() >= 0.1   # integers: none near a cut
        if h >= 48:
            assert 0.05 <= share <= 0.95, (c, share)


# sha256 (synthetic.state_dict_checksum) of the default routing networks -- 3 classes, one-hot head -- of every
# (seed, c_in) the bitwise tests use, taken before routing_state_dict learnt class counts and the dense head
ROUTING_CHECKSUMS = {
    (0, 3): "2151dffba750b32561f57d1b45d79737129a05c50ca11b227b21e606ed943d9f",
    (1, 1): "6a416bae79c9693c62ac1171454d4288004e1427bf86b7704cca8f06271c186a",
    (2, 3): "c39682ecb80657071559892703bbca72aa82da97b4409d9b440cae604ad3b4b1",
    (3, 1): "7928c805f967c06a1840fe47dfc2858884fbe3012d74bb220ef75675cb7d835f",
    (4, 3): "5e9807510889fbacc35f4eb4f612fd37f466289b5d7a7377d0322ba2247569d9",
    (5, 1): "82284f4c5fabb66a8ff37aa09a66af6a8d2d4d1cfb67c74f55d1e36827794706",
    (6, 3): "1a648b81b3244c675826b56197f9cb611c9d3bb4577d9040dee010808541a393",
    (7, 3): "8c5170f49588e7943806072ef5a9f131aea6b407200d4a81dbbaa9883f1c15b7",
    (8, 3): "60f5ee963fa36a10ef20e33324398ec3c290d236a4cf674bb82237818ed9f025",
}


def test_default_routing_nets_are_unchanged():
    """The 3-class one-hot routing networks are byte for byte what they were before the class count and the
    dense head became arguments (the generator's draw order is kept), however the defaults are spelt."""
    from unet_mi355x import synthetic as syn
    used = {(s, c) for s, c, *_ in en.ROUTING_SMALL + en.ROUTING_RAGGED + [en.ROUTING_FORCED] + en.ROUTING_LARGE}
    assert used == set(ROUTING_CHECKSUMS)
    assert not used & {(s, c) for s, c, *_ in en.ROUTING_CLASSES}, "the class-count cases take seeds of their own"
    for (seed, c_in), want in ROUTING_CHECKSUMS.items():
        assert syn.state_dict_checksum(en.routing_state_dict(seed, c_in)) == want, (seed, c_in)
    assert en.routing_state_dict(8, 3, 3, "onehot") is en.routing_state_dict(8, 3)
    # the other class counts of the one-hot head: the first classes of the same draw
    sd3 = en.routing_state_dict(8, 3)
    for ncls in (1, 2, 4):
        sd = en.routing_state_dict(8, 3, ncls)
        k = min(ncls, 3)
        assert sd["out_conv.weight"].shape == (ncls, 64, 1, 1)
        assert np.array_equal(sd["out_conv.weight"][:k], sd3["out_conv.weight"][:k])
        assert np.array_equal(sd["out_conv.bias"][:k], sd3["out_conv.bias"][:k])
        assert all(np.array_equal(sd[key], sd3[key]) for key in sd3 if not key.startswith("out_conv"))


CLASS_COUNTS = [1, 2, 3, 4]
# A cut's distance to the nearest integer, for the thresholds 0.35 / 0.5 / 0.1 / 0.9 of the class-count tests:
# logit = -0.619 / 0 / -2.197 / +2.197, so 0.38 / 0 / 0.197 / 0.197.  Integer logits therefore keep 0.19 from
# every cut but that of 0.5, which the integer 0 meets exactly -- a tie that is exact on both sides: the fp32
# sigmoid of 0 is 0.5, which is not > 0.5, and 0 is not above the library's cut either (asserted below).
CUT_MARGIN = 0.19


@pytest.mark.parametrize("n_classes", CLASS_COUNTS)
@pytest.mark.parametrize("case", en.ROUTING_CLASSES, ids=str)
def test_dense_head_routing_net_premises(case, n_classes):
    """What makes the dense-head networks of tests/test_classes_gpu.py exact in every plan: out_conv in
    {-1, 0, +1} over all 64 channels (every channel in some class, rows different, both signs), an integer bias
    that puts 30 .. 70 % of the probe's logits above the class's cut; c8 integer-valued with |v| <= 256 (so the
    16-bit head's rounding of its B operand changes nothing, and +-1 is a bf16 and an fp16 value); integer
    logits below 2^24; the float64 forward equal to the fp32 oracle; and no logit near a cut of ANY class
    (CUT_MARGIN), so that the masks -- also those a kernel would cut at a neighbour's slot -- do not hang on
    a rounding: the library's ``logit > unet_logit_cut(thr)`` and the oracle's fp32 sigmoid > thr agree."""
    import torch
    from unet_mi355x import native
    seed, c_in, n, h, w = case
    thr = en.CLASS_THRESHOLDS[:n_classes]
    sd = en.routing_state_dict(seed, c_in, n_classes, "dense", thr)
    hw = sd["out_conv.weight"].reshape(n_classes, 64)
    assert set(np.unique(hw)) <= {-1.0, 0.0, 1.0} and (hw != 0).any(axis=0).all()
    assert all((r > 0).any() and (r < 0).any() for r in hw)
    assert len({r.tobytes() for r in hw}) == n_classes
    assert np.array_equal(sd["out_conv.bias"], np.round(sd["out_conv.bias"]))
    probe = en.routing_forward_f64(sd, en.routing_input(seed, 1, c_in, 32, 32))["logits"]
    for c in range(n_classes):
        share = float((probe[:, c] > en.logit_cut64(thr[c])).mean())
        assert 0.3 <= share <= 0.7, (c, share)
    x, ref = en.routing_reference(seed, c_in, n, h, w, n_classes=n_classes, head="dense", thresholds=thr)
    f64 = en.routing_forward_f64(sd, x)
    for k in en.FORWARD_ORDER:
        assert np.array_equal(ref[k].astype(np.float64), f64[k]), k
        assert np.array_equal(en.bf16_rne(ref[k]), ref[k]) or k == "logits", k
    c8 = f64["c8"]
    assert np.array_equal(c8, np.round(c8)) and np.abs(c8).max() <= 256
    assert np.array_equal(en.bf16_rne(c8.astype(np.float32)), c8) and np.array_equal(en.f16_rne(c8.astype(np.float32)), c8)
    logits = ref["logits"]
    assert np.array_equal(logits, np.round(logits)) and np.abs(logits).max() < 2.0 ** 24
    lib = native.load_library()
    masks = en.reference_masks(logits, thr)
    for c in range(n_classes):
        share = float(masks[:, c].mean())
        print(f"{case} {n_classes} classes, class {c}: bias {sd['out_conv.bias'][c]:.0f}, logits in "
              f"[{logits[:, c].min():.0f}, {logits[:, c].max():.0f}], {100 * share:.0f} % above the cut")
        if h >= 48:
            assert 0.05 <= share <= 0.95, (c, share)
        for t in thr:   # every class's cut: a logit compared against the wrong slot is decided as firmly
            d = np.abs(logits[:, c].astype(np.float64) - en.logit_cut64(t))
            tie = (logits[:, c] == 0) & (t == 0.5)
            assert d[~tie].min() >= CUT_MARGIN, (c, t, float(d[~tie].min()))
            cut = np.float32(lib.unet_logit_cut(np.float32(t)))
            vals = np.unique(logits[:, c])
            assert np.array_equal(vals > cut, torch.sigmoid(torch.from_numpy(vals)).numpy() > np.float32(t)), (c, t)
        assert np.array_equal(masks[:, c], logits[:, c] > np.float32(lib.unet_logit_cut(np.float32(thr[c]))))


@pytest.mark.parametrize("case", en.ROUTING_WIDE, ids=str)
def test_routing_net_on_wide_inputs(case):
    """The routing networks on 23-bit inputs (the fp32 plans' whole-network run): still oracle == float64
    element for element, and every stored layer carries all three terms of the three-term split -- a nonzero
    mid and a nonzero lo term on at least a thousand of its elements (a share that falls with depth, to 3 %
    of the 7-pixel bottleneck: max-pooling pushes values towards 2^23, so more differences a - b end
    negative or small) -- against weights that are bf16 values, so the three dropped products vanish."""
    seed, c_in, n, h, w = case
    x, ref = en.routing_reference(seed, c_in, n, h, w, en.WIDE_BITS)
    sd = en.routing_state_dict(seed, c_in)
    f64 = en.routing_forward_f64(sd, x)
    assert all(np.array_equal(en.bf16_rne(v), v) for k, v in sd.items()      # exact_fold: the folded ones too
               if v.dtype == np.float32 and not k.endswith("running_var"))
    for k in en.FORWARD_ORDER:
        assert np.array_equal(ref[k].astype(np.float64), f64[k]), k
        assert ref[k].max() < 2.0 ** 24
        _, mid, lo = en.split3(ref[k])
        print(f"{case} {k}: max {ref[k].max():.0f}, mid != 0 on {100 * (mid != 0).mean():.0f} %, "
              f"lo != 0 on {100 * (lo != 0).mean():.0f} %")
        assert (mid != 0).sum() >= 1000 and (lo != 0).sum() >= 1000, k


WIDE_W_TERMS = {"b18": {(0, 0), (0, 1), (0, 2)}, "c10": {(0, 0), (0, 1), (1, 0), (1, 1)}}


@pytest.mark.parametrize("kind", list(en.WIDE_W_KINDS))
@pytest.mark.parametrize("layer", en.WIDE_W_LAYERS)
@pytest.mark.parametrize("case", en.ROUTING_WIDE, ids=str)
def test_routing_net_with_one_wide_weight_layer(case, layer, kind):
    """A routing network whose one layer carries wide weights: oracle == float64 element for element (so
    every sum is an fp32 value); at the wide layer sum |w||x| + |b| stays below 2^24, every nonzero weight
    has the terms its kind is there for, the three dropped products (mid.lo, lo.mid, lo.lo) are identically
    zero and exactly the intended kept products are nonzero: hi.hi, hi.mid, hi.lo (b18) and hi.hi, hi.mid,
    mid.hi, mid.mid (c10)."""
    seed, c_in, n, h, w = case
    bits, wbits, terms = en.WIDE_W_KINDS[kind]
    x, ref = en.routing_reference(seed, c_in, n, h, w, bits, (layer, kind))
    sd = en.routing_state_dict_wide_w(seed, c_in, layer, kind)
    f64 = en.routing_forward_f64(sd, x)
    for k in en.FORWARD_ORDER:
        assert np.array_equal(ref[k].astype(np.float64), f64[k]), k
    wv = np.abs(sd[f"{layer}.weight"][sd[f"{layer}.weight"] != 0])
    _, mid, lo = en.split3(wv)
    assert wv.min() >= 2 ** (wbits - 1) and wv.max() < 2 ** wbits and (mid != 0).all() and ((lo != 0).all() or terms < 2)
    if layer == "down4.net.3":
        import torch
        src = en._conv_relu64(torch.from_numpy(f64["p3"]), sd["down4.net.0.weight"], sd["down4.net.1.bias"]).numpy()
    else:
        src = f64[{"down4.net.0": "p3", "conv1.net.3": "c8a", "up4": "bn", "up1": "c7"}[layer]]
    worst, used, dropped = en.wide_layer_terms(sd, layer, src.astype(np.float32))
    on = {t for t, v in used.items() if v}
    out = ref[{"down4.net.0": "c4", "down4.net.3": "c4", "conv1.net.3": "logits", "up4": "u4", "up1": "u1"}[layer]]
    print(f"{case} {layer} {kind}: input max {src.max():.0f}, sum |w||x| <= {worst:.4g}, output max {out.max():.4g}, "
          f"{100 * (out > 2 ** wbits).mean():.0f} % of the outputs wide; products: {sorted(TERM[t] for t in on)}")
    assert worst + 4 < 2.0 ** 24
    assert dropped == 0.0
    assert on == WIDE_W_TERMS[kind]
    assert (out > 2 ** wbits).mean() >= 0.2


def test_routing_k_coverage_over_seeds():
    """One +1 (and every second channel one -1) per output channel touches at most 1.5 cout of a layer's
    9 cin positions: the share of (cin, tap) positions carrying a nonzero weight for some output channel,
    per 3x3 layer, over the ragged shape's seeds.  The dense blocks cover every position
    (test_dense_block_premises); here only the first layers and the head's producers are covered fully."""
    every = [en.routing_state_dict(s, c) for s, c, *_ in en.ROUTING_RAGGED]
    for blk, idx in en.CONV_LAYERS:
        key = f"{blk}.net.{idx}.weight"
        sds = [sd for sd in every if sd[key].shape == every[0][key].shape]   # down1.0: the 3-channel seeds
        hit = np.zeros(sds[0][key].shape[1:], bool)
        for sd in sds:
            hit |= (sd[key] != 0).any(axis=0)
        cout = sds[0][key].shape[0]
        print(f"{key}: {100 * hit.mean():.1f} % of {hit.size} (cin, tap) positions nonzero over {len(sds)} seeds")
        # occupancy of K cells after 1.5 cout throws per seed, with a wide margin
        expect = 1 - np.exp(-1.5 * cout * len(sds) / hit.size)
        assert hit.mean() >= 0.6 * expect, key
        assert all(np.array_equal(np.abs(sd[key]).reshape(cout, -1).sum(1), 1 + (np.arange(cout) % 2)) for sd in sds)


@pytest.mark.parametrize("name", list(en.BLOCKS))
def test_dense_block_premises(name):
    """Per dense block: the fp32 accumulation of both convs is exact in any order (sum |w||x| + |b| below
    2^24 quanta), the first conv's output is a bf16 and an fp16 value (so stored or kept in registers it is
    the same number), every (cin, tap) position of both convs carries a nonzero weight, and the output is
    lively."""
    b = en.dense_block(name)
    assert b.x.min() == 0 and b.x.max() == 3
    for i in range(2):
        worst, limit = b.bound(i)
        print(f"{name} conv {i}: sum |w||x| + |b| <= {worst:.4g}, limit 2^24 qx qw = {limit:.4g} ({limit / worst:.0f}x)")
        assert worst < limit
        assert set(np.unique(b.w[i])) == {-1.0, 0.0, 1.0}
        assert (b.w[i] != 0).any(axis=0).all(), "a (cin, tap) position carries no weight"
        assert ((b.w[i] != 0).sum(axis=0) >= 4).all()
    assert en.representable(b.mid)
    for dtype in ("fp32", "bf16", "fp16"):
        e = b.expected(dtype)
        assert np.isfinite(e).all()
        print(f"{name} {dtype}: first-conv nonzero weights {100 * b.p_first:.1f} %, mid max {b.mid.max():.4g}, "
              f"out max {e.max():.4g}, {100 * (e != 0).mean():.0f} % nonzero, {len(np.unique(e))} distinct")
        assert 0.25 <= (e != 0).mean() and len(np.unique(e)) >= 64
    assert 0.25 <= (b.mid != 0).mean()


def test_mismatch_report_localises():
    """The GPU tests' failure text: tensor, count, first (n, c, y, x) with got / want, and the launch."""
    want = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    got = want.copy()
    got[1, 2, 0, 4] += 1
    got[1, 2, 3, 4] = 0
    msg = en.describe_mismatch("c3", got, want, "conv3x3_ring8_kernel<...>")
    assert msg.startswith("c3: 2 of 120 elements differ") and "(1, 2, 0, 4) got" in msg and "(1, 2, 3, 4) got" in msg
    assert msg.endswith("launch: conv3x3_ring8_kernel<...>")
    assert sorted(en.LAUNCH_OF) == sorted(en.FORWARD_ORDER)


TERM = {(0, 0): "hi.hi", (0, 1): "hi.mid", (1, 0): "mid.hi", (1, 1): "mid.mid", (0, 2): "hi.lo", (2, 0): "lo.hi"}


def test_wide_cases_split3_claim():
    """The three-term plan on the wide-operand cases (restated in numpy): the three dropped products
    (mid.lo, lo.mid, lo.lo) are identically zero, the six kept ones sum to the exact convolution, the fp32
    accumulation bound holds, and each case exercises the products it is there for -- over all cases, all
    six."""
    want = {"a": {(0, 0), (1, 0)}, "b": {(0, 0), (0, 1)}, "c": {(0, 0), (0, 1), (1, 0), (1, 1)},
            "a_lo": {(0, 0), (1, 0), (2, 0)}, "b_lo": {(0, 0), (0, 1), (0, 2)}}
    seen = set()
    for name in en.WIDE_BLOCKS:
        for case in en.WIDE_CASES:
            b = en.wide_block(name, case)
            worst, limit = b.bound(0)
            assert worst < limit == 2.0 ** 24, (name, case, worst)
            kept, used, dropped = en.six_and_dropped(b)
            assert dropped == 0.0, (name, case)
            pre = np.maximum(kept + b.beta[0].reshape(1, -1, 1, 1), 0)
            assert np.array_equal(pre, b.mid), (name, case)
            assert np.array_equal(b.out, b.mid)          # the identity second conv
            on = {t for t, v in used.items() if v}
            print(f"{name} {case}: |sum| <= {worst:.4g}; products exercised: {sorted(TERM[t] for t in on)}")
            assert on == want[case], (name, case)
            assert (b.out != 0).mean() >= 0.25
            seen |= on
    assert seen == set(TERM)
