"""The premises of the bitwise rounding tests (tests/test_rounding_gpu.py), checked on the CPU: the rounding
networks of tests/exact_nets.py really make every 16-bit conversion of the forward round -- a floor on the
share of elements each store changes and on its exact ties, per shape and plan, printed as a table -- while
every accumulator stays an exact fp32 value (asserted inside the reference); and the reference is sharp: with
any ONE conversion done wrongly (truncated, rounded half away, in the other 16-bit type, done twice, left out)
it differs from the true reference at that tensor and at the logits.  No kernel is altered here."""
import numpy as np
import pytest
import torch

import exact_nets as en
from oracle import unet_oracle as orc

PLANS16 = ["bf16", "fp16", "mixed"]
LARGER = en.ROUNDING_LARGER + [en.ROUNDING_FORCED]
FETCHABLE = set(en.FORWARD_ORDER)
# the shape of the negative controls: 48 x 80 at N = 3 (every store has some 200 ties there: enough for one to reach the logits)
CONTROL = en.ROUNDING_LARGER[1]
# the layers the small-batch plan may split over K (the 8-wave 128-row ring: down2.0 .. conv2.3), whose
# splitk_reduce_kernel must convert the fp32 sum once
SPLITK_STORES = ["c2a", "c2", "c3a", "c3", "c4a", "c4", "bna", "bn", "c5a", "c5", "c6a", "c6", "c7a", "c7"]
# multiples of 2^-4 (the rounding networks' logits) and of 2^-8 (r12 on out_conv) keep this far from the cuts
# logit(0.25) = -1.0986, logit(0.40) = -0.4055, logit(0.30) = -0.8473: 16 x = -17.58, -6.49, -13.56 and
# 256 x = -281.2, -103.8, -216.9, all at least 0.1 of a step from a multiple.  The fp32 sigmoid resolves 1e-4.
CUT_MARGIN = {4: 0.1 / 16, 8: 0.1 / 256}


def test_round_sig_is_the_16_bit_conversion():
    """round_sig's "rne" is RNE[dtype] (the bit-level bf16 rounding, numpy's fp16 cast) on random fp32 values
    and on every kind of tie; "trunc" and "away" differ from it exactly where they should."""
    rng = np.random.default_rng(0)
    v = (rng.integers(-2 ** 20, 2 ** 20, 200000) / 16.0).astype(np.float32)
    v = v[np.abs(v) <= en.F16_MAX]
    for t, bits in en.SIG_BITS.items():
        r = en.round_sig(v, t)
        assert np.array_equal(r, en.RNE[t](v).astype(np.float64)), t
        tie = en.is_tie(v, t)
        tr, aw = en.round_sig(v, t, "trunc"), en.round_sig(v, t, "away")
        assert np.all(np.abs(tr) <= np.abs(v)) and np.all(np.abs(aw - v) <= np.abs(tr - v))
        assert np.array_equal(aw != r, tie & (np.abs(r) < np.abs(v)))      # half away differs on ties RNE took down
        exact = r == v
        assert np.array_equal(tr == v, exact) and np.array_equal(aw == v, exact)
        assert tie.sum() >= 20 and (aw != r).sum() >= 10 and (tr != r).sum() >= 1000
        # hand-made: 1 + 2^-bits is the tie between 1 and 1 + 2^(1 - bits): RNE goes to the even 1, away to the upper
        h = np.array([1.0 + 2.0 ** -bits, 1.0 + 3 * 2.0 ** -bits, -(1.0 + 2.0 ** -bits)])
        assert en.is_tie(h, t).all()
        assert np.array_equal(en.round_sig(h, t), [1.0, 1.0 + 4 * 2.0 ** -bits, -1.0])
        assert np.array_equal(en.round_sig(h, t, "away"), [1.0 + 2 * 2.0 ** -bits, 1.0 + 4 * 2.0 ** -bits, -(1.0 + 2 * 2.0 ** -bits)])
        assert np.array_equal(en.round_sig(h, t, "trunc"), [1.0, 1.0 + 2 * 2.0 ** -bits, -1.0])


def test_rounding_state_dict_premises():
    """+-1 3x3 weights, dyadic betas with a fractional part on most channels, two +-1 weights per ConvTranspose
    (cout, dy, dx) with an integer bias, the dense head; the body's routing draws are untouched."""
    for seed, c_in in sorted({(s, c) for s, c, *_ in en.ROUNDING_MIN + LARGER}):
        sd, base = en.rounding_state_dict(seed, c_in), en.routing_state_dict(seed, c_in)
        for blk, idx in [(b, i) for b in en.BLOCKS for i in (0, 3)]:
            assert np.array_equal(sd[f"{blk}.net.{idx}.weight"], base[f"{blk}.net.{idx}.weight"])
            beta = sd[f"{blk}.net.{idx + 1}.bias"].astype(np.float64)
            assert np.array_equal(beta * 16, np.round(beta * 16)) and beta.min() >= 0 and beta.max() < 3
            assert np.array_equal(np.floor(beta), base[f"{blk}.net.{idx + 1}.bias"])
            assert (beta != np.floor(beta)).mean() >= 0.8
        for up in ("up4", "up3", "up2", "up1"):
            w, b = sd[f"{up}.weight"], sd[f"{up}.bias"]
            assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and np.all((w != 0).sum(axis=0) == 2)
            assert np.all((w == 1).sum(axis=0) >= 1) and (w == -1).any()
            assert np.array_equal(b, np.round(b)) and b.min() >= 0 and b.max() <= 2 and b.any()
        hw = sd["out_conv.weight"].reshape(3, 64)
        assert set(np.unique(hw)) <= {-1.0, 0.0, 1.0} and (hw != 0).any(axis=0).all()
        assert np.array_equal(sd["out_conv.bias"], np.round(sd["out_conv.bias"]))
    x = en.rounding_input(2, 6, 3, 16, 112)
    assert x.dtype == np.float32 and x.min() >= 0 and x.max() < 2048 and np.array_equal(x * 16, np.round(x * 16))
    assert (x != en.bf16_rne(x)).mean() > 0.9 and (x != en.f16_rne(x)).mean() > 0.8


@pytest.mark.parametrize("case", en.ROUNDING_MIN + LARGER, ids=str)
def test_fp32_plans_are_the_unrounded_chain(case):
    """In the fp32 plans nothing converts: the reference equals the fp32 oracle (PyTorch's own ops on the same
    state dict) element for element, which also says that every accumulator of the unrounded chain is an
    fp32 value whatever the order of its sum."""
    seed, c_in, n, h, w = case
    x, ref = en.rounding_reference(*case, "fp32")
    _, ref2 = en.rounding_reference(*case, "fp32_exact")
    assert all(np.array_equal(ref[k], ref2[k]) for k in ref)
    assert np.array_equal(ref["x"], x)
    sdt = {k: torch.from_numpy(np.array(v)) for k, v in en.rounding_state_dict(seed, c_in).items()}
    logits, it = orc.unet_forward(sdt, torch.from_numpy(np.array(x)), return_intermediates=True)
    assert np.array_equal(logits.numpy(), ref["logits"])
    for k in ("c1", "p1", "c2", "p2", "c3", "p3", "c4", "p4", "bn", "c7"):
        assert np.array_equal(it[k].numpy(), ref[k]), k
    with torch.no_grad():
        assert np.array_equal(orc.up(sdt, "up4", it["bn"]).numpy(), ref["u4"])
        assert np.array_equal(orc.up(sdt, "up1", it["c7"]).numpy(), ref["u1"])
    assert np.abs(ref["logits"]).max() < 2.0 ** 15


def _table(case, plan, cov):
    print(f"{case} {plan}: store type elements changed (share) ties")
    for name, (size, changed, ties) in cov.items():
        t = en.PLAN_TYPES[plan][en.STORE_LEVEL[name]]
        print(f"  {name:5s} {t} {size:8d} {changed:8d} ({100 * changed / size:5.1f} %) {ties:6d}"
              + ("" if name in FETCHABLE or name == "head" else "   (not fetchable: seen through its consumers)"))


@pytest.mark.parametrize("plan", PLANS16)
@pytest.mark.parametrize("case", en.ROUNDING_MIN + LARGER, ids=str)
def test_every_store_rounds(case, plan):
    """Per stored tensor (the network input, both outputs of every DoubleConv, every pooled map, every
    ConvTranspose output, the head's operand), counted on the fp32 values its conversion receives: at the three
    larger shapes at least MIN_CHANGED = 1 % of the elements are changed by the conversion and at least MIN_TIES =
    20 lie exactly half way between two values of the store's type; at 16 x 16 (a handful of elements around
    the 1-pixel bottleneck) at least one element of every tensor is changed and the network holds ties.  A
    condition on the generators, not a measurement: a seed that misses it is replaced, the floor stays."""
    seed, c_in, n, h, w = case
    x, ref = en.rounding_reference(*case, plan)
    cov = en.rounding_coverage(*case, plan)
    _table(case, plan, cov)
    assert list(cov) == [s for s, _ in en.ROUNDING_STORES]
    for name, (size, changed, ties) in cov.items():
        assert changed >= 1, name
        if case in LARGER:
            assert changed >= en.MIN_CHANGED * size, (name, changed, size)
            assert ties >= en.MIN_TIES, (name, ties)
    assert sum(c[2] for c in cov.values()) >= en.MIN_TIES
    for k in en.FORWARD_ORDER:
        assert ref[k].dtype == np.float32 and np.isfinite(ref[k]).all(), k
    # the stored values are values of their type
    for name, level in en.ROUNDING_STORES:
        assert np.array_equal(en.RNE[en.PLAN_TYPES[plan][level]](ref[name]), ref[name]), name
    # the head: logits are multiples of 2^-4 that keep clear of every cut and straddle their own
    lg = ref["logits"].astype(np.float64)
    assert np.array_equal(lg * 16, np.round(lg * 16)) and np.abs(lg).max() < 2.0 ** 15
    masks = en.reference_masks(ref["logits"], en.DEFAULT_THRESHOLDS[:3])
    for c in range(3):
        for t in en.DEFAULT_THRESHOLDS[:3]:
            assert np.abs(lg[:, c] - en.logit_cut64(t)).min() >= CUT_MARGIN[4], (c, t)
        assert np.array_equal(masks[:, c], lg[:, c] > en.logit_cut64(en.DEFAULT_THRESHOLDS[c]))
        share = float(masks[:, c].mean())
        print(f"  class {c}: {100 * share:.0f} % of the logits above the cut")
        if case in LARGER:
            assert 0.05 <= share <= 0.95, (c, share)


def _differs(case, plan, alter, at, true=None, **kw):
    true = true if true is not None else en.rounding_reference(*case, plan, **kw)[1]
    alt = en.rounding_reference(*case, plan, alter=alter, **kw)[1]
    out = [k for k in at if np.array_equal(alt[k], true[k])]
    return out, int((alt["logits"] != true["logits"]).sum())


@pytest.mark.parametrize("plan", PLANS16)
def test_negative_controls_one_wrong_conversion(plan):
    """The reference recomputed with ONE store truncating, or rounding half away from zero: different from the
    true reference at that tensor and at the logits, for every store of the forward."""
    for name, _ in en.ROUNDING_STORES:
        for mode in ("trunc", "away"):
            same, nlog = _differs(CONTROL, plan, ((name, mode),), [name, "logits"])
            print(f"{plan} {name} {mode}: {nlog} logits differ")
            assert not same, (name, mode, same)


def test_negative_controls_one_level_in_the_other_type():
    """One level of "mixed" stored in the other 16-bit type (a layer whose TO / TQ ignores level_dtype)."""
    true = en.rounding_reference(*CONTROL, "mixed")[1]
    for level in range(5):
        types = list(en.PLAN_TYPES["mixed"])
        types[level] = "bf16" if types[level] == "fp16" else "fp16"
        alt = en.rounding_reference(*CONTROL, tuple(types))[1]
        at = [s for s, l in en.ROUNDING_STORES if l == level] + ["logits"]
        same = [k for k in at if np.array_equal(alt[k], true[k])]
        print(f"level {level} as {types[level]}: differs at {[k for k in at if k not in same]}")
        assert not same, (level, same)
    # and a single store of it: the skip's TO, the pooled map's TQ, a ConvTranspose's output type
    for name in ("c1", "p1", "c2", "p2", "u2", "u1", "c3", "u3", "head"):
        same, _ = _differs(CONTROL, "mixed", ((name, "other"),), [name, "logits"], true)
        assert not same, (name, same)


def test_negative_controls_double_rounding_and_head():
    """A doubled rounding through bf16 at a layer the small-batch plan splits over K (a 16-bit partial), at N = 3,
    where the store's own type is fp16; the pooled map of "mixed" level 1 -> 2 taken from the rounded skip instead
    of the fp32 maximum; the head's operand, and out_conv's weights, left in fp32."""
    case = en.ROUNDING_LARGER[1]
    assert case[2] <= 4
    for plan in ("fp16", "mixed"):
        for name in SPLITK_STORES:
            if en.PLAN_TYPES[plan][en.STORE_LEVEL[name]] != "fp16":
                continue
            same, nlog = _differs(case, plan, ((name, "double"),), [name, "logits"])
            print(f"{plan} {name} twice: {nlog} logits differ")
            assert not same, (plan, name, same)
    same, nlog = _differs(case, "mixed", (("p2", "via_skip"),), ["p2", "logits"])
    print(f"mixed p2 from the rounded skip: {nlog} logits differ")
    assert not same, same
    for plan in PLANS16:
        same, nlog = _differs(case, plan, (("head", "none"),), ["head", "logits"])
        assert not same, (plan, same)
        r12 = en.R12_LAYERS[-1]
        same, nlog = _differs(case, plan, ((r12, "none"),), ["logits"], r12=r12)
        assert not same, (plan, "out_conv weights")


R12_OUT = {"down4.net.0": "c4a", "down4.net.3": "c4", "conv1.net.3": "head", "up4": "u4", "up1": "u1", "out_conv": "logits"}


@pytest.mark.parametrize("layer", en.R12_LAYERS)
@pytest.mark.parametrize("case", en.ROUNDING_R12, ids=str)
def test_r12_weight_layer_premises(case, layer):
    """One layer on r12 weights: at least R12_MIN_INEXACT of its nonzero weights are changed by each 16-bit
    conversion and at least R12_MIN_TIES are exact ties (every odd W in fp16, W = 8 mod 16 in bf16); every
    accumulator is an fp32 value and sum |w||x| + |b| stays below 2^24 quanta (asserted inside the reference);
    and the weight conversion matters: truncated, rounded half away or left in fp32 it changes the layer's output
    and at least one tensor the GPU test compares (the layer's own output where it can be fetched; deep in the
    network a one-ulp change of a weight does not always survive the later roundings as far as the logits)."""
    seed, c_in = case[:2]
    sd = en.routing_state_dict_r12(seed, c_in, layer)
    w = sd[f"{layer}.weight"]
    if ".net." in layer:
        blk, _, idx = layer.partition(".net.")
        w = w * sd[f"{blk}.net.{int(idx) + 1}.weight"].reshape(-1, 1, 1, 1)
    mag = np.abs(w[w != 0]).astype(np.float64) / en.R12_SCALE
    assert np.array_equal(mag, np.round(mag)) and mag.min() >= 2048 and mag.max() < 4096
    stats = en.r12_weight_stats(w)
    print(f"{case} {layer}: {mag.size} weights; " + ", ".join(f"{t}: {100 * a:.0f} % inexact, {100 * b:.0f} % ties"
                                                             for t, (a, b) in stats.items()))
    for t, (inexact, ties) in stats.items():
        assert inexact >= en.R12_MIN_INEXACT and ties >= en.R12_MIN_TIES, (t, inexact, ties)
    for plan in ("bf16", "fp16"):     # ("mixed" gives the layer one of these two types)
        x, ref = en.rounding_reference(*case, plan, r12=layer)
        assert x.max() == 3 and np.array_equal(x, np.round(x))
        for mode in ("trunc", "away", "none"):
            alt = en.rounding_reference(*case, plan, r12=layer, alter=((layer, mode),))[1]
            seen = [k for k in en.FORWARD_ORDER if not np.array_equal(alt[k], ref[k])]
            print(f"  {plan} weights {mode}: differs at {seen}")
            assert not np.array_equal(alt[R12_OUT[layer]], ref[R12_OUT[layer]]), (plan, mode)
            assert seen, (plan, mode)       # ... and in a tensor the GPU test fetches
        lg = ref["logits"].astype(np.float64)
        for c in range(3):
            for t in en.DEFAULT_THRESHOLDS[:3]:
                assert np.abs(lg[:, c] - en.logit_cut64(t)).min() >= CUT_MARGIN[8], (plan, c, t)
        masks = en.reference_masks(ref["logits"], en.DEFAULT_THRESHOLDS[:3])
        assert 0.02 <= masks.mean() <= 0.98


@pytest.mark.parametrize("name", en.WIDE_BLOCKS)
def test_r12_block_premises(name):
    """The stand-alone DoubleConv on r12 weights: fp32 accumulation exact (sum |w||x| + |b| below 2^24 quanta of
    2^-8), the weight floors, a lively output that the weight rounding changes."""
    b = en.wide_block(name, "r12")
    assert b.x.max() == 3 and b.scale[0] == en.R12_SCALE
    stats = en.r12_weight_stats(b.w[0])
    for t in ("bf16", "fp16"):
        mid, out, worst = en.block_expected_rounded(b, t)
        print(f"{name} {t}: sum |w||x| + |b| <= {worst:.4g}, out max {out.max():.4g}, {100 * (out != 0).mean():.0f} % nonzero, "
              f"{100 * (out != b.out).mean():.0f} % differ from the unrounded weights' output; weights {stats[t]}")
        assert worst < 2.0 ** 24 * en.R12_SCALE
        assert stats[t][0] >= en.R12_MIN_INEXACT and stats[t][1] >= en.R12_MIN_TIES
        assert np.array_equal(mid, out)                       # the identity second conv
        assert (out != 0).mean() >= 0.25 and (out != b.out).mean() >= 0.25
    # the existing cases' draws are what they were
    assert "r12" not in en.WIDE_CASES


def test_rounding_fault_names_the_fault():
    """The GPU tests' diagnosis: a tensor that equals the reference with one conversion done wrongly is named
    by that fault."""
    args = (*CONTROL, "mixed")
    for name, mode, word in (("c2", "trunc", "truncation"), ("p2", "away", "round-half-away"),
                             ("u2", "other", "the other 16-bit type"), ("p2", "via_skip", "rounded skip"),
                             ("logits", "none", "no rounding")):
        store = "head" if name == "logits" else name
        got = en.rounding_reference(*args, alter=((store, mode),))[1][name]
        msg = en.rounding_fault(name, got, args, {})
        print(msg)
        assert word in msg and f"'{store}'" in msg, msg
    assert "none of" in en.rounding_fault("c2", en.rounding_reference(*args)[1]["c2"] + 1, args, {})
