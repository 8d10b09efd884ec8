"""Bitwise tests of the whole small-batch split-K plan space.  Needs a GPU: run with -m gpu (premises:
tests/test_split_cpu.py; the table of forced plans: tests/split_cases.py).

csrc/unet_capi.cpp layer_split picks, per launch of a forward of N <= 4 images, a slice count ks and on the 8-wave ring
a row tile.  At the small test shapes its cost model never splits, so every (ks, rows) it can emit anywhere is FORCED
here (UNET_MI355X_KSPLIT_FORCE) and checked:

  a. the force took effect: unet_launch_split_at reports the intended (ks, rows) on every intended launch, (1, 0) on
     the rest, and a split launch's label names splitk_reduce_kernel with the layer's epilogue;
  b. bitwise: exact_nets.check_routing_model (logits, every stored intermediate, u8 and packed masks, boxes) on every
     forced plan, in all five precision plans, at (3, 48, 80) and (1, 16, 16), on the networks of split_cases.NETS, the
     scratch filled with 0xFF before every forward; the fp32 plans also on 23-bit inputs;
  c. dense K, real values: logits against the golden and stored intermediates against the oracle within
     test_forward_gpu's TOL, image 0 bitwise the same at N = 1, 2 and 4, two runs bitwise the same;
  d. NaN and +inf through the reduce;
  e. the auto plan, swept over N in {1, 4} and H, W up to 2048, never leaves the set that a. and b. verified;
  f. the auto plan at 512 x 512 is pinned to a literal table.

Value-only mutations of the kernels (no address and no loop bound changes upward), each applied to a scratch copy of
csrc/unet_kernels.hip, and the tests of b. that fail under it on an MI355X -- in each case exactly the runs whose
entry reaches the mutated condition, on all three networks, and no other:

  1. splitk_reduce_kernel's slice loop stops at ksplit - 1 when ksplit >= 4
       78 of 111: test_forced_plan_bitwise[<plan>-ks{4,8,16,32}_own-net*] and [<plan>-ks{4,8,16}_r64-net*], every plan;
       e.g. [bf16-ks4_own-net0], [fp32-ks32_own-net0], [mixed-ks16_r64-net2]
  2. splitk_reduce_kernel adds slice 0 in place of slice ksplit - 1 when ksplit >= 8
       54 of 111: [<plan>-ks{8,16,32}_own-net*] and [<plan>-ks{8,16}_r64-net*]; e.g. [fp32_exact-ks8_own-net0]
  3. partial_store writes acc of pixel group 0 for every group when a.ksplit >= 4 and the 64-row tiles are in use
       27 of 111: [{fp16,bf16,mixed}-ks{4,8,16}_r64-net*]; e.g. [fp16-ks4_r64-net0]

The cost model does split at the older suite's small shapes -- 48 x 80 and 16 x 16 have so few tiles that a deep layer's
4 us launch term is won back -- so test_exact_gpu's routing tests also fail under all three; what they reach is what
the model happens to pick at their shapes (32 of the 76 forced choices of a 16-bit plan, 37 and 43 of the 62 of the
fp32 plans), where this module reaches every pair it can pick at any."""
import functools
import os
import re
import time

import numpy as np
import pytest
import torch

import exact_nets as en
import split_cases as sc
from oracle import unet_oracle as orc
from test_forward_gpu import GOLD, TOL, _forward_state, _positive_state_dict, make_model, rel_err
from unet_mi355x import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = en.HISTORY_FILL
_ENV = ("UNET_MI355X_KSPLIT", "UNET_MI355X_KSPLIT_FORCE", "UNET_MI355X_FUSE_UP1", "UNET_MI355X_CFG",
        "UNET_MI355X_UPCFG", "UNET_MI355X_F32X3")


def _set_env(monkeypatch, force=None, ksplit=None):
    """A clean plan environment (unet_create reads it), then the forced string."""
    for k in _ENV:
        monkeypatch.delenv(k, raising=False)
    if force is not None:
        monkeypatch.setenv("UNET_MI355X_KSPLIT_FORCE", force)
    if ksplit is not None:
        monkeypatch.setenv("UNET_MI355X_KSPLIT", ksplit)


def _routing_model(net, plan):
    return make_model(en.routing_state_dict(*net), net[1], plan)


def _handle(m):
    return m.native_handle(torch.device(DEV))


def _assert_splits(m, plan, entry, shape):
    """a.: unet_launch_split_at against split_cases.expected_splits, and what the labels can show of it."""
    h = _handle(m)
    got, want = h.launch_split_at(*shape), sc.expected_splits(plan, entry, *shape)
    assert got == want, (plan, entry, shape, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w])
    labels = h.launch_labels_at(*shape)
    for i, (ks, rows) in entry.want[plan].items():
        label = labels[sc.LAUNCH_OF_ID[i]]
        red = re.search(r" \+ splitk_reduce_kernel<[^<>]*, (\d)>$", label)
        if ks > 1:
            assert red and int(red.group(1)) == sc.EPI[i], (plan, entry, i, label)
        else:
            assert "splitk_reduce_kernel" not in label, (plan, entry, i, label)
        if rows == 64:   # the 8-wave ring's 64-row tiles: BR / 16 = 4
            assert re.match(r"conv3x3_ring8_kernel<\w+, 4, ", label), (plan, entry, i, label)
    return labels


# ------------------------------------------------------------------------------------------------ a.
@pytest.mark.parametrize("plan,entry", sc.FORCED_RUNS, ids=sc.RUN_IDS)
def test_force_took_effect(plan, entry, monkeypatch):
    """Every forced value is reported by unet_launch_split_at on its launch, at every N of the small-batch plan and
    at every shape the other tests use; the fused first conv, the head, the fused up1 and every launch the value is
    illegal on report (1, 0); above the small-batch limit and at N = 0 nothing is split."""
    _set_env(monkeypatch, entry.force[plan])
    m = _routing_model(sc.NETS[0], plan)
    try:
        for shape in sc.SHAPES + [(1, 48, 80), (4, 48, 80), (1, 64, 64), (2, 64, 64), (4, 64, 64)]:
            _assert_splits(m, plan, entry, shape)
        for n in (0, 5):
            assert _handle(m).launch_split_at(n, 48, 80) == [(1, 0)] * sc.NUM_LAUNCHES
    finally:
        m.close()


def test_launch_split_at_arguments():
    """UNET_EINVAL (a ValueError) for a bad index, a negative shape and null pointers."""
    import ctypes
    m = _routing_model(sc.NETS[0], "mixed")
    try:
        h = _handle(m)
        ks, rows = ctypes.c_int(7), ctypes.c_int(7)
        for args in ((-1, 1, 16, 16), (sc.NUM_LAUNCHES, 1, 16, 16), (3, -1, 16, 16), (3, 1, -16, 16), (3, 1, 16, -16)):
            assert h.lib.unet_launch_split_at(h._h, *args, ctypes.byref(ks), ctypes.byref(rows)) == -1, args
        assert h.lib.unet_launch_split_at(h._h, 3, 1, 16, 16, None, ctypes.byref(rows)) == -1
        assert h.lib.unet_launch_split_at(h._h, 3, 1, 16, 16, ctypes.byref(ks), None) == -1
        assert h.lib.unet_launch_split_at(None, 3, 1, 16, 16, ctypes.byref(ks), ctypes.byref(rows)) == -1
        assert h.lib.unet_launch_split_at(h._h, 3, 1, 16, 16, ctypes.byref(ks), ctypes.byref(rows)) == 0
        assert (ks.value, rows.value) != (7, 7)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ b.
@pytest.mark.parametrize("net", range(len(sc.NETS)), ids=lambda i: f"net{i}")
@pytest.mark.parametrize("plan,entry", sc.FORCED_RUNS, ids=sc.RUN_IDS)
def test_forced_plan_bitwise(plan, entry, net, monkeypatch):
    """One forced plan on one routing network: the whole routing check, bitwise, at N = 3, 48 x 80 (ragged tiles at
    every level) and N = 1, 16 x 16 (a 1-pixel bottleneck) on a workspace reserved once and filled with 0xFF before
    every forward; the plan that ran is the forced one (a.).  The fp32 plans run split_cases.WIDE_NET also on 23-bit
    inputs: three-term activation planes inside every K slice."""
    seed, c_in = sc.NETS[net]
    _set_env(monkeypatch, entry.force[plan])
    m = _routing_model(sc.NETS[net], plan)
    try:
        m.reserve(*sc.SHAPES[0])
        room = _handle(m).workspace_bytes(*sc.SHAPES[0])
        fill = lambda: m.debug_fill(FILL)   # noqa: E731
        for shape in sc.SHAPES:
            assert 0 < _handle(m).workspace_bytes(*shape) <= room, shape
            _assert_splits(m, plan, entry, shape)
            en.check_routing_model(m, (seed, c_in) + shape, plan, f"forced {entry}, filled", before=fill)
        if plan in sc.PLANS32 and sc.NETS[net] == sc.WIDE_NET:
            en.check_routing_model(m, (seed, c_in) + sc.WIDE_SHAPE, plan, f"forced {entry}, 23-bit inputs, filled",
                                   en.WIDE_BITS, before=fill)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ c.
@functools.lru_cache(maxsize=None)
def _dense_case():
    z = np.load(os.path.join(GOLD, "unet_c3_h64w64_n2_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    ref = en.oracle_stored(sd, z["x"])
    assert rel_err(ref["logits"], z["logits"]) <= 1e-6      # the golden IS this oracle's output
    return sd, z["x"], z["logits"], ref


DENSE_RUNS = [(p, e) for p, e in sc.FORCED_RUNS if p in ("fp32", "fp32_exact", "bf16", "mixed")]


@pytest.mark.parametrize("plan,entry", DENSE_RUNS, ids=[f"{p}-{e.name}" for p, e in DENSE_RUNS])
def test_forced_plan_dense_weights(plan, entry, monkeypatch):
    """Real-valued dense weights (every K position of every slice carries one) at N = 2, 64 x 64 under every forced
    plan: logits against the golden and every stored intermediate against the oracle within test_forward_gpu's TOL;
    image 0 bitwise the same at N = 1, N = 2 and inside N = 4; two runs bitwise the same."""
    sd, x, gold, ref = _dense_case()
    _set_env(monkeypatch, entry.force[plan])
    m = make_model(sd, 3, plan)
    try:
        xd = torch.from_numpy(x).to(DEV)
        _assert_splits(m, plan, entry, (2, 64, 64))
        st2 = _forward_state(m, xd)
        errs = {"logits": rel_err(st2["logits"].cpu().numpy(), gold)}
        for k, v in st2.items():
            if k in ref and k != "logits":
                errs[k] = rel_err(v.cpu().numpy().reshape(ref[k].shape), ref[k])
        print(f"{plan} {entry}: rel err " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert len(errs) >= 14, sorted(errs)
        bad = {k: v for k, v in errs.items() if not v <= TOL[plan]}
        assert not bad, (plan, entry, bad, TOL[plan])
        again = _forward_state(m, xd)
        st1 = _forward_state(m, xd[:1].contiguous())
        st4 = _forward_state(m, torch.cat([xd, xd]))
        for k, v in st2.items():
            per = v.numel() // 2
            assert torch.equal(again[k], v), f"{k}: two runs differ"
            assert torch.equal(st1[k].reshape(-1), v.reshape(-1)[:per]), f"{k}: image 0 at N = 1 != N = 2"
            assert torch.equal(st4[k].reshape(-1)[:per], v.reshape(-1)[:per]), f"{k}: image 0 at N = 4 != N = 2"
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ d.
@functools.lru_cache(maxsize=None)
def _nonfinite_case(kind):
    """(state dict, input, oracle logits): N = 1 at 64 x 64 with one NaN pixel on the structured weights, or one +inf
    pixel on test_forward_gpu._positive_state_dict's (which carry +inf to class 0, -inf to class 1, NaN to class 2)."""
    x = syn.uniform_batch(8, 1, 3, 64, 64)
    if kind == "nan":
        sd = syn.make_state_dict(3, 3, 3, profile="structured")
        x[0, 1, 7, 9] = np.nan
    else:
        sd = _positive_state_dict(3, np.array(x))
        x[0, 1, 7, 9] = np.inf
    return sd, x, orc.unet_forward(sd, torch.from_numpy(x)).numpy()


@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("plan", ["mixed", "fp32"])
def test_nonfinite_through_the_reduce(plan, kind, monkeypatch):
    """Four K slices forced everywhere it is legal: the fp32 partials and splitk_reduce_kernel (relu_nan, max_nan)
    carry a NaN or an infinity like the unsplit epilogues.  NaN: the NaN set of the logits is the oracle's and a NaN
    logit gives a False mask.  +inf: the 16-bit plan keeps the kind (+inf True, -inf and NaN False); the three-term
    fp32 plan turns every infinity into NaN, so the non-finite SET is the oracle's and its masks are
    False -- the assertions of test_forward_gpu.test_inf_input_pixels."""
    sd, x, ref = _nonfinite_case(kind)
    entry = sc.FORCED["ks4_own"]
    _set_env(monkeypatch, entry.force[plan])
    m = make_model(sd, 3, plan)
    try:
        _assert_splits(m, plan, entry, (1, 64, 64))
        with torch.no_grad():
            masks, lg = m.forward_masks(torch.from_numpy(x).to(DEV), with_logits=True)
        lg, masks = lg.cpu().numpy(), masks.cpu().numpy().astype(bool)
    finally:
        m.close()
    bad_ref, bad_got = ~np.isfinite(ref), ~np.isfinite(lg)
    print(f"{plan} {kind}: non-finite logits {int(bad_got.sum())} (oracle {int(bad_ref.sum())}: {int(np.isnan(ref).sum())} "
          f"NaN, {int(np.isposinf(ref).sum())} +inf, {int(np.isneginf(ref).sum())} -inf) of {lg.size}")
    assert bad_ref.sum() > 0
    assert np.array_equal(bad_got, bad_ref)
    if kind == "nan":
        assert np.array_equal(np.isnan(lg), np.isnan(ref)) and not np.isinf(ref).any()
        assert not masks[np.isnan(lg)].any()
        return
    assert np.isposinf(ref[0, 0]).any() and np.isneginf(ref[0, 1]).any() and np.isnan(ref[0, 2]).any()
    if plan == "fp32":
        assert not masks[bad_got].any()
    else:
        assert np.array_equal(np.isnan(lg), np.isnan(ref))
        assert np.array_equal(np.isposinf(lg), np.isposinf(ref))
        assert np.array_equal(np.isneginf(lg), np.isneginf(ref))
        assert masks[np.isposinf(lg)].all() and not masks[np.isnan(lg) | np.isneginf(lg)].any()


# ------------------------------------------------------------------------------------------------ e.
def _sweep_shapes():
    """H, W multiples of 16 up to 2048: squares, 2:1, 1:2 and W in {16, 512, 1024}."""
    out = set()
    for a in range(16, 2049, 16):
        out |= {(a, a), (a, 16), (a, 512), (a, 1024)}
        if 2 * a <= 2048:
            out |= {(a, 2 * a), (2 * a, a)}
    return sorted(out)


@pytest.mark.parametrize("plan", sc.PLANS)
def test_auto_plan_stays_inside_the_forced_set(plan, monkeypatch):
    """Host-only: the cost model's own choices over a few thousand shapes.  Every (launch, ks, rows) other than (1, 0)
    is one that FORCED forces (b. ran it bitwise, a. confirmed it ran) or the 16-bit ConvTranspose halves; N = 4
    chooses what N = 1 chooses; N = 5 splits nothing; ks is a power of two <= 32 dividing the chunk count; and the
    workspace grows over UNET_MI355X_KSPLIT=0's by at least the plan's largest partial buffer."""
    _set_env(monkeypatch, ksplit="0")
    m0 = _routing_model(sc.NETS[0], plan)
    h0 = _handle(m0)   # unet_create reads the environment: the handle exists before the variable goes
    _set_env(monkeypatch)
    m = _routing_model(sc.NETS[0], plan)
    try:
        h = _handle(m)
        assert h.small_batch_limit() == 4 and h0.small_batch_limit() == 0
        covered, seen, outside = sc.covered_pairs()[plan], {}, {}
        id_of = {slot: i for i, slot in sc.LAUNCH_OF_ID.items()}
        t0 = time.perf_counter()
        shapes = _sweep_shapes()
        for hh, ww in shapes:
            one = h.launch_split_at(1, hh, ww)
            assert h.launch_split_at(4, hh, ww) == one, (hh, ww)
            assert h.launch_split_at(5, hh, ww) == [(1, 0)] * sc.NUM_LAUNCHES, (hh, ww)
            assert h0.launch_split_at(1, hh, ww) == [(1, 0)] * sc.NUM_LAUNCHES, (hh, ww)
            part = 0
            for slot, (ks, rows) in enumerate(one):
                if (ks, rows) == (1, 0):
                    continue
                i = id_of[slot]
                assert ks in (1, 2, 4, 8, 16, 32) and (sc.CIN[i] // sc.CHUNK) % ks == 0 and rows in (0, 64, 128), (slot, ks, rows)
                seen.setdefault((slot, ks, rows), (hh, ww))
                if (slot, ks, rows) not in covered:
                    outside.setdefault((slot, ks, rows), (hh, ww))
                if ks > 1:
                    lv = sc.LAYER[i][1]
                    part = max(part, ks * (hh >> lv) * (ww >> lv) * sc.ROWS[i] * 4)
            for n in (1, 4):
                grown = h.workspace_bytes(n, hh, ww) - h0.workspace_bytes(n, hh, ww)
                assert grown >= n * part, (n, hh, ww, grown, n * part)
        by = {}
        for slot, ks, rows in sorted(seen):
            by.setdefault((ks, rows), []).append(slot)
        print(f"{plan}: {len(shapes)} shapes in {time.perf_counter() - t0:.2f} s; (ks, rows) -> launches: {by}")
        assert not outside, f"{plan}: the auto plan chooses (launch, ks, rows) that FORCED lacks, first at (H, W): {outside}"
    finally:
        m.close()
        m0.close()


# ------------------------------------------------------------------------------------------------ f.
_S16 = [(1, 0), (1, 0), (1, 64), (1, 64), (1, 64), (1, 64), (1, 64), (4, 64), (4, 64), (8, 64), (1, 128), (4, 64),
        (4, 64), (1, 128), (2, 64), (1, 64), (1, 0), (1, 64), (1, 0), (1, 0), (1, 0), (1, 0)]
AUTO_512 = {   # (ks, rows) per launch slot of a forward of (1, 512, 512): a retune of layer_split changes a line here
    "fp32": [(1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (2, 0), (4, 0), (4, 0), (8, 0), (8, 0), (2, 0), (4, 0), (4, 0),
             (1, 0), (2, 0), (2, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],
    "fp32_exact": [(1, 0), (1, 0), (1, 0), (1, 0), (2, 0), (1, 0), (4, 0), (2, 0), (8, 0), (8, 0), (4, 0), (4, 0),
                   (4, 0), (2, 0), (2, 0), (2, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (1, 0)],
    "fp16": _S16, "bf16": _S16, "mixed": _S16,
}


@pytest.mark.parametrize("plan", sc.PLANS)
def test_auto_plan_at_512_is_pinned(plan, monkeypatch):
    """The production shape's plan, slot by slot, against the table recorded when this test was written."""
    _set_env(monkeypatch)
    m = _routing_model(sc.NETS[0], plan)
    try:
        got = _handle(m).launch_split_at(1, 512, 512)
    finally:
        m.close()
    diff = [(slot, g, w) for slot, (g, w) in enumerate(zip(got, AUTO_512[plan])) if g != w]
    assert not diff, (f"{plan}: the auto split-K plan at (1, 512, 512) is no longer AUTO_512[{plan!r}] of "
                      f"tests/test_split_gpu.py; (slot, got, pinned): {diff} -- a deliberate retune updates the table")
