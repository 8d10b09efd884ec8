"""Bitwise checks of the native forward against the reference on exact-arithmetic operands
(tests/exact_nets.py; premises asserted on the CPU by tests/test_exact_cpu.py).  Needs a GPU: run with -m gpu.

Every comparison here is np.array_equal -- no tolerance, in every precision plan: the operands are chosen so
that every product and partial sum is exactly representable, hence independent of accumulation order, split-K,
fusion and of where the bias is added.  A mismatch names the first wrong tensor in forward order, how many
elements differ, the first (n, c, y, x) with got / want, and the kernel that wrote it."""
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANS = ["fp32", "fp32_exact", "fp16", "bf16", "mixed"]
HALO_CFGS, RING_CFGS, UP_CFGS = [0, 1, 2], [3, 4, 5, 8, 9, 10, 11], [2, 6, 7]   # csrc/unet_internal.h Cfg


def _routing_model(seed, c_in, dtype, wide_w=None):
    sd = en.routing_state_dict(seed, c_in) if wide_w is None else en.routing_state_dict_wide_w(seed, c_in, *wide_w)
    m = UNet(c_in, 3, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def _check_routing(case, dtype, tag="", bits=4, wide_w=None):
    """One model, one input: logits and every stored intermediate, masks (u8 and packed) and boxes, all
    bitwise against the oracle.  Returns the launch labels of the forward."""
    m = _routing_model(case[0], case[1], dtype, wide_w)
    try:
        return en.check_routing_model(m, case, dtype, tag, bits, wide_w)   # the assertions (shared with test_history_gpu)
    finally:
        m.close()


def _print_labels(what, labels):
    print(f"{what}: " + " | ".join(f"{i}: {s}" for i, s in enumerate(labels)))


@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("case", en.ROUTING_SMALL, ids=str)
def test_routing_minimum_sizes(case, dtype):
    """16 x 16 at N = 1 (1-pixel bottleneck, the small-batch split-K plan) and 16 x 112 at N = 6 (the
    large-batch plan, partial tiles at every level), 3 and 1 input channels, every plan."""
    _print_labels(f"{dtype} {case}", _check_routing(case, dtype))


@pytest.mark.parametrize("dtype", PLANS)
@pytest.mark.parametrize("case", en.ROUTING_RAGGED, ids=str)
def test_routing_ragged(case, dtype):
    """N = 3 at 48 x 80 (ragged tiles at every level), three seeds for K coverage (test_exact_cpu prints it)."""
    _check_routing(case, dtype)


@pytest.mark.parametrize("dtype", ["mixed", "fp32"])
@pytest.mark.parametrize("case", en.ROUTING_LARGE, ids=str)
def test_routing_full_size_pages(case, dtype):
    """N = 2 at 512 x 512: persistent walkers take several tiles per block and the rings wrap."""
    _print_labels(f"{dtype} {case}", _check_routing(case, dtype))


@pytest.mark.parametrize("dtype", ["fp32", "fp32_exact"])
@pytest.mark.parametrize("case", en.ROUTING_WIDE, ids=str)
def test_routing_wide_inputs_fp32_plans(case, dtype):
    """The routing networks on 23-bit inputs: every layer of the whole forward, in the kernels the
    three-term plan really runs there (split-per-tap, split-once, conv1.3 + head, both ConvTranspose
    variants), multiplies activations with nonzero hi, mid and lo terms by +-1; the three dropped products
    are identically zero, so the plan must be exact."""
    _print_labels(f"{dtype} wide {case}", _check_routing(case, dtype, "23-bit inputs", en.WIDE_BITS))


@pytest.mark.parametrize("dtype", ["fp32", "fp32_exact"])
@pytest.mark.parametrize("kind", list(en.WIDE_W_KINDS))
@pytest.mark.parametrize("layer", en.WIDE_W_LAYERS)
@pytest.mark.parametrize("case", en.ROUTING_WIDE, ids=str)
def test_routing_one_wide_weight_layer_fp32_plans(case, layer, kind, dtype):
    """The whole network with ONE layer on wide weights, so that the weight-side terms of the three-term plan
    are checked in the kernels the network really runs: the split-once kernel (down4.0, down4.3), the conv1.3
    tile with the head, and the ConvTranspose both at N = 3 (weights pre-split on the host, 64-row tiles)
    and at N = 6 (weights split on the fly, 128-row tiles).  b18: 18-bit weights with nonzero mid and lo
    against activations below 32 (hi.hi, hi.mid, hi.lo); c10: 10-bit weights against 10-bit activations
    (hi.hi, hi.mid, mid.hi, mid.mid).  The dropped products are identically zero (asserted on the CPU), so
    a missing, doubled or mis-addressed term plane gives a wrong integer."""
    labels = _check_routing(case, dtype, f"wide weights {kind} on {layer}", en.WIDE_W_KINDS[kind][0], (layer, kind))
    launch = {"down4.net.0": 6, "down4.net.3": 7, "conv1.net.3": 21, "up4": 10, "up1": 19}[layer]
    print(f"{dtype} {case} {layer} {kind}: {labels[launch]}")
    if dtype == "fp32":   # the kernels this test is about
        want = {"down4.net.0": "conv3x3_x3s_kernel", "down4.net.3": "conv3x3_x3s_kernel",
                "conv1.net.3": "conv3x3_x3w_kernel"}.get(layer, "conv3x3_halo_kernel<float, 1, 4, ")
        assert labels[launch].startswith(want), labels[launch]
        if layer.startswith("up"):   # 128-row tiles splitting both operands above the small-batch limit, 64-row below
            assert labels[launch].startswith("conv3x3_halo_kernel<float, 1, 4, 8, " if case[2] > 4 else
                                             "conv3x3_halo_kernel<float, 1, 4, 4, "), labels[launch]


FAMILY = {**{c: "conv3x3_halo_kernel<" for c in HALO_CFGS}, **{c: "conv3x3_ring_kernel<" for c in (3, 4, 5)},
          **{c: "conv3x3_ring8_kernel<" for c in (8, 9, 10, 11)}}
UP_FAMILY = {2: "conv3x3_halo_kernel<", 6: "convT_ring_kernel<", 7: "convT_ring_kernel<"}
UP_LAUNCHES = (10, 13, 16, 19)

FORCED = ([("UNET_MI355X_CFG", ",".join(f"{i}:{c}" for i in range(17)), f"cfg{c}") for c in HALO_CFGS + RING_CFGS] +
          [("UNET_MI355X_UPCFG", ",".join(f"{i}:{c}" for i in range(4)), f"upcfg{c}") for c in UP_CFGS] +
          [("UNET_MI355X_KSPLIT", "0", "ksplit0"), ("UNET_MI355X_FUSE_UP1", "0", "fuse0"),
           ("UNET_MI355X_FUSE_UP1", "1", "fuse1")])


@pytest.mark.parametrize("dtype", ["bf16", "fp32_exact"])
@pytest.mark.parametrize("var,value,tag", FORCED, ids=[f[2] for f in FORCED])
def test_routing_forced_configurations(var, value, tag, dtype, monkeypatch):
    """N = 2 at 64 x 64 with every 3x3 configuration forced on all layers that support it, every ConvTranspose
    configuration (up1 as its own launch, so that all four run it), the small-batch split-K plan off, and
    conv2.3 + up1 fused and not: the same integers in every one of them."""
    monkeypatch.setenv(var, value)
    if var == "UNET_MI355X_UPCFG":
        monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    labels = _check_routing(en.ROUTING_FORCED, dtype, tag)
    _print_labels(f"{dtype} {tag}", labels)
    assert_forced_labels(var, value, tag, dtype, labels)


def assert_forced_labels(var, value, tag, dtype, labels):
    """The override took effect: every 3x3 launch (a layer that does not support the configuration falls back
    within its family) or every ConvTranspose launch runs the forced kernel family."""
    if var == "UNET_MI355X_CFG":
        fam = FAMILY[int(tag[3:])]
        bad = [(i, s) for i, s in enumerate(labels) if i > 0 and i not in UP_LAUNCHES and s and not s.startswith(fam)]
        assert not bad, bad
    elif var == "UNET_MI355X_UPCFG":
        assert all(labels[i].startswith(UP_FAMILY[int(tag[5:])]) for i in UP_LAUNCHES), [labels[i] for i in UP_LAUNCHES]
    elif var == "UNET_MI355X_KSPLIT":
        assert not any("splitk_reduce" in s for s in labels), labels
    elif dtype == "bf16":
        assert (labels[19] == "") == (value == "1"), labels[19]
    else:
        assert labels[19] != ""          # the fp32 plans never fuse up1


# ------------------------------------------------------------------------------------------------ blocks
@functools.lru_cache(maxsize=None)
def _unet(dtype):
    """One module tree per plan; the blocks under test get their weights loaded into it."""
    return UNet(3, 3, compute_dtype=dtype).to(DEV).eval()


def _run_block(blk: en.ExactBlock, dtype, pre=None):
    dc = getattr(_unet(dtype), blk.name)
    dc.close()                                   # a fresh native block (it reads its environment when created)
    dc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in blk.sd.items()})
    try:
        if pre is not None:                      # (the DoubleConv, before its forward)
            pre(dc)
        with torch.no_grad():
            got = dc(torch.from_numpy(np.array(blk.x)).to(DEV)).cpu().numpy()
    finally:
        dc.close()
    return got


def _check_block(blk, dtype, what, pre=None):
    got, want = _run_block(blk, dtype, pre), blk.expected(dtype)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        pytest.fail(f"{dtype} {what}: " + en.describe_mismatch(
            f"{blk.name} output", got, want, f"unet_block_forward DoubleConv({blk.cin}, {blk.cout})"))


@pytest.mark.parametrize("dtype", ["fp32", "fp32_exact", "bf16", "fp16"])
@pytest.mark.parametrize("name", list(en.BLOCKS))
def test_dense_block_bitwise(name, dtype):
    """Every block shape of the network through the stand-alone DoubleConv (unet_block_*) on dense
    {-1, 0, 1} weights -- every (cin, tap) position of both convs carries weights -- at ragged sizes, N = 2.

    Expected: relu(exact) on the fp32 plans.  On bf16 / fp16 the block stores its last layer in the plan's
    16-bit type (the epilogue's round-to-nearest-even conversion) and unet_block_forward widens that buffer
    to the fp32 output (launch_nhwc_to_nchw): RNE_T(relu(exact)).  The first conv's output is a bf16 and an
    fp16 value by construction, so storing it changes nothing.  ("mixed" is a per-level choice of these.)"""
    _check_block(en.dense_block(name), dtype, "dense")


@pytest.mark.parametrize("dtype", ["fp32", "fp32_exact"])
@pytest.mark.parametrize("case", list(en.WIDE_CASES))
@pytest.mark.parametrize("name", en.WIDE_BLOCKS)
def test_wide_operands_three_term_bitwise(name, case, dtype):
    """The three-term fp32 plan on operands that need the mid and lo terms but whose three dropped products
    (mid.lo, lo.mid, lo.lo) are identically zero: a short-K block (down2), a long-K block (down4) and conv1,
    bitwise, and the exact-fp32 MFMA on the same operands.  The second conv is a centre-tap identity and
    passes integers of up to 24 bits through all three terms of the activation split."""
    _check_block(en.wide_block(name, case), dtype, f"wide case {case}")


def test_f32x3_override_leaves_fp32_exact_alone(monkeypatch):
    """UNET_MI355X_F32X3 is an A/B switch of the "fp32" plan: an "fp32_exact" model keeps its kernels
    (launch labels) with the variable set, and its stand-alone blocks stay bitwise."""
    def labels():
        m = UNet(3, 3, compute_dtype="fp32_exact").to(DEV).eval()
        h = m.native_handle(torch.device(DEV))
        out = (h.launch_labels(), h.launch_labels_at(1, 512, 512))
        m.close()
        return out
    monkeypatch.delenv("UNET_MI355X_F32X3", raising=False)
    plain = labels()
    monkeypatch.setenv("UNET_MI355X_F32X3", "1")
    assert labels() == plain
    for name in ("down1", "down2", "down4", "conv1"):
        _check_block(en.dense_block(name), "fp32_exact", "dense, UNET_MI355X_F32X3=1")
    _check_block(en.wide_block("down2", "c"), "fp32_exact", "wide case c, UNET_MI355X_F32X3=1")
