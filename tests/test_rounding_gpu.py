"""Bitwise checks of every fp32 -> 16-bit conversion of the native forward (tests/exact_nets.py section 3;
premises asserted on the CPU by tests/test_rounding_cpu.py).  Needs a GPU: run with -m gpu.

The exact-arithmetic tests (tests/test_exact_gpu.py) use operands that no plan ever has to round.  Here every
accumulator is still an exact fp32 value -- so the result does not depend on accumulation order, split-K or
fusion -- but the activations (multiples of 2^-4 below 2^15) and, in the r12 cases, the weights need more bits
than bf16 or fp16 hold: every store and every register cast rounds, exact ties included.  The reference
(en.rounding_reference) is the forward in float64 with round-to-nearest-even applied where the plan's type map
(level_dtype) says the library converts.  Every comparison is np.array_equal; a mismatch names the first wrong
tensor, the element, the kernel that wrote it, and which single fault (truncation, round-half-away, the other
16-bit type, a doubled rounding, no rounding) reproduces the wrong tensor."""
import functools

import numpy as np
import pytest
import torch

import exact_nets as en
from oracle import unet_oracle as orc
from test_exact_gpu import FAMILY, FORCED, UP_FAMILY, UP_LAUNCHES
from unet_mi355x import native
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANS = ["bf16", "fp16", "mixed", "fp32", "fp32_exact"]
PLANS16 = ["bf16", "fp16", "mixed"]


def _model(sd, c_in, plan):
    m = UNet(c_in, 3, compute_dtype=plan)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV).eval()


def _reference_masks(ref, n):
    return np.stack([np.stack([orc.masks_from_logits(np.array(ref["logits"][i]))[f] for f in orc.FIELDS])
                     for i in range(n)])


def _check(case, plan, tag="", r12=None, pre=None):
    """One model, one input: logits and every stored intermediate, masks (u8 and packed) and boxes, all bitwise
    against the rounding reference (tests/test_exact_gpu.py _check_routing on the rounding operands).  ``pre``
    (optional) is called with the model before its first forward.  Returns the launch labels of the forward."""
    seed, c_in, n, h, w = case
    x, ref = en.rounding_reference(*case, plan, r12=r12)
    sd = en.rounding_state_dict(seed, c_in) if r12 is None else en.routing_state_dict_r12(seed, c_in, r12)
    m = _model(sd, c_in, plan)
    try:
        if pre is not None:
            pre(m)
        xd = torch.from_numpy(np.array(x)).to(DEV)
        with torch.no_grad():
            logits = m(xd)
        torch.cuda.synchronize()
        labels = m.native_handle(torch.device(DEV)).launch_labels_at(n, h, w)
        lg = logits.cpu().numpy()
        bad = en.first_stored_mismatch(m, lg, ref, labels)
        if bad:
            name = bad.split(":")[0]
            got = lg if name == "logits" else m.intermediate(name).cpu().numpy().reshape(ref[name].shape)
            fault = en.rounding_fault(name, got, (*case, plan), {"r12": r12}) if plan in PLANS16 else "an fp32 plan"
            pytest.fail(f"{plan} {case} {tag}: {bad}; {fault}")
        ref_masks = _reference_masks(ref, n)
        with torch.no_grad():
            masks, lg2 = m.forward_masks(xd, with_logits=True)
            packed = m.forward_masks(xd, packed=True)
            bmasks, boxes = m.forward_boxes(xd, masks="u8")
        assert np.array_equal(lg2.cpu().numpy(), ref["logits"]), "logits of forward_masks"
        for name, mk in (("u8", masks.cpu().numpy()), ("boxes' u8", bmasks.cpu().numpy()),
                         ("packed", np.unpackbits(packed.cpu().numpy(), axis=-1, bitorder="little"))):
            if not np.array_equal(mk.astype(bool), ref_masks):
                pytest.fail(f"{plan} {case} {tag}: " + en.describe_mismatch(
                    f"{name} masks", mk.astype(bool), ref_masks, labels[21]))
        assert np.array_equal(boxes.cpu().numpy(), en.np_boxes(ref_masks)), (boxes.cpu().numpy(), en.np_boxes(ref_masks))
        return labels
    finally:
        m.close()


def _print_labels(what, labels):
    print(f"{what}: " + " | ".join(f"{i}: {s}" for i, s in enumerate(labels)))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("case", en.ROUNDING_MIN + en.ROUNDING_LARGER, ids=str)
def test_rounding_whole_network(case, plan):
    """16 x 16 at N = 1, 3 and 1 input channels (the small-batch plan; at this size it picks finer row tiles and
    the small-batch ConvTranspose variants, and splits no layer over K: test_rounding_forced_split_k does), 16 x 112
    at N = 6 (the large-batch kernels' epilogues, partial tiles at every level) and 48 x 80 at N = 3 (ragged
    tiles).  In the fp32 plans nothing converts: the unrounded chain."""
    _print_labels(f"{plan} {case}", _check(case, plan))


@pytest.mark.parametrize("plan", PLANS16)
@pytest.mark.parametrize("var,value", [("UNET_MI355X_CFG", "0:10"), ("UNET_MI355X_FUSE_UP1", "0")])
@pytest.mark.parametrize("case", [en.ROUNDING_MIN[0], en.ROUNDING_LARGER[1]], ids=str)
def test_rounding_unfused(case, var, value, plan, monkeypatch):
    """The same bits with the first conv as its own launch (UNET_MI355X_CFG=0:10: the input is then converted in
    first_conv_mfma_kernel's B fragments and down1.0's output goes through a store instead of the fused
    kernel's LDS tile), and with up1 as its own launch (UNET_MI355X_FUSE_UP1=0, the switch of
    test_golden_intermediates: c7 is then stored, and compared, instead of being cast in registers)."""
    monkeypatch.setenv(var, value)
    labels = _check(case, plan, f"{var}={value}")
    _print_labels(f"{plan} {case} {var}={value}", labels)
    if var == "UNET_MI355X_CFG":
        assert not labels[0].startswith("x_to_px4_kernel"), labels[0]
    else:
        assert labels[19] != "", labels


@pytest.mark.parametrize("plan", ["mixed", "bf16"])
@pytest.mark.parametrize("var,value,tag", FORCED, ids=[f[2] for f in FORCED])
def test_rounding_forced_configurations(var, value, tag, plan, monkeypatch):
    """N = 2 at 64 x 64 with every 3x3 configuration forced on all layers that support it, every ConvTranspose
    configuration, the small-batch split-K plan off, and conv2.3 + up1 fused and not (the FORCED list and the
    label assertions of tests/test_exact_gpu.py): every kernel family's epilogue converts alike -- in particular
    u1 has the same bits whether c7 was stored or cast in registers (EPI_UPFUSE)."""
    monkeypatch.setenv(var, value)
    if var == "UNET_MI355X_UPCFG":
        monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    labels = _check(en.ROUNDING_FORCED, plan, tag)
    _print_labels(f"{plan} {tag}", labels)
    if var == "UNET_MI355X_CFG":
        fam = FAMILY[int(tag[3:])]
        # the LDS-halo family stores its own operand type only: unet_create keeps it off the seam of "mixed" (down2.3,
        # launch 3: fp16 skip, bf16 pooled map), which runs the 4-wave ring whatever is forced
        seam = {3: "conv3x3_ring_kernel<"} if plan == "mixed" and fam == "conv3x3_halo_kernel<" else {}
        bad = [(i, s) for i, s in enumerate(labels)
               if i > 0 and i not in UP_LAUNCHES and s and not s.startswith(seam.get(i, fam))]
        assert not bad, bad
    elif var == "UNET_MI355X_UPCFG":
        # the other seam of "mixed": up2 (launch 16) reads bf16 and writes fp16, which only the ConvTranspose ring does
        fam = UP_FAMILY[int(tag[5:])]
        seam = {16: "convT_ring_kernel<"} if plan == "mixed" and fam == "conv3x3_halo_kernel<" else {}
        assert all(labels[i].startswith(seam.get(i, fam)) for i in UP_LAUNCHES), [labels[i] for i in UP_LAUNCHES]
    elif var == "UNET_MI355X_KSPLIT":
        assert not any("splitk_reduce" in s for s in labels), labels
    else:
        assert (labels[19] == "") == (value == "1"), labels[19]


# the layers the small-batch plan may split over K (the 8-wave 128-row ring, plain or pooled store) with at least two
# 32-channel chunks left per slice at two slices: down2.3 .. conv2.3, layer id (UNET_MI355X_KSPLIT_FORCE's index) -> launch
SPLIT_LAUNCH = {2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 9, 9: 11, 10: 12, 11: 14, 12: 15, 13: 17, 14: 18}


@pytest.mark.parametrize("plan", PLANS16)
def test_rounding_forced_split_k(plan, monkeypatch):
    """Two K slices forced on every layer that can split (UNET_MI355X_KSPLIT_FORCE), N = 3 at 48 x 80 with up1 as
    its own launch: the kernels write fp32 partials and splitk_reduce_kernel adds them to the bias and converts
    ONCE -- the skip to TO and, from the fp32 maximum, the pooled map to TQ (fp16 and bf16 at down2.3 of "mixed")."""
    monkeypatch.setenv("UNET_MI355X_KSPLIT_FORCE", ",".join(f"{i}:2" for i in SPLIT_LAUNCH))
    monkeypatch.setenv("UNET_MI355X_FUSE_UP1", "0")
    labels = _check(en.ROUNDING_LARGER[1], plan, "two K slices forced")
    _print_labels(f"{plan} forced split", labels)
    unsplit = [(i, labels[i]) for i in SPLIT_LAUNCH.values() if "splitk_reduce_kernel" not in labels[i]]
    assert not unsplit, unsplit


@pytest.mark.parametrize("plan", PLANS16)
@pytest.mark.parametrize("layer", en.R12_LAYERS)
@pytest.mark.parametrize("case", en.ROUNDING_R12, ids=str)
def test_rounding_one_r12_weight_layer(case, layer, plan):
    """The whole network with ONE layer on 12-bit weights (bf16 keeps 8 of the bits, fp16 11; a quarter of the
    weights are exact ties in each type), at N = 3 (the small-batch plan's packings) and N = 6: the host's
    put_elem must pack RNE_T(fp32(folded)) for the layer's own level type in every packing a kernel family reads
    (ring, split-once, fused up1, both ConvTranspose variants), and for out_conv the head kernel must cast its
    fp32 weights to HT on the device the same way."""
    labels = _check(case, plan, f"r12 weights on {layer}", r12=layer)
    launch = {"down4.net.0": 6, "down4.net.3": 7, "conv1.net.3": 21, "up4": 10, "up1": 19, "out_conv": 21}[layer]
    print(f"{plan} {case} {layer}: {labels[launch] or labels[18]}")


@functools.lru_cache(maxsize=None)
def _unet(plan):
    return UNet(3, 3, compute_dtype=plan).to(DEV).eval()


@pytest.mark.parametrize("plan", ["bf16", "fp16"])
@pytest.mark.parametrize("name", en.WIDE_BLOCKS)
def test_rounding_r12_blocks(name, plan):
    """The stand-alone DoubleConv (unet_block_*) on r12 weights: its own weight packing rounds like the
    network's, and both of its stores round to nearest even."""
    blk = en.wide_block(name, "r12")
    _, want, _ = en.block_expected_rounded(blk, plan)
    dc = getattr(_unet(plan), blk.name)
    dc.close()
    dc.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in blk.sd.items()})
    try:
        with torch.no_grad():
            got = dc(torch.from_numpy(np.array(blk.x)).to(DEV)).cpu().numpy()
    finally:
        dc.close()
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        pytest.fail(f"{plan} r12: " + en.describe_mismatch(
            f"{blk.name} output", got, want, f"unet_block_forward DoubleConv({blk.cin}, {blk.cout})"))


def test_rounding_graph_replay():
    """The hipGraph-captured forward of the "mixed" plan replays the eager forward's bits -- logits, packed
    masks and boxes -- and both are the reference's."""
    case = en.ROUNDING_LARGER[1]
    seed, c_in, n, h, w = case
    x, ref = en.rounding_reference(*case, "mixed")
    m = _model(en.rounding_state_dict(seed, c_in), c_in, "mixed")
    try:
        hd = m.native_handle(torch.device(DEV))
        stream = torch.cuda.current_stream().cuda_stream
        xd = torch.from_numpy(np.array(x)).to(DEV)
        lg = torch.empty((n, 3, h, w), device=DEV)
        mk = torch.empty((n, 3, h, w // 8), dtype=torch.uint8, device=DEV)
        bx = torch.empty((n, 3, 4), dtype=torch.int32, device=DEV)
        hd.reserve(n, h, w)
        hd.forward_boxes(xd, lg, mk, native.MASK_BITS, bx, stream)
        torch.cuda.synchronize()
        eager = (lg.clone(), mk.clone(), bx.clone())
        g = hd.graph(xd, lg, mk, native.MASK_BITS, boxes=bx)
        for t in (lg, mk, bx):
            t.zero_()
        for _ in range(2):
            g.launch(stream)
        torch.cuda.synchronize()
        assert torch.equal(lg, eager[0]) and torch.equal(mk, eager[1]) and torch.equal(bx, eager[2])
        g.close()
        got = lg.cpu().numpy()
        if not np.array_equal(got, ref["logits"]):
            pytest.fail("graph replay: " + en.describe_mismatch("logits", got, ref["logits"], "graph"))
        ref_masks = _reference_masks(ref, n)
        assert np.array_equal(np.unpackbits(mk.cpu().numpy(), axis=-1, bitorder="little").astype(bool), ref_masks)
        assert np.array_equal(bx.cpu().numpy(), en.np_boxes(ref_masks))
    finally:
        m.close()
