"""The premises of the history-independence GPU tests (tests/test_history_gpu.py), checked without a GPU: the
poison is a poison, every probe fits the reservation it runs in, and every step has a mask that stale all-ones
bits would change."""
import numpy as np
import pytest
import torch

import exact_nets as en
from oracle import unet_oracle as orc


def test_fill_byte_is_a_nan_in_every_float_format():
    """0xFF repeated: a NaN as fp16, bf16, fp32 and fp64 (exponent all ones, mantissa nonzero), all-ones mask
    bits, -1 as an integer count."""
    raw = np.full(8, en.HISTORY_FILL, np.uint8)
    for t in (np.float16, np.float32, np.float64):
        assert np.isnan(raw.view(t)).all(), t
    bf16 = (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)   # a bf16 is the top half of an fp32
    assert np.isnan(bf16).all()
    assert torch.isnan(torch.from_numpy(raw.copy()).view(torch.bfloat16)).all()
    assert (raw.view(np.int32) == -1).all() and (raw.view(np.int64) == -1).all()
    assert np.unpackbits(raw).all()


@pytest.mark.parametrize("net", en.HISTORY_NETS, ids=str)
def test_nan_input_floods_every_stored_tensor(net):
    """The oracle on an all-NaN input: all-NaN logits and intermediates, on the routing networks' sparse weights
    too (0 x NaN is NaN), so the hook-free flood poisons every buffer a forward stores.  One image: the
    propagation does not depend on N."""
    seed, c_in = net
    _, h, w = en.HISTORY_RESERVE
    sd = {k: torch.from_numpy(np.array(v)) for k, v in en.routing_state_dict(seed, c_in).items()}
    x = torch.full((1, c_in, h, w), float("nan"))
    logits, it = orc.unet_forward(sd, x, return_intermediates=True)
    assert torch.isnan(logits).all()
    for k, v in it.items():
        assert torch.isnan(v).all(), k
    with torch.no_grad():
        for name, src in (("up4", "bn"), ("up3", "c5"), ("up2", "c6"), ("up1", "c7")):
            assert torch.isnan(orc.up(sd, name, it[src])).all(), name
    # and a NaN logit is a False mask (sigmoid(NaN) > thr is False)
    assert not any(m.any() for m in orc.masks_from_logits(logits[0].numpy()).values())


def _smaller(probe, reserve):
    return all(p <= r for p, r in zip(probe, reserve)) and int(np.prod(probe)) < int(np.prod(reserve))


def test_every_probe_is_smaller_than_its_reservation():
    """In N x H x W and per dimension: no probe can make its handle re-allocate (the GPU tests also assert
    workspace_bytes of the probe <= that of the reservation)."""
    for probe in en.HISTORY_STEPS + en.HISTORY_GRAPHS + [en.ROUTING_FORCED[2:], en.HISTORY_SPLIT[2:]]:
        assert _smaller(probe, en.HISTORY_RESERVE), probe
    assert set(en.HISTORY_GRAPHS) <= set(en.HISTORY_STEPS) and en.HISTORY_STEPS[0] not in en.HISTORY_GRAPHS
    for name in en.BLOCKS:
        assert _smaller((en.BLOCK_N,) + en.BLOCK_SIZE[name], en.history_block_reserve(name)), name


def test_steps_cover_what_they_claim():
    n = [s[0] for s in en.HISTORY_STEPS]
    assert 4 in n and 5 in n and 1 in n                                   # both sides of the small-batch limit (4)
    assert any(a > 4 >= b or b > 4 >= a for a, b in zip(n, n[1:]))        # the two plans alternate
    assert any(h == 16 and w == 16 for _, h, w in en.HISTORY_STEPS)       # 1-pixel bottleneck
    assert {w % 32 == 0 for _, _, w in en.HISTORY_STEPS} == {True, False}
    assert len(set(en.HISTORY_STEPS)) == len(en.HISTORY_STEPS)


@pytest.mark.parametrize("net", en.HISTORY_NETS, ids=str)
def test_every_step_has_a_mask_that_stale_bits_would_change(net):
    """By the oracle, every step has at least one (image, class) mask that is neither empty nor full: all-ones
    (or any other) stale mask bits read in its place change a box."""
    seed, c_in = net
    for n, h, w in en.HISTORY_STEPS + [en.HISTORY_RESERVE]:
        _, ref = en.routing_reference(seed, c_in, n, h, w)
        masks = en.reference_masks(ref["logits"], en.DEFAULT_THRESHOLDS)
        share = masks.reshape(n, masks.shape[1], -1).mean(-1)
        assert ((share > 0) & (share < 1)).any(), ((n, h, w), share)
        boxes = en.np_boxes(masks)
        full = np.array([0, 0, w - 1, h - 1])
        assert (boxes != full).any(axis=-1).any(), (n, h, w)   # some box is not the whole page
