"""Exact-arithmetic operands for the bitwise tests (tests/test_exact_cpu.py, tests/test_exact_gpu.py; the
history-independence tests, tests/test_history_*.py, run the same routing check on a handle with a past).

Every generator here builds operands for which every product and every partial sum of a layer is exactly
representable in fp32 -- and every stored activation in bf16 and fp16 where a 16-bit plan stores it -- so a
convolution's result does not depend on the accumulation order, on split-K, on where the bias is added or on
whether an intermediate stays in registers.  A kernel must then reproduce the reference bit for bit, and any
addressing, packing, border, concat or pixel-shuffle error shows as a wrong value at a named (n, c, y, x).

  exact_fold          BatchNorm parameters whose fold (csrc/unet_capi.cpp fold()) is exact, asserted
  routing_state_dict  whole network: one +1 (and on every second channel one -1) per output channel; run on
                      integers in [0, 15] in every plan, and on 23-bit integers in the fp32 plans
  dense_block         one DoubleConv with dense {-1, 0, 1} weights: every K position carries a weight
  wide_block          one DoubleConv whose first conv carries wide integers (the three-term fp32 plan's
                      hi / mid / lo products), the second being a centre-tap identity

The rounding networks (section 3; tests/test_rounding_cpu.py, tests/test_rounding_gpu.py) keep the exact
fp32 accumulation but carry operands that the 16-bit plans cannot store: every conversion to bf16 / fp16 then
rounds, ties included, and ``rounding_reference`` restates in float64 where the library rounds and to what.

A helper module, not a conftest: it holds no fixtures and changes nothing about how the suite runs.
"""
from __future__ import annotations

import functools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as orc
from unet_mi355x import synthetic as syn

# running_var such that var + eps is within 7e-9 of 1: the folded scale g / sqrt(var + 1e-5) then rounds
# w * g to itself in fp32 for every integer |w| < 2^24 and g a power of two (asserted by exact_fold)
RUNNING_VAR = np.float32(1.0 - 1e-5)

# name -> (in_ch, out_ch) of the reference's DoubleConv blocks (in_ch of down1 = n_channels)
BLOCKS = OrderedDict([("down1", (3, 64)), ("down2", (64, 128)), ("down3", (128, 256)), ("down4", (256, 512)),
                      ("bottleneck", (512, 1024)), ("conv4", (1024, 512)), ("conv3", (512, 256)),
                      ("conv2", (256, 128)), ("conv1", (128, 64))])


# ------------------------------------------------------------------------------------------------ roundings
def bf16_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), returned as fp32 (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).reshape(np.shape(x))


def f16_rne(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest fp16 (ties to even), returned as fp32."""
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


RNE = {"bf16": bf16_rne, "fp16": f16_rne}


def split3(x: np.ndarray):
    """x = hi + mid + lo, each a bf16 (csrc/unet_kernels.hip split3_bf16, unet_capi.cpp split3_host)."""
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = bf16_rne(r)
    lo = bf16_rne((r - m).astype(np.float32))
    return h, m, lo


# ------------------------------------------------------------------------------------------------ section 0
def fold_f64(w, bias, g, beta, mean, var):
    """csrc/unet_capi.cpp fold() restated in float64: s = g / sqrt((double)var + 1e-5), w * s and
    (bias - mean) * s + beta, both still in double (the library rounds them to fp32 when it packs)."""
    f8 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)   # noqa: E731  the fp32 tensors it reads
    s = f8(g) / np.sqrt(f8(var) + 1e-5)
    wf = f8(w) * s.reshape((-1,) + (1,) * (np.ndim(w) - 1))
    bf = (f8(bias) - f8(mean)) * s + f8(beta)
    return wf, bf


def exact_fold(w_int: np.ndarray, scale: float, beta: np.ndarray) -> dict:
    """State-dict entries {weight, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var} of one
    conv + BatchNorm whose folded fp32 weights are exactly ``w_int * scale`` and whose folded bias is exactly
    ``beta`` -- asserted here, so no test rests on the fold being merely close."""
    cout = w_int.shape[0]
    w = np.asarray(w_int, dtype=np.float32)
    assert np.array_equal(w.astype(np.float64), np.asarray(w_int, dtype=np.float64)), "weights not fp32 integers"
    ent = dict(weight=w, bias=np.zeros(cout, np.float32), g=np.full(cout, scale, np.float32),
               beta=np.asarray(beta, dtype=np.float32), mean=np.zeros(cout, np.float32),
               var=np.full(cout, RUNNING_VAR, np.float32))
    wf, bf = fold_f64(ent["weight"], ent["bias"], ent["g"], ent["beta"], ent["mean"], ent["var"])
    want_w = np.asarray(w_int, dtype=np.float64) * float(scale)
    assert np.array_equal(wf.astype(np.float32), want_w.astype(np.float32)) and \
        np.array_equal(want_w.astype(np.float32).astype(np.float64), want_w), "BatchNorm fold is not exact (weights)"
    assert np.array_equal(bf.astype(np.float32).astype(np.float64), np.asarray(beta, dtype=np.float64)), \
        "BatchNorm fold is not exact (bias)"
    return ent


def _put_conv_bn(sd: dict, block: str, idx: int, ent: dict) -> None:
    sd[f"{block}.net.{idx}.weight"] = ent["weight"]
    sd[f"{block}.net.{idx}.bias"] = ent["bias"]
    sd[f"{block}.net.{idx + 1}.weight"] = ent["g"]
    sd[f"{block}.net.{idx + 1}.bias"] = ent["beta"]
    sd[f"{block}.net.{idx + 1}.running_mean"] = ent["mean"]
    sd[f"{block}.net.{idx + 1}.running_var"] = ent["var"]
    sd[f"{block}.net.{idx + 1}.num_batches_tracked"] = np.array(0, dtype=np.int64)


def _ordered(sd: dict, n_channels: int, n_classes: int = 3) -> "OrderedDict[str, np.ndarray]":
    out = OrderedDict()
    for key, shape in syn.unet_shapes(n_channels, n_classes):
        assert tuple(sd[key].shape) == tuple(shape), key
        out[key] = sd[key]
    assert len(out) == len(sd)
    return out


# ------------------------------------------------------------------------------------------------ section 1
def _routing_conv(rng, cout: int, cin: int) -> np.ndarray:
    """[cout, cin, 3, 3]: one +1 per output channel at a random (cin, ky, kx); every second channel also
    one -1 at another position."""
    k = cin * 9
    w = np.zeros((cout, k), np.float32)
    pos = rng.integers(0, k, cout)
    neg = (pos + rng.integers(1, k, cout)) % k
    rows = np.arange(cout)
    w[rows, pos] = 1.0
    w[rows[1::2], neg[1::2]] = -1.0
    return w.reshape(cout, cin, 3, 3)


def _conv_relu64(x, w, beta, scale=1.0):
    y = F.conv2d(x, torch.from_numpy(np.asarray(w, dtype=np.float64)), padding=w.shape[-1] // 2)
    return F.relu(y * scale + torch.from_numpy(np.asarray(beta, dtype=np.float64)).view(1, -1, 1, 1))


def routing_forward_f64(sd, x: np.ndarray) -> dict:
    """The network in float64 straight from the intended operands (integer weights, BatchNorm taken as
    `+ beta`): independent of the oracle's BatchNorm arithmetic.  Every stored tensor by its
    ``UNet.intermediate`` name (u4..u1: the up-sampled half of each concat; c8a: conv1.0's output)."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float64))
    o = {}

    def dc(name, v, first=None):
        a = _conv_relu64(v, sd[f"{name}.net.0.weight"], sd[f"{name}.net.1.bias"])
        if first is not None:
            o[first] = a
        return _conv_relu64(a, sd[f"{name}.net.3.weight"], sd[f"{name}.net.4.bias"])

    def upc(name, v):
        return F.conv_transpose2d(v, torch.from_numpy(sd[f"{name}.weight"].astype(np.float64)), stride=2)

    with torch.no_grad():
        o["c1"] = dc("down1", t); o["p1"] = F.max_pool2d(o["c1"], 2)
        o["c2"] = dc("down2", o["p1"]); o["p2"] = F.max_pool2d(o["c2"], 2)
        o["c3"] = dc("down3", o["p2"]); o["p3"] = F.max_pool2d(o["c3"], 2)
        o["c4"] = dc("down4", o["p3"]); o["p4"] = F.max_pool2d(o["c4"], 2)
        o["bn"] = dc("bottleneck", o["p4"])
        o["u4"] = upc("up4", o["bn"]); o["c5"] = dc("conv4", torch.cat([o["u4"], o["c4"]], 1))
        o["u3"] = upc("up3", o["c5"]); o["c6"] = dc("conv3", torch.cat([o["u3"], o["c3"]], 1))
        o["u2"] = upc("up2", o["c6"]); o["c7"] = dc("conv2", torch.cat([o["u2"], o["c2"]], 1))
        o["u1"] = upc("up1", o["c7"]); o["c8"] = dc("conv1", torch.cat([o["u1"], o["c1"]], 1), first="c8a")
        o["logits"] = F.conv2d(o["c8"], torch.from_numpy(sd["out_conv.weight"].astype(np.float64)),
                               torch.from_numpy(sd["out_conv.bias"].astype(np.float64)))
    return {k: v.numpy() for k, v in o.items()}


def routing_input(seed: int, n: int, c_in: int, h: int, w: int, bits: int = 4) -> np.ndarray:
    """Integers in [0, 2^bits), fp32 NCHW: [0, 15] by default; 23 bits for the three-term plan's wide run."""
    rng = np.random.default_rng([seed, n, c_in, h, w, 7])
    return rng.integers(0, 2 ** bits, (n, c_in, h, w)).astype(np.float32)


# UNet's default thresholds, padded to four classes as native.Handle pads them
DEFAULT_THRESHOLDS = (0.25, 0.40, 0.30, 0.5)


def logit_cut64(thr: float) -> float:
    """logit(thr) in float64: where sigmoid crosses ``thr`` (the library's unet_logit_cut is the fp32 value below it)."""
    return float(np.log(thr / (1.0 - thr)))


@functools.lru_cache(maxsize=None)
def _routing_body(seed: int, c_in: int):
    """Every layer of a routing network but out_conv, and the generator's state after drawing them (the
    one-hot head goes on drawing from it).  Shared between the class counts and heads of one (seed, c_in)."""
    rng = np.random.default_rng([seed, c_in, 1])
    sd = {}
    for name, (ci, co) in BLOCKS.items():
        ci = c_in if name == "down1" else ci
        for idx, cin in ((0, ci), (3, co)):
            _put_conv_bn(sd, name, idx, exact_fold(_routing_conv(rng, co, cin), 1.0, rng.integers(0, 3, co)))
    for name, ci in (("up4", 1024), ("up3", 512), ("up2", 256), ("up1", 128)):
        co = ci // 2
        w = np.zeros((ci, co, 2, 2), np.float32)
        src = rng.integers(0, ci, (co, 2, 2))
        o, dy, dx = np.meshgrid(np.arange(co), np.arange(2), np.arange(2), indexing="ij")
        w[src, o, dy, dx] = 1.0
        sd[f"{name}.weight"] = w
        sd[f"{name}.bias"] = np.zeros(co, np.float32)
    for v in sd.values():
        v.setflags(write=False)
    return sd, rng.bit_generator.state


def _dense_head_weights(seed: int, c_in: int, n_classes: int) -> np.ndarray:
    """[n_classes, 64] in {-1, 0, +1}: every channel nonzero in at least one class, the class rows pairwise
    different, each with both signs.  Its own generator, so the one-hot networks' draws stay what they were."""
    rng = np.random.default_rng([seed, c_in, n_classes, 11])
    while True:
        w = rng.integers(-1, 2, (n_classes, 64))
        dead = np.flatnonzero(~(w != 0).any(axis=0))
        w[rng.integers(0, n_classes, dead.size), dead] = rng.choice([-1, 1], dead.size)
        if all((r > 0).any() and (r < 0).any() for r in w) and len({r.tobytes() for r in w}) == n_classes:
            return w.astype(np.float32)


def routing_state_dict(seed: int, c_in: int, n_classes: int = 3, head: str = "onehot",
                       thresholds=None) -> "OrderedDict[str, np.ndarray]":
    """A UNet state_dict that only routes and adds small integers (module docstring).  BatchNorm is the
    identity of ``exact_fold`` with an integer beta in [0, 2]; ConvTranspose has one +1 per (cout, dy, dx)
    and bias 0.  out_conv, ``head`` = "onehot": one +1 per class and a negative integer bias, chosen from the
    float64 run of a 32 x 32 probe input so that each class's logits straddle its cut.  ``head`` = "dense":
    weights in {-1, 0, +1} over all 64 channels (_dense_head_weights), so that every K slot of the head's dot
    carries a term, and per class the integer bias that puts 30 .. 70 % of the probe's logits above the class's
    cut -- that of ``thresholds`` (a tuple of at least n_classes probabilities; default: the model's).  The
    returned arrays are shared (cached): treat them as read-only."""
    assert head in ("onehot", "dense") and 1 <= n_classes <= 4
    thr = None
    if head == "dense":   # the one-hot head does not read them
        thr = tuple(float(t) for t in (DEFAULT_THRESHOLDS if thresholds is None else thresholds))[:n_classes]
        assert len(thr) == n_classes
    return _routing_state_dict(seed, c_in, n_classes, head, thr)


@functools.lru_cache(maxsize=None)
def _routing_state_dict(seed, c_in, n_classes, head, thr):
    body, state = _routing_body(seed, c_in)
    sd = dict(body)
    # out_conv: placeholder, then the probe picks channel and bias
    sd["out_conv.weight"] = np.zeros((n_classes, 64, 1, 1), np.float32)
    sd["out_conv.bias"] = np.zeros(n_classes, np.float32)
    c8 = routing_forward_f64(sd, routing_input(seed, 1, c_in, 32, 32))["c8"][0].reshape(64, -1)
    if head == "dense":
        w = _dense_head_weights(seed, c_in, n_classes)
        s = w.astype(np.float64) @ c8
        for k in range(n_classes):
            first = int(np.floor(logit_cut64(thr[k]))) + 1        # the smallest integer logit above the cut
            levels = [t for t in np.unique(s[k]).astype(np.int64) if 0.3 <= (s[k] >= t).mean() <= 0.7]
            assert levels, "routing net: a dense head row whose probe sums do not straddle any level"
            sd["out_conv.bias"][k] = float(first - levels[len(levels) // 2])   # s >= level  <=>  logit >= first
            share = float((s[k] + sd["out_conv.bias"][k] > logit_cut64(thr[k])).mean())
            assert 0.3 <= share <= 0.7, (k, share)
        sd["out_conv.weight"][:] = w.reshape(n_classes, 64, 1, 1)
    else:
        rng = np.random.default_rng()
        rng.bit_generator.state = state
        # a channel and an integer level t >= 1 that 30 .. 70 % of the channel's probe pixels reach; the logit
        # c8 - t is then >= 0 (above the cuts -0.41 and -0.85) on that share, and c8 - t - 1 >= -1 (above -1.10)
        picks = []
        for c in rng.permutation(64):
            levels = [t for t in range(1, int(c8[c].max()) + 1) if 0.3 <= (c8[c] >= t).mean() <= 0.7]
            if levels:
                picks.append((int(c), levels[len(levels) // 2]))
        assert len(picks) >= max(3, n_classes), "routing net: conv1.3 has too few lively channels for the head"
        for k, (c, t) in enumerate(picks[:n_classes]):
            sd["out_conv.weight"][k, c, 0, 0] = 1.0
            sd["out_conv.bias"][k] = -float(t + 1 if k == 0 else t)
        assert np.all(sd["out_conv.bias"] < 0)
    out = _ordered(sd, c_in, n_classes)
    for v in out.values():
        v.setflags(write=False)
    return out


# One wide-WEIGHT layer per routing network (fp32 plans only): the layer's +-1 weights become +-W.  Each kind
# is (input bits, weight bits, terms every W must have):
#   b18: inputs in [0, 3] (activations stay below 32) x 18-bit W with nonzero mid AND lo: hi.hi, hi.mid, hi.lo
#   c10: 10-bit inputs x 10-bit W with a nonzero mid: hi.hi, hi.mid, mid.hi, mid.mid
# The layers: both convs of down4 (the split-once kernel), conv1.3 (the 16x32 tile with the head) and two
# ConvTranspose layers (weights split on the fly at large batch, pre-split at N <= 4).  Products and sums of the
# layer stay below 2^24 (asserted on the CPU); every later layer routes the wide results with +-1.
WIDE_W_KINDS = OrderedDict([("b18", (2, 18, 2)), ("c10", (10, 10, 1))])
WIDE_W_LAYERS = ["down4.net.0", "down4.net.3", "conv1.net.3", "up4", "up1"]


def _wide_weight_values(rng, count: int, wbits: int, terms: int) -> np.ndarray:
    """``count`` integers in [2^(wbits-1), 2^wbits) whose three-term split has a nonzero mid (terms >= 1)
    and a nonzero lo (terms >= 2)."""
    out = np.empty(0, np.float32)
    while out.size < count:
        v = rng.integers(2 ** (wbits - 1), 2 ** wbits, 4 * count).astype(np.float32)
        _, mid, lo = split3(v)
        out = np.concatenate([out, v[(mid != 0) & ((lo != 0) | (terms < 2))]])
    return out[:count]


@functools.lru_cache(maxsize=None)
def routing_state_dict_wide_w(seed: int, c_in: int, layer: str, kind: str) -> "OrderedDict[str, np.ndarray]":
    """``routing_state_dict(seed, c_in)`` with the nonzero weights of ``layer`` scaled to wide integers."""
    _, wbits, terms = WIDE_W_KINDS[kind]
    base = routing_state_dict(seed, c_in)
    key = f"{layer}.weight"
    rng = np.random.default_rng([seed, c_in, wbits, WIDE_W_LAYERS.index(layer)])
    w = np.array(base[key])
    nz = w != 0
    w[nz] = np.sign(w[nz]) * _wide_weight_values(rng, int(nz.sum()), wbits, terms)
    if ".net." in layer:   # through the BatchNorm fold: still exact (asserted)
        blk, _, idx = layer.partition(".net.")
        w = exact_fold(w, 1.0, base[f"{blk}.net.{int(idx) + 1}.bias"])["weight"]
    w.setflags(write=False)
    out = OrderedDict(base)
    out[key] = w
    return out


def wide_layer_terms(sd, layer: str, src: np.ndarray):
    """The wide layer under the three-term split, in float64, on its input ``src`` (NCHW): (largest
    sum |w||x| over outputs, {(i, j): any nonzero product a_i w_j} for the kept i + j <= 2, largest |dropped
    product|), i the activation's term and j the weight's (0 = hi, 1 = mid, 2 = lo)."""
    w = np.asarray(sd[f"{layer}.weight"])
    op = (lambda a, b: F.conv_transpose2d(a, b, stride=2)) if layer.startswith("up") else \
        (lambda a, b: F.conv2d(a, b, padding=1))
    ta = [torch.from_numpy(np.abs(t).astype(np.float64)) for t in split3(src)]
    tw = [torch.from_numpy(np.abs(t).astype(np.float64)) for t in split3(w)]
    used, dropped = {}, 0.0
    with torch.no_grad():
        worst = float(op(torch.from_numpy(np.abs(src).astype(np.float64)),
                         torch.from_numpy(np.abs(w).astype(np.float64))).max())
        for i in range(3):
            for j in range(3):
                mag = float(op(ta[i], tw[j]).max())
                if i + j <= 2:
                    used[(i, j)] = mag > 0
                else:
                    dropped = max(dropped, mag)
    return worst, used, dropped


@functools.lru_cache(maxsize=None)
def routing_reference(seed: int, c_in: int, n: int, h: int, w: int, bits: int = 4, wide_w=None,
                      n_classes: int = 3, head: str = "onehot", thresholds=None, mirror: bool = False):
    """(x, ref): the input and the fp32 oracle's logits and intermediates by ``UNet.intermediate`` name, in
    forward order (u4..u1 and c8a: the oracle's own ops applied to the oracle's own tensors).  ``wide_w`` =
    (layer, kind): on ``routing_state_dict_wide_w``; ``n_classes``, ``head``, ``thresholds``: those of
    ``routing_state_dict``; ``mirror``: the input flipped left to right.  Cached and shared between tests:
    read-only."""
    if wide_w is None:
        sd = routing_state_dict(seed, c_in, n_classes, head, thresholds)
    else:
        assert n_classes == 3 and head == "onehot"
        sd = routing_state_dict_wide_w(seed, c_in, *wide_w)
    x = routing_input(seed, n, c_in, h, w, bits)
    if mirror:
        x = np.ascontiguousarray(x[..., ::-1])
    sdt = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    logits, it = orc.unet_forward(sdt, torch.from_numpy(x), return_intermediates=True)
    with torch.no_grad():
        ups = {"u4": orc.up(sdt, "up4", it["bn"]), "u3": orc.up(sdt, "up3", it["c5"]),
               "u2": orc.up(sdt, "up2", it["c6"]), "u1": orc.up(sdt, "up1", it["c7"])}
        u1cat = torch.cat([ups["u1"], it["c1"]], 1)
        c8a = F.relu(F.conv2d(u1cat, sdt["conv1.net.0.weight"], padding=1) + sdt["conv1.net.1.bias"].view(1, -1, 1, 1))
    ref = OrderedDict()
    for k in FORWARD_ORDER[:-1]:
        src = ups[k] if k in ups else c8a if k == "c8a" else it[k]
        ref[k] = src.numpy()
    ref["logits"] = logits.numpy()
    x.setflags(write=False)
    for v in ref.values():
        v.setflags(write=False)
    return x, ref


def oracle_stored(sd, x: np.ndarray) -> "OrderedDict[str, np.ndarray]":
    """The fp32 oracle's logits and every tensor a forward stores but c8a, by ``UNet.intermediate`` name, for ANY
    weights (conv1.0's BatchNorm is not the identity there, so c8a is left to the routing networks): what a
    tolerance test of real-valued weights compares the stored intermediates with."""
    sdt = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    logits, it = orc.unet_forward(sdt, torch.from_numpy(np.array(x)), return_intermediates=True)
    with torch.no_grad():
        ups = {"u4": orc.up(sdt, "up4", it["bn"]), "u3": orc.up(sdt, "up3", it["c5"]),
               "u2": orc.up(sdt, "up2", it["c6"]), "u1": orc.up(sdt, "up1", it["c7"])}
    ref = OrderedDict((k, (ups[k] if k in ups else it[k]).numpy()) for k in FORWARD_ORDER[:-1] if k != "c8a")
    ref["logits"] = logits.numpy()
    return ref


# (seed, c_in, n, h, w) of the routing tests: the minimum size (1-pixel bottleneck; N = 1 takes the small-batch
# split-K plan, N = 6 the large-batch plan with partial tiles at every level), a ragged size on three seeds, the
# size forced kernel configurations run at, and full-size pages (persistent walkers and rings wrap)
ROUTING_SMALL = [(0, 3, 1, 16, 16), (1, 1, 1, 16, 16), (2, 3, 6, 16, 112), (3, 1, 6, 16, 112)]
ROUTING_RAGGED = [(4, 3, 3, 48, 80), (5, 1, 3, 48, 80), (6, 3, 3, 48, 80)]
ROUTING_FORCED = (8, 3, 2, 64, 64)
ROUTING_LARGE = [(7, 3, 2, 512, 512)]
# the same networks on 23-bit inputs (fp32 plans only): every layer of the whole forward -- the split-once and
# conv1.3 kernels of the three-term plan and its ConvTranspose, which the stand-alone blocks do not run -- then
# carries activations with nonzero hi, mid and lo terms against +-1 weights; a - b + beta stays below 2^24
ROUTING_WIDE = [(4, 3, 3, 48, 80), (2, 3, 6, 16, 112)]
WIDE_BITS = 23
# the class-count tests (tests/test_classes_gpu.py), dense head, 1 / 2 / 4 (and 3) classes at non-default thresholds:
# the small-batch plan with every tile partial (masks packed per byte); ragged with W % 32 != 0; W % 32 == 0 (the
# 16 x 32-tile kernels pack a dword per class and row); above the small-batch limit, several such tiles per row
ROUTING_CLASSES = [(9, 3, 1, 16, 16), (10, 1, 3, 48, 80), (11, 3, 2, 64, 64), (12, 3, 5, 32, 96)]
CLASS_THRESHOLDS = (0.35, 0.5, 0.1, 0.9)

# tensors a forward stores, in forward order, and the launch (include/unet_mi355x.h order) that writes each
FORWARD_ORDER = ["c1", "p1", "c2", "p2", "c3", "p3", "c4", "p4", "bn", "u4", "u3", "u2", "c7", "u1", "c8a", "logits"]
LAUNCH_OF = {"c1": 1, "p1": 1, "c2": 3, "p2": 3, "c3": 5, "p3": 5, "c4": 7, "p4": 7, "bn": 9, "u4": 10, "u3": 13,
             "u2": 16, "c7": 18, "u1": 19, "c8a": 20, "logits": 21}
# the 3x3 layers in launch order: (state_dict block, conv index) of UNET_MI355X_CFG's layer indices 0..16 + head
CONV_LAYERS = [(b, i) for b in ("down1", "down2", "down3", "down4", "bottleneck", "conv4", "conv3", "conv2", "conv1")
               for i in (0, 3)]


def describe_mismatch(name: str, got: np.ndarray, want: np.ndarray, label: str, limit: int = 6) -> str:
    """'<tensor>: <count> of <size> differ; (n, c, y, x) got/want ...; launch <label>'."""
    bad = np.argwhere(got != want)
    head = "; ".join(f"{tuple(int(i) for i in p)} got {got[tuple(p)]!r} want {want[tuple(p)]!r}" for p in bad[:limit])
    return f"{name}: {len(bad)} of {got.size} elements differ; first (n, c, y, x): {head}; launch: {label}"


def first_stored_mismatch(model, logits: np.ndarray, ref: dict, labels: list):
    """The logits and every tensor the model's last forward stored (``UNet.intermediate``) against ``ref``
    (routing_reference), bitwise, in forward order: None, or describe_mismatch of the first wrong tensor with the
    kernel that wrote it.  With up1 fused into conv2.3 (an empty label 19) c7 is never stored: fetching it must
    raise."""
    import pytest
    fused = labels[19] == ""
    got = {}
    for k in FORWARD_ORDER[:-1]:
        if k == "c7" and fused:
            with pytest.raises(RuntimeError, match="not stored"):
                model.intermediate(k)
            continue
        got[k] = model.intermediate(k).cpu().numpy().reshape(ref[k].shape)
    got["logits"] = np.asarray(logits)
    for k in FORWARD_ORDER:
        if k in got and not np.array_equal(got[k], ref[k]):
            launch = 18 if (k == "u1" and fused) else LAUNCH_OF[k]
            return describe_mismatch(k, got[k], ref[k], labels[launch])
    return None


def np_boxes(masks: np.ndarray) -> np.ndarray:
    """[N, C, H, W] bool -> int32 [N, C, 4] (x_min, y_min, x_max, y_max), -1s for an empty mask."""
    out = np.full(masks.shape[:2] + (4,), -1, dtype=np.int32)
    for i in range(masks.shape[0]):
        for c in range(masks.shape[1]):
            ys, xs = np.where(masks[i, c])
            if len(xs):
                out[i, c] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def reference_masks(logits: np.ndarray, thresholds) -> np.ndarray:
    """[N, C, H, W] logits -> bool masks, the oracle's sigmoid > thresholds[c] in fp32."""
    return np.stack([np.stack(list(orc.masks_from_logits(np.array(lg), thresholds).values())) for lg in logits])


# The history-independence tests (tests/test_history_cpu.py, tests/test_history_gpu.py): one handle, reserved once at
# HISTORY_RESERVE (n, h, w), runs HISTORY_STEPS in this order -- the large-batch and the small-batch (split-K) plan
# alternating, N = 4 | 5 on either side of the small-batch limit, a 1-pixel bottleneck, ragged tiles at every level,
# W % 32 both ways -- so that every forward's buffers lie over what a forward of another shape left there.
HISTORY_RESERVE = (6, 64, 128)
HISTORY_STEPS = [(6, 16, 112), (1, 16, 16), (3, 48, 80), (4, 32, 32), (5, 16, 16), (1, 48, 80), (2, 64, 64)]
HISTORY_NETS = [(4, 3), (5, 1)]   # (seed, c_in) of the routing networks
HISTORY_GRAPHS = [(1, 16, 16), (3, 48, 80)]   # captured shapes; HISTORY_STEPS[0] runs eagerly between their replays
HISTORY_SPLIT = (0, 3, 1, 16, 16)   # the forced two-slice split-K case (ROUTING_SMALL[0])
HISTORY_FILL = 0xFF   # a NaN in every float format, all-ones mask bits, -1 as an integer


def history_block_reserve(name: str):
    """(n, h, w) a stand-alone block's workspace is reserved at before it runs dense_block(name)."""
    h, w = BLOCK_SIZE[name]
    return BLOCK_N + 2, 2 * h + 3, 2 * w + 1


def check_routing_model(m, case, dtype: str, tag: str = "", bits: int = 4, wide_w=None, before=None,
                        every_box_path: bool = False) -> list:
    """One routing model ``m`` (already holding the case's weights, on its device), one input: logits and every
    stored intermediate, masks (u8 and packed) and boxes, all bitwise against the oracle.  ``before`` (optional)
    is called in front of every forward-type call -- never between a forward and the ``UNet.intermediate``
    fetches that read its workspace.  ``every_box_path``: also forward_boxes with masks=None (the masks then live
    in the workspace) and masks="bits".  Returns the launch labels of the forward."""
    import pytest
    seed, c_in, n, h, w = case
    before = before or (lambda: None)
    dev = next(m.parameters()).device
    x, ref = routing_reference(seed, c_in, n, h, w, bits, wide_w)
    xd = torch.from_numpy(np.array(x)).to(dev)
    before()
    with torch.no_grad():
        logits = m(xd)
    torch.cuda.synchronize()
    labels = m.native_handle(dev).launch_labels_at(n, h, w)
    # logits and every stored tensor (with up1 fused into conv2.3, EPI_UPFUSE, c7 is never stored)
    bad = first_stored_mismatch(m, logits.cpu().numpy(), ref, labels)
    if bad:
        pytest.fail(f"{dtype} {case} {tag}: {bad}")
    ref_masks = np.stack([np.stack([orc.masks_from_logits(np.array(ref["logits"][i]))[f] for f in orc.FIELDS])
                          for i in range(n)])
    with torch.no_grad():
        before()
        masks, lg2 = m.forward_masks(xd, with_logits=True)
        before()
        packed = m.forward_masks(xd, packed=True)
        before()
        bmasks, boxes = m.forward_boxes(xd, masks="u8")
    assert np.array_equal(lg2.cpu().numpy(), ref["logits"]), "logits of forward_masks"
    for name, mk in (("u8", masks.cpu().numpy()), ("boxes' u8", bmasks.cpu().numpy()),
                     ("packed", np.unpackbits(packed.cpu().numpy(), axis=-1, bitorder="little"))):
        if not np.array_equal(mk.astype(bool), ref_masks):
            pytest.fail(f"{dtype} {case} {tag}: " + describe_mismatch(
                f"{name} masks", mk.astype(bool), ref_masks, labels[21]))
    assert np.array_equal(boxes.cpu().numpy(), np_boxes(ref_masks)), (boxes.cpu().numpy(), np_boxes(ref_masks))
    if every_box_path:
        with torch.no_grad():
            before()
            only = m.forward_boxes(xd, masks=None)
            before()
            bits_m, bits_b = m.forward_boxes(xd, masks="bits")
        assert np.array_equal(only.cpu().numpy(), np_boxes(ref_masks)), \
            ("boxes with the masks in the workspace", only.cpu().numpy(), np_boxes(ref_masks))
        assert np.array_equal(bits_b.cpu().numpy(), np_boxes(ref_masks)), \
            ("boxes with packed masks", bits_b.cpu().numpy(), np_boxes(ref_masks))
        got = np.unpackbits(bits_m.cpu().numpy(), axis=-1, bitorder="little").astype(bool)
        if not np.array_equal(got, ref_masks):
            pytest.fail(f"{dtype} {case} {tag}: " + describe_mismatch("boxes' packed masks", got, ref_masks, labels[21]))
    return labels


# ------------------------------------------------------------------------------------------------ section 2
BLOCK_SIZE ={"down1": (19, 37), "down2": (19, 37), "conv2": (19, 37), "conv1": (19, 37),
              "down3": (9, 21), "down4": (9, 21), "conv3": (9, 21), "bottleneck": (5, 7), "conv4": (5, 7)}
BLOCK_N = 2


class ExactBlock:
    """One DoubleConv case: state_dict ``sd`` (14 keys, 'net.*'), input ``x``, the exact float64 ``mid``
    (first conv + ReLU) and ``out``, the intended integer weights ``w`` and power-of-two scales ``scale`` and
    biases ``beta`` of both convs, and the operand quanta of each conv (``qx``, ``qw``)."""

    def __init__(self, name, cin, cout, x, w, scale, beta):
        self.name, self.cin, self.cout, self.x, self.w, self.scale, self.beta = name, cin, cout, x, w, scale, beta
        sd = {}
        for i, idx in enumerate((0, 3)):
            _put_conv_bn(sd, "b", idx, exact_fold(w[i], scale[i], beta[i]))
        self.sd = OrderedDict((k[2:], v) for k, v in sd.items())
        t = torch.from_numpy(x.astype(np.float64))
        with torch.no_grad():
            mid = _conv_relu64(t, w[0], beta[0], scale[0])
            out = _conv_relu64(mid, w[1], beta[1], scale[1])
        self.mid, self.out = mid.numpy(), out.numpy()

    def bound(self, i: int):
        """(max over outputs of sum |w||x| + |b|, 2^24 * qx * qw) of conv i, with qx and qw the largest powers
        of two dividing every activation and every folded weight (and the bias a multiple of qx * qw)."""
        src = self.x.astype(np.float64) if i == 0 else self.mid
        wf = np.abs(self.w[i].astype(np.float64)) * self.scale[i]
        with torch.no_grad():
            s = F.conv2d(torch.from_numpy(np.abs(src)), torch.from_numpy(wf), padding=1).numpy()
        worst = float((s + np.abs(self.beta[i].astype(np.float64)).reshape(1, -1, 1, 1)).max())
        qx, qw = quantum(src), quantum(wf)
        assert np.all(np.mod(self.beta[i].astype(np.float64), qx * qw) == 0), "bias is not a multiple of qx * qw"
        return worst, 2.0 ** 24 * qx * qw

    def expected(self, dtype: str) -> np.ndarray:
        """fp32 plans: relu(exact).  16-bit plans: unet_block_forward stores the last layer in the plan's
        16-bit type (round to nearest even) and widens it to fp32: RNE_T(relu(exact))."""
        out = self.out.astype(np.float32)
        assert np.array_equal(out.astype(np.float64), self.out), "block output is not an fp32 value"
        return out if dtype in ("fp32", "fp32_exact") else RNE[dtype](out)


def block_expected_rounded(blk: ExactBlock, dtype: str):
    """(mid, out, largest sum |w||x| + |b|) of a stand-alone DoubleConv on operands that round, in a 16-bit plan
    T: the host packs RNE_T(fp32(folded weights)) (put_elem), each conv's fp32 accumulator + fp32 bias goes
    through ReLU and is stored as T (round to nearest even), and unet_block_forward widens the last buffer to
    fp32.  In float64, with every value a conversion receives asserted to be an fp32 value within fp16's range."""
    v = torch.from_numpy(blk.x.astype(np.float64))
    assert np.array_equal(RNE[dtype](blk.x), blk.x)
    outs, worst = [], 0.0
    with torch.no_grad():
        for i in range(2):
            wf = (blk.w[i].astype(np.float64) * blk.scale[i]).astype(np.float32)
            w = torch.from_numpy(RNE[dtype](wf).astype(np.float64))
            b = torch.from_numpy(blk.beta[i].astype(np.float64))
            worst = max(worst, float(F.conv2d(v.abs(), w.abs(), b.abs(), padding=1).max()))
            a = F.relu(F.conv2d(v, w, b, padding=1)).numpy()
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.abs(a).max() <= F16_MAX
            outs.append(RNE[dtype](a.astype(np.float32)))
            v = torch.from_numpy(outs[-1].astype(np.float64))
    return outs[0], outs[1], worst


def quantum(a: np.ndarray) -> float:
    """The largest power of two that divides every (dyadic) element of ``a`` (1.0 for all zeros)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[a != 0]
    if a.size == 0:
        return 1.0
    q = 2.0 ** 30
    while np.any(np.mod(a, q) != 0):
        q /= 2.0
        assert q > 2.0 ** -40, "operands are not dyadic"
    return q


def _dense_weights(rng, cout, cin, p_nonzero):
    u = rng.random((cout, cin, 3, 3))
    return np.where(u < p_nonzero / 2, -1.0, np.where(u < p_nonzero, 1.0, 0.0)).astype(np.float32)


def representable(a: np.ndarray) -> bool:
    """Every element exactly representable in fp32, bf16 and fp16."""
    f = a.astype(np.float32)
    return bool(np.array_equal(f.astype(np.float64), a) and np.array_equal(bf16_rne(f), f) and
                np.array_equal(f16_rne(f), f))


@functools.lru_cache(maxsize=None)
def dense_block(name: str, seed: int = 0) -> ExactBlock:
    """Dense exact DoubleConv: inputs in [0, 3], i.i.d. weights in {-1, 0, 1} at EVERY K position of every
    output channel, integer beta in [-4, 4], folded scale 2^-3 on the first conv (1 on down1.0) and 2^-6 on the
    second.

    The first conv's ReLU output must be a bf16 and an fp16 value, so that it does not matter whether a path
    stores it or keeps it in registers.  A power-of-two scale cannot achieve that (it does not change how
    many significant bits the integer sum needs), so the free parameter is the share of nonzero weights of
    the FIRST conv: 2/3 (uniform over {-1, 0, 1}), halved until every mid value is representable -- the sum
    over K = 9 Cin terms then stays below 2^8 quanta.  Every (cin, tap) position still carries a nonzero
    weight for many output channels (asserted on the CPU).  The second conv keeps 2/3."""
    cin, cout = BLOCKS[name]
    h, w = BLOCK_SIZE[name]
    rng = np.random.default_rng([seed, cin, cout, 2])
    x = rng.integers(0, 4, (BLOCK_N, cin, h, w)).astype(np.float32)
    beta = [rng.integers(-4, 5, cout), rng.integers(-4, 5, cout)]
    scale = [1.0 if name == "down1" else 2.0 ** -3, 2.0 ** -6]
    w1 = _dense_weights(rng, cout, cout, 2 / 3)
    p = 2 / 3
    while True:
        blk = ExactBlock(name, cin, cout, x, [_dense_weights(rng, cout, cin, p), w1], scale, beta)
        if representable(blk.mid):
            blk.p_first = p
            return blk
        p /= 2
        assert p > 1e-3, name


# wide-operand cases of the three-term fp32 plan: (activation bits, weight bits, nonzeros per output channel)
#   a, b, c: the issue's cases.  A 17-bit integer never has a lo term (hi takes 8 bits and the signed mid the
#   other 9), so a_lo / b_lo add 20-bit operands against +-1: the lo.hi and hi.lo products.
WIDE_CASES = OrderedDict([("a", (17, 4, 8)), ("b", (4, 17, 8)), ("c", (10, 10, 8)),
                          ("a_lo", (20, 1, 8)), ("b_lo", (1, 20, 8))])
WIDE_BLOCKS = ("down2", "down4", "conv1")
WIDE_R12 = (2, 12, 8)     # the 16-bit plans' weight-rounding case "r12": not a three-term case, so not in WIDE_CASES
WIDE_SIZE = {"down2": (19, 37), "down4": (9, 21), "conv1": (19, 37)}


@functools.lru_cache(maxsize=None)
def wide_block(name: str, case: str, seed: int = 0) -> ExactBlock:
    """First conv: activations below 2^abits, ``nnz`` weights per output channel of magnitude below 2^wbits
    and random sign at random (cin, tap) positions, integer beta in [-4, 4], scale 1 (case "r12", for the 16-bit
    plans: WIDE_R12, weights r12_values x 2^-8 -- see R12_LAYERS -- expected by ``expected_rounded``).  Second conv: the
    centre-tap identity (+1 at (o, o, 1, 1)), beta 0.  nnz * 2^abits * 2^wbits + 4 < 2^24 in every case."""
    abits, wbits, nnz = WIDE_R12 if case == "r12" else WIDE_CASES[case]
    cin, cout = BLOCKS[name]
    h, w = WIDE_SIZE[name]
    rng = np.random.default_rng([seed, cin, cout, abits, wbits])
    x = rng.integers(0, 2 ** abits, (BLOCK_N, cin, h, w)).astype(np.float32)
    k = cin * 9
    w0 = np.zeros((cout, k), np.float32)
    for o in range(cout):
        pos = rng.choice(k, nnz, replace=False)
        mag = r12_values(rng, nnz) if case == "r12" else rng.integers(1, 2 ** wbits, nnz)
        w0[o, pos] = mag * rng.choice([-1.0, 1.0], nnz)
    ident = np.zeros((cout, cout, 3, 3), np.float32)
    ident[np.arange(cout), np.arange(cout), 1, 1] = 1.0
    return ExactBlock(name, cin, cout, x, [w0.reshape(cout, cin, 3, 3), ident], [R12_SCALE if case == "r12" else 1.0, 1.0],
                      [rng.integers(-4, 5, cout), np.zeros(cout, np.int64)])


def six_and_dropped(blk: ExactBlock):
    """The first conv of ``blk`` under the three-term split, in float64: (sum of the six kept products i + j
    <= 2, per-term flags {(i, j): any nonzero product}, largest |dropped product|) with i the activation's
    term and j the weight's (0 = hi, 1 = mid, 2 = lo)."""
    tx = [torch.from_numpy(t.astype(np.float64)) for t in split3(blk.x)]
    tw = [torch.from_numpy(t.astype(np.float64)) for t in split3(blk.w[0] * np.float32(blk.scale[0]))]
    kept, used, dropped = 0.0, {}, 0.0
    with torch.no_grad():
        for i in range(3):
            for j in range(3):
                mag = float(F.conv2d(tx[i].abs(), tw[j].abs(), padding=1).max())
                if i + j <= 2:
                    kept = kept + F.conv2d(tx[i], tw[j], padding=1)
                    used[(i, j)] = mag > 0
                else:
                    dropped = max(dropped, mag)
    return kept.numpy(), used, dropped


# ------------------------------------------------------------------------------------------------ section 3
# Rounding networks: the routing body on operands that the 16-bit plans must ROUND when they store them.
PLAN_TYPES = {"bf16": ("bf16",) * 6, "fp16": ("fp16",) * 6,
              "mixed": ("fp16", "fp16", "bf16", "bf16", "bf16", "bf16"),   # csrc/unet_capi.cpp level_dtype
              "fp32": (None,) * 6, "fp32_exact": (None,) * 6}
SIG_BITS = {"bf16": 8, "fp16": 11}
F16_MAX = 65504.0
# every conversion to a storage type in forward order: (name, level whose type it takes)
ROUNDING_STORES = [("x", 0), ("c1a", 0), ("c1", 0), ("p1", 1), ("c2a", 1), ("c2", 1), ("p2", 2), ("c3a", 2), ("c3", 2),
                   ("p3", 3), ("c4a", 3), ("c4", 3), ("p4", 4), ("bna", 4), ("bn", 4), ("u4", 3), ("c5a", 3), ("c5", 3),
                   ("u3", 2), ("c6a", 2), ("c6", 2), ("u2", 1), ("c7a", 1), ("c7", 1), ("u1", 0), ("c8a", 0), ("head", 0)]
STORE_LEVEL = dict(ROUNDING_STORES)


def round_sig(x: np.ndarray, dtype: str, mode: str = "rne") -> np.ndarray:
    """float64 -> ``dtype``'s significand width (8 bits bf16, 11 bits fp16) by plain arithmetic, returned as
    float64.  ``mode``: "rne" (nearest, ties to even), "trunc" (towards zero: a conversion by shift), "away"
    (nearest, ties away from zero).  For values in both types' normal range (asserted: 2^-14 <= |v| <= 65504 or
    0), where "rne" is RNE[dtype] (asserted by tests/test_rounding_cpu.py)."""
    x = np.asarray(x, dtype=np.float64)
    nz = x != 0
    assert np.all(np.abs(x[nz]) >= 2.0 ** -14) and np.all(np.abs(x) <= F16_MAX), "outside the shared normal range"
    _, e = np.frexp(x)                                     # |x| = m 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, e - SIG_BITS[dtype])                 # the spacing of dtype's values in [2^(e-1), 2^e)
    y = x / q
    r = {"rne": np.rint, "trunc": np.trunc, "away": lambda t: np.sign(t) * np.floor(np.abs(t) + 0.5)}[mode](y)
    return np.where(nz, r * q, 0.0)


def is_tie(x: np.ndarray, dtype: str) -> np.ndarray:
    """Elementwise: x lies exactly half way between two neighbouring ``dtype`` values."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    y = x / np.ldexp(1.0, e - SIG_BITS[dtype])
    return y - np.floor(y) == 0.5


@functools.lru_cache(maxsize=None)
def _rounding_body(seed: int, c_in: int):
    """The routing body (_routing_body, its draws untouched) with, from generators of its own: every BatchNorm beta
    + j / 16, j in [0, 16); every ConvTranspose a second nonzero weight, +-1, per (cout, dy, dx) and an integer
    bias in [0, 2]."""
    base, _ = _routing_body(seed, c_in)
    rng = np.random.default_rng([seed, c_in, 13])
    sd = dict(base)
    for name, (_, co) in BLOCKS.items():
        for idx in (0, 3):
            beta = base[f"{name}.net.{idx + 1}.bias"].astype(np.float64) + rng.integers(0, 16, co) / 16.0
            _put_conv_bn(sd, name, idx, exact_fold(base[f"{name}.net.{idx}.weight"], 1.0, beta))
    for name, ci in (("up4", 1024), ("up3", 512), ("up2", 256), ("up1", 128)):
        co = ci // 2
        w = np.array(base[f"{name}.weight"])
        src = w.argmax(axis=0)                                       # [co, 2, 2]: the +1's input channel
        other = (src + rng.integers(1, ci, (co, 2, 2))) % ci
        o, dy, dx = np.meshgrid(np.arange(co), np.arange(2), np.arange(2), indexing="ij")
        w[other, o, dy, dx] = rng.choice([-1.0, 1.0], (co, 2, 2)).astype(np.float32)
        assert np.array_equal((w != 0).sum(axis=0), np.full((co, 2, 2), 2))
        sd[f"{name}.weight"] = w
        sd[f"{name}.bias"] = rng.integers(0, 3, co).astype(np.float32)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def rounding_input(seed: int, n: int, c_in: int, h: int, w: int) -> np.ndarray:
    """k / 16, k uniform in [0, 2^15), fp32 NCHW: 15 significant bits, below 2048."""
    rng = np.random.default_rng([seed, n, c_in, h, w, 17])
    return (rng.integers(0, 2 ** 15, (n, c_in, h, w)) / 16.0).astype(np.float32)


def _head_bias(s: np.ndarray, thr) -> np.ndarray:
    """Per class the integer bias that puts the share of ``s[k] + bias > logit(thr[k])`` nearest one half
    (asserted within 30 .. 70 %); s = the head's dot products on a probe."""
    out = np.zeros(len(thr), np.float32)
    for k, t in enumerate(thr):
        b = float(np.ceil(logit_cut64(t) - np.median(s[k])))
        best = min((b + d for d in range(-2, 3)), key=lambda v: abs(float((s[k] + v > logit_cut64(t)).mean()) - 0.5))
        share = float((s[k] + best > logit_cut64(t)).mean())
        assert 0.3 <= share <= 0.7, (k, share)
        out[k] = best
    return out


@functools.lru_cache(maxsize=None)
def rounding_state_dict(seed: int, c_in: int, n_classes: int = 3) -> "OrderedDict[str, np.ndarray]":
    """A UNet state_dict whose every 16-bit storage point rounds on ``rounding_input``: _rounding_body (+-1 3x3
    weights, exact in every type, so only activations round; dyadic betas through exact_fold; two-term
    ConvTranspose with an integer bias) under the dense {-1, 0, +1} head (_dense_head_weights), whose integer
    biases are chosen, as routing_state_dict does, from the float64 run of a 32 x 32 probe so that each class's
    logits straddle its cut (the model's default thresholds).  Shared (cached): read-only."""
    sd = dict(_rounding_body(seed, c_in))
    w = _dense_head_weights(seed, c_in, n_classes)
    sd["out_conv.weight"] = w.reshape(n_classes, 64, 1, 1)
    sd["out_conv.bias"] = np.zeros(n_classes, np.float32)
    probe = _round_forward(sd, rounding_input(seed, 1, c_in, 32, 32), PLAN_TYPES["fp32"])
    s = w.astype(np.float64) @ probe["head"][0].reshape(64, -1).astype(np.float64)
    sd["out_conv.bias"] = _head_bias(s, DEFAULT_THRESHOLDS[:n_classes])
    out = _ordered(sd, c_in, n_classes)
    for v in out.values():
        v.setflags(write=False)
    return out


# alter = ((store, mode), ...): the reference recomputed with ONE conversion done wrongly -- what the diagnosis
# compares a wrong tensor with, and the negative controls of tests/test_rounding_cpu.py.  Modes: "trunc", "away"
# (round_sig); "other": the other 16-bit type; "double": through bf16 first (a 16-bit split-K partial); "none":
# not rounded at all (an fp32 operand where a 16-bit one is documented); "via_skip" (pooled maps only): the max of
# the ROUNDED skip instead of the fp32 values.
ALTER_MODES = ("trunc", "away", "other", "double", "none")
_WEIGHT_MEMO = {}   # prepared weights of the shared (cached, read-only) state dicts, by array identity


# the first store a layer's weights act on (where an altered weight conversion first shows)
WEIGHT_STORE = {"down4.net.0": "c4a", "down4.net.3": "c4", "conv1.net.3": "head", "up4": "u4", "up1": "u1"}


class _Lazy:
    """A tensor computed when first asked for (a reused prefix of the forward is never computed)."""

    def __init__(self, fn):
        self.fn, self.v = fn, None

    def get(self):
        if self.v is None:
            self.v = self.fn()
        return self.v


def _round_forward(sd, x: np.ndarray, types, alter=(), bound: float = 2.0 ** 20, pre=None,
                   reuse=None) -> "OrderedDict[str, np.ndarray]":
    """The forward in float64 with the library's conversions (rounding_reference's docstring lists them);
    ``types``: the storage type of levels 0..4 (None: fp32, nothing rounds).  Returns every store of
    ROUNDING_STORES and the logits as fp32 arrays (and into ``pre``, a dict, the fp32 values each conversion
    received).  ``reuse``: the unaltered result for the same operands and types -- the stores in front of the
    first altered conversion are taken from it instead of being computed again.  Asserted on the way: every
    value a conversion receives is exactly an fp32 value, none exceeds fp16's largest finite value, and every
    accumulation has sum |w||x| + |b| < ``bound`` (2^20 for operands that are multiples of 2^-4: 24 bits)."""
    alter = dict(alter)
    o = OrderedDict()
    order = [n for n, _ in ROUNDING_STORES]
    first = 0
    if reuse is not None and alter:
        first = min(order.index(k) if k in order else order.index(WEIGHT_STORE[k]) if k in WEIGHT_STORE else len(order)
                    for k in alter)

    def cvt(a: np.ndarray, t, mode="rne"):
        if t is None or mode == "none":
            return a
        if mode in ("rne", "via_skip"):
            return RNE[t](a.astype(np.float32)).astype(np.float64)
        if mode == "other":
            return cvt(a, "fp16" if t == "bf16" else "bf16")
        if mode == "double":
            return cvt(cvt(a, "bf16"), t)
        return round_sig(a, t, mode)

    def store(name: str, lazy: _Lazy) -> _Lazy:
        if order.index(name) < first:
            o[name] = reuse[name]
            return _Lazy(lambda: torch.from_numpy(reuse[name].astype(np.float64)))
        a = lazy.get().numpy()
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{name}: not an fp32 value"
        assert np.abs(a).max() <= F16_MAX, f"{name}: beyond fp16's range"
        r = cvt(a, types[STORE_LEVEL[name]], alter.get(name, "rne"))
        o[name] = r.astype(np.float32)
        if pre is not None:
            pre[name] = a.astype(np.float32)
        return _Lazy(lambda: torch.from_numpy(r))

    def weights(key: str, level: int, fold=None):
        """RNE_T(fp32(folded weight)) -- unet_capi.cpp put_elem -- and the fp32 bias, both as float64."""
        t, mode = types[level], alter.get(key, "rne")
        used = [sd[f"{key}.weight"], sd[f"{key}.bias"]]                    # what the result depends on
        if fold:
            used += [sd[f"{fold[0]}.net.{fold[1] + 1}.{f}"] for f in ("weight", "bias", "running_mean", "running_var")]
        memo = (tuple(id(u) for u in used), t, mode)
        if memo not in _WEIGHT_MEMO:
            if fold is None:
                w, b = sd[f"{key}.weight"].astype(np.float64), sd[f"{key}.bias"].astype(np.float64)
            else:
                blk, idx = fold
                w, b = fold_f64(*(sd[f"{blk}.net.{i}"] for i in (f"{idx}.weight", f"{idx}.bias", f"{idx + 1}.weight",
                                                                 f"{idx + 1}.bias", f"{idx + 1}.running_mean",
                                                                 f"{idx + 1}.running_var")))
            w = w.astype(np.float32).astype(np.float64)
            b = b.astype(np.float32).astype(np.float64)
            red = (0,) if key.startswith("up") else (1, 2, 3)
            wt = torch.from_numpy(cvt(w, t, mode))
            # (weights, bias, the arrays whose ids are the key -- kept alive, so that no id is ever reused --, the
            # largest sum |w| of an output, the largest |bias|)
            _WEIGHT_MEMO[memo] = (wt, torch.from_numpy(b), used, float(wt.abs().sum(dim=red).max()), float(np.abs(b).max()))
        return _WEIGHT_MEMO[memo]

    def exact(v, wsum, bmax):
        worst = wsum * float(v.abs().max()) + bmax
        assert worst < bound, f"accumulation bound: {worst} >= {bound}"

    def conv(v: _Lazy, blk, idx, level) -> _Lazy:
        def run():
            w, b, _, wsum, bmax = weights(f"{blk}.net.{idx}", level, (blk, idx))
            exact(v.get(), wsum, bmax)
            return F.relu(F.conv2d(v.get(), w, b, padding=1))
        return _Lazy(run)

    def dc(blk, v, level, mid, out, pooled=None):
        a = store(mid, conv(v, blk, 0, level))
        y = conv(a, blk, 3, level)                  # fp32 accumulators + bias, ReLU: what the epilogue holds
        s = store(out, y)
        if pooled:                                  # the pooled map: the max of the fp32 values, then ONE conversion
            src = s if alter.get(pooled) == "via_skip" else y
            return s, store(pooled, _Lazy(lambda: F.max_pool2d(src.get(), 2)))
        return s

    def up(key, v, level, out):
        def run():
            w, b, _, wsum, bmax = weights(key, level)
            exact(v.get(), wsum, bmax)
            return F.conv_transpose2d(v.get(), w, b, stride=2)
        return store(out, _Lazy(run))

    def cat(u, c):
        return _Lazy(lambda: torch.cat([u.get(), c.get()], 1))

    with torch.no_grad():
        t = store("x", _Lazy(lambda: torch.from_numpy(np.asarray(x, dtype=np.float64))))
        c1, p1 = dc("down1", t, 0, "c1a", "c1", "p1")
        c2, p2 = dc("down2", p1, 1, "c2a", "c2", "p2")
        c3, p3 = dc("down3", p2, 2, "c3a", "c3", "p3")
        c4, p4 = dc("down4", p3, 3, "c4a", "c4", "p4")
        bn = dc("bottleneck", p4, 4, "bna", "bn")
        c5 = dc("conv4", cat(up("up4", bn, 4, "u4"), c4), 3, "c5a", "c5")
        c6 = dc("conv3", cat(up("up3", c5, 3, "u3"), c3), 2, "c6a", "c6")
        c7 = dc("conv2", cat(up("up2", c6, 2, "u2"), c2), 1, "c7a", "c7")
        hd = dc("conv1", cat(up("up1", c7, 1, "u1"), c1), 0, "c8a", "head").get()
        w, b, _, wsum, bmax = weights("out_conv", 0)
        exact(hd, wsum, bmax)
        lg = F.conv2d(hd, w, b).numpy()
    assert np.array_equal(lg.astype(np.float32).astype(np.float64), lg), "logits: not fp32 values"
    o["logits"] = lg.astype(np.float32)
    return o


# One r12 WEIGHT layer per network (16-bit plans): the weight-side conversions -- the host's put_elem when it packs
# a layer for its level's type, and for out_conv the head kernel's device-side cast of the fp32 weights to HT.  The
# layer's nonzero weights of the integer routing network become +-W with W a 12-bit integer in [2048, 4096): bf16
# keeps 8 of the 12 bits (exact only for multiples of 16, a tie at 8 mod 16), fp16 keeps 11 (every odd W is a tie).
# A quarter of the weights are forced to 8 mod 16 and a quarter to odd values, the rest drawn uniformly.  Inputs are
# integers in [0, 3] (routing_input, 2 bits).  The layer's folded weights are W 2^-8, in [8, 16): a power of two
# changes neither the 12-bit significand nor what a type keeps of it, and the activations behind the layer (up to 40 W
# unscaled: past fp16's 65504 at conv1.3, up4 and up1) stay in range.  Everything is a multiple of 2^-8 and
# sum |w||x| + |b| < 2^16 at every layer (asserted by _round_forward): products and sums below 2^24 quanta.
R12_SCALE = 2.0 ** -8
R12_LAYERS = WIDE_W_LAYERS + ["out_conv"]
R12_INPUT_BITS = 2
R12_MIN_INEXACT, R12_MIN_TIES = 0.25, 0.2     # floors per type, as shares of the layer's nonzero weights


def r12_values(rng, count: int) -> np.ndarray:
    v = rng.integers(2048, 4096, count)
    i = np.arange(count)
    v[i % 4 == 0] = (v[i % 4 == 0] & ~15) | 8
    v[i % 4 == 1] |= 1
    return v.astype(np.float32)


def r12_weight_stats(w: np.ndarray) -> dict:
    """Per 16-bit type: (share of the nonzero weights the conversion changes, share that are exact ties)."""
    v = np.abs(np.asarray(w, np.float64)[np.asarray(w) != 0])
    return {t: (float((round_sig(v, t) != v).mean()), float(is_tie(v, t).mean())) for t in SIG_BITS}


@functools.lru_cache(maxsize=None)
def routing_state_dict_r12(seed: int, c_in: int, layer: str) -> "OrderedDict[str, np.ndarray]":
    """``routing_state_dict(seed, c_in, 3, "dense")`` (the dense head: all 64 channels reach the logits, and
    out_conv itself has 64 weights per class to round; its integer biases re-chosen on a 2-bit 32 x 32 probe)
    with ``layer``'s nonzero weights scaled to r12 values.  The floors R12_MIN_INEXACT and R12_MIN_TIES are
    asserted for both 16-bit types."""
    base = routing_state_dict(seed, c_in, 3, "dense")
    key = f"{layer}.weight"
    rng = np.random.default_rng([seed, c_in, 12, R12_LAYERS.index(layer)])
    w = np.array(base[key])
    nz = w != 0
    w[nz] = np.sign(w[nz]) * r12_values(rng, int(nz.sum()))
    out = OrderedDict(base)
    if ".net." in layer:   # the scale through the BatchNorm fold (gamma = 2^-8): still exact (asserted)
        blk, _, idx = layer.partition(".net.")
        ent = exact_fold(w, R12_SCALE, base[f"{blk}.net.{int(idx) + 1}.bias"])
        w = ent["weight"]
        ent["g"].setflags(write=False)
        out[f"{blk}.net.{int(idx) + 1}.weight"] = ent["g"]
    else:
        w = w * np.float32(R12_SCALE)
    for t, (inexact, ties) in r12_weight_stats(w).items():
        assert inexact >= R12_MIN_INEXACT and ties >= R12_MIN_TIES, (layer, t, inexact, ties)
    w.setflags(write=False)
    out[key] = w
    # the head's integer biases again, from the unrounded float64 run of a 2-bit 32 x 32 probe
    out["out_conv.bias"] = np.zeros(3, np.float32)
    probe = _round_forward(out, routing_input(seed, 1, c_in, 32, 32, R12_INPUT_BITS), PLAN_TYPES["fp32"], (),
                           2.0 ** 24 * R12_SCALE)
    bias = _head_bias(probe["logits"][0].reshape(3, -1).astype(np.float64), DEFAULT_THRESHOLDS[:3])
    bias.setflags(write=False)
    out["out_conv.bias"] = bias
    return out


def _alter_key(alter):
    return tuple(sorted(dict(alter).items()))


@functools.lru_cache(maxsize=None)
def _rounding_reference(seed, c_in, n, h, w, plan, n_classes, r12, alter):
    if r12 is None:
        sd, x = rounding_state_dict(seed, c_in, n_classes), rounding_input(seed, n, c_in, h, w)
        bound = 2.0 ** 20                              # multiples of 2^-4: 24 bits
    else:
        assert n_classes == 3
        sd, x = routing_state_dict_r12(seed, c_in, r12), routing_input(seed, n, c_in, h, w, R12_INPUT_BITS)
        bound = 2.0 ** 24 * R12_SCALE                  # multiples of 2^-8
    types = PLAN_TYPES[plan] if isinstance(plan, str) else tuple(plan)
    pre = {} if not alter else None                    # kept for the true references only
    reuse = _rounding_reference(seed, c_in, n, h, w, plan, n_classes, r12, ())[1] if alter else None
    ref = _round_forward(sd, x, types, alter, bound, pre, reuse)
    x.setflags(write=False)
    for v in list(ref.values()) + list((pre or {}).values()):
        v.setflags(write=False)
    return x, ref, pre


def rounding_reference(seed: int, c_in: int, n: int, h: int, w: int, plan, n_classes: int = 3, r12=None, alter=()):
    """(x, ref): the input and the forward in float64 with RNE_T applied wherever ``plan`` converts fp32 to a
    16-bit type T -- the logits and every tensor of FORWARD_ORDER by its ``UNet.intermediate`` name, and the
    stores nothing can fetch (ROUNDING_STORES), as fp32 arrays.  On ``rounding_state_dict`` and
    ``rounding_input``; ``r12`` = a layer of R12_LAYERS: on ``routing_state_dict_r12`` and 2-bit integer inputs.
    ``plan``: a precision plan, or the five levels' types spelt out (the negative controls flip one);
    ``alter``: see ALTER_MODES.  Cached and shared between tests: read-only.

    T(l) = level_dtype(plan, l) (csrc/unet_capi.cpp): "mixed" is fp16 at levels 0-1 and bf16 at 2-4; the fp32
    plans convert nothing, so theirs is the unrounded chain.  The conversions, read from csrc/:

      x       the network input -> T(0): x_to_px4_kernel (the fused first conv), first_conv_mfma_kernel's B
              fragments (unfused)
      weights every 3x3 and ConvTranspose layer at level l: RNE_T(l)(fp32(folded)) on the host (put_elem); the
              folded biases stay fp32 and join the fp32 accumulator
      mid     a DoubleConv's first ReLU output -> T(l): store64_grouped<TO> (the shared epilogue), the fused
              first conv's LDS tile, splitk_reduce_kernel's store8<TO> under the small-batch plan
      skip    its second ReLU output -> T(l) likewise (TO)
      pooled  max over the 2 x 2 window of the fp32 ReLU values -> T(l + 1) (TQ): ONE conversion of the fp32
              maximum, not a second one of the stored skip (the two differ where T(l) != T(l + 1): p2 of "mixed";
              here the reference follows the code, which rounds each value it stores once)
      u_k     ConvTranspose at level l (operands T(l)): fp32 accumulator + fp32 bias -> T(l - 1), the
              pixel-shuffle store (store64_grouped<TO> in the shared epilogue's EPI_UPSCATTER branch, reached from
              convT_ring_kernel and from the halo family);
              with up1 fused into conv2.3 (EPI_UPFUSE) c7 is cast to T(1) in registers (conv_to_xb) exactly as
              it would have been stored, so u1 has the same bits either way
      head    conv1.3's ReLU output -> HT = T(0) in registers, and out_conv's fp32 weights -> HT on the device
              (head_epilogue); the dot accumulates in fp32 and the fp32 bias is added to it: the logits are
              never rounded
    Every one is a conversion of an fp32 value by the compiler's (T) cast or the host's f32_to_bf16 / f32_to_f16:
    round to nearest, ties to even.  Asserted inside: every value converted is exactly an fp32 value (so the
    result does not depend on accumulation order, split-K or fusion), none exceeds 65504."""
    return _rounding_reference(seed, c_in, n, h, w, plan if isinstance(plan, str) else tuple(plan), n_classes, r12,
                               _alter_key(alter))[:2]


# shapes of the rounding tests: (seed, c_in, n, h, w).  Seeds of their own generators; the body is the routing body of
# that seed.  16 x 16 at N = 1: the small-batch plan, 3 and 1 channels.
ROUNDING_MIN = [(0, 3, 1, 16, 16), (1, 1, 1, 16, 16)]
ROUNDING_LARGER = [(2, 3, 6, 16, 112), (4, 3, 3, 48, 80)]
ROUNDING_FORCED = (8, 3, 2, 64, 64)
ROUNDING_R12 = [(4, 3, 3, 48, 80), (2, 3, 6, 16, 112)]          # N = 3 (small-batch plan) and N = 6
MIN_CHANGED, MIN_TIES = 0.01, 20                                # per stored tensor at the larger shapes


def rounding_coverage(seed, c_in, n, h, w, plan: str, r12=None) -> "OrderedDict[str, tuple]":
    """Per store of ``plan``'s reference: (elements, elements the conversion changed, exact ties among them),
    counted on the fp32 values the conversion received."""
    pre = _rounding_reference(seed, c_in, n, h, w, plan, 3, r12, ())[2]
    out = OrderedDict()
    for name, level in ROUNDING_STORES:
        t = PLAN_TYPES[plan][level]
        a = pre[name].astype(np.float64)
        out[name] = (a.size, int((round_sig(a, t) != a).sum()), int(is_tie(a, t).sum()))
    return out


def rounding_fault(name: str, got: np.ndarray, ref_args: tuple, ref_kwargs: dict) -> str:
    """What a wrong tensor ``name`` (a FORWARD_ORDER name) equals instead: the reference recomputed with the
    conversion that writes it truncating, rounding half away, converting to the other 16-bit type, rounding
    twice or (pooled maps) taking the max of the rounded skip -- names the fault, not just the element."""
    store = "head" if name == "logits" else name
    modes = ALTER_MODES + (("via_skip",) if name in ("p1", "p2", "p3", "p4") else ())
    hits = []
    for mode in modes:
        alt = rounding_reference(*ref_args, **ref_kwargs, alter=((store, mode),))[1][name]
        if alt.shape == got.shape and np.array_equal(alt, got):
            hits.append(mode)
    names = {"trunc": "truncation", "away": "round-half-away", "other": "the other 16-bit type", "none": "no rounding",
             "double": "a doubled rounding through bf16", "via_skip": "the max of the rounded skip"}
    return (f"{name} equals the reference with " + " / ".join(names[m] for m in hits) + f" at store '{store}'") if hits \
        else f"{name} matches none of the single-fault references (truncation, half-away, other type, double, none)"
