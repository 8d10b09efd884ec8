"""Exact-arithmetic operands for the bitwise tests (tests/test_exact_cpu.py, tests/test_exact_gpu.py).

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


# ------------------------------------------------------------------------------------------------ section 2
BLOCK_SIZE = {"down1": (19, 37), "down2": (19, 37), "conv2": (19, 37), "conv1": (19, 37),
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
WIDE_SIZE = {"down2": (19, 37), "down4": (9, 21), "conv1": (19, 37)}


@functools.lru_cache(maxsize=None)
def wide_block(name: str, case: str, seed: int = 0) -> ExactBlock:
    """First conv: activations below 2^abits, ``nnz`` weights per output channel of magnitude below 2^wbits
    and random sign at random (cin, tap) positions, integer beta in [-4, 4], scale 1.  Second conv: the
    centre-tap identity (+1 at (o, o, 1, 1)), beta 0.  nnz * 2^abits * 2^wbits + 4 < 2^24 in every case."""
    abits, wbits, nnz = WIDE_CASES[case]
    cin, cout = BLOCKS[name]
    h, w = WIDE_SIZE[name]
    rng = np.random.default_rng([seed, cin, cout, abits, wbits])
    x = rng.integers(0, 2 ** abits, (BLOCK_N, cin, h, w)).astype(np.float32)
    k = cin * 9
    w0 = np.zeros((cout, k), np.float32)
    for o in range(cout):
        pos = rng.choice(k, nnz, replace=False)
        w0[o, pos] = rng.integers(1, 2 ** wbits, nnz) * rng.choice([-1.0, 1.0], nnz)
    ident = np.zeros((cout, cout, 3, 3), np.float32)
    ident[np.arange(cout), np.arange(cout), 1, 1] = 1.0
    return ExactBlock(name, cin, cout, x, [w0.reshape(cout, cin, 3, 3), ident], [1.0, 1.0],
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
