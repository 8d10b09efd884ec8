"""Scoring of labelled pages, the parts that need no GPU: the numpy restatement of unet_score (score_ref)
against the reference's InvoiceLoss results of the fixture, metrics.Score's assembly of loss / Dice / IoU / sweep
from 64-byte entries, and the argument checks of unet_score / unet_score_reserve (made before any HIP call)."""
import ctypes

import numpy as np
import pytest

import score_ref
from score_ref import SPREAD_FACTOR, rel

CASES = score_ref.fixture()
BAR = SPREAD_FACTOR * max(c["spread"] for c in CASES)
IDS = ["x".join(str(v) for v in c["shape"]) for c in CASES]


def logit_cuts(probs):
    from unet_mi355x import native
    lib = native.load_library()
    return np.array([lib.unet_logit_cut(float(p)) for p in probs], np.float32)


@pytest.fixture(scope="module")
def scored():
    """Per case: (logits, target uint8 NHWC, target fp32 NCHW, thresholds, Score of score_ref's entries)."""
    from unet_mi355x.metrics import Score
    out = []
    for case in CASES:
        logits, tu8 = score_ref.case_tensors(case)
        tf = score_ref.target_f32(tu8)
        thr = (0.25, 0.40, 0.30, 0.5)[:case["shape"][1]]
        entries, hist = score_ref.score(logits, tf, logit_cuts(thr), logit_cuts(score_ref.SWEEP))
        out.append((logits, tu8, tf, thr, Score(entries, hist, score_ref.SWEEP)))
    return out


def test_fixture_holds_the_issue_cases():
    assert [(c["shape"], c["scale"], c["shift"]) for c in CASES] == [(s, a, b) for s, a, b, _, _ in score_ref.CASES]
    assert (96 * 160 + 4095) // 4096 >= 4          # one plane over at least 4 spans of the kernel
    assert 0 < BAR < 1e-5                          # a bar of a few fp32 ulps, whatever the fixture says
    from unet_mi355x import metrics, native
    assert native.SCORE_DTYPE == metrics.ENTRY_DTYPE and metrics.ENTRY_DTYPE.itemsize == 64
    assert ctypes.sizeof(native.ScoreEntry) == 64


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_restatement_reproduces_reference_losses(i, scored):
    """score_ref + metrics.Score vs the reference's InvoiceLoss / Dice / focal (CPU fp32), also called per
    batch and averaged: relative distance <= 8 x the fixture's largest spread."""
    case, s = CASES[i], scored[i][4]
    got = dict(dice=s.dice(), focal=s.focal(), loss=s.loss(), loss_b1=s.loss(batch=1), loss_b2=s.loss(batch=2))
    for k, v in got.items():
        d = rel(v, case[k])
        print(f"{IDS[i]} {k}: ours {v!r} reference {case[k]!r} rel {d:.3e} (bar {BAR:.3e})")
        assert d <= BAR, (k, v, case[k])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_iou_matches_oracle_mask_iou(i, scored):
    from oracle import unet_oracle as orc
    logits, _, tf, thr, s = scored[i]
    cuts = logit_cuts(thr)
    iou = s.iou()
    n, c = logits.shape[:2]
    pooled_i, pooled_u = np.zeros(c), np.zeros(c)
    for a in range(n):
        for b in range(c):
            pred, tgt = logits[a, b] > cuts[b], tf[a, b] > 0.5
            assert iou[a, b] == orc.mask_iou(pred, tgt)
            pooled_i[b] += (pred & tgt).sum()
            pooled_u[b] += (pred | tgt).sum()
    want = np.where(pooled_u == 0, 1.0, pooled_i / np.maximum(pooled_u, 1))
    assert np.array_equal(s.pooled_iou(), want)


def test_iou_of_two_empty_masks_is_one():
    from unet_mi355x.metrics import ENTRY_DTYPE, Score
    e = np.zeros((1, 2), ENTRY_DTYPE)
    e["n_px"] = 16
    e["n_tgt"][0, 1] = 4
    s = Score(e)
    assert s.iou().tolist() == [[1.0, 0.0]] and s.pooled_iou().tolist() == [1.0, 0.0]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_matches_brute_force(i, scored):
    """sweep_iou / best_thresholds from the histogram's suffix sums vs thresholding at every candidate."""
    logits, _, tf, _, s = scored[i]
    cuts = logit_cuts(score_ref.SWEEP)
    n, c = logits.shape[:2]
    want = np.zeros((c, len(cuts)))
    pred_k, both_k, tgt_n = s.sweep_counts()
    for k, cut in enumerate(cuts):
        pred, tgt = logits > cut, tf > 0.5
        assert np.array_equal(pred_k[..., k], pred.reshape(n, c, -1).sum(-1))
        assert np.array_equal(both_k[..., k], (pred & tgt).reshape(n, c, -1).sum(-1))
        inter = (pred & tgt).transpose(1, 0, 2, 3).reshape(c, -1).sum(-1)
        union = (pred | tgt).transpose(1, 0, 2, 3).reshape(c, -1).sum(-1)
        want[:, k] = np.where(union == 0, 1.0, inter / np.maximum(union, 1))
    assert np.array_equal(tgt_n, (tf > 0.5).reshape(n, c, -1).sum(-1))
    assert np.array_equal(s.sweep_iou(), want)
    best = [score_ref.SWEEP[int(np.flatnonzero(row == row.max())[0])] for row in want]   # ties: the lowest
    assert s.best_thresholds().tolist() == best


def test_best_thresholds_ties_go_to_the_lowest():
    from unet_mi355x.metrics import ENTRY_DTYPE, Score
    hist = np.zeros((1, 1, 2, 4), np.int64)
    hist[0, 0, 1, 3] = 5          # 5 target pixels above every cut: IoU 1 at all three candidates
    e = np.zeros((1, 1), ENTRY_DTYPE)
    s = Score(e, hist, [0.2, 0.5, 0.8])
    assert s.sweep_iou().tolist() == [[1.0, 1.0, 1.0]] and s.best_thresholds().tolist() == [0.2]


def test_scores_concatenate_along_n(scored):
    from unet_mi355x.metrics import Score
    s = scored[2][4]   # N = 3
    parts = [s[0:2], s[2:3]]
    cat = Score.concat(parts)
    assert cat.entries.tobytes() == s.entries.tobytes() and np.array_equal(cat.hist, s.hist)
    assert (parts[0] + parts[1]).loss(batch=2) == s.loss(batch=2)
    assert s.loss(batch=2) == np.mean([s[0:2].loss(), s[2:3].loss()])
    with pytest.raises(ValueError):
        Score.concat([s, Score(s.entries)])
    raw = Score(np.frombuffer(s.entries.tobytes(), np.uint8).reshape(3, 3, 64))   # the device's bytes
    assert raw.loss() == s.loss()


def test_nan_logit_marks_the_four_sums_of_its_entry(scored):
    logits, _, tf, thr, s = scored[2]
    x = logits.copy()
    x[1, 2, 3, 5] = np.nan
    e, _ = score_ref.score(x, tf, logit_cuts(thr))
    for k in ("sum_p", "sum_t", "sum_pt", "sum_focal"):
        assert np.isnan(e[k][1, 2]) and np.isnan(e[k]).sum() == 1
    want = s.entries["n_pred"].copy()
    want[1, 2] -= int(logits[1, 2, 3, 5] > logit_cuts(thr)[2])
    assert np.array_equal(e["n_pred"], want)


# ---------------------------------------------------------------- argument checks, no GPU
def _call_score(lib, **kw):
    from unet_mi355x import native
    dummy = ctypes.create_string_buffer(1 << 16)   # stands for every non-NULL pointer; never read by a refused call
    ptr = ctypes.cast(dummy, ctypes.c_void_p).value
    probs = kw.pop("probs", None)
    a = dict(h=ptr, logits=ptr, target=ptr, kind=native.TGT_F32_NCHW, N=1, C=3, H=16, W=16, thr=None, entries=ptr,
             K=0 if probs is None else len(probs), hist=None if probs is None else ptr)
    a.update(kw)
    p = None if probs is None else (ctypes.c_float * max(1, len(probs)))(*probs)
    return lib.unet_score(a["h"], a["logits"], a["target"], a["kind"], a["N"], a["C"], a["H"], a["W"], a["thr"],
                          a["entries"], p, a["K"], a["hist"], None)


@pytest.mark.parametrize("kw, word", [
    (dict(h=None), b"handle"),
    (dict(logits=None), b"NULL"),
    (dict(target=None), b"NULL"),
    (dict(entries=None), b"NULL"),
    (dict(C=0), b"C must be 1..4"),
    (dict(C=5), b"C must be 1..4"),
    (dict(kind=2), b"target_kind"),
    (dict(kind=-1), b"target_kind"),
    (dict(probs=[i / 100.0 for i in range(1, 66)]), b"K"),
    (dict(probs=[0.2, 0.2]), b"ascending"),
    (dict(probs=[0.5, 0.4]), b"ascending"),
    (dict(probs=[0.5, float("nan")]), b"ascending"),
    (dict(probs=[0.5], hist=None), b"without hist"),
    (dict(hist=1 << 12), b"without sweep_probs"),
    (dict(N=0), b"positive"),
    (dict(H=0), b"positive"),
])
def test_score_rejects_bad_arguments_without_gpu(kw, word):
    from unet_mi355x import native
    lib = native.load_library()
    assert _call_score(lib, **kw) == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()


@pytest.mark.parametrize("args, word", [
    ((None, 1, 16, 16, 0), b"handle"),
    ((1, 0, 16, 16, 0), b"positive"),
    ((1, 1, 16, -1, 0), b"positive"),
    ((1, 1, 16, 16, 65), b"K"),
    ((1, 1, 16, 16, -1), b"K"),
])
def test_score_reserve_rejects_bad_arguments_without_gpu(args, word):
    from unet_mi355x import native
    lib = native.load_library()
    dummy = ctypes.create_string_buffer(1 << 16)
    h = None if args[0] is None else ctypes.cast(dummy, ctypes.c_void_p).value
    assert lib.unet_score_reserve(h, *args[1:]) == native.UNET_EINVAL
    assert word in lib.unet_last_error(), lib.unet_last_error()
