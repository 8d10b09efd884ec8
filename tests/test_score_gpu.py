"""unet_score on the device against its numpy restatement (tests/score_ref.py) and the reference's InvoiceLoss
results (tests/golden/score_cases.npz), through the C-ABI and UNet.score / inference.evaluate.  Needs a GPU: run
with -m gpu.

Bars: integer counts and histograms bitwise; float sums, Dice, focal and loss within 8 x the fixture's largest
spread (the distance of the reference's fp32 result from the numpy restatement -- two fp32 implementations of
the same arithmetic; the device's expf / logf / reciprocal are a third).

Largest distances observed on MI355X: see test_fixture_cases' docstring.
"""
import os

import numpy as np
import pytest
import torch

import score_ref
from score_ref import SPREAD_FACTOR, rel
from unet_mi355x import native
from unet_mi355x import synthetic as syn
from unet_mi355x.metrics import Score
from unet_mi355x.model import UNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = score_ref.fixture()
BAR = SPREAD_FACTOR * max(c["spread"] for c in CASES)
IDS = ["x".join(str(v) for v in c["shape"]) for c in CASES]
THR = (0.25, 0.40, 0.30, 0.5)
SUMS = ("sum_p", "sum_t", "sum_pt", "sum_focal")
COUNTS = ("n_pred", "n_tgt", "n_both", "n_px")


def logit_cuts(probs):
    lib = native.load_library()
    return np.array([lib.unet_logit_cut(float(p)) for p in probs], np.float32)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def run_score(h, logits, target, sweep=None, thresholds=None):
    """numpy logits / target -> Score through Handle.score (target fp32 NCHW or uint8 NHWC)."""
    entries, hist = h.score(torch.from_numpy(np.ascontiguousarray(logits)).to(DEV),
                            torch.from_numpy(np.ascontiguousarray(target)).to(DEV), stream(),
                            thresholds=thresholds, sweep=sweep)
    return Score(entries.cpu().numpy(), None if hist is None else hist.cpu().numpy(), sweep)


@pytest.fixture(scope="module")
def handles():
    hs = {c: native.Handle(3, c, "fp32", 0, THR) for c in (1, 3, 4)}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def refs():
    """Per case, once: (logits, target uint8 NHWC, target fp32 NCHW, score_ref entries, score_ref hist)."""
    out = []
    for case in CASES:
        logits, tu8 = score_ref.case_tensors(case)
        tf = score_ref.target_f32(tu8)
        e, hist = score_ref.score(logits, tf, logit_cuts(THR[:case["shape"][1]]), logit_cuts(score_ref.SWEEP))
        out.append((logits, tu8, tf, e, hist))
    return out


@pytest.mark.parametrize("form", ["f32_nchw", "u8_nhwc"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fixture_cases(i, form, handles, refs):
    """Every fixture case in both target forms: counts and histogram bitwise equal to score_ref, float sums
    within 8 x spread of score_ref's float64 sums, Dice / focal / loss within the same bar of the reference.

    Largest distances observed on MI355X (both forms, all cases), against a bar of 4.7e-6: float sums 5.7e-8
    from score_ref's (3x3x16x16); Dice / focal / loss 5.9e-7 from the reference's (the one-element case, whose
    fixture spread is the same 5.9e-7: the reference's fp32 ``1 - ratio`` cancels there), 1.2e-7 on the other
    cases (focal of 1x3x96x160)."""
    case = CASES[i]
    logits, tu8, tf, e, hist = refs[i]
    s = run_score(handles[case["shape"][1]], logits, tf if form == "f32_nchw" else tu8, sweep=score_ref.SWEEP)
    for k in COUNTS:
        assert np.array_equal(s.entries[k], e[k]), k
    assert np.array_equal(s.hist, hist)
    worst = 0.0
    for k in SUMS:
        for got, want in zip(s.entries[k].ravel(), e[k].ravel()):
            worst = max(worst, rel(got, want))
    print(f"{IDS[i]} {form}: sums rel {worst:.3e} (bar {BAR:.3e})")
    worst_loss = 0.0
    got = dict(dice=s.dice(), focal=s.focal(), loss=s.loss(), loss_b1=s.loss(batch=1), loss_b2=s.loss(batch=2))
    for k, v in got.items():
        worst_loss = max(worst_loss, rel(v, case[k]))
        print(f"{IDS[i]} {form} {k}: device {v!r} reference {case[k]!r} rel {rel(v, case[k]):.3e}")
    assert worst <= BAR
    assert worst_loss <= BAR
    # without the sweep: the same entries, bit for bit
    s0 = run_score(handles[case["shape"][1]], logits, tf if form == "f32_nchw" else tu8)
    assert s0.hist is None and s0.entries.tobytes() == s.entries.tobytes()


def test_both_target_forms_agree_bitwise(handles, refs):
    logits, tu8, tf, _, _ = refs[4]
    a = run_score(handles[3], logits, tf, sweep=score_ref.SWEEP)
    b = run_score(handles[3], logits, tu8, sweep=score_ref.SWEEP)
    assert a.entries.tobytes() == b.entries.tobytes() and np.array_equal(a.hist, b.hist)


@pytest.mark.parametrize("i", [1, 3, 5], ids=[IDS[1], IDS[3], IDS[5]])
def test_deterministic_and_independent_of_the_batch(i, handles, refs):
    """The same inputs twice: bitwise-equal entries.  Image i alone, in its batch, in the reversed batch and
    behind another image (another alignment of its planes): bitwise the same entry."""
    logits, tu8, tf, _, _ = refs[i]
    h = handles[logits.shape[1]]
    for tgt in (tf, tu8):
        a = run_score(h, logits, tgt, sweep=score_ref.SWEEP)
        b = run_score(h, logits, tgt, sweep=score_ref.SWEEP)
        assert a.entries.tobytes() == b.entries.tobytes() and np.array_equal(a.hist, b.hist)
        rev = run_score(h, logits[::-1].copy(), tgt[::-1].copy(), sweep=score_ref.SWEEP)
        assert rev.entries[::-1].tobytes() == a.entries.tobytes() and np.array_equal(rev.hist[::-1], a.hist)
        for j in range(logits.shape[0]):
            one = run_score(h, logits[j:j + 1], tgt[j:j + 1], sweep=score_ref.SWEEP)
            assert one.entries.tobytes() == a.entries[j:j + 1].tobytes() and np.array_equal(one.hist, a.hist[j:j + 1])
        two = run_score(h, np.concatenate([logits[-1:], logits]), np.concatenate([tgt[-1:], tgt]))
        assert two.entries[1:].tobytes() == a.entries.tobytes()


def test_nan_logit(handles, refs):
    """One NaN logit: its entry's four sums are NaN, its n_pred is that without the pixel, every other entry is
    bitwise unchanged."""
    logits, tu8, tf, e, _ = refs[4]
    h = handles[3]
    base = run_score(h, logits, tu8)
    x = logits.copy()
    x[1, 2, 17, 5] = np.nan
    s = run_score(h, x, tu8)
    for k in SUMS:
        assert np.isnan(s.entries[k][1, 2])
    want = e["n_pred"][1, 2] - int(logits[1, 2, 17, 5] > logit_cuts(THR)[2])
    assert s.entries["n_pred"][1, 2] == want
    for k in ("n_tgt", "n_px"):
        assert s.entries[k][1, 2] == e[k][1, 2]
    keep = np.ones((2, 3), bool)
    keep[1, 2] = False
    assert s.entries[keep].tobytes() == base.entries[keep].tobytes()


def test_thresholds_argument_overrides_the_handles(handles, refs):
    logits, tu8, tf, _, _ = refs[2]
    thr = (0.6, 0.1, 0.5)
    s = run_score(handles[3], logits, tf, thresholds=thr)
    e, _ = score_ref.score(logits, tf, logit_cuts(thr))
    assert np.array_equal(s.entries["n_pred"], e["n_pred"]) and np.array_equal(s.entries["n_both"], e["n_both"])


@pytest.mark.parametrize("dtype", ["fp32", "mixed"])
def test_score_is_consistent_with_the_forward(dtype):
    """UNet.score(x, target): counts equal numpy counts on forward_masks(x) and the target; entries bitwise those
    of score_logits(model(x), target)."""
    z = np.load(os.path.join(GOLD, "unet_c3_h64w64_n2_structured.npz"))
    sd = syn.make_state_dict(int(z["seed"]), 3, 3, profile=str(z["profile"]))
    m = UNet(3, 3, compute_dtype=dtype)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.to(DEV).eval()
    x = torch.from_numpy(z["x"]).to(DEV)
    tu8 = np.random.RandomState(5).randint(0, 256, size=(2, 64, 64, 3)).astype(np.uint8)
    t = torch.from_numpy(tu8).to(DEV)
    with torch.no_grad():
        s = m.score(x, t, sweep=score_ref.SWEEP)
        masks = m.forward_masks(x).cpu().numpy().astype(bool)
        s2 = m.score_logits(m(x), t, sweep=score_ref.SWEEP)
    tgt = (tu8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)) > np.float32(0.5)
    assert np.array_equal(s.entries["n_pred"], masks.reshape(2, 3, -1).sum(-1))
    assert np.array_equal(s.entries["n_tgt"], tgt.reshape(2, 3, -1).sum(-1))
    assert np.array_equal(s.entries["n_both"], (masks & tgt).reshape(2, 3, -1).sum(-1))
    assert s.entries.tobytes() == s2.entries.tobytes() and np.array_equal(s.hist, s2.hist)
    m.close()


def test_evaluate_directory(tmp_path):
    """Five 32x48 PNG pages with .npy masks, batch 4: bitwise the Score of the same arrays through UNet.score in
    chunks of 4 and 1; loss(batch=4) follows from the entries."""
    from PIL import Image
    from unet_mi355x import inference as inf
    rs = np.random.RandomState(9)
    img_dir, mask_dir = tmp_path / "images", tmp_path / "masks"
    img_dir.mkdir()
    mask_dir.mkdir()
    pages = (syn.invoice_pages(3, 5, 32, 48, 3) * 255.0 + 0.5).astype(np.uint8).transpose(0, 2, 3, 1)
    masks = np.where(rs.rand(5, 32, 48, 3) < 0.2, 255, 0).astype(np.uint8)
    for i in (3, 0, 4, 1, 2):   # written out of order: evaluate sorts the stems
        Image.fromarray(np.ascontiguousarray(pages[i]), mode="RGB").save(str(img_dir / f"page{i}.png"))
        np.save(str(mask_dir / f"page{i}.npy"), masks[i])
    ckpt = str(tmp_path / "ckpt.pth")
    sd = syn.make_state_dict(3, 3, 3, profile="structured")
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, ckpt)
    s = inf.evaluate(str(img_dir), str(mask_dir), ckpt, batch=4, sweep=score_ref.SWEEP, compute_dtype="fp32")
    assert s.entries.shape == (5, 3) and s.hist.shape == (5, 3, 2, len(score_ref.SWEEP) + 1)

    m = inf.load_model(ckpt, "fp32")
    x = torch.from_numpy(np.ascontiguousarray(pages.transpose(0, 3, 1, 2).astype(np.float32) / 255.0)).to(DEV)
    t = torch.from_numpy(masks).to(DEV)
    with torch.no_grad():
        want = Score.concat([m.score(x[:4], t[:4], score_ref.SWEEP), m.score(x[4:], t[4:], score_ref.SWEEP)])
    assert s.entries.tobytes() == want.entries.tobytes() and np.array_equal(s.hist, want.hist)
    assert s.loss(batch=4) == np.mean([s[:4].loss(), s[4:].loss()])
    assert np.array_equal(s.entries["n_tgt"], (masks > 127).transpose(0, 3, 1, 2).reshape(5, 3, -1).sum(-1))
    m.close()

    Image.fromarray(np.zeros((32, 32, 3), np.uint8), mode="RGB").save(str(img_dir / "page9.png"))
    np.save(str(mask_dir / "page9.npy"), np.zeros((32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="one size"):
        inf.evaluate(str(img_dir), str(mask_dir), ckpt, batch=4, compute_dtype="fp32")


def test_scratch_grows_and_leaves_the_forward_workspace_alone(refs):
    logits, tu8, tf, e, hist = refs[4]
    h = native.Handle(3, 3, "fp32", 0, THR)
    before = h.workspace_bytes(2, 64, 64)
    h.score_reserve(1, 16, 16, 0)            # smaller N, smaller pages, no sweep: the score below must grow it
    s = run_score(h, logits, tu8, sweep=score_ref.SWEEP)
    for k in COUNTS:
        assert np.array_equal(s.entries[k], e[k]), k
    assert np.array_equal(s.hist, hist)
    h.score_reserve(4, 64, 48, len(score_ref.SWEEP))
    s2 = run_score(h, logits, tu8, sweep=score_ref.SWEEP)
    assert s2.entries.tobytes() == s.entries.tobytes() and np.array_equal(s2.hist, s.hist)
    assert h.workspace_bytes(2, 64, 64) == before
    h.close()
