"""svk_roc_dcf: minDCF, its threshold and the EER threshold from the device ROC, against sklearn's
roc_curve(drop_intermediate=False) for the counts and evaluation.get_min_dcf for the costs."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OPS = ((0.01, 1, 1), (0.05, 1, 1), (0.5, 1, 1), (0.001, 10, 1))


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def dyadic_case(seed=22):
    """128 pairs, 64 / 64, alternating non-target, target in descending score order, stored shuffled (see
    tests/test_trials_host.py): with p_target = 0.5 and costs 1 every rate and cost is exact and the minimum cost, 0.5, is
    reached at the origin and after every target."""
    rank = np.arange(128)
    labels = (rank % 2).astype(np.uint8)
    scores = ((127 - rank) / 32.0 - 2.0).astype(np.float32)
    order = np.random.default_rng(seed).permutation(128)
    return labels[order], scores[order]


def make_cases():
    rng = np.random.default_rng(70)
    cases = {"n2": (np.array([0, 1], np.uint8), np.array([0.1, 0.3], np.float32)),
             "n3": (np.array([1, 0, 1], np.uint8), np.array([0.2, 0.1, 0.3], np.float32))}
    lab = (rng.random(2049) < 0.2).astype(np.uint8)
    cases["n2049"] = (lab, (rng.standard_normal(2049) + 1.5 * lab).astype(np.float32))
    lab = (rng.random(5000) < 0.3).astype(np.uint8)
    cases["n5000_16_levels"] = (lab, (np.floor((rng.standard_normal(5000) + 1.2 * lab) * 2).clip(-8, 7) / 4).astype(np.float32))
    lab = (rng.random(300_000) < 0.05).astype(np.uint8)
    cases["n300000"] = (lab, (rng.standard_normal(300_000) + 2.0 * lab).astype(np.float32))
    lab = (rng.random(1000) < 0.5).astype(np.uint8)
    lab[:2] = (0, 1)
    cases["all_equal"] = (lab, np.full(1000, 0.25, np.float32))
    cases["signed_zeros"] = ((rng.random(4099) < 0.3).astype(np.uint8),
                             rng.choice(np.array([0.0, -0.0, 0.5, -0.5], np.float32), 4099))
    cases["dyadic"] = dyadic_case()
    for lab, sc in cases.values():
        lab.setflags(write=False)
        sc.setflags(write=False)
    return cases


CASES = make_cases()


def roc_eer4(eng, sc, lab):
    """svk_roc_eer's four values, straight from the library."""
    s, l = eng.to_device(sc, torch.float32), eng.to_device(lab, torch.uint8)
    work = torch.empty(int(eng.lib.svk_roc_workspace_bytes(s.numel())), dtype=torch.uint8, device=eng.device)
    out = (C.c_double * 4)()
    eng._stream()
    assert eng.lib.svk_roc_eer(eng.ctx, eng._ptr(s), eng._ptr(l), s.numel(), eng._ptr(work), work.numel(), out) == 0
    return list(out)


def rates_at(eng, sc, lab, threshold):
    """(tp, fp, P, N) by svk_decision_counts at one threshold"""
    acc, (P, N) = eng.decision_counts(sc, lab, [threshold])
    return int(acc[0, 0]), int(acc[0, 1]), P, N


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_host(eng, name):
    from sklearn.metrics import roc_curve
    from speaker_verification_amd.evaluation import get_min_dcf
    lab, sc = CASES[name]
    res = eng.roc_dcf(sc, lab, OPS)
    fpr, tpr, _ = roc_curve(lab, sc, pos_label=1, drop_intermediate=False)
    # the ROC itself: svk_roc_eer's values, bit for bit; the counts are sklearn's
    want4 = roc_eer4(eng, sc, lab)
    assert [res["eer"], res["auc"], float(res["positives"]), float(res["points"])] == want4
    assert res["positives"] == int(lab.sum()) and res["points"] == fpr.size - 1
    none = eng.roc_dcf(sc, lab, ())                                      # n_op = 0: the same ROC, no operating point
    assert none["min_dcf"] == [] and all(none[k] == res[k] for k in ("eer", "auc", "positives", "points", "eer_threshold"))
    assert eng.roc_eer(sc, lab) == (res["eer"], res["auc"])
    values = np.where(sc == 0, np.float32(0), sc)
    for o, (p, c_miss, c_fa) in enumerate(OPS):
        a, b = c_miss * p, c_fa * (1 - p)
        want = get_min_dcf(lab, sc, p, c_miss, c_fa)
        got = tuple(res[k][o] for k in ("min_dcf", "threshold", "p_miss", "p_fa"))
        print(name, (p, c_miss, c_fa), "device", got, "host", want)
        assert got[0] == pytest.approx(want[0], rel=1e-13)
        thr = got[1]
        assert thr == np.inf or np.any(values == np.float32(thr))        # a score of the input, or +inf
        tp, fp, P, N = rates_at(eng, sc, lab, thr)
        assert got[2] == 1.0 - tp / P and got[3] == fp / N               # the rates there, ratios of the same integers
        host_cost = a * (1.0 - tp / P) + b * (fp / N)                    # whichever of two near-equal minima either side took
        assert host_cost == pytest.approx(want[0] * min(a, b), rel=1e-13)
    # eer_threshold: the first point with 1 - fpr - tpr <= 0
    thr = res["eer_threshold"]
    assert np.any(values == np.float32(thr))
    tp, fp, P, N = rates_at(eng, sc, lab, thr)
    assert 1.0 - fp / N - tp / P <= 0
    higher = values[values > np.float32(thr)]
    if higher.size:                                                      # (none: the point before it is the origin, g = 1)
        tp, fp, P, N = rates_at(eng, sc, lab, float(higher.min()))
        assert 1.0 - fp / N - tp / P > 0


def test_exact_case_ties_go_to_the_origin(eng):
    from speaker_verification_amd.evaluation import get_min_dcf
    lab, sc = CASES["dyadic"]
    res = eng.roc_dcf(sc, lab, [(0.5, 1, 1)])
    got = (res["min_dcf"][0], res["threshold"][0], res["p_miss"][0], res["p_fa"][0])
    assert got == (1.0, float("inf"), 1.0, 0.0) == get_min_dcf(lab, sc, 0.5, 1, 1)
    # the two best scores swapped: a unique minimum at the first point, still exact
    s2 = sc.copy()
    i, j = int(np.argmax(sc)), int(np.argsort(sc)[-2])
    s2[i], s2[j] = sc[j], sc[i]
    res = eng.roc_dcf(s2, lab, [(0.5, 1, 1)])
    got = (res["min_dcf"][0], res["threshold"][0], res["p_miss"][0], res["p_fa"][0])
    assert got == (1.0 - 1 / 64, float(sc.max()), 63 / 64, 0.0) == get_min_dcf(lab, s2, 0.5, 1, 1)


def test_errors(eng):
    from speaker_verification_amd import _lib
    lab, sc = CASES["n2049"]
    x = sc.copy()
    x[77] = np.nan
    with pytest.raises(_lib.SvkError, match="non-finite"):
        eng.roc_dcf(x, lab, OPS)
    for one in (np.zeros_like(lab), np.ones_like(lab)):
        with pytest.raises(_lib.SvkError, match="one class"):
            eng.roc_dcf(sc, one, OPS)
    for p in (0.0, 1.0, -0.1, np.nan):
        with pytest.raises(_lib.SvkError, match="operating point 1"):
            eng.roc_dcf(sc, lab, [(0.01, 1, 1), (p, 1, 1)])
    for op in ((0.01, 0, 1), (0.01, 1, -2), (0.01, np.inf, 1)):
        with pytest.raises(_lib.SvkError, match="operating point 0"):
            eng.roc_dcf(sc, lab, [op])
    with pytest.raises(_lib.SvkError, match="operating points"):
        eng.roc_dcf(sc, lab, [(0.01, 1, 1)] * 9)
    with pytest.raises(_lib.SvkError):
        eng.roc_dcf(sc[:1], lab[:1], OPS)                                # n < 2
    # a workspace one byte short
    s, l = eng.to_device(sc, torch.float32), eng.to_device(lab, torch.uint8)
    need = int(eng.lib.svk_roc_dcf_workspace_bytes(s.numel()))
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    ops = (C.c_double * 3)(0.01, 1, 1)
    out = (C.c_double * 9)(*([-7.0] * 9))
    eng._stream()
    rc = eng.lib.svk_roc_dcf(eng.ctx, eng._ptr(s), eng._ptr(l), s.numel(), ops, 1, eng._ptr(work), need - 1, out)
    assert rc == _lib.SVK_ERR_BAD_ARG and b"workspace" in eng.lib.svk_last_error(eng.ctx) and list(out) == [-7.0] * 9
    assert eng.lib.svk_roc_dcf(eng.ctx, eng._ptr(s), eng._ptr(l), s.numel(), ops, 1, eng._ptr(work), need, out) == 0
    assert out[0] == eng.roc_eer(sc, lab)[0]
