"""Calibration through the device statistics, evaluate_trials and VerificationPipeline, on synthetic embeddings drawn from a
two-covariance model (dim 24: x = mu + A y + G e, y per speaker, e per utterance; seed 11).

Three disjoint speaker sets: `dev` fits the PLDA, `cal` (60 speakers x 4 rows: 300 target and 6 000 non-target trials from
make_trials) fits the calibrations, `eval` (80 x 4: 400 / 8 000) is judged.

The bars: device fit against NumPy fit |dw| <= 1e-9 max(1, |w|) (a relative perturbation of 1e-13 of G and H moves the weights
by < 1e-14); min_dcf - 1e-12 <= act_dcf (the minimum over thresholds cannot exceed the cost at one threshold; 1e-12 for the two
normalising divisions); fused Cllr <= the better single calibrated system + 1e-9 on the training trials at p_target = 0.5, where
Cllr IS the objective (over ln 2) and a single system is the point w_other = 0 of the fused family."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_f64_ref as ref  # noqa: E402

DIM = 24
TODAY = {"eer", "auc", "eer_threshold", "min_dcf", "threshold", "p_miss", "p_fa", "scores"}


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.evaluation import make_trials
    from speaker_verification_amd.plda import Plda
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    rng = np.random.default_rng(11)
    mu, a, g = rng.standard_normal(DIM), 0.6 * rng.standard_normal((DIM, DIM)), rng.standard_normal((DIM, DIM))

    def draw(ids):
        y = rng.standard_normal((int(ids.max()) + 1, DIM))
        return (mu + y[ids] @ a.T + rng.standard_normal((ids.size, DIM)) @ g.T).astype(np.float32)
    dev_ids = np.repeat(np.arange(60), rng.integers(2, 9, 60))
    cal_ids, eval_ids = np.repeat(np.arange(60), 4), np.repeat(np.arange(80), 4)
    w = {"eng": eng, "cal": eng.to_device(draw(cal_ids)), "eval": eng.to_device(draw(eval_ids))}
    w["plda"] = Plda().fit(eng.to_device(draw(dev_ids)), dev_ids, l2_in=False, shrinkage=1e-3, engine=eng)
    w["cal_trials"] = make_trials(cal_ids, 300, 6000, seed=1)
    w["eval_trials"] = make_trials(eval_ids, 400, 8000, seed=2)
    labels, ia, ib = w["cal_trials"]
    w["cal_cos"] = eng.pair_scores(w["cal"], w["cal"], ia, ib)
    u = w["plda"].project(w["cal"], engine=eng)
    w["cal_llr"] = w["plda"].score_trials(u, ia, ib, engine=eng)
    return w


@pytest.mark.parametrize("systems", [("cal_cos",), ("cal_llr",), ("cal_cos", "cal_llr")])
@pytest.mark.parametrize("p_target", [0.01, 0.5])
def test_device_fit_agrees_with_the_numpy_fit(world, systems, p_target):
    from speaker_verification_amd.calibration import Calibration
    eng, labels = world["eng"], world["cal_trials"][0]
    scores = [world[name] for name in systems]
    dev = Calibration(p_target=p_target).fit(scores if len(scores) > 1 else scores[0], labels, engine=eng)
    host = Calibration(p_target=p_target).fit(np.stack([s.cpu().numpy() for s in scores]), labels, stats=ref.stats_float64)
    print("%s, p = %g: %d iterations, w = %s, |dw| = %.2e" % (systems, p_target, dev.n_iter_, dev.weights_,
                                                                np.max(np.abs(dev.weights_ - host.weights_))))
    assert dev.converged_ and host.converged_ and max(dev.n_iter_, host.n_iter_) <= 30
    assert dev.weights_.shape == (len(systems) + 1,)
    assert np.all(np.abs(dev.weights_ - host.weights_) <= 1e-9 * np.maximum(1.0, np.abs(host.weights_)))
    if len(systems) == 1:
        assert dev.weights_[0] > 0                                               # a higher score, a higher LLR


def test_evaluate_trials_with_and_without_a_calibration(world):
    from speaker_verification_amd import calibration as cal
    from speaker_verification_amd.evaluation import DEFAULT_OPERATING_POINTS, evaluate_trials
    eng = world["eng"]
    labels, ia, ib = world["eval_trials"]
    c = cal.Calibration(p_target=0.05).fit(world["cal_cos"], world["cal_trials"][0], engine=eng)
    assert c.converged_ and c.weights_[0] > 0
    plain = evaluate_trials(world["eval"], labels, ia, ib)
    assert set(plain) == TODAY                                                   # off by default: today's dict, today's bits
    assert torch.equal(plain["scores"], eng.pair_scores(world["eval"], world["eval"], ia, ib))
    res = evaluate_trials(world["eval"], labels, ia, ib, calibration=c)
    assert set(res) == TODAY | {"cllr", "act_dcf"}
    assert torch.equal(res["scores"], c.apply(plain["scores"], engine=eng))
    # an increasing map changes no rank: the ROC is the same unless the rounding to float32 made new ties
    raw, llr = plain["scores"].cpu().numpy(), res["scores"].cpu().numpy()
    merged = np.unique(raw).size - np.unique(llr).size
    assert merged >= 0
    assert abs(res["eer"] - plain["eer"]) <= merged / 400.0 + 1e-12 and abs(res["auc"] - plain["auc"]) <= merged / 400.0 + 1e-12
    np.testing.assert_allclose(res["min_dcf"], plain["min_dcf"], rtol=0, atol=merged / 400.0 / 0.01 + 1e-12)
    assert len(res["act_dcf"]) == len(DEFAULT_OPERATING_POINTS)
    for low, act in zip(res["min_dcf"], res["act_dcf"]):
        assert low - 1e-12 <= act
    assert res["cllr"] == cal.cllr(res["scores"], labels, engine=eng)
    assert res["cllr"] < cal.cllr(plain["scores"], labels, engine=eng)           # cosines read as LLRs are far off
    # act_dcf is the cost at the Bayes thresholds, counted in NumPy
    got, p_miss, p_fa = cal.act_dcf(res["scores"], labels, DEFAULT_OPERATING_POINTS, engine=eng)
    assert got == res["act_dcf"]
    tar = labels != 0
    for (p, c_miss, c_fa), d, miss, fa in zip(DEFAULT_OPERATING_POINTS, got, p_miss, p_fa):
        accept = llr >= np.float32(cal.bayes_threshold(p, c_miss, c_fa))
        want_miss, want_fa = 1.0 - float((accept & tar).sum()) / tar.sum(), float((accept & ~tar).sum()) / (~tar).sum()
        assert (miss, fa) == (want_miss, want_fa)
        assert d == (c_miss * p * want_miss + c_fa * (1 - p) * want_fa) / min(c_miss * p, c_fa * (1 - p))
    print("eval: Cllr %.4f, minDCF %s, actDCF %s" % (res["cllr"], res["min_dcf"], res["act_dcf"]))
    fused = cal.Calibration().fit([world["cal_cos"], world["cal_llr"]], world["cal_trials"][0], engine=eng)
    with pytest.raises(ValueError, match="one system"):
        evaluate_trials(world["eval"], labels, ia, ib, calibration=fused)


def test_pipeline_scores_calibrated_llrs_and_decides(world, tmp_path):
    from speaker_verification_amd import calibration as cal
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    eng, plda = world["eng"], world["plda"]
    labels, ia, ib = world["eval_trials"]
    c = cal.Calibration(p_target=0.05).fit(world["cal_llr"], world["cal_trials"][0], engine=eng)
    path = str(tmp_path / "cal.npz")
    c.save(path)
    model = C3D2(4, 1)
    plain = VerificationPipeline(model, use_vad=False, plda=plda)
    pipe = VerificationPipeline(model, use_vad=False, plda=plda, calibration=cal.Calibration.load(path))
    assert plain.calibration is None
    raw = plain.score_trials(world["eval"], ia, ib)
    llr = pipe.score_trials(world["eval"], ia, ib)
    assert torch.equal(llr, c.apply(raw, engine=eng)) and not torch.equal(llr, raw)
    a, b = world["eval"][:50], world["eval"][50:120]
    matrix = pipe.score(a, b)
    assert matrix.shape == (50, 70)
    assert torch.equal(matrix.reshape(-1), c.apply(plain.score(a, b).reshape(-1), engine=eng))
    for op in ((0.01, 1, 1), (0.5, 1, 1), (0.05, 10, 1)):
        got = pipe.decide(llr, *op)
        assert got.dtype == torch.bool
        want = llr.cpu().numpy() >= np.float32(cal.bayes_threshold(*op))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert 0 < int(pipe.decide(llr, 0.5).sum()) < llr.numel()
    with pytest.raises(ValueError, match="search"):
        VerificationPipeline(model, use_vad=False, calibration=c).search(a, b, k=1)
    fused = cal.Calibration().fit([world["cal_cos"], world["cal_llr"]], world["cal_trials"][0], engine=eng)
    with pytest.raises(ValueError, match="one system"):
        VerificationPipeline(model, use_vad=False, calibration=fused)


def test_fusion_is_no_worse_than_its_best_system(world):
    from speaker_verification_amd import calibration as cal
    eng, labels = world["eng"], world["cal_trials"][0]
    cos, llr = world["cal_cos"], world["cal_llr"]
    single = {}
    for name, s in (("cosine", cos), ("plda", llr)):
        c = cal.Calibration(p_target=0.5).fit(s, labels, engine=eng)
        assert c.converged_
        applied = c.apply(s, engine=eng)
        single[name] = cal.cllr(applied, labels, engine=eng)
        # at p = 0.5 Cllr is the objective over ln 2, up to the rounding of the applied scores to float32 (|d softplus| <= |d llr|)
        assert abs(single[name] - c.objective_ / math.log(2)) <= 2.0 ** -24 * float(applied.abs().max()) / math.log(2)
        single[name + " objective"] = c.objective_ / math.log(2)
    fused = cal.Calibration(p_target=0.5).fit([cos, llr], labels, engine=eng)
    assert fused.converged_ and fused.n_sys == 2
    both = cal.cllr(fused.apply([cos, llr], engine=eng), labels, engine=eng)
    print("Cllr on the calibration trials: cosine %.4f, PLDA %.4f, fused %.4f" % (single["cosine"], single["plda"], both))
    assert fused.objective_ / math.log(2) <= min(single["cosine objective"], single["plda objective"]) + 1e-9
    assert both <= min(single["cosine"], single["plda"]) + 1e-9
