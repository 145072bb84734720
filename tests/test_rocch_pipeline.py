"""minCllr, the ROCCH-EER and PavCalibration through evaluate_trials and VerificationPipeline, on random embeddings (dim 24,
seed 31) and 6 000 trials whose labels follow the cosine score with noise: overlapping classes, the best trial a non-target
and the worst a target, so that every PAV LLR is finite without the Laplace rule.

The bars.  PAV fitted on a list maps it to the LLRs that minimise Cllr: cllr = min_cllr to 1e-6 relative (float32 LLRs round
each term by 2^-24).  The map is monotone and only merges ties inside a bin, so the mapped list's ROC points ARE the raw list's
hull vertices: the same hull, the same host arithmetic on it (min_cllr, rocch_eer: equal bits); eer becomes the hull's EER,
computed by the device in float64 (a few roundings of 2^-53 on values <= 1: 8 * 2^-52 absolute); each min_dcf is the minimum of
the same costs over fewer points, every cost two products and a sum (8 * 2^-52 relative) -- and never below it: the vertices are
a subset of the raw points and their costs come from the same integers through the same kernel."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rocch_ref as R                    # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

TODAY = {"eer", "auc", "eer_threshold", "min_dcf", "threshold", "p_miss", "p_fa", "scores"}
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    rng = np.random.default_rng(31)
    emb = eng.to_device(rng.standard_normal((200, 24)).astype(np.float32))
    ia, ib = rng.integers(0, 200, 6000), rng.integers(0, 200, 6000)
    raw = eng.pair_scores(emb, emb, ia, ib)
    host = raw.cpu().numpy()
    labels = (host + 0.25 * rng.standard_normal(6000) > 0.15).astype(np.uint8)
    labels[int(np.argmax(host))], labels[int(np.argmin(host))] = 0, 1
    assert 600 < int(labels.sum()) < 3000
    return {"eng": eng, "emb": emb, "ia": ia, "ib": ib, "raw": raw, "labels": labels}


def test_pav_reaches_min_cllr_on_its_own_list(world):
    from speaker_verification_amd.calibration import PavCalibration
    from speaker_verification_amd.evaluation import evaluate_trials
    eng, emb, labels, ia, ib = (world[k] for k in ("eng", "emb", "labels", "ia", "ib"))
    before = evaluate_trials(emb, labels, ia, ib, rocch=True)
    assert set(before) == TODAY | {"min_cllr", "rocch_eer"} and torch.equal(before["scores"], world["raw"])
    hull = eng.rocch(world["raw"], labels)
    assert (before["min_cllr"], before["rocch_eer"]) == (hull["min_cllr"], hull["rocch_eer"])
    pav = PavCalibration().fit(world["raw"], labels, engine=eng)
    assert pav.n_sys == 1 and pav.edges_.size == len(hull["vertices"]) - 1 and np.isfinite(pav.llr_).all()
    res = evaluate_trials(emb, labels, ia, ib, calibration=pav, rocch=True)
    assert set(res) == TODAY | {"min_cllr", "rocch_eer", "cllr", "act_dcf", "calibration_loss"}
    assert torch.equal(res["scores"], pav.apply(world["raw"], engine=eng))
    print("bins %d, cllr %.17g, min_cllr %.17g, eer %.17g -> %.17g, rocch_eer %.17g" % (
        pav.edges_.size, res["cllr"], res["min_cllr"], before["eer"], res["eer"], res["rocch_eer"]))
    assert abs(res["cllr"] - res["min_cllr"]) <= 1e-6 * res["min_cllr"]
    assert res["calibration_loss"] == res["cllr"] - res["min_cllr"]
    # the map changes neither the hull nor what is computed from it
    after = eng.rocch(res["scores"], labels)
    assert np.array_equal(after["vertices"], hull["vertices"]) and after["points"] == len(hull["vertices"]) - 1
    assert (res["min_cllr"], res["rocch_eer"]) == (before["min_cllr"], before["rocch_eer"])
    assert abs(res["eer"] - before["rocch_eer"]) <= 8 * EPS and before["rocch_eer"] <= before["eer"]
    for got, want in zip(res["min_dcf"], before["min_dcf"]):
        assert want <= got <= want + 8 * EPS * want
    # the raw cosines read as LLRs are far off; the calibration loss is what PAV removes
    from speaker_verification_amd import calibration as cal
    assert cal.cllr(world["raw"], labels, engine=eng) - before["min_cllr"] > 0.05 > res["calibration_loss"]


def test_laplace_keeps_the_separated_case_finite(world):
    from speaker_verification_amd import calibration as cal
    eng = world["eng"]
    lab, sc = R.gpu_cases()["separated"]
    plain = cal.PavCalibration().fit(sc, lab, engine=eng)
    assert plain.llr_.tolist() == [np.inf, -np.inf]
    pav = cal.PavCalibration(laplace=True).fit(sc, lab, engine=eng)
    edges, llr = R.pav_table(lab, sc, laplace=True)
    assert np.array_equal(pav.edges_, edges) and np.array_equal(pav.llr_, llr) and np.isfinite(pav.llr_).all()
    out = pav.apply(sc, engine=eng).cpu().numpy()
    assert np.isfinite(out).all() and np.array_equal(out.view(np.uint32), R.pav_apply(sc, edges, llr))
    assert out[lab != 0].min() > out[lab == 0].max()
    assert 0.0 < cal.cllr(out, lab, engine=eng) < 0.2


def test_the_defaults_change_nothing(world):
    from speaker_verification_amd.calibration import PavCalibration
    from speaker_verification_amd.evaluation import DEFAULT_OPERATING_POINTS, evaluate_trials
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    eng, emb, labels, ia, ib = (world[k] for k in ("eng", "emb", "labels", "ia", "ib"))
    default, off = evaluate_trials(emb, labels, ia, ib), evaluate_trials(emb, labels, ia, ib, rocch=False)
    dcf = eng.roc_dcf(eng.pair_scores(emb, emb, ia, ib), labels, [tuple(float(v) for v in op) for op in DEFAULT_OPERATING_POINTS])
    assert set(default) == set(off) == TODAY
    for k in TODAY - {"scores"}:
        assert default[k] == off[k] == dcf[k]
    assert torch.equal(default["scores"], world["raw"]) and torch.equal(off["scores"], world["raw"])
    with pytest.raises(ValueError, match="rocch"):
        evaluate_trials(emb, labels, ia, ib, device=False, rocch=True)
    model = C3D2(4, 1)
    plain = VerificationPipeline(model, use_vad=False, calibration=None)
    assert plain.calibration is None and torch.equal(plain.score_trials(emb, ia, ib), world["raw"])
    pav = PavCalibration().fit(world["raw"], labels, engine=eng)
    piped = VerificationPipeline(model, use_vad=False, calibration=pav).score_trials(emb, ia, ib)
    assert torch.equal(piped, pav.apply(world["raw"], engine=eng)) and torch.equal(world["raw"], eng.pair_scores(emb, emb, ia, ib))
