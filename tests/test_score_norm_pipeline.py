"""Score normalisation through `ScoreNorm`, `VerificationPipeline` and `evaluate_trials`, on a seeded Gaussian mixture: 40
speakers x 6 rows of dim 128 (a speaker centre of unit variance per coordinate plus session noise of standard deviation 2:
within-speaker cosines around 0.2, an EER of several percent), a cohort of 300 rows from 100 other speakers, and a third set
of speakers that fits the PLDA.

The EER check compares the device chain with a float64 / longdouble restatement of it (`reference_snorm`).  The two agree to
1e-12 when both order the scores around the EER point alike; the device's normalised scores carry the float32 rounding of
the cohort cosines and of the result (CHAIN_TOL below), so the seed is chosen -- and `test_the_seed_...` checks on the CPU --
that no two reference scores around the EER point lie within CHAIN_TOL of each other (1e-6 is what is needed at least)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_f64_ref as ref  # noqa: E402

DIM, SEED, TOP_K = 128, 1, 50
# what the device's normalised scores may differ from the float64 restatement by: the cohort cosines are f32 sums over 128
# products (their error, some 1e-7, is averaged by the mean of 50 but divided by a std of about 0.03), and the result, below
# 16 in magnitude, is rounded to float32 (2^-24 * 16 = 1e-6)
CHAIN_TOL = 1e-4
gpu = pytest.mark.gpu


def corpus():
    """-> dict of float32 embeddings and their speaker ids: eval (40 x 6), cohort (100 x 3), dev (60 x 5)."""
    rng = np.random.default_rng(SEED)

    def draw(n_spk, per):
        ids = np.repeat(np.arange(n_spk), per)
        centres = rng.standard_normal((n_spk, DIM))
        return (centres[ids] + 2.0 * rng.standard_normal((ids.size, DIM))).astype(np.float32), ids
    out = {}
    out["eval"], out["eval_ids"] = draw(40, 6)
    out["cohort"], out["cohort_ids"] = draw(100, 3)
    out["dev"], out["dev_ids"] = draw(60, 5)
    return out


def trials(ids):
    from speaker_verification_amd.evaluation import make_trials
    return make_trials(ids, 400, 4000, seed=3)


def reference_snorm(emb, cohort, ia, ib, top_k):
    """Cosine S-norm of the trials in float64 / longdouble, nothing from the library -> float64 [n_trials]."""
    def unit(x):
        x = x.astype(np.float64)
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    e, c = unit(emb), unit(cohort)
    against = e @ c.T
    mom = np.empty((e.shape[0], 2), dtype=ref.LD)
    for i in range(e.shape[0]):
        top = np.sort(against[i])[against.shape[1] - top_k:].astype(ref.LD)
        mom[i] = top.mean(), np.sqrt(((top - top.mean()) ** 2).mean())
    raw = np.einsum("ij,ij->i", e[ia], e[ib]).astype(ref.LD)
    return (0.5 * ((raw - mom[ia, 0]) / mom[ia, 1] + (raw - mom[ib, 0]) / mom[ib, 1])).astype(np.float64)


def test_the_seed_keeps_the_reference_scores_around_the_eer_point_apart():
    data = corpus()
    labels, ia, ib = trials(data["eval_ids"])
    scores = reference_snorm(data["eval"], data["cohort"], ia, ib, TOP_K)
    order = np.argsort(-scores)
    s, tar = scores[order], labels[order] != 0
    miss, fa = 1.0 - np.cumsum(tar) / tar.sum(), np.cumsum(~tar) / (~tar).sum()
    at = int(np.nonzero(fa >= miss)[0][0])                    # the first threshold at which false accepts reach the misses
    assert 0.02 < fa[at] < 0.3                                # a crossing worth the name
    near = s[max(0, at - 8):at + 9]
    assert np.min(-np.diff(near)) > CHAIN_TOL                 # (1e-6 would do for exact cohort scores; seed 1 leaves 6e-4)


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.plda import Plda
    from speaker_verification_amd.score_norm import ScoreNorm
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    w = {k: (eng.to_device(v) if v.dtype == np.float32 else v) for k, v in corpus().items()}
    w["host"] = corpus()
    w["eng"], w["model"] = eng, C3D2(4, 1)
    w["trials"] = trials(w["eval_ids"])
    w["sn"] = ScoreNorm(top_k=TOP_K, mode="s").fit(w["cohort"], engine=eng)
    w["plda"] = Plda().fit(w["dev"], w["dev_ids"], l2_in=False, shrinkage=1e-3, engine=eng)
    return w


def pipeline(world, **kw):
    from speaker_verification_amd.pipeline import VerificationPipeline
    return VerificationPipeline(world["model"], use_vad=False, **kw)


@gpu
def test_none_is_the_default_and_changes_no_bit(world):
    from speaker_verification_amd.evaluation import evaluate_trials
    labels, ia, ib = world["trials"]
    a, b = world["eval"][:100], world["eval"][100:]
    plain, off = pipeline(world), pipeline(world, score_norm=None)
    assert plain.score_norm is None
    assert torch.equal(plain.score(a, b), off.score(a, b))
    assert torch.equal(plain.score(a, b), world["eng"].cosine_scores(a, b))
    assert torch.equal(plain.score_trials(world["eval"], ia, ib), off.score_trials(world["eval"], ia, ib))
    today, same = evaluate_trials(world["eval"], labels, ia, ib), evaluate_trials(world["eval"], labels, ia, ib, score_norm=None)
    assert set(today) == set(same)
    assert torch.equal(today.pop("scores"), same.pop("scores")) and today == same
    assert torch.equal(plain.score_trials(world["eval"], ia, ib), world["eng"].pair_scores(world["eval"], world["eval"], ia, ib))


@gpu
@pytest.mark.parametrize("mode", ["s", "t", "z"])
def test_cosine_norm_through_the_pipeline_equals_the_entries_composed_by_hand(world, mode):
    from speaker_verification_amd.score_norm import ScoreNorm
    eng, cohort = world["eng"], world["cohort"]
    a, b = world["eval"][:100], world["eval"][100:]
    sn = ScoreNorm(top_k=TOP_K, mode=mode).fit(cohort, engine=eng)
    got = pipeline(world, score_norm=sn).score(a, b)
    raw = eng.cosine_scores(a, b)
    tm = eng.cohort_moments(eng.cosine_scores(a, cohort), TOP_K)
    em = eng.cohort_moments(eng.cosine_scores(b, cohort), TOP_K)
    want = eng.score_norm(raw, tm if mode in "ts" else None, em if mode in "zs" else None)
    assert torch.equal(got, want) and not torch.equal(got, raw)
    assert torch.equal(sn.moments(a, "test"), tm) and torch.equal(sn.moments(b, "enroll"), em)
    # and the whole chain against the float64 restatement, for the S-norm
    if mode == "s":
        ia, ib = np.repeat(np.arange(100), 140), np.tile(np.arange(100, 240), 100)
        want64 = reference_snorm(world["host"]["eval"], world["host"]["cohort"], ia, ib, TOP_K).reshape(100, 140)
        assert np.max(np.abs(got.cpu().numpy() - want64)) < CHAIN_TOL


@gpu
def test_chunked_cohort_scores_give_the_bits_of_one_chunk(world):
    from speaker_verification_amd.score_norm import ScoreNorm
    eng = world["eng"]
    small = ScoreNorm(top_k=TOP_K).fit(world["cohort"], engine=eng)
    small.SCORE_BYTES = 7 * 4 * 300                            # seven rows of cohort scores at a time
    for side in ("test", "enroll"):
        assert torch.equal(small.moments(world["eval"], side), world["sn"].moments(world["eval"], side))
    assert ScoreNorm.SCORE_BYTES == 256 << 20


@gpu
def test_score_trials_gives_the_entries_of_the_normalised_matrix(world):
    eng, sn = world["eng"], world["sn"]
    _, ia, ib = world["trials"]
    emb = world["eval"]
    pipe, plain = pipeline(world, score_norm=sn), pipeline(world)
    got = pipe.score_trials(emb, ia, ib)
    tm, em = sn.moments(emb, "test"), sn.moments(emb, "enroll")
    raw_trials, raw_matrix = plain.score_trials(emb, ia, ib), plain.score(emb, emb)
    assert torch.equal(got, eng.score_norm_pairs(raw_trials, tm, ia, em, ib))
    matrix = pipe.score(emb, emb)
    ja, jb = torch.from_numpy(ia).to(eng.device), torch.from_numpy(ib).to(eng.device)
    # the same raw scores through both forms: the same bits
    assert torch.equal(sn.normalize_trials(raw_matrix[ja, jb], tm, ia, em, ib), matrix[ja, jb])
    # the trial list's raw cosines are float64 sums rounded once, the matrix's are f32 sums: what separates the two raw
    # scores, scaled by the normalisation's slope, plus one float32 rounding of each result
    slope = 0.5 * (1.0 / tm[ja, 1] + 1.0 / em[jb, 1])
    tol = (raw_trials.double() - raw_matrix[ja, jb].double()).abs() * slope * (1 + 1e-6) + 2.0 ** -23 * matrix[ja, jb].abs().double()
    assert bool(((got.double() - matrix[ja, jb].double()).abs() <= tol).all())


@gpu
def test_plda_enrol_side_moments_take_the_cohort_as_the_test_side(world):
    from speaker_verification_amd.pipeline import enroll_mean
    from speaker_verification_amd.score_norm import ScoreNorm
    eng, plda = world["eng"], world["plda"]
    sn = ScoreNorm(top_k=TOP_K).fit(world["cohort"], speaker_ids=world["cohort_ids"], plda=plda, engine=eng)
    assert tuple(sn.cohort.shape) == (100, plda.out_dim) and sn.cohort_counts.cpu().tolist() == [3] * 100
    _, models, counts = plda.enroll(world["eval"], world["eval_ids"], engine=eng)
    assert counts.cpu().tolist() == [6] * 40
    enrol_side = sn.moments(models, "enroll", counts)
    by_hand = eng.cohort_moments(plda.score(sn.cohort, models, counts=counts, engine=eng).t().contiguous(), TOP_K)
    assert torch.equal(enrol_side, by_hand)
    test_side = sn.moments(models, "test")
    assert torch.equal(test_side, eng.cohort_moments(plda.score(models, sn.cohort, counts=sn.cohort_counts, engine=eng), TOP_K))
    # the LLR is not symmetric: a model of six utterances against a cohort model is not the cohort model against it
    assert float((enrol_side[:, 0] - test_side[:, 0]).abs().median()) > 1e-3 and not torch.allclose(enrol_side, test_side)
    # through the pipeline: raw mean models, which the pipeline projects (a model fitted with l2_in=False)
    test_rows = world["eval"][::6]
    _, raw_models = enroll_mean(world["eval"], world["eval_ids"], l2=False)
    pipe = pipeline(world, plda=plda, score_norm=sn)
    got = pipe.score(test_rows, raw_models, counts=counts)
    u_t, u_m = pipe.project(test_rows), pipe.project(raw_models)
    raw = plda.score(u_t, u_m, counts=counts, engine=eng)
    want = eng.score_norm(raw, sn.moments(u_t, "test"), sn.moments(u_m, "enroll", counts))
    assert torch.equal(got, want) and torch.equal(pipeline(world, plda=plda).score(test_rows, raw_models, counts=counts), raw)
    with pytest.raises(ValueError, match="another back end"):
        pipeline(world, score_norm=sn)                         # fitted for the PLDA scorer, not the cosine
    with pytest.raises(ValueError, match="counts"):
        world["sn"].moments(world["eval"], "enroll", counts=np.ones(240, dtype=np.int32))


@gpu
def test_the_calibration_comes_after_the_normalisation(world):
    from speaker_verification_amd import calibration as cal
    eng, sn = world["eng"], world["sn"]
    labels, ia, ib = world["trials"]
    emb = world["eval"]
    normed = pipeline(world, score_norm=sn).score_trials(emb, ia, ib)
    c = cal.Calibration(p_target=0.05).fit(normed, labels, engine=eng)
    assert c.converged_
    both = pipeline(world, score_norm=sn, calibration=c)
    got = both.score_trials(emb, ia, ib)
    assert torch.equal(got, c.apply(normed, engine=eng))
    raw = pipeline(world).score_trials(emb, ia, ib)
    tm, em = sn.moments(emb, "test"), sn.moments(emb, "enroll")
    other_order = eng.score_norm_pairs(c.apply(raw, engine=eng), tm, ia, em, ib)
    assert not torch.allclose(got, other_order)
    a, b = emb[:50], emb[50:120]
    assert torch.equal(both.score(a, b).reshape(-1), c.apply(pipeline(world, score_norm=sn).score(a, b).reshape(-1), engine=eng))
    with pytest.raises(ValueError, match="search"):
        both.search(a, b)
    with pytest.raises(ValueError, match="normalised"):
        pipeline(world, score_norm=sn).search(a, b)


@gpu
def test_evaluate_trials_reports_the_metrics_of_the_normalised_scores(world):
    from speaker_verification_amd.evaluation import evaluate_trials, get_eer_auc
    eng, sn = world["eng"], world["sn"]
    labels, ia, ib = world["trials"]
    res = evaluate_trials(world["eval"], labels, ia, ib, score_norm=sn)
    assert torch.equal(res["scores"], pipeline(world, score_norm=sn).score_trials(world["eval"], ia, ib))
    direct = eng.roc_dcf(res["scores"], labels, [(0.01, 1, 1), (0.05, 1, 1)])
    assert res["eer"] == direct["eer"] and res["min_dcf"] == direct["min_dcf"]
    want = reference_snorm(world["host"]["eval"], world["host"]["cohort"], ia, ib, TOP_K)
    assert np.max(np.abs(res["scores"].cpu().numpy() - want)) < CHAIN_TOL
    eer = get_eer_auc(labels, want)[0]
    raw = evaluate_trials(world["eval"], labels, ia, ib)
    print("EER raw %.4f, S-normed %.4f (reference %.4f)" % (raw["eer"], res["eer"], eer))
    assert abs(res["eer"] - eer) <= 1e-12
    host = evaluate_trials(world["eval"], labels, ia, ib, score_norm=sn, device=False)
    assert abs(host["eer"] - eer) <= 1e-12
