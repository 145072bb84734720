"""Plda.fit / project / enroll / score through VerificationPipeline and evaluate_trials, on data drawn from the model itself.

THE SET (seed default_rng(7)): dim 24, x = mu + A y + G e with A = 0.6 N(0, 1) and G = N(0, 1) [24, 24] matrices, mu = N(0, 1),
y ~ N(0, I) per speaker and e ~ N(0, I) per utterance.  Development: 60 speakers of 2 .. 8 rows.  Evaluation: 80 UNSEEN speakers
with 1 enrolment and 3 test utterances each, every test against every enrolment (19 200 trials, 240 targets).  No length
normalisation (l2_in=False): the data IS the model.

THE CONDITION.  In float64 NumPy on the CPU (`cpu_reference()` below: solve_plda on NumPy statistics, tests/plda_f64_ref.llr,
the cosine of the rows minus the development mean) this set gives an EER of 0.83 % for the LLR against 30.32 % for the centred
cosine.  The test asks the device LLRs for an EER strictly below the centred cosine's on the same trials: a condition the
float64 reference meets with a wide margin, not a measurement of the code under test.

THE BOUNDS are the ones tests/test_plda_scores.py and tests/test_plda_pair_scores.py derive, applied to the float32 rows the
scorer was given (the device's own projection); the projection is held to tests/test_embedding_project.py's bound
(dim + 8) 2^-24 sum_k (|x_k| + |mu_k|) |V_kj| against the float64 projection, and the whole chain to the sum of the score's
bound and that projection error carried through the LLR's gradient,
    |d llr| <= sum_k |alpha_k u_k - beta_k v_k| dv_k + |alpha_k v_k - gamma_k u_k| du_k     (first order; the second order is
    2^-24 of it)."""
import numpy as np
import pytest

import plda_f64_ref as ref

torch = pytest.importorskip("torch")

DIM, N_DEV, N_EVAL, TESTS_PER = 24, 60, 80, 3
SHRINK = 1e-3


def make_world():
    """-> dict of float32 rows and ids: dev / dev_ids, enroll [80, 24], tests [240, 24] / test_ids, extra (1 .. 4 utterances
    per evaluation speaker for the enrolment test) / extra_ids."""
    rng = np.random.default_rng(7)
    mu = rng.standard_normal(DIM)
    a = 0.6 * rng.standard_normal((DIM, DIM))
    g = rng.standard_normal((DIM, DIM))

    def draw(y, ids):
        return (mu + y[ids] @ a.T + rng.standard_normal((ids.size, DIM)) @ g.T).astype(np.float32)
    dev_ids = np.repeat(np.arange(N_DEV), rng.integers(2, 9, N_DEV))
    dev = draw(rng.standard_normal((N_DEV, DIM)), dev_ids)
    y_eval = rng.standard_normal((N_EVAL, DIM))
    enroll = draw(y_eval, np.arange(N_EVAL))
    test_ids = np.repeat(np.arange(N_EVAL), TESTS_PER)
    tests = draw(y_eval, test_ids)
    extra_ids = rng.permutation(np.repeat(np.arange(N_EVAL), 1 + np.arange(N_EVAL) % 4))
    extra = draw(y_eval, extra_ids)
    return {"dev": dev, "dev_ids": dev_ids, "enroll": enroll, "tests": tests, "test_ids": test_ids, "extra": extra,
            "extra_ids": extra_ids}


def numpy_stats(x, ids):
    x = x.astype(np.float64)
    uniq = np.unique(ids)
    cm = np.stack([x[ids == c].mean(0) for c in uniq])
    d = x - cm[np.searchsorted(uniq, ids)]
    return cm, np.array([(ids == c).sum() for c in uniq]), d.T @ d


def eer64(scores, labels):
    """The EER of a score list in float64: the ROC at every distinct threshold, the crossing of fnr and fpr interpolated."""
    order = np.argsort(-scores, kind="stable")
    lab = labels[order].astype(np.float64)
    tp, fp = np.cumsum(lab), np.cumsum(1.0 - lab)
    last = np.r_[np.nonzero(np.diff(scores[order]))[0], lab.size - 1]
    fnr, fpr = np.r_[1.0, 1.0 - tp[last] / tp[-1]], np.r_[0.0, fp[last] / fp[-1]]
    k = int(np.nonzero(fpr - fnr >= 0)[0][0])
    if k == 0:
        return 0.0
    d0, d1 = fnr[k - 1] - fpr[k - 1], fnr[k] - fpr[k]
    w = d0 / (d0 - d1)
    return float(fpr[k - 1] + w * (fpr[k] - fpr[k - 1]))


def cpu_reference():
    """(EER of the float64 LLR, EER of the float64 centred cosine) on the evaluation trials."""
    from speaker_verification_amd import plda
    w = make_world()
    mean, v, psi = plda.solve_plda(*numpy_stats(w["dev"], w["dev_ids"]), shrinkage=SHRINK)
    labels = (w["test_ids"][:, None] == np.arange(N_EVAL)[None, :]).reshape(-1)
    t, e = w["tests"].astype(np.float64) - mean, w["enroll"].astype(np.float64) - mean
    llr = ref.llr(t @ v, e @ v, psi)[0].reshape(-1)
    cos = ((t / np.linalg.norm(t, axis=1, keepdims=True)) @ (e / np.linalg.norm(e, axis=1, keepdims=True)).T).reshape(-1)
    return eer64(llr, labels), eer64(cos, labels)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    from speaker_verification_amd.plda import Plda
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    w = make_world()
    model = C3D2(4, 1)
    p = Plda().fit(eng.to_device(w["dev"]), w["dev_ids"], l2_in=False, shrinkage=SHRINK, engine=eng)
    w.update(eng=eng, plda=p, model=model, plain=VerificationPipeline(model, use_vad=False),
             pipe=VerificationPipeline(model, use_vad=False, plda=p))
    return w


def project64(p, x):
    return (x.astype(np.float64) - p.mean) @ p.v


def project_bound(p, x):
    return (DIM + 8) * ref.U32 * ((np.abs(x.astype(np.float64)) + np.abs(p.mean)) @ np.abs(p.v))


def test_fit_matches_numpy(world):
    from speaker_verification_amd import plda
    p = world["plda"]
    mean, v, psi = plda.solve_plda(*numpy_stats(world["dev"], world["dev_ids"]), shrinkage=SHRINK)
    assert p.out_dim == DIM and p.psi.dtype == np.float64 and not p.l2_in
    assert np.abs(p.mean - mean).max() <= 1e-12
    np.testing.assert_allclose(p.psi, psi, rtol=1e-8, atol=0)
    print("psi: %.3f .. %.3g" % (p.psi[0], p.psi[-1]))
    # eigenvector signs are arbitrary: V diag(psi) V^T is not
    assert np.abs((p.v * p.psi) @ p.v.T - (v * psi) @ v.T).max() <= 1e-8 * np.abs((v * psi) @ v.T).max()


def test_pipeline_scores_against_the_float64_chain(world):
    eng, p, pipe = world["eng"], world["plda"], world["pipe"]
    tests, enroll = world["tests"], world["enroll"]
    got = pipe.score(tests, enroll).cpu().numpy()
    assert got.shape == (240, 80) and got.dtype == np.float32
    # the projection against float64
    tu, eu = pipe.project(tests).cpu().numpy(), pipe.project(enroll).cpu().numpy()
    t64, e64 = project64(p, tests), project64(p, enroll)
    dt, de = project_bound(p, tests), project_bound(p, enroll)
    assert (np.abs(tu - t64) <= dt).all() and (np.abs(eu - e64) <= de).all()
    # the scorer on the rows it was given
    want, _ = ref.llr(tu, eu, p.psi)
    err = np.abs(got - want)
    bound = ref.matrix_bound(tu, eu, p.psi, None, want)
    print("scores on the device's projection: worst error / bound = %.4f" % float((err / bound).max()))
    assert (err <= bound).all()
    # the whole chain: plus the projection error through the gradient of the LLR
    chain, _ = ref.llr(t64, e64, p.psi)
    alpha, beta, gamma, _ = ref.coef(p.psi, 1.0)
    carried = np.einsum("ijk,ik->ij", np.abs(alpha * e64[None, :, :] - beta * t64[:, None, :]), dt) \
        + np.einsum("ijk,jk->ij", np.abs(alpha * t64[:, None, :] - gamma * e64[None, :, :]), de)
    err = np.abs(got - chain)
    total = ref.matrix_bound(t64, e64, p.psi, None, chain) + (1.0 + ref.U32) * carried
    print("whole chain: worst error / bound = %.4f" % float((err / total).max()))
    assert (err <= total).all()


def test_llr_beats_the_centred_cosine(world):
    from speaker_verification_amd.backend import EmbeddingBackend
    from speaker_verification_amd.evaluation import evaluate_trials
    from speaker_verification_amd.pipeline import VerificationPipeline
    eng, p, pipe = world["eng"], world["plda"], world["pipe"]
    both = np.concatenate([world["tests"], world["enroll"]])
    ia = np.repeat(np.arange(240), N_EVAL)
    ib = 240 + np.tile(np.arange(N_EVAL), 240)
    labels = (world["test_ids"][ia] == ib - 240).astype(np.uint8)
    res = evaluate_trials(both, labels, ia, ib, plda=p)
    centre = EmbeddingBackend().fit(eng.to_device(world["dev"]), world["dev_ids"], method="center", l2_in=False)
    cos = evaluate_trials(both, labels, ia, ib, backend=centre)
    print("EER: LLR %.4f, centred cosine %.4f" % (res["eer"], cos["eer"]))
    assert res["eer"] < cos["eer"]
    # the trial scores: the pipeline's, bit for bit, and the pair kernel's bound on the rows it was given
    dev_both = eng.to_device(both)
    assert torch.equal(res["scores"], pipe.score_trials(dev_both, ia, ib))
    assert torch.equal(res["scores"], pipe.score_trials(dev_both[:240], ia, ib - 240, emb_b=dev_both[240:]))
    u = pipe.project(dev_both).cpu().numpy()
    want, mag = ref.llr_pairs(u, u, ia, ib, p.psi)
    err = np.abs(res["scores"].cpu().numpy() - want)
    bound = ref.U32 * np.abs(want) + (DIM + 8) * 2.0 ** -52 * mag
    print("trial scores: worst error / bound = %.4f" % float((err / bound).max()))
    assert (err <= bound).all()
    assert res["eer"] == eng.roc_dcf(res["scores"], labels)["eer"]
    # ... and the matrix entry agrees with the trial within the matrix entry's bound
    full = pipe.score(world["tests"], world["enroll"]).cpu().numpy().reshape(-1)
    mb = ref.matrix_bound(u[:240], u[240:], p.psi, None, want.reshape(240, N_EVAL)).reshape(-1)
    assert (np.abs(full - want) <= mb).all()
    with pytest.raises(ValueError, match="metric"):
        evaluate_trials(both, labels, ia, ib, metric="l2", plda=p)
    with pytest.raises(ValueError, match="index outside"):
        evaluate_trials(both, labels, ia, ib + 1, plda=p)


def test_enrolled_means_and_counts(world):
    eng, p = world["eng"], world["plda"]
    extra, ids = world["extra"], world["extra_ids"]
    uniq, models, counts = p.enroll(extra, ids, engine=eng)
    want_counts = 1 + np.arange(N_EVAL) % 4
    assert np.array_equal(uniq, np.arange(N_EVAL)) and counts.dtype == torch.int32 and models.dtype == torch.float32
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    u = p.project(extra, engine=eng)
    m64 = np.stack([u.cpu().numpy()[ids == s].astype(np.float64).mean(0) for s in range(N_EVAL)])
    got_models = models.cpu().numpy()
    assert (np.abs(got_models - m64) <= np.spacing(np.abs(m64).astype(np.float32))).all()        # float64 mean, rounded once
    _, again, _ = p.enroll(u, ids, projected=True, engine=eng)
    assert torch.equal(again, models)
    tu = p.project(world["tests"], engine=eng)
    got = p.score(tu, models, counts=counts, engine=eng).cpu().numpy()
    want, _ = ref.llr(tu.cpu().numpy(), got_models, p.psi, counts=want_counts)
    err = np.abs(got - want)
    bound = ref.matrix_bound(tu.cpu().numpy(), got_models, p.psi, want_counts, want)
    print("models of 1 .. 4 utterances: worst error / bound = %.4f" % float((err / bound).max()))
    assert (err <= bound).all()
    # by the book: a few entries against the joint Gaussians (float64 agreement 1e-10: tests/test_plda_host.py)
    for i, j in ((0, 0), (5, 1), (100, 33), (239, 79), (7, 78)):
        joint = ref.llr_joint(got_models[j].astype(np.float64), want_counts[j], tu[i].cpu().numpy().astype(np.float64), p.psi)
        assert abs(got[i, j] - joint) <= bound[i, j] + 1e-10 * abs(joint)
    # the count matters: the same models scored as single utterances differ
    single = p.score(tu, models, engine=eng).cpu().numpy()
    many = want_counts > 1
    assert (single[:, many] != got[:, many]).any()
    labels = (world["test_ids"][:, None] == np.arange(N_EVAL)[None, :]).reshape(-1)
    print("EER with mean models and counts %.4f, the same models scored as n = 1: %.4f"
          % (eng.roc_dcf(got.reshape(-1), labels)["eer"], eng.roc_dcf(single.reshape(-1), labels)["eer"]))
    with pytest.raises(ValueError, match="counts"):
        p.score(tu, models, counts=np.zeros(N_EVAL, np.int32), engine=eng)
    with pytest.raises(ValueError, match="counts"):
        p.score(tu, models, counts=want_counts[:-1], engine=eng)


def test_without_plda_nothing_changes(world, tmp_path):
    from speaker_verification_amd.evaluation import evaluate_trials
    from speaker_verification_amd.plda import Plda
    eng, plain, pipe, p = world["eng"], world["plain"], world["pipe"], world["plda"]
    tests, enroll = eng.to_device(world["tests"]), eng.to_device(world["enroll"])
    assert plain.plda is None and plain.project(tests) is tests
    assert torch.equal(plain.score(tests, enroll), eng.cosine_scores(tests, enroll))
    ia, ib = np.arange(240), np.arange(240) % N_EVAL
    assert torch.equal(plain.score_trials(tests, ia, ib, emb_b=enroll), eng.pair_scores(tests, enroll, ia, ib))
    assert torch.equal(plain.score_trials(tests, ia, ib, emb_b=enroll, metric="l2"), eng.pair_scores(tests, enroll, ia, ib, metric="l2"))
    labels = (world["test_ids"] == ib).astype(np.uint8)
    both = torch.cat([tests, enroll])
    assert torch.equal(evaluate_trials(both, labels, ia, ib + 240)["scores"], eng.pair_scores(both, both, ia, ib + 240))
    with pytest.raises(ValueError, match="counts"):
        plain.score(tests, enroll, counts=np.ones(N_EVAL, np.int32))
    with pytest.raises(ValueError, match="search"):
        pipe.search(tests, enroll, k=1)
    plain.search(tests, enroll, k=1)
    # the projection is svk_embedding_project with the model's float32 mean and V, no length norm
    proj = pipe.project(tests)
    assert torch.equal(proj, eng.embedding_project(tests, mean=p.mean.astype(np.float32), w=p.v.astype(np.float32)))
    assert torch.equal(pipe.score(tests, enroll), eng.plda_scores(proj, pipe.project(enroll), p.psi))
    # save / load: identical bits
    path = str(tmp_path / "plda.npz")
    p.save(path)
    again = Plda.load(path)
    assert torch.equal(again.score(again.project(tests), again.project(enroll)), pipe.score(tests, enroll))
