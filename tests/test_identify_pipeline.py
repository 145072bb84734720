"""`VerificationPipeline.identify` and `evaluation.rank_speakers(pipeline=...)`: the k best enrolled rows under the scores
`score` gives, without the matrix.  A seeded Gaussian mixture (tests/test_score_norm_pipeline.py's: 40 speakers x 6 rows of
dim 128, a cohort of 300 rows, a development set for the back end and the calibration).

`identify` is held to `Engine.cosine_topk_norm` fed by `ScoreNorm.side_moments` AS BYTES (whole, chunked, from a host gallery),
and to `search` as bytes without normalisation and calibration.  Against `score` the two routes may differ: `score` takes its
raw cosines from svk_cosine_scores, `identify` from the search's product.  Each is held to float64 within 1e-5 elsewhere
(tests/test_scoring_float64.py, tests/test_cosine_topk.py), so two raw scores differ by at most 2e-5; the expression scales
that by its gain g = 0.5 (1 / sd_q + 1 / sd_g) (1 / sd for a single table) and each result is rounded to float32 once:
BOUND = 2e-5 g + 2^-23 |value|."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DIM, SEED, TOP_K, K = 128, 1, 50, 5


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


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.backend import EmbeddingBackend
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.score_norm import ScoreNorm
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    w = {k: (eng.to_device(v) if v.dtype == np.float32 else v) for k, v in corpus().items()}
    w["host"] = corpus()
    w["eng"], w["model"] = eng, C3D2(4, 1)
    w["test"], w["enroll"] = w["eval"][:100], w["eval"][100:]
    w["backend"] = EmbeddingBackend().fit(w["dev"], w["dev_ids"], method="lda", out_dim=20, shrinkage=1e-3, engine=eng)
    w["sn"] = {(mode, b): ScoreNorm(top_k=TOP_K, mode=mode).fit(w["cohort"], backend=w["backend"] if b else None, engine=eng)
               for mode in "zts" for b in (False, True)}
    return w


def pipeline(world, **kw):
    from speaker_verification_amd.pipeline import VerificationPipeline
    return VerificationPipeline(world["model"], use_vad=False, **kw)


def same(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


@pytest.mark.parametrize("with_backend", (False, True), ids=("cosine", "lda"))
@pytest.mark.parametrize("mode", ("z", "t", "s"))
def test_identify_is_the_engine_entry_fed_by_side_moments(world, mode, with_backend):
    eng, sn = world["eng"], world["sn"][(mode, with_backend)]
    backend = world["backend"] if with_backend else None
    pipe = pipeline(world, backend=backend, score_norm=sn)
    test, enroll = world["test"], world["enroll"]
    u_t, u_e = pipe.project(test), pipe.project(enroll)
    tm, em = sn.side_moments(u_t, u_e)
    want = eng.cosine_topk_norm(u_t, u_e, K, query_moments=tm, gallery_moments=em)
    assert (tm is None) == (mode == "z") and (em is None) == (mode == "t")
    assert same(pipe.identify(test, enroll, k=K), want)
    assert same(pipe.identify(test, enroll, k=K, chunk_rows=7), want)
    assert same(pipe.identify(test, world["host"]["eval"][100:], k=K), want)
    small = pipeline(world, backend=backend, score_norm=sn)
    small.SEARCH_UPLOAD_BYTES = 4 * 128 * 33                      # a host gallery above this goes up in chunks of 33 rows
    assert same(small.identify(test, world["host"]["eval"][100:], k=K), want)
    if mode != "t":
        assert not torch.equal(want[1], eng.cosine_topk(u_t, u_e, K)[1])     # not the raw ranking
    # a self-search: row q is no candidate for query q
    own = pipe.identify(enroll, enroll, k=K, exclude_self=True, chunk_rows=50)
    row, col = sn._tables(*sn.side_moments(u_e, u_e))            # (one tensor on both sides: one table serves both)
    n = int(u_e.shape[0])
    assert same(own, eng.cosine_topk_norm(u_e, u_e, K, query_moments=row, gallery_moments=col, exclude=torch.arange(n)))
    assert not bool((own[1] == torch.arange(n, device=eng.device)[:, None]).any())


def test_without_normalisation_and_calibration_it_is_search(world):
    test, enroll = world["test"], world["enroll"]
    for backend in (None, world["backend"]):
        pipe = pipeline(world, backend=backend)
        assert same(pipe.identify(test, enroll, k=K), pipe.search(test, enroll, k=K))
        assert same(pipe.identify(test, enroll, k=K, chunk_rows=7), pipe.search(test, enroll, k=K))
        assert same(pipe.identify(enroll, enroll, k=K, exclude_self=True), pipe.search(enroll, enroll, k=K, exclude_self=True))


@pytest.mark.parametrize("mode", ("z", "t", "s"))
def test_against_the_matrix_of_score(world, mode):
    sn = world["sn"][(mode, False)]
    pipe = pipeline(world, score_norm=sn)
    test, enroll = world["test"], world["enroll"]
    matrix = pipe.score(test, enroll).double().cpu().numpy()
    tm, em = sn.side_moments(test, enroll)
    gain = np.zeros_like(matrix)
    if tm is not None:
        gain += (0.5 if mode == "s" else 1.0) / tm.cpu().numpy()[:, 1][:, None]
    if em is not None:
        gain += (0.5 if mode == "s" else 1.0) / em.cpu().numpy()[:, 1][None, :]
    assert np.isfinite(gain).all() and (gain > 0).all()
    scores, indices = (t.cpu().numpy() for t in pipe.identify(test, enroll, k=K))
    rows = np.arange(matrix.shape[0])[:, None]
    bound = 2e-5 * gain[rows, indices] + 2.0 ** -23 * np.abs(scores.astype(np.float64))
    worst = np.abs(scores.astype(np.float64) - matrix[rows, indices]) / bound
    print("mode %s: largest |identify - score| / bound = %.3g" % (mode, worst.max()))
    assert (worst <= 1.0).all()
    # nothing outside a list beats the list's last entry by more than the bound
    outside = np.ones_like(matrix, dtype=bool)
    outside[rows, indices] = False
    last = scores[:, -1].astype(np.float64)[:, None]
    excess = (matrix - last) / (2e-5 * gain + 2.0 ** -23 * np.abs(matrix))
    print("mode %s: largest (outside entry - last listed) / bound = %.3g" % (mode, excess[outside].max()))
    assert (excess[outside] <= 1.0).all()
    assert (np.diff(scores, axis=1) <= 0).all()


def _calibration(world, pipe):
    """An affine calibration fitted on this pipeline's scores of labelled development trials."""
    from speaker_verification_amd import calibration as cal
    from speaker_verification_amd.evaluation import make_trials
    labels, ia, ib = make_trials(world["dev_ids"], 400, 4000, seed=3)
    scores = pipe.score_trials(world["dev"], ia, ib)
    return cal.Calibration(p_target=0.05).fit(scores, labels, engine=world["eng"])


def test_calibrated_identify_and_open_set_rejection(world):
    from speaker_verification_amd import calibration as cal
    from speaker_verification_amd.evaluation import rank_speakers
    eng, sn = world["eng"], world["sn"][("s", False)]
    normed = pipeline(world, score_norm=sn)
    c = _calibration(world, normed)
    assert c.n_sys == 1 and c.weights_[0] > 0
    both = pipeline(world, score_norm=sn, calibration=c)
    test, enroll = world["test"], world["enroll"]
    plain, got = normed.identify(test, enroll, k=K), both.identify(test, enroll, k=K)
    assert torch.equal(got[1], plain[1])
    assert torch.equal(got[0].reshape(-1).view(torch.int32), c.apply(plain[0].reshape(-1).clone(), engine=eng).view(torch.int32))
    assert bool((got[0][:, 1:] <= got[0][:, :-1]).all())                   # non-increasing along a list
    # past the enrolled rows: -1 and -inf, which an increasing map leaves -inf
    few = both.identify(test[:3], enroll[:2], k=4)
    assert bool((few[1][:, 2:] == -1).all()) and bool((few[0][:, 2:] == -np.inf).all())
    # a calibration alone (no normalisation) ranks as search does
    c_raw = _calibration(world, pipeline(world))
    alone = pipeline(world, calibration=c_raw).identify(test, enroll, k=K)
    raw = pipeline(world).search(test, enroll, k=K)
    assert torch.equal(alone[1], raw[1]) and torch.equal(alone[0].reshape(-1), c_raw.apply(raw[0].reshape(-1).clone(), engine=eng))
    # open set: rank_speakers rejects the calibrated scores at the Bayes threshold
    ids = ["spk%d" % s for s in world["eval_ids"][100:]]
    thr = cal.bayes_threshold(0.05)
    ranked = rank_speakers(test, enroll, ids, k=K, threshold=thr, pipeline=both)
    assert np.array_equal(ranked["indices"], got[1].cpu().numpy()) and np.array_equal(ranked["scores"], got[0].cpu().numpy())
    keep = ~(ranked["scores"] < np.float32(thr))
    assert keep.any() and not keep.all()
    for row, row_keep, row_idx in zip(ranked["ids"], keep, ranked["indices"]):
        assert row == [ids[j] if ok else None for j, ok in zip(row_idx, row_keep)]
    # the default path is untouched
    default = rank_speakers(test, enroll, ids, k=K)
    assert np.array_equal(default["indices"], eng.cosine_topk(test, enroll, K)[1].cpu().numpy())


def test_what_identify_refuses(world):
    from speaker_verification_amd import calibration as cal
    from speaker_verification_amd.plda import Plda
    eng = world["eng"]
    test, enroll = world["test"], world["enroll"]
    plda = Plda().fit(world["dev"], world["dev_ids"], l2_in=False, shrinkage=1e-3, engine=eng)
    with pytest.raises(ValueError, match="PLDA"):
        pipeline(world, plda=plda).identify(test, enroll)
    for weight in (0.0, -1.5):
        c = cal.Calibration()
        c.weights_ = np.array([weight, 0.25])
        with pytest.raises(ValueError, match="weight"):
            pipeline(world, calibration=c).identify(test, enroll)
    two = cal.Calibration()
    two.weights_ = np.array([1.0, 0.5, 0.0])
    pipe = pipeline(world)
    pipe.calibration = two                                          # (the constructor refuses it already)
    with pytest.raises(ValueError, match="ONE system"):
        pipe.identify(test, enroll)
    pipe = pipeline(world, backend=world["backend"])
    pipe.score_norm = world["sn"][("s", False)]                     # fitted without the back end
    with pytest.raises(ValueError, match="another back end"):
        pipe.identify(test, enroll)
    with pytest.raises(ValueError, match="exclude_self"):
        pipeline(world, score_norm=world["sn"][("s", False)]).identify(test, enroll, exclude_self=True)
    # search keeps refusing, in the words it always used
    for kw, word in ((dict(plda=plda), "PLDA"), (dict(score_norm=world["sn"][("s", False)]), "normalised")):
        with pytest.raises(ValueError, match=word):
            pipeline(world, **kw).search(test, enroll)
