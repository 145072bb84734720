"""EmbeddingBackend.fit / transform through VerificationPipeline and evaluate_trials on a synthetic set whose nuisance a back end
must remove.

THE SET.  A shared generator (seed 1234) draws the speaker map B = N(0, 1) / sqrt(128) [128, 128] and 8 nuisance directions
N [8, 128].  A set is  spk @ B  (one N(0, 1) [128] draw per speaker, repeated per utterance)  + 3 N(0, 1)[., 8] @ N / sqrt(8)
(a session offset in the nuisance subspace, larger than the speaker term)  + 0.15 N(0, 1)  + 0.5.  Training: 40 speakers x 12,
seed 1; evaluation: 30 UNSEEN speakers x 8, seed 2.  In float64 NumPy the all-pairs cosine EER of the raw evaluation rows is
0.44 and after LDA (l2_in on or off, out_dim 39 or 20, shrinkage 1e-3) it is 0.000: the assertions below (raw >= 0.30,
projected <= 0.05) are conditions that reference meets with a wide margin, not measurements of the code under test."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def make_set(seed, n_spk, per):
    g = np.random.default_rng(1234)
    b = g.standard_normal((128, 128)) / np.sqrt(128)
    nuis = g.standard_normal((8, 128))
    r = np.random.default_rng(seed)
    spk = r.standard_normal((n_spk, 128))
    n = n_spk * per
    x = np.repeat(spk @ b, per, axis=0) + 3.0 * r.standard_normal((n, 8)) @ nuis / np.sqrt(8) \
        + 0.15 * r.standard_normal((n, 128)) + 0.5
    return x.astype(np.float32), np.repeat(np.arange(n_spk), per)


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.backend import EmbeddingBackend
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    train, train_ids = make_set(1, 40, 12)
    test, test_ids = make_set(2, 30, 8)
    model = C3D2(4, 1)
    plain = VerificationPipeline(model, use_vad=False)
    return {"eng": eng, "train": eng.to_device(train), "train_ids": train_ids, "test": eng.to_device(test), "test_ids": test_ids,
            "plain": plain, "model": model, "Backend": EmbeddingBackend, "Pipeline": VerificationPipeline}


def all_pairs_eer(eng, scores, ids):
    i, j = np.triu_indices(len(ids), 1)
    sc = scores.cpu().numpy()[i, j]
    return eng.roc_dcf(sc, (ids[i] == ids[j]).astype(np.uint8))["eer"]


@pytest.mark.parametrize("l2_in,out_dim", [(True, None), (True, 20), (False, 39), (False, 20)])
def test_lda_removes_the_nuisance(world, l2_in, out_dim):
    from speaker_verification_amd.evaluation import evaluate_trials, make_trials
    eng, test, ids = world["eng"], world["test"], world["test_ids"]
    b = world["Backend"]().fit(world["train"], world["train_ids"], method="lda", out_dim=out_dim, l2_in=l2_in, shrinkage=1e-3)
    assert b.out_dim == (39 if out_dim is None else out_dim) and b.w.dtype == np.float64
    pipe = world["Pipeline"](world["model"], use_vad=False, backend=b)
    raw = all_pairs_eer(eng, world["plain"].score(test, test), ids)
    projected = all_pairs_eer(eng, pipe.score(test, test), ids)
    labels, ia, ib = make_trials(ids, 800, 4000, 7)
    raw_t = eng.roc_dcf(world["plain"].score_trials(test, ia, ib), labels)["eer"]
    proj_scores = pipe.score_trials(test, ia, ib)
    proj_t = eng.roc_dcf(proj_scores, labels)["eer"]
    print("l2_in %d out_dim %s: all-pairs EER %.4f -> %.4f, trial-list EER %.4f -> %.4f" % (l2_in, out_dim, raw, projected, raw_t, proj_t))
    assert raw >= 0.30 and raw_t >= 0.30
    assert projected <= 0.05 and proj_t <= 0.05
    # evaluate_trials with the back end: the same scores
    res = evaluate_trials(test, labels, ia, ib, backend=b)
    assert torch.equal(res["scores"], proj_scores) and res["eer"] == proj_t
    assert torch.equal(evaluate_trials(test, labels, ia, ib)["scores"], world["plain"].score_trials(test, ia, ib))


def test_wiring_bits(world, tmp_path):
    eng, test = world["eng"], world["test"]
    b = world["Backend"]().fit(world["train"], world["train_ids"], method="lda", out_dim=20)
    pipe, plain = world["Pipeline"](world["model"], use_vad=False, backend=b), world["plain"]
    proj = pipe.project(test)
    assert tuple(proj.shape) == (240, 20) and proj.dtype == torch.float32 and proj.is_cuda
    assert torch.equal(proj, b.transform(test)) and plain.project(test) is test
    unit = proj.double().norm(dim=1).cpu().numpy()
    assert np.abs(unit - 1.0).max() < 1e-6                                                # l2_out is on by default
    gallery, query = test[::8], test[1::8]
    # with the back end: score == score on the projected rows; without: today's bits
    assert torch.equal(pipe.score(query, gallery), plain.score(pipe.project(query), pipe.project(gallery)))
    assert torch.equal(plain.score(query, gallery), eng.cosine_scores(query, gallery))
    ia = torch.arange(0, 30, dtype=torch.int64)
    assert torch.equal(pipe.score_trials(query, ia, ia, emb_b=gallery),
                       plain.score_trials(pipe.project(query), ia, ia, emb_b=pipe.project(gallery)))
    # search: the top-1 of the projected score matrix, chunked or not
    want = pipe.score(test, gallery).argmax(dim=1)
    for chunk_rows in (None, 7):
        _, idx = pipe.search(test, gallery, k=1, chunk_rows=chunk_rows)
        assert torch.equal(idx[:, 0], want)
    _, idx = pipe.search(test, gallery.cpu().numpy(), k=3)                                # a host gallery
    assert torch.equal(idx[:, 0], want)
    _, idx_plain = plain.search(test, gallery, k=1)
    assert torch.equal(idx_plain[:, 0], plain.score(test, gallery).argmax(dim=1))
    # every query's own speaker wins after the projection
    assert torch.equal(want.cpu(), torch.arange(30).repeat_interleave(8))
    # save / load: identical bits
    path = str(tmp_path / "lda.npz")
    b.save(path)
    again = world["Backend"].load(path)
    assert torch.equal(again.transform(test), proj) and again.method == "lda" and again.out_dim == 20


@pytest.mark.parametrize("method", ["center", "whiten", "wccn"])
def test_other_methods_against_float64(world, method):
    """fit + transform against the float64 NumPy route on the same rows: statistics, solve, projection."""
    from speaker_verification_amd import backend
    x = world["train"].cpu().numpy().astype(np.float64)
    ids = world["train_ids"]
    v = x / np.linalg.norm(x, axis=1, keepdims=True)
    cm = np.stack([v[ids == c].mean(0) for c in range(40)])
    d = v - cm[ids]
    mean, w = backend.solve(cm, np.full(40, 12), d.T @ d, method, shrinkage=1e-3)
    b = world["Backend"]().fit(world["train"], ids, method=method, l2_in=True, shrinkage=1e-3)
    # the device statistics differ from NumPy's by float64 roundings; solve is conditioned by the shrinkage (cond ~ 1e3-1e5)
    assert np.abs(b.mean - mean).max() <= 1e-12
    t = world["test"].cpu().numpy().astype(np.float64)
    t = t / np.linalg.norm(t, axis=1, keepdims=True)
    # eigenvector signs are arbitrary: compare what scoring sees, the cosine matrix of the projected rows (f32 products: 1e-4)
    y = (t - mean) if w is None else (t - mean) @ w
    y = y / np.linalg.norm(y, axis=1, keepdims=True)
    got = b.transform(world["test"]).cpu().numpy().astype(np.float64)
    assert got.shape == y.shape
    assert np.abs(got @ got.T - y @ y.T).max() <= 1e-4
