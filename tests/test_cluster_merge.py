"""`clustering.merge_clusters` and `clustering.adopt_rows` on the device, step by step: with trace=True every
round's centroids are `clustering.centroids`' bits, every k-NN round's labels EQUAL tests/knn_cluster_ref.py run on that
round's device lists, the linkage stage's labels EQUAL tests/ahc_f64_ref.py run on its device affinity, the labels compose as
the reference composes them, and the end is the truth: 40 pure clusters of 25, 8 of 123.  tests/test_cluster_merge_host.py
establishes in float64 that every centroid cosine these runs decide on lies at least 0.08 from the threshold 0.5 (same
speaker >= 0.586, others <= 0.378), where the device's float32 centroids and cosines move a value by about 1e-6: that is
why equality with the truth is a fair demand.  The first-stage labels are the float64 reference's (k = 10, threshold 0.5,
min_shared 3), the fragments tests/test_cluster_merge_host.py looks at."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ahc_f64_ref as A           # noqa: E402  (tests/ is on sys.path)
import cluster_corpus as D        # noqa: E402
import cluster_merge_ref as M     # noqa: E402
import knn_cluster_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    w = dict(eng=eng, pipe=VerificationPipeline(C3D2(4, 1), use_vad=False))
    for name, corpus in (("40", D.corpus), ("8", M.corpus8)):
        emb, speaker = corpus(0)
        w[name] = dict(emb=emb, dev=eng.to_device(emb), speaker=speaker, first=M.first_stage(emb, 10, 0.5, 3, 1))
    w["40"]["first5"] = M.first_stage(w["40"]["emb"], 10, 0.5, 3, 5)
    return w


def _np(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and \
        [(r["kind"], r["clusters_in"], r["clusters_out"]) for r in a.rounds] == \
        [(r["kind"], r["clusters_in"], r["clusters_out"]) for r in b.rounds]


def held_to_the_references(eng, dev, first, got, threshold, k, mutual=True, min_shared=0, num_clusters=None):
    """Walks the trace; -> the rows' labels as the references compose them."""
    from speaker_verification_amd import clustering as K
    cur = np.asarray(first, dtype=np.int64)
    for rnd in got.rounds:
        C = int(cur.max()) + 1
        assert rnd["clusters_in"] == C
        cent = K.centroids(eng, dev, cur, l2_rows=True, l2_mean=True)
        assert rnd["centroids"].dtype == torch.float32 and torch.equal(rnd["centroids"].view(torch.int32), cent.view(torch.int32))
        if rnd["kind"] == "knn":
            assert tuple(rnd["scores"].shape) == tuple(rnd["indices"].shape) == (C, k)
            want, _, _, counts = R.cluster(_np(rnd["indices"]), _np(rnd["scores"]), k, threshold, min_shared, mutual, 1)
            left = int(counts[0])
        else:
            assert rnd is got.rounds[-1] and tuple(rnd["affinity"].shape) == (C, C)
            want, left, _, _ = A.ahc(_np(rnd["affinity"]), C, threshold, 1, C, num_clusters)
        assert rnd["labels"].dtype == torch.int32 and np.array_equal(_np(rnd["labels"]), want) and rnd["clusters_out"] == left
        cur = M.through(want, cur)
    labels, sizes, counts, fragment_map = (_np(t) for t in got[:4])
    C = int(cur.max()) + 1
    assert all(a.dtype == np.int32 for a in (labels, sizes, counts, fragment_map)) and np.array_equal(labels, cur)
    assert np.array_equal(sizes[:C], np.bincount(cur[cur >= 0], minlength=C)) and not sizes[C:].any() and sizes.size == cur.size
    assert np.array_equal(M.through(fragment_map, first), labels) and fragment_map.size == int(np.max(first)) + 1
    knn = [r for r in got.rounds if r["kind"] == "knn"]
    assert counts.tolist() == [C, int((cur < 0).sum()), sum(r["clusters_out"] < r["clusters_in"] for r in knn),
                               len(got.rounds) - len(knn)]
    rows = M.first_rows(labels)
    assert rows == sorted(rows)                                           # numbered by the smallest row, through every round
    return cur


def is_the_truth(got, speaker, n_speakers, each):
    from speaker_verification_amd import clustering as K
    labels = _np(got.labels)
    return int(got.counts[0]) == n_speakers and got.sizes[:n_speakers].tolist() == [each] * n_speakers and \
        M.pure(labels, speaker) and K.purity(labels, speaker) == 1.0 and \
        K.pair_precision_recall_f(got.labels, speaker) == (1.0, 1.0, 1.0)


@pytest.mark.parametrize("ahc_max, kinds, counts", [(None, ["ahc"], [40, 0, 0, 1]), (16, ["knn", "knn"], [40, 0, 1, 0]),
                                                    (45, ["knn", "ahc"], [40, 0, 1, 1]), (0, ["knn", "knn"], [40, 0, 1, 0])])
def test_the_40_speaker_corpus_step_by_step(world, ahc_max, kinds, counts):
    from speaker_verification_amd import clustering as K
    c = world["40"]
    got = K.merge_clusters(world["eng"], c["dev"], c["first"], threshold=0.5, k=5, ahc_max=ahc_max, trace=True)
    assert isinstance(got, K.Merged) and [r["kind"] for r in got.rounds] == kinds and got.counts.tolist() == counts
    held_to_the_references(world["eng"], c["dev"], c["first"], got, 0.5, 5)
    assert is_the_truth(got, c["speaker"], 40, 25)
    assert np.array_equal(_np(got.labels), M.merge(c["emb"], c["first"], 0.5, 5, ahc_max=ahc_max)["labels"])


def test_the_8_speaker_corpus_step_by_step(world):
    from speaker_verification_amd import clustering as K
    c = world["8"]
    got = K.merge_clusters(world["eng"], c["dev"], c["first"], threshold=0.5, k=5, ahc_max=64, trace=True)
    kinds = [r["kind"] for r in got.rounds]
    assert kinds[-1] == "ahc" and len(kinds) >= 3 and set(kinds[:-1]) == {"knn"} and got.rounds[-1]["clusters_in"] <= 64
    assert int(got.counts[2]) == len(kinds) - 1 and int(got.counts[3]) == 1
    cur = held_to_the_references(world["eng"], c["dev"], c["first"], got, 0.5, 5)
    for rnd in got.rounds:                                                # a merged cluster's centroid is one speaker's
        assert rnd["clusters_out"] < rnd["clusters_in"]
    assert is_the_truth(got, c["speaker"], 8, 123) and M.pure(cur, c["speaker"])
    assert np.array_equal(_np(got.labels), M.merge(c["emb"], c["first"], 0.5, 5, ahc_max=64)["labels"])


def test_num_clusters_acts_in_the_linkage_stage_alone(world):
    from speaker_verification_amd import clustering as K
    c, eng = world["40"], world["eng"]
    got = K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5, num_clusters=20, trace=True)
    assert got.counts.tolist() == [20, 0, 0, 1] and int(got.sizes[:20].sum()) == 1000
    held_to_the_references(eng, c["dev"], c["first"], got, 0.5, 5, num_clusters=20)
    assert np.array_equal(_np(got.labels), M.merge(c["emb"], c["first"], 0.5, 5, num_clusters=20)["labels"])
    # never reached: the result says so and is the k-NN result
    skipped = K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5, num_clusters=20, ahc_max=0, trace=True)
    assert skipped.counts.tolist() == [40, 0, 1, 0]
    assert same_bytes(skipped, K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5, ahc_max=0))


def test_max_rounds_stops_the_rounds(world):
    from speaker_verification_amd import clustering as K
    c, eng = world["8"], world["eng"]
    got = K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5, ahc_max=64, max_rounds=1, trace=True)
    assert [r["kind"] for r in got.rounds] == ["knn"] and got.counts.tolist()[2:] == [1, 0]
    assert 64 < int(got.counts[0]) < int(c["first"].max()) + 1
    cur = held_to_the_references(eng, c["dev"], c["first"], got, 0.5, 5)
    assert M.pure(cur, c["speaker"])
    none = K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5, ahc_max=64, max_rounds=0, trace=True)
    assert none.rounds == [] and np.array_equal(_np(none.labels), c["first"]) and none.counts.tolist()[2:] == [0, 0]


@pytest.mark.parametrize("labels, C", [(np.zeros(0, dtype=np.int32), 0), (np.full(7, -1, dtype=np.int32), 0),
                                       (np.zeros(7, dtype=np.int32), 1), (np.array([0, -1, 0, -1, 0, 0, -1], dtype=np.int32), 1)])
def test_no_cluster_one_cluster_and_nothing_labelled(world, labels, C):
    from speaker_verification_amd import clustering as K
    eng = world["eng"]
    emb = world["40"]["dev"][:labels.size]
    got = K.merge_clusters(eng, emb, labels, threshold=0.5, k=5, trace=True)
    assert got.rounds == [] and got.labels.is_cuda and np.array_equal(_np(got.labels), labels)
    assert got.counts.tolist() == [C, int((labels < 0).sum()), 0, 0] and got.fragment_map.tolist() == list(range(C))
    assert got.sizes.tolist() == ([int((labels == 0).sum())] + [0] * (labels.size - 1) if C else [0] * labels.size)
    back = K.adopt_rows(eng, emb, labels, threshold=-1.0)
    assert back.labels.tolist() == ([0] * labels.size if C else labels.tolist())
    assert back.counts.tolist() == [C, 0 if C else labels.size, int((labels < 0).sum()) if C else 0, 0]


def test_a_host_array_a_device_tensor_and_two_runs_give_the_same_bytes(world):
    from speaker_verification_amd import clustering as K
    eng = world["eng"]
    for name, kw in (("40", dict(k=5)), ("8", dict(k=5, ahc_max=64))):
        c = world[name]
        runs = [K.merge_clusters(eng, emb, labels, threshold=0.5, **kw)
                for emb, labels in ((c["dev"], c["first"]), (c["dev"], c["first"]), (c["emb"], eng.to_device(c["first"])),
                                    (c["emb"], K.Clustering(eng.to_device(c["first"]), None, None, None)))]
        assert all(same_bytes(runs[0], r) for r in runs[1:])
        assert all(t.is_cuda and t.dtype == torch.int32 for t in runs[0][:4])
        assert all(set(r) == {"kind", "clusters_in", "clusters_out"} for r in runs[0].rounds)       # no trace: no tensors kept


def test_unlabelled_rows_stay_unlabelled(world):
    from speaker_verification_amd import clustering as K
    c, eng = world["40"], world["eng"]
    first = c["first5"]
    assert (first < 0).any()
    got = K.merge_clusters(eng, c["dev"], first, threshold=0.5, k=5, trace=True)
    cur = held_to_the_references(eng, c["dev"], first, got, 0.5, 5)
    assert np.array_equal(cur < 0, first < 0) and got.counts.tolist() == [40, int((first < 0).sum()), 0, 1]


def test_with_a_back_end_the_rows_are_projected_first(world):
    from speaker_verification_amd import clustering as K
    from speaker_verification_amd.backend import EmbeddingBackend
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    c, eng = world["40"], world["eng"]
    dev_emb, dev_speaker = D.corpus(1)
    backend = EmbeddingBackend().fit(eng.to_device(dev_emb), dev_speaker, method="lda", out_dim=20, shrinkage=1e-3, engine=eng)
    pipe = VerificationPipeline(C3D2(4, 1), use_vad=False, backend=backend)
    projected = pipe.project(c["dev"])
    assert tuple(projected.shape) == (1000, 20)
    first = pipe.cluster(c["dev"], k=10, threshold=0.5, min_shared=3, min_size=5)
    rule = dict(threshold=0.5, k=5, ahc_max=16)
    want = K.merge_clusters(eng, projected, first, trace=True, **rule)
    assert len(want.rounds) >= 1 and tuple(want.rounds[0]["centroids"].shape) == (int(first.counts[0]), 20)
    assert same_bytes(pipe.merge_clusters(c["dev"], first, **rule), want)
    assert same_bytes(pipe.merge_clusters(c["emb"], first.labels, **rule), want)                   # a host array
    adopted = K.adopt_rows(eng, projected, first, threshold=0.5)
    got = pipe.adopt_rows(c["emb"], first, threshold=0.5)
    assert isinstance(got, K.Adopted) and all(torch.equal(a, b) for a, b in zip(got, adopted))
    # without a back end the pipeline's calls are the functions on the rows as they are
    assert same_bytes(world["pipe"].merge_clusters(c["dev"], c["first"], threshold=0.5, k=5),
                      K.merge_clusters(eng, c["dev"], c["first"], threshold=0.5, k=5))


def test_a_plda_a_normalisation_or_a_calibration_raises(world):
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    c = world["40"]
    for name in ("plda", "score_norm", "calibration"):
        pipe = VerificationPipeline(C3D2(4, 1), use_vad=False)
        setattr(pipe, name, object())
        with pytest.raises(ValueError, match="cosine"):
            pipe.merge_clusters(c["dev"], c["first"], threshold=0.5, k=5)
        with pytest.raises(ValueError, match="cosine"):
            pipe.adopt_rows(c["dev"], c["first5"], threshold=0.5)
    with pytest.raises(TypeError):
        world["pipe"].merge_clusters(c["dev"], c["first"], k=5)                      # the threshold has no default
    with pytest.raises(TypeError):
        world["pipe"].adopt_rows(c["dev"], c["first5"])


def test_a_nan_row_makes_the_linkage_stage_raise(world):
    from speaker_verification_amd import clustering as K
    c = world["40"]
    emb = c["emb"].copy()
    emb[3, 5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        K.merge_clusters(world["eng"], emb, c["first"], threshold=0.5, k=5)
    with pytest.raises(ValueError, match="512"):
        K.merge_clusters(world["eng"], np.zeros((1000, 516), dtype=np.float32), c["first"], threshold=0.5, k=5)


def test_adopt_rows_on_the_rows_min_size_left(world):
    from speaker_verification_amd import clustering as K
    c, eng = world["40"], world["eng"]
    first, speaker = c["first5"], c["speaker"]
    lone = np.flatnonzero(first < 0)
    assert int(first.max()) + 1 == 40 and lone.size == 19
    of = speaker[M.first_rows(first)]
    got = K.adopt_rows(eng, c["dev"], first, threshold=0.5)                          # every row, to its own speaker
    labels = _np(got.labels)
    assert isinstance(got, K.Adopted) and all(t.is_cuda and t.dtype == torch.int32 for t in got)
    assert got.counts.tolist() == [40, 0, 19, 0] and np.array_equal(of[labels], speaker) and got.sizes[:40].tolist() == [25] * 40
    assert not got.sizes[40:].any() and np.array_equal(labels[first >= 0], first[first >= 0])
    assert np.array_equal(labels, M.adopt(c["emb"], first, 0.5)[0])
    assert K.pair_precision_recall_f(got.labels, speaker) == (1.0, 1.0, 1.0)
    none = K.adopt_rows(eng, c["emb"], eng.to_device(first), threshold=0.9)          # no row
    assert none.counts.tolist() == [40, 19, 0, 0] and np.array_equal(_np(none.labels), first)
    assert np.array_equal(_np(none.sizes)[:40], np.bincount(first[first >= 0])) and not none.sizes[40:].any()
    again = K.adopt_rows(eng, c["emb"], K.Clustering(eng.to_device(first), None, None, None), threshold=0.5)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
