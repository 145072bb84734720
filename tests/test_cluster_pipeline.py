"""`VerificationPipeline.cluster` and speaker_verification_amd/clustering.py on real k-NN lists: the corpus of
tests/cluster_corpus.py (40 speakers x 25 utterances, dim 128; tests/test_knn_cluster_host.py establishes in float64 that
every same-speaker cosine is >= 0.58 and every other <= 0.38, far more than float32 moves a cosine, so the threshold 0.5
separates them on the device too).  The labels are held EXACTLY to the plain-Python reference run on the lists `search`
returned, and to the truth: 40 pure clusters of 25 at k = 32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cluster_corpus as D        # noqa: E402  (tests/ is on sys.path)
import knn_cluster_ref as R       # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = dict(threshold=0.5, min_shared=3, mutual=True)


@pytest.fixture(scope="module")
def world():
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    assert torch.cuda.is_available(), "these tests need the MI355X"
    eng = get_engine(0)
    emb, speaker = D.corpus(0)
    pipe = VerificationPipeline(C3D2(4, 1), use_vad=False)
    lists = {k: pipe.search(emb, emb, k=k, exclude_self=True) for k in (10, 32)}
    want = {k: R.cluster(lists[k][1].cpu().numpy(), lists[k][0].cpu().numpy(), k, 0.5, 3, True, 1) for k in (10, 32)}
    return dict(eng=eng, emb=emb, dev=eng.to_device(emb), speaker=speaker, pipe=pipe, lists=lists, want=want)


def equal(got, want):
    got = [t.cpu().numpy() for t in got]
    return all(g.dtype == np.int32 and np.array_equal(g, w) for g, w in zip(got, want)) and got[3][3] == 0


def test_cluster_is_the_reference_on_the_lists_of_search(world):
    from speaker_verification_amd import clustering as K
    got = world["pipe"].cluster(world["dev"], k=32, **SETTINGS)
    assert isinstance(got, K.Clustering) and equal(got, world["want"][32])
    labels, speaker = got.labels.cpu().numpy(), world["speaker"]
    assert got.counts.tolist() == [40, 0, 0, 0] and got.sizes[:40].tolist() == [25] * 40       # exactly 40 clusters of 25
    assert all(len(set(speaker[labels == c])) == 1 for c in range(40))                          # ... each one speaker
    assert K.purity(labels, speaker) == 1.0 and K.pair_precision_recall_f(got.labels, speaker) == (1.0, 1.0, 1.0)
    assert equal(world["pipe"].cluster(world["emb"], k=32, **SETTINGS), world["want"][32])      # a host array
    assert equal(K.cluster_embeddings(world["pipe"], world["dev"], 32, 0.5, min_shared=3), world["want"][32])
    assert equal(K.cluster_embeddings(world["eng"], world["dev"], 32, 0.5, min_shared=3), world["want"][32])


def test_k_10_fragments_as_the_reference_does(world):
    got = world["pipe"].cluster(world["dev"], k=10, **SETTINGS)
    assert equal(got, world["want"][10])
    assert 51 <= int(got.counts[0]) <= 61 and int(got.counts[0]) == world["want"][10][3][0]
    # k = 10 read out of the k = 32 lists through list_stride is the k = 10 search
    scores, indices = world["lists"][32]
    assert equal(world["eng"].knn_cluster(scores, indices, k=10, **SETTINGS), world["want"][10])
    assert torch.equal(indices[:, :10], world["lists"][10][1])


def test_chunk_rows_gives_the_same_labels(world):
    for k in (10, 32):
        assert equal(world["pipe"].cluster(world["dev"], k=k, chunk_rows=300, **SETTINGS), world["want"][k])
    assert equal(world["pipe"].cluster(world["emb"], k=32, chunk_rows=300, **SETTINGS), world["want"][32])


def test_segments_and_centroids_equal_enroll_mean(world):
    from speaker_verification_amd import clustering as K
    from speaker_verification_amd.pipeline import enroll_mean
    got = world["pipe"].cluster(world["dev"], k=10, min_size=20, **SETTINGS)          # fragments: some rows stay unlabelled
    labels = got.labels.cpu().numpy()
    assert 0 < int(got.counts[1]) == int((labels < 0).sum())
    kept = np.flatnonzero(labels >= 0)
    ids, models = enroll_mean(world["dev"][torch.from_numpy(kept).to(world["dev"].device)], labels[kept])
    assert list(ids) == list(range(int(got.counts[0])))
    centres = K.centroids(world["eng"], world["dev"], got)
    assert torch.equal(centres.view(torch.int32), models.view(torch.int32))
    seg_start, row_index = K.segments(got)
    assert np.array_equal(np.diff(seg_start), got.sizes[:int(got.counts[0])].cpu().numpy())


def test_with_a_back_end_the_rows_are_projected_first(world):
    from speaker_verification_amd.backend import EmbeddingBackend
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    eng = world["eng"]
    dev_emb, dev_speaker = D.corpus(1)
    backend = EmbeddingBackend().fit(eng.to_device(dev_emb), dev_speaker, method="lda", out_dim=20, shrinkage=1e-3, engine=eng)
    pipe = VerificationPipeline(C3D2(4, 1), use_vad=False, backend=backend)
    projected = pipe.project(world["dev"])
    assert tuple(projected.shape) == (1000, 20)
    scores, indices = world["pipe"].search(projected, projected, k=32, exclude_self=True)
    want = R.cluster(indices.cpu().numpy(), scores.cpu().numpy(), 32, 0.5, 3, True, 1)
    assert equal(pipe.cluster(world["dev"], k=32, **SETTINGS), want)
    assert equal(pipe.cluster(world["emb"], k=32, chunk_rows=300, **SETTINGS), want)
    assert not torch.equal(indices, world["lists"][32][1])                           # other lists than the raw rows'


def test_a_plda_a_normalisation_or_a_calibration_raises(world):
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    for name in ("plda", "score_norm", "calibration"):
        pipe = VerificationPipeline(C3D2(4, 1), use_vad=False)
        setattr(pipe, name, object())
        with pytest.raises(ValueError, match="cosine"):
            pipe.cluster(world["dev"], k=32, **SETTINGS)
    with pytest.raises(TypeError):
        world["pipe"].cluster(world["dev"], k=32)                                    # the threshold has no default
