"""Corpus clustering without a GPU: the names of the entries of include/svk.h's section "shared-neighbour (Jarvis-Patrick)
clustering of k-NN lists" in the binding, the returns that need no device, the reference of tests/knn_cluster_ref.py against
scipy's connected components, the host metrics on hand-made labelings, `clustering.segments` against
`pipeline.speaker_segments`, and the separation the pipeline test's corpus relies on."""
import os

import numpy as np
import pytest

import knn_cluster_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from speaker_verification_amd import _lib as binding
    if not os.path.exists(binding.LIB_PATH):
        entry.build()
    return binding.load()


# ---- the entries in the binding ----------------------------------------------------------------------------------------
def test_the_two_entries_are_bound():
    """(tests/test_cabi.py walks the header, the table and the library for every entry, and holds SVK_KNN_CLUSTER_MUTUAL to
    the binding's value; this pins the names)"""
    from speaker_verification_amd import _lib as binding
    assert sorted(n for n in binding.SIGNATURES if n.startswith("svk_knn_cluster")) == [
        "svk_knn_cluster", "svk_knn_cluster_workspace_bytes"]
    assert binding.KNN_CLUSTER_MUTUAL == 1


def test_refusals_need_no_device(lib):
    from speaker_verification_amd import _lib as binding
    assert lib.svk_knn_cluster(None, None, None, 5, 3, 3, 0.5, 0, 1, 1, None, 0, None, None, None, None) == binding.SVK_ERR_BAD_ARG
    for shape in ((-1, 5), (5, 0), (5, 33), (5, -1), (1 << 31, 5)):
        assert lib.svk_knn_cluster_workspace_bytes(*shape) == 0
    assert lib.svk_knn_cluster_workspace_bytes(0, 5) == 0       # nothing is launched for an empty corpus
    # the shape alone: k changes nothing, and the size grows with n
    sizes = [lib.svk_knn_cluster_workspace_bytes(n, k) for n in (1, 2048, 2049, 148642, (1 << 31) - 1) for k in (1, 32)]
    assert sizes[0::2] == sizes[1::2] and sizes[0::2] == sorted(sizes[0::2]) and sizes[0] > 0 and all(s % 16 == 0 for s in sizes)
    assert sizes[-1] >= 2 * 4 * ((1 << 31) - 1)


# ---- the reference -------------------------------------------------------------------------------------------------------
def _random_lists(rng, n, k, bad=0.05):
    """Every slot drawn from the row's own block of 8 rows (so that arcs are often returned and components stay small), a
    share `bad` of them replaced by empty and hostile values, a quarter of that by the row itself."""
    index = (np.arange(n)[:, None] // 8 * 8 + rng.integers(0, 8, (n, k))).astype(np.int64)
    hostile = np.array([-1, -2, n, (1 << 63) - 1, -(1 << 63)], dtype=np.int64)
    hit = rng.random((n, k)) < bad
    index[hit] = rng.choice(hostile, int(hit.sum()))
    self_hit = rng.random((n, k)) < bad / 4
    index[self_hit] = np.broadcast_to(np.arange(n)[:, None], (n, k))[self_hit]
    score = rng.choice(np.array([0.25, 0.5, 0.5, 0.75, np.nan], dtype=np.float32), (n, k))
    return index, score


@pytest.mark.parametrize("mutual", (True, False))
@pytest.mark.parametrize("seed", range(3))
def test_reference_equals_scipy_connected_components(seed, mutual):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(seed)
    n, k = 400, 3
    index, score = _random_lists(rng, n, k)
    arcs = np.zeros((n, n), dtype=bool)                 # an independent statement: the first occurrence of an in-range index
    n_bad = 0
    for i in range(n):
        for a in range(k):
            v = int(index[i, a])
            if v == -1:
                continue
            if not 0 <= v < n or v == i or v in [int(x) for x in index[i, :a]]:
                n_bad += 1
            elif score[i, a] >= np.float32(0.5):
                arcs[i, v] = True
    graph = (arcs & arcs.T) if mutual else (arcs | arcs.T)
    count, comp = connected_components(csr_matrix(graph), directed=False)
    labels, root, sizes, counts = R.cluster(index, score, k, 0.5, 0, mutual, 1)
    assert counts[2] == n_bad > 0 and counts[0] == count and counts[1] == 0 and 1 < count < n
    for c in range(count):
        members = np.flatnonzero(comp == c)
        assert np.all(root[members] == members.min())
    assert np.array_equal(np.unique(labels), np.arange(count)) and sizes[:count].sum() == n and not sizes[count:].any()
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(count)]
    assert first == sorted(first)                       # numbered by their smallest member


def test_reference_on_a_hand_made_case():
    # 0 - 1 mutual; 2 -> 0 one way; 3 alone; row 4: a duplicate, a self reference and an index past the end
    index = np.array([[1, -1, -1], [0, -1, -1], [0, -1, -1], [-1, -1, -1], [3, 3, 4]], dtype=np.int64)
    index[3, 2] = 5
    score = np.full((5, 3), 0.9, dtype=np.float32)
    labels, root, sizes, counts = R.cluster(index, score, 3, 0.5, 0, True, 1)
    assert list(root) == [0, 0, 2, 3, 4] and list(labels) == [0, 0, 1, 2, 3] and list(counts) == [4, 0, 3, 0]
    labels, root, sizes, counts = R.cluster(index, score, 3, 0.5, 0, False, 2)
    assert list(root) == [0, 0, 0, 3, 3] and list(labels) == [0, 0, 0, 1, 1] and list(sizes) == [3, 2, 0, 0, 0]
    labels, root, sizes, counts = R.cluster(index, score, 3, 0.5, 0, False, 3)
    assert list(labels) == [0, 0, 0, -1, -1] and list(counts) == [1, 2, 3, 0]
    # a narrower k reads the first slots only; a NaN score and a score below the threshold give no arc, -inf takes both
    score[0, 0], score[2, 0] = np.nan, 0.25
    assert list(R.cluster(index, score, 1, 0.5, 0, False, 1)[1]) == [0, 0, 2, 3, 3]
    assert list(R.cluster(index, score, 1, -np.inf, 0, True, 1)[1]) == [0, 0, 2, 3, 4]
    assert list(R.cluster(index, score, 1, -np.inf, 0, False, 1)[1]) == [0, 0, 0, 3, 3]
    # shared neighbours: rows 0 and 1 share exactly {2}
    index = np.array([[1, 2], [0, 2], [-1, -1]], dtype=np.int64)
    score = np.ones((3, 2), dtype=np.float32)
    assert list(R.cluster(index, score, 2, 0.5, 1, True, 1)[1]) == [0, 0, 2]
    assert list(R.cluster(index, score, 2, 0.5, 2, True, 1)[1]) == [0, 1, 2]


# ---- the host side of speaker_verification_amd/clustering.py ---------------------------------------------------------------
def test_metrics_on_hand_made_labelings():
    from speaker_verification_amd import clustering as K
    truth = np.array([7, 7, 7, 9, 9, 9])
    assert K.purity(truth, truth) == 1.0 and K.pair_precision_recall_f(truth, truth) == (1.0, 1.0, 1.0)
    assert K.pair_precision_recall_f([0, 0, 0, 1, 1, 1], truth) == (1.0, 1.0, 1.0)     # the names of the clusters do not count
    # one cluster of everything: 15 pairs predicted, 6 of them true
    p, r, f = K.pair_precision_recall_f(np.zeros(6, dtype=int), truth)
    assert (p, r) == (6 / 15, 1.0) and f == pytest.approx(2 * 0.4 / 1.4) and K.purity(np.zeros(6, dtype=int), truth) == 0.5
    # -1 rows are singletons: {0, 1}, {2}, {3}, {4, 5} -> 2 pairs predicted, both true, of 6
    labels = np.array([0, 0, -1, -1, 1, 1])
    assert K.pair_precision_recall_f(labels, truth) == (1.0, 2 / 6, pytest.approx(0.5)) and K.purity(labels, truth) == 1.0
    # a mixed cluster {0, 1, 3}: 3 pairs predicted, 1 true; rows 2, 4, 5 alone
    labels = np.array([0, 0, -1, 0, -1, -1])
    assert K.pair_precision_recall_f(labels, truth)[:2] == (1 / 3, 1 / 6) and K.purity(labels, truth) == 5 / 6
    assert K.pair_precision_recall_f(np.full(6, -1), truth) == (1.0, 0.0, 0.0)
    assert K.purity([], []) == 1.0
    with pytest.raises(ValueError):
        K.purity([0, 1], [0])


def test_segments_against_speaker_segments():
    from speaker_verification_amd import clustering as K
    from speaker_verification_amd.pipeline import speaker_segments
    rng = np.random.default_rng(5)
    labels = rng.integers(-1, 6, 200).astype(np.int32)
    seg_start, row_index = K.segments(labels)
    kept = np.flatnonzero(labels >= 0)
    uniq, want_start, order = speaker_segments(labels[kept])
    assert list(uniq) == list(range(6)) and np.array_equal(seg_start, want_start) and seg_start.dtype == row_index.dtype == np.int64
    assert np.array_equal(row_index[:kept.size], kept[order]) and np.array_equal(np.sort(row_index), np.arange(200))
    for c in range(6):
        rows = row_index[seg_start[c]:seg_start[c + 1]]
        assert np.array_equal(rows, np.flatnonzero(labels == c))             # a cluster's rows, in row order
    assert np.all(labels[row_index[seg_start[-1]:]] == -1)                   # the unlabelled rows lie behind the last segment
    # without -1 rows it IS speaker_segments
    dense = np.where(labels < 0, 0, labels)
    assert all(np.array_equal(a, b) for a, b in zip(K.segments(dense), speaker_segments(dense)[1:]))
    assert K.segments(K.Clustering(labels, None, None, None))[0].tolist() == seg_start.tolist()
    with pytest.raises(ValueError):
        K.segments(np.array([0, 2, 2]))
    empty_start, empty_rows = K.segments(np.full(3, -1))
    assert empty_start.tolist() == [0] and empty_rows.tolist() == [0, 1, 2]


# ---- the corpus of tests/test_cluster_pipeline.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_the_pipeline_corpus_is_separated_as_claimed(seed):
    """40 speakers x 25 utterances, dim 128, centre + 0.05 N(0, I) on random unit centres: in float64 the smallest
    same-speaker cosine is at least 0.58 and the largest cross-speaker cosine at most 0.38, so a threshold of 0.5 keeps every
    same-speaker arc of a 32-NN list and no other, and the reference recovers the 40 speakers exactly."""
    import cluster_corpus as D
    emb, speaker = D.corpus(seed)
    x = emb.astype(np.float64)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    cos = x @ x.T
    same = speaker[:, None] == speaker[None, :]
    np.fill_diagonal(cos, np.nan)
    assert np.nanmin(np.where(same, cos, np.nan)) >= 0.58 and np.nanmax(np.where(same, np.nan, cos)) <= 0.38
    score, index = D.topk_f64(cos, 32)
    labels, root, sizes, counts = R.cluster(index, score, 32, 0.5, 3, True, 1)
    assert list(counts) == [40, 0, 0, 0] and np.all(sizes[:40] == 25)
    assert all(len(set(speaker[labels == c])) == 1 for c in range(40))
