"""Corpus clustering: unlabelled embeddings -> pseudo-speaker labels, on the device.

`cluster_embeddings` is a self-search (`svk_cosine_topk`, no [n x n] matrix) followed by `svk_knn_cluster`
(include/svk.h, "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists"): the connected components of the shared-neighbour (Jarvis-Patrick) graph read off the k-NN lists.
`segments` turns the labels into the CSR form `svk_embedding_pool` and `svk_class_scatter` take, so the clusters feed
`centroids`, `backend.solve` and `plda.solve_plda` like speaker labels.  `purity` and `pair_precision_recall_f` measure a
clustering against known labels on the host.  Nothing is tuned in here: k and the threshold are the caller's."""
from collections import namedtuple

import numpy as np

from .pipeline import speaker_segments

Clustering = namedtuple("Clustering", "labels roots sizes counts")
Clustering.__doc__ = """What `Engine.knn_cluster` returns, on the device: labels int32 [n] (-1: a component below min_size), roots
int32 [n] (the smallest row of the row's component), sizes int32 [n] (the C cluster sizes, then zeros) and counts int32 [4] =
(C, rows labelled -1, bad slots, gave_up)."""


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cluster_embeddings(pipeline_or_engine, emb, k, threshold, min_shared=0, mutual=True, min_size=1, chunk_rows=None):
    """emb [n, dim] -> `Clustering`.  With a VerificationPipeline this is `pipeline.cluster` (its back end projects the rows
    first; chunk_rows searches the corpus chunk by chunk, the same bits); with an Engine the rows are searched as they are,
    in one call."""
    if hasattr(pipeline_or_engine, "cluster"):
        return pipeline_or_engine.cluster(emb, k=k, threshold=threshold, min_shared=min_shared, mutual=mutual, min_size=min_size,
                                          chunk_rows=chunk_rows)
    import torch
    eng = pipeline_or_engine
    if chunk_rows is not None:
        raise ValueError("chunk_rows belongs to a pipeline's search: an Engine searches the rows in one call")
    x = eng.to_device(emb, torch.float32)
    scores, indices = eng.cosine_topk(x, x, k, exclude=torch.arange(int(x.shape[0]), dtype=torch.int64, device=eng.device))
    return Clustering(*eng.knn_cluster(scores, indices, threshold=threshold, min_shared=min_shared, mutual=mutual,
                                       min_size=min_size))


def segments(labels):
    """Cluster labels [n] (a `Clustering`, a device tensor or an array; -1 = in no cluster) -> (seg_start int64 [C + 1],
    row_index int64 [n]) in the form `svk_embedding_pool` and `svk_class_scatter` take: cluster c is rows
    row_index[seg_start[c] : seg_start[c + 1]] in row order (`pipeline.speaker_segments` on the rows with label >= 0); the
    rows labelled -1 follow behind the last segment, in no segment.  Cluster c must be label c: dense labels, as
    `svk_knn_cluster` numbers them."""
    labels = _host(labels.labels if isinstance(labels, Clustering) else labels).reshape(-1)
    kept = np.flatnonzero(labels >= 0)
    uniq, seg_start, order = speaker_segments(labels[kept])
    if uniq.size and not np.array_equal(uniq, np.arange(uniq.size)):
        raise ValueError("segments wants dense cluster labels 0 .. C-1 (and -1)")
    return seg_start, np.concatenate([kept[order], np.flatnonzero(labels < 0)]).astype(np.int64)


def centroids(engine, emb, labels, l2_rows=True, l2_mean=False):
    """The mean embedding of every cluster -> float32 [C, dim] on the device: one `svk_embedding_pool` launch over
    `segments(labels)`, what `pipeline.enroll_mean` is for speaker labels (l2_rows is its `l2`)."""
    seg_start, row_index = segments(labels)
    return engine.embedding_pool(emb, seg_start=seg_start, row_index=row_index, l2_rows=l2_rows, l2_mean=l2_mean)


def _pairs(counts):
    counts = np.asarray(counts, dtype=np.int64)
    return int((counts * (counts - 1) // 2).sum())


def _as_singletons(labels):
    """Every -1 row as a cluster of its own."""
    labels = _host(labels).reshape(-1).astype(np.int64)
    out = labels.copy()
    lone = np.flatnonzero(labels < 0)
    out[lone] = (labels.max() + 1 if labels.size else 0) + np.arange(lone.size)
    return out


def _contingency(labels, truth):
    truth = _host(truth).reshape(-1)
    labels = _as_singletons(labels)
    if labels.size != truth.size:
        raise ValueError("one true label per clustered row")
    _, t = np.unique(truth, return_inverse=True)
    _, c = np.unique(labels, return_inverse=True)
    table = np.zeros((int(c.max()) + 1 if c.size else 0, int(t.max()) + 1 if t.size else 0), dtype=np.int64)
    np.add.at(table, (c, t), 1)
    return table


def purity(labels, truth):
    """The share of rows that carry their cluster's most frequent true label; a row labelled -1 is a cluster of its own (and
    pure).  1.0 for an empty labeling."""
    table = _contingency(labels, truth)
    return float(table.max(axis=1).sum()) / float(table.sum()) if table.size else 1.0


def pair_precision_recall_f(labels, truth):
    """Pairwise (precision, recall, F) over the n (n - 1) / 2 row pairs: a pair is predicted when both rows share a cluster
    and true when they share a true label; rows labelled -1 are singletons, so they predict no pair.  A quotient without
    pairs in its denominator is 1.0."""
    table = _contingency(labels, truth)
    both = _pairs(table.reshape(-1))
    predicted, true = _pairs(table.sum(axis=1)), _pairs(table.sum(axis=0))
    p = both / predicted if predicted else 1.0
    r = both / true if true else 1.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)
