"""Corpus clustering: unlabelled embeddings -> pseudo-speaker labels, on the device.

`cluster_embeddings` is a self-search (`svk_cosine_topk`, no [n x n] matrix) followed by `svk_knn_cluster`
(include/svk.h, "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists"): the connected components of the shared-neighbour (Jarvis-Patrick) graph read off the k-NN lists.
`segments` turns the labels into the CSR form `svk_embedding_pool` and `svk_class_scatter` take, so the clusters feed
`centroids`, `backend.solve` and `plda.solve_plda` like speaker labels.  `purity` and `pair_precision_recall_f` measure a
clustering against known labels on the host.  `merge_clusters` is the second stage for when k fragments a speaker (the
clusters' centroids merged by k-NN rounds, then average linkage) and `adopt_rows` gives the rows left at -1 to the nearest
centroid; both run on entries the library already has.  Nothing is tuned in here: k and the threshold are the
caller's."""
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


Merged = namedtuple("Merged", "labels sizes counts fragment_map rounds")
Merged.__doc__ = """What `merge_clusters` returns: labels int32 [n] (-1 kept), sizes int32 [n] (the C sizes, then zeros), counts
int32 [4] = (C, rows labelled -1, k-NN rounds that merged something, 1 if the average-linkage stage ran else 0) and
fragment_map int32 [C0] (first-stage cluster -> final cluster), all on the device; rounds: a host list, one dict per round
(kind "knn" or "ahc", clusters_in, clusters_out; with trace=True the round's device tensors as well: centroids, the lists
`scores` / `indices` or the `affinity`, and the round's `labels` [clusters_in])."""

Adopted = namedtuple("Adopted", "labels sizes counts")
Adopted.__doc__ = """What `adopt_rows` returns, on the device: labels int32 [n], sizes int32 [n] (the C sizes, then zeros) and
counts int32 [4] = (C, rows still -1, rows adopted, 0)."""


def _dense(labels):
    """Cluster labels (a `Clustering`, a device tensor or an array) -> (int64 [n] on the host, C): every label is -1 or one
    of 0 .. C-1 and each of those occurs, as `svk_knn_cluster` numbers them."""
    labels = _host(labels.labels if isinstance(labels, Clustering) else labels).reshape(-1).astype(np.int64)
    C = int(labels.max()) + 1 if labels.size else 0
    if labels.size and (labels.min() < -1 or np.any(np.bincount(labels[labels >= 0], minlength=C) == 0)):
        raise ValueError("dense cluster labels 0 .. C-1 (and -1) are wanted, as svk_knn_cluster writes them")
    return labels, max(C, 0)


def _through(step, labels):
    """The labels of a round's centroids carried to what those centroids stand for: step[labels] where labels >= 0."""
    out = labels.copy()
    out[labels >= 0] = step[labels[labels >= 0]]
    return out


def _rows_and_labels(emb, labels):
    """-> (dense labels int64 [n] on the host, C), with emb [n, dim] checked against them."""
    labels, C = _dense(labels)
    if len(emb.shape) != 2 or int(emb.shape[0]) != labels.size:
        raise ValueError("rows emb [n, dim] and one label per row are wanted")
    return labels, C


def _result(engine, torch, labels, C):
    """(labels, sizes) of a result on the device: int32 [n] each."""
    sizes = np.zeros(labels.size, dtype=np.int32)
    sizes[:C] = np.bincount(labels[labels >= 0], minlength=C)
    return engine.to_device(labels.astype(np.int32), torch.int32), engine.to_device(sizes, torch.int32)


def merge_clusters(engine, emb, labels, *, threshold, k, mutual=True, min_shared=0, num_clusters=None, ahc_max=None,
                   max_rounds=16, trace=False):
    """The second stage of corpus clustering: the fragments a k-NN clustering leaves of one speaker are merged
    on their centroids -> `Merged`.  emb [n, dim] float32 (dim <= 512, `svk_segment_affinity`'s limit), labels dense as
    `svk_knn_cluster` writes them.  A round pools the L2-normalised rows of every cluster into its L2-normalised centroid
    (`svk_embedding_pool`, from the ROWS every round: a mean over all rows, not a mean of means).  While there are more than
    ahc_max clusters (None: `ahc_limits()[1]`; 0: never link) a round is the self-search of the centroids (`svk_cosine_topk`,
    k in 1 .. 32) and `svk_knn_cluster` on its lists (threshold, mutual, min_shared; min_size 1), up to max_rounds rounds and
    until a round merges nothing; at ahc_max or fewer, `svk_segment_affinity` and average linkage (`svk_ahc`) down to
    `threshold` end it -- or down to exactly num_clusters, which acts in that stage alone (counts[3] tells whether it ran).
    Every stage numbers a cluster by its lowest member, so cluster c < c' iff its smallest row is the smaller.  The float
    work is those five entries'; the host composes integer label maps.  A non-finite centroid in the linkage stage raises
    ValueError."""
    threshold = float(threshold)
    k, max_rounds = int(k), int(max_rounds)
    if threshold != threshold:
        raise ValueError("a NaN threshold merges nothing and refuses nothing: give a number")
    if not 1 <= k <= 32:
        raise ValueError("k = %d is outside 1 .. 32, the lists' own limit" % k)
    if max_rounds < 0:
        raise ValueError("max_rounds must be at least 0")
    if num_clusters is not None and int(num_clusters) < 1:
        raise ValueError("num_clusters must be at least 1")
    import torch
    cur, C = _rows_and_labels(emb, labels)
    if int(emb.shape[1]) > 512:
        raise ValueError("dim = %d: the linkage stage's cosines (svk_segment_affinity) take dim <= 512" % int(emb.shape[1]))
    limit = engine.ahc_limits()[1]
    ahc_max = limit if ahc_max is None else int(ahc_max)
    if not 0 <= ahc_max <= limit:
        raise ValueError("ahc_max = %d is outside 0 .. %d, the largest matrix svk_ahc takes" % (ahc_max, limit))

    x = engine.to_device(emb, torch.float32)
    fragment_map = np.arange(C, dtype=np.int64)
    rounds, merged_rounds, linked = [], 0, 0

    def step(kind, C_out, into, **tensors):
        rounds.append(dict(kind=kind, clusters_in=C, clusters_out=C_out, **(tensors if trace else {})))
        return _through(into, cur), into[fragment_map]

    while C > 1 and (C <= ahc_max or merged_rounds < max_rounds):
        cent = centroids(engine, x, cur, l2_rows=True, l2_mean=True)
        if C <= ahc_max:
            bad = torch.zeros((1,), dtype=torch.int32, device=engine.device)
            aff = engine.segment_affinity(cent[None], np.array([C], dtype=np.int32))
            lab, count = engine.ahc(aff, np.array([C], dtype=np.int32), threshold=threshold, min_clusters=1, max_clusters=C,
                                    target=None if num_clusters is None else np.array([int(num_clusters)], dtype=np.int32),
                                    bad_count=bad)
            C_out = int(count[0])
            if C_out < 0 or int(bad[0]):
                raise ValueError("a cluster's centroid is not finite (a NaN or Inf row): the linkage stage refuses the corpus")
            cur, fragment_map = step("ahc", C_out, _host(lab[0, :C]).astype(np.int64), centroids=cent, affinity=aff[0],
                                     labels=lab[0, :C])
            C, linked = C_out, 1
            break
        scores, indices = engine.cosine_topk(cent, cent, k, exclude=torch.arange(C, dtype=torch.int64, device=engine.device))
        lab, _, _, counts = engine.knn_cluster(scores, indices, threshold=threshold, min_shared=min_shared, mutual=mutual,
                                               min_size=1)
        C_out, _, _, gave_up = (int(v) for v in counts.tolist())
        if gave_up:
            raise RuntimeError("svk_knn_cluster gave up on the centroids' lists")
        cur, fragment_map = step("knn", C_out, _host(lab).astype(np.int64), centroids=cent, scores=scores, indices=indices,
                                 labels=lab)
        if C_out == C:              # nothing merged: the next round would be this one again
            break
        C, merged_rounds = C_out, merged_rounds + 1

    out_labels, sizes = _result(engine, torch, cur, C)
    counts = np.array([C, int((cur < 0).sum()), merged_rounds, linked], dtype=np.int32)
    return Merged(out_labels, sizes, engine.to_device(counts, torch.int32),
                  engine.to_device(fragment_map.astype(np.int32), torch.int32), rounds)


def adopt_rows(engine, emb, labels, *, threshold):
    """The rows a clustering left at -1 (`min_size`) join the cluster whose centroid is nearest, when that cosine reaches
    `threshold` -> `Adopted`.  The centroids are those of the labelled rows (`centroids`, L2-normalised rows, L2-normalised
    mean) and are taken ONCE; the -1 rows are gathered and searched against them (`svk_cosine_topk`, k = 1); a row takes the
    returned cluster iff its score >= threshold as a float32 comparison (a NaN score fails) and stays -1 otherwise.  One
    pass, no centroid moves: the result does not depend on the order of the rows.  Without clusters or without -1 rows the
    labels come back as they are."""
    threshold = np.float32(threshold)
    if np.isnan(threshold):
        raise ValueError("a NaN threshold adopts nothing and refuses nothing: give a number")
    import torch
    cur, C = _rows_and_labels(emb, labels)
    lone = np.flatnonzero(cur < 0)
    adopted = 0
    if C and lone.size:
        x = engine.to_device(emb, torch.float32)
        cent = centroids(engine, x, cur, l2_rows=True, l2_mean=True)
        rows = x.index_select(0, engine.to_device(lone, torch.int64))
        scores, indices = engine.cosine_topk(rows, cent, 1)
        nearest = _host(indices).reshape(-1)
        take = (_host(scores).reshape(-1) >= threshold) & (nearest >= 0)
        cur[lone[take]] = nearest[take]
        adopted = int(take.sum())
    out_labels, sizes = _result(engine, torch, cur, C)
    counts = np.array([C, int((cur < 0).sum()), adopted, 0], dtype=np.int32)
    return Adopted(out_labels, sizes, engine.to_device(counts, torch.int32))


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
