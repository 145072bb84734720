"""The rule of `clustering.merge_clusters` and `clustering.adopt_rows` in NumPy, on top of the references the
first stage already has: tests/knn_cluster_ref.py for a k-NN round, tests/ahc_f64_ref.py for the average-linkage stage,
`cluster_corpus.topk_f64` for the lists.  Nothing from the package in the rule.

    centroid   the float64 mean of a cluster's float64-normalised rows, normalised, rounded to float32
    cosine     float64 on the float32 centroids (normalised again in float64)
    round      see `merge`: centroids from the ROWS every round; average linkage once there are <= ahc_max clusters, else a
               self-search of the centroids and the shared-neighbour components of its lists, until nothing merges

`HostEngine` stands in for the Engine with these float64 forms on torch CPU tensors, so that the package's own control flow
and bookkeeping run without a device (tests/test_cluster_merge_host.py).  The second corpus, `corpus8`: 8 speakers x 123
utterances, where k = 10 lists fragment every speaker into dozens of pieces and several merging rounds are needed."""
import numpy as np

import ahc_f64_ref as A
import cluster_corpus as D
import knn_cluster_ref as R

AHC_LIMITS = (128, 2048)          # svk_ahc_limits
SPEAKERS8, UTTERANCES8, STREAM8 = 8, 123, 77


def corpus8(seed):
    """-> (emb float32 [984, 128], speaker int64 [984]), built as `cluster_corpus.corpus` builds its own."""
    rng = np.random.default_rng([seed, STREAM8])
    centres = rng.standard_normal((SPEAKERS8, D.DIM))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    speaker = rng.permutation(np.repeat(np.arange(SPEAKERS8), UTTERANCES8))
    emb = centres[speaker] + D.NOISE * rng.standard_normal((speaker.size, D.DIM))
    return emb.astype(np.float32), speaker.astype(np.int64)


def unit(x):
    x = np.asarray(x, dtype=np.float64)
    norm = np.linalg.norm(x, axis=-1, keepdims=True)
    return x / np.where(norm == 0, 1.0, norm)


def centroids(emb, labels):
    """float32 [C, dim]; labels dense, -1 in no cluster."""
    labels = np.asarray(labels)
    x = unit(emb)
    C = int(labels.max()) + 1 if labels.size else 0
    return unit(np.stack([x[labels == c].mean(axis=0) for c in range(C)])).astype(np.float32) if C else \
        np.zeros((0, np.shape(emb)[1]), dtype=np.float32)


def cosines(a, b=None):
    a = unit(a)
    return a @ (a if b is None else unit(b)).T


def lists(cent, k):
    """The self-search of the centroids: (score float32 [C, k], index int64 [C, k]), -inf / -1 past the C - 1 candidates."""
    C = cent.shape[0]
    cos = cosines(cent)
    np.fill_diagonal(cos, np.nan)
    score, index = np.full((C, k), -np.inf, dtype=np.float32), np.full((C, k), -1, dtype=np.int64)
    have = min(k, C - 1)
    if have > 0:
        score[:, :have], index[:, :have] = D.topk_f64(cos, have)
    return score, index


def first_stage(emb, k, threshold=0.5, min_shared=3, min_size=1):
    """The first stage in float64: the labels of `knn_cluster_ref.cluster` on the rows' own lists."""
    score, index = lists(np.asarray(emb), k)
    return R.cluster(index, score, k, threshold, min_shared, True, min_size)[0]


def through(step, labels):
    out = np.array(labels, dtype=np.int64)
    out[out >= 0] = np.asarray(step)[out[out >= 0]]
    return out


def knn_round(score, index, k, threshold, min_shared, mutual):
    """-> (labels of the centroids int32 [C], clusters left)."""
    labels, _, _, counts = R.cluster(index, score, k, threshold, min_shared, mutual, 1)
    return labels, int(counts[0])


def ahc_round(aff, threshold, num_clusters=None):
    """-> (labels of the centroids int32 [C], clusters left, the accepted merges' similarities); -1 left: not finite."""
    C = aff.shape[0]
    labels, count, _, sims = A.ahc(aff, C, threshold, 1, C, num_clusters)
    return labels, int(count), sims[~np.isnan(sims)]


def merge(emb, labels, threshold, k, mutual=True, min_shared=0, num_clusters=None, ahc_max=None, max_rounds=16):
    """-> dict(labels int32 [n], sizes int32 [n], counts int32 [4], fragment_map int32 [C0], rounds): every round a dict of
    kind, clusters_in, clusters_out, centroids, the round's labels, `entering` (the rows' labels it started from), and the
    lists (scores, indices) or the affinity and merge_sim."""
    cur = np.array(labels, dtype=np.int64)
    C = int(cur.max()) + 1 if cur.size else 0
    ahc_max = AHC_LIMITS[1] if ahc_max is None else ahc_max
    fmap, rounds, r, linked = np.arange(C), [], 0, 0
    while C > 1:
        cent = centroids(emb, cur)
        here = dict(clusters_in=C, centroids=cent, entering=cur.copy())
        if C <= ahc_max:
            aff = cosines(cent).astype(np.float32)
            lab, left, sims = ahc_round(aff, threshold, num_clusters)
            if left < 0:
                raise ValueError("a centroid is not finite")
            rounds.append(dict(here, kind="ahc", clusters_out=left, affinity=aff, labels=lab, merge_sim=sims))
            cur, fmap, C, linked = through(lab, cur), lab[fmap], left, 1
            break
        if r == max_rounds:
            break
        score, index = lists(cent, k)
        lab, left = knn_round(score, index, k, threshold, min_shared, mutual)
        rounds.append(dict(here, kind="knn", clusters_out=left, scores=score, indices=index, labels=lab))
        cur, fmap = through(lab, cur), lab[fmap]
        if left == C:
            break
        C, r = left, r + 1
    sizes = np.zeros(cur.size, dtype=np.int32)
    sizes[:C] = np.bincount(cur[cur >= 0], minlength=C)
    return dict(labels=cur.astype(np.int32), sizes=sizes, counts=np.array([C, (cur < 0).sum(), r, linked], dtype=np.int32),
                fragment_map=fmap.astype(np.int32), rounds=rounds)


def adopt(emb, labels, threshold):
    """-> (labels int32 [n], counts int32 [4] = (C, rows still -1, rows adopted, 0), the -1 rows' cosines to every centroid)."""
    cur = np.array(labels, dtype=np.int64)
    C = int(cur.max()) + 1 if cur.size else 0
    lone = np.flatnonzero(cur < 0)
    cos = np.zeros((lone.size, C))
    adopted = 0
    if C and lone.size:
        cos = cosines(np.asarray(emb)[lone], centroids(emb, cur))
        best = np.argmax(cos, axis=1)
        take = cos[np.arange(lone.size), best].astype(np.float32) >= np.float32(threshold)
        cur[lone[take]] = best[take]
        adopted = int(take.sum())
    return cur.astype(np.int32), np.array([C, (cur < 0).sum(), adopted, 0], dtype=np.int32), cos


def first_rows(labels):
    """The smallest row of every cluster, by cluster number: increasing is the numbering invariant."""
    labels = np.asarray(labels)
    return [int(np.flatnonzero(labels == c)[0]) for c in range(int(labels.max()) + 1 if labels.size else 0)]


def pure(labels, speaker):
    labels = np.asarray(labels)
    return all(len(set(speaker[labels == c])) == 1 for c in range(int(labels.max()) + 1))


class HostEngine:
    """The five entries `merge_clusters` and `adopt_rows` call, as the float64 forms above on torch CPU tensors.  `calls`
    counts them by name."""

    def __init__(self):
        import torch
        self.torch, self.device, self.calls = torch, torch.device("cpu"), {}

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def to_device(self, x, dtype=None):
        t = x if isinstance(x, self.torch.Tensor) else self.torch.from_numpy(np.ascontiguousarray(x).copy())
        return (t if dtype is None else t.to(dtype)).contiguous()

    def ahc_limits(self):
        return AHC_LIMITS

    def embedding_pool(self, emb, seg_start=None, row_index=None, l2_rows=False, l2_mean=False):
        self._count("embedding_pool")
        assert l2_rows and l2_mean
        x, labels = emb.numpy(), np.full(emb.shape[0], -1, dtype=np.int64)
        for c in range(len(seg_start) - 1):
            labels[row_index[seg_start[c]:seg_start[c + 1]]] = c
        return self.torch.from_numpy(centroids(x, labels))

    def cosine_topk(self, query, gallery, k, exclude=None):
        self._count("cosine_topk")
        cos = cosines(query.numpy(), gallery.numpy())
        if exclude is not None:
            cos[np.arange(cos.shape[0]), exclude.numpy()] = np.nan
        have = min(k, int((~np.isnan(cos[0])).sum())) if cos.shape[0] else 0
        score = np.full((cos.shape[0], k), -np.inf, dtype=np.float32)
        index = np.full((cos.shape[0], k), -1, dtype=np.int64)
        if have:
            score[:, :have], index[:, :have] = D.topk_f64(cos, have)
        return self.torch.from_numpy(score), self.torch.from_numpy(index)

    def knn_cluster(self, scores, indices, *, threshold, min_shared=0, mutual=True, min_size=1):
        self._count("knn_cluster")
        out = R.cluster(indices.numpy(), scores.numpy(), scores.shape[1], threshold, min_shared, mutual, min_size)
        return tuple(self.torch.from_numpy(np.asarray(o)) for o in out)

    def segment_affinity(self, emb, n_seg):
        self._count("segment_affinity")
        assert emb.dim() == 3 and emb.shape[0] == 1 and list(n_seg) == [emb.shape[1]]
        return self.torch.from_numpy(cosines(emb[0].numpy()).astype(np.float32)[None])

    def ahc(self, aff, n_seg, threshold=None, min_clusters=1, max_clusters=None, target=None, bad_count=None):
        self._count("ahc")
        n = int(n_seg[0])
        labels, count, _, _ = A.ahc(aff[0].numpy(), n, threshold, min_clusters, max_clusters,
                                    None if target is None else int(target[0]))
        if count < 0:
            bad_count += 1
        return self.torch.from_numpy(labels[None]), self.torch.tensor([count], dtype=self.torch.int32)
