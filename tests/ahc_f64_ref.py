"""The definition of svk_ahc in NumPy float64, as the naive form: every step looks at every live pair.

    W        float64, W[i][j] = W[j][i] = float64(aff[i][j]) for i < j < n (only entries above the diagonal are read)
    step     the live pair i < j with the largest W[i][j]; ties to the lowest i, then the lowest j (np.argmax over the
             row-major upper triangle returns exactly that one).  Taken if k > max_clusters, or if k > min_clusters and
             W[i][j] >= threshold; otherwise clustering stops
    merge    j into i: W[m][i] = W[i][m] = (s_i W[m][i] + s_j W[m][j]) / (s_i + s_j) for every other live m -- NumPy rounds each
             product, the sum and the quotient once (no fused multiply-add); s_i += s_j, j is retired
    labels   clusters numbered in the order of their lowest member; dead rows read -1 here
A recording with a non-finite entry above the diagonal of its live rows, or n outside [0, stride], is not clustered: labels -1
(its live rows'; every row when n is out of range), count -1, no merges."""
import numpy as np


def ahc(aff, n, threshold=np.inf, min_clusters=1, max_clusters=None, target=None):
    """aff: [stride, stride] float32.  Returns (labels int32 [stride], n_clusters, merge_pair int32 [stride, 2],
    merge_sim float64 [stride]); unused merge slots hold -1 / NaN."""
    aff = np.asarray(aff)
    stride = aff.shape[0]
    labels = np.full(stride, -1, np.int32)
    pairs = np.full((stride, 2), -1, np.int32)
    sims = np.full(stride, np.nan, np.float64)
    n = int(n)
    if n < 0 or n > stride:
        return labels, -1, pairs, sims
    if target is not None and int(target) >= 1:
        min_clusters = max_clusters = int(target)
    if max_clusters is None:
        max_clusters = 2 ** 31 - 1
    upper = np.triu(np.ones((n, n), bool), 1)
    W = np.zeros((n, n), np.float64)
    W[upper] = aff[:n, :n][upper].astype(np.float64)
    if not np.all(np.isfinite(W[upper])):
        return labels, -1, pairs, sims
    W = W + W.T
    live = np.ones(n, bool)
    size = np.ones(n, np.float64)
    rep = np.arange(n)
    k, t = n, 0
    while k >= 2:
        cand = np.where(upper & live[:, None] & live[None, :], W, -np.inf)
        flat = int(np.argmax(cand))
        i, j = divmod(flat, n)
        best = W[i, j]
        if not (k > max_clusters or (k > min_clusters and best >= threshold)):
            break
        pairs[t] = (i, j)
        sims[t] = best
        others = live.copy()
        others[i] = others[j] = False
        new = (size[i] * W[others, i] + size[j] * W[others, j]) / (size[i] + size[j])
        W[others, i] = new
        W[i, others] = new
        size[i] += size[j]
        live[j] = False
        rep[rep == j] = i
        k -= 1
        t += 1
    roots = np.flatnonzero(live)            # ascending: a cluster's representative is its lowest member
    number = {int(r): c for c, r in enumerate(roots)}
    for m in range(n):
        labels[m] = number[int(rep[m])]
    return labels, k if n else 0, pairs, sims


def ahc_batch(aff, n_seg, threshold=np.inf, min_clusters=1, max_clusters=None, target=None):
    """The same over a padded batch [n_rec, stride, stride]: stacked outputs."""
    outs = [ahc(aff[r], n_seg[r], threshold, min_clusters, max_clusters, None if target is None else target[r])
            for r in range(len(n_seg))]
    return (np.stack([o[0] for o in outs]), np.array([o[1] for o in outs], np.int32),
            np.stack([o[2] for o in outs]), np.stack([o[3] for o in outs]))
