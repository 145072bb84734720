"""The rule of include/svk.h ("shared-neighbour (Jarvis-Patrick) clustering of k-NN lists") in plain Python: sets, one float32 comparison per slot and a union-find by minimum.
Nothing from the package.  The GPU tests hold svk_knn_cluster to it exactly; tests/test_knn_cluster_host.py holds it to
scipy's connected components."""
import numpy as np


def neighbour_sets(index, k):
    """-> (one {neighbour: slot} dict per row: the valid slots of its first k, n_bad)."""
    index = np.asarray(index)
    n = index.shape[0]
    rows, n_bad = [], 0
    for i in range(n):
        valid = {}
        for a in range(k):
            v = int(index[i, a])
            if v == -1:                                           # empty
                continue
            if v < -1 or v >= n or v == i or v in valid:          # bad: counted once, treated as empty
                n_bad += 1
                continue
            valid[v] = a
        rows.append(valid)
    return rows, n_bad


def edges(index, score, k, threshold, min_shared=0, mutual=True):
    """-> (the sorted list of edges (i, j), i < j, n_bad)."""
    score = np.asarray(score, dtype=np.float32)
    thr = np.float32(threshold)
    assert not np.isnan(thr)
    rows, n_bad = neighbour_sets(index, k)

    def arc(i, j):
        a = rows[i].get(j)
        if a is None:
            return False
        return bool(thr == -np.inf or score[i, a] >= thr)          # IEEE: a NaN score fails, -0 >= +0 holds

    found = set()
    for i, valid in enumerate(rows):
        for j in valid:
            there, back = arc(i, j), arc(j, i)
            if not ((there and back) if mutual else (there or back)):
                continue
            if min_shared > 0 and len(set(valid) & set(rows[j])) < min_shared:
                continue
            found.add((min(i, j), max(i, j)))
    return sorted(found), n_bad


def components(n, edge_list):
    """root[i] = the smallest row of i's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in edge_list:
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def relabel(root, min_size=1):
    """-> (labels, sizes, C, unlabelled): components of >= min_size rows numbered by their smallest member."""
    root = np.asarray(root)
    n = root.size
    count = np.bincount(root, minlength=n) if n else np.zeros(0, dtype=np.int64)
    labels = np.full(n, -1, dtype=np.int32)
    sizes = np.zeros(n, dtype=np.int32)
    label_of, C = {}, 0
    for r in range(n):                                             # increasing smallest member
        if root[r] == r and count[r] >= min_size:
            label_of[r] = C
            sizes[C] = count[r]
            C += 1
    for i in range(n):
        labels[i] = label_of.get(int(root[i]), -1)
    return labels, sizes, C, int((labels < 0).sum())


def cluster(index, score, k, threshold, min_shared=0, mutual=True, min_size=1):
    """What svk_knn_cluster writes: (labels int32 [n], root int32 [n], sizes int32 [n], counts int32 [4] = (C, rows labelled
    -1, n_bad, 0))."""
    n = np.asarray(index).shape[0]
    edge_list, n_bad = edges(index, score, k, threshold, min_shared, mutual)
    root = components(n, edge_list)
    labels, sizes, C, unlabelled = relabel(root, min_size)
    return labels, root, sizes, np.array([C, unlabelled, n_bad, 0], dtype=np.int32)
