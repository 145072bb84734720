"""The definition of svk_spectral_embed (include/svk.h) in NumPy float64.

    nodes       without groups node a is window a; with groups M[a][b] is the mean of the affinities that join a member of a to
                a member of b, added one at a time into one accumulator (i over a ascending, j over b ascending inside it:
                np.cumsum adds in exactly that order).  Only entries above the diagonal are read
    graph(p)    row a keeps its p largest M[a][b], b != a, ties to the lower b (a stable descending sort); S = (B + B^T) / 2,
                L = diag(S 1) - S.  Returned as 2 S in uint8, as the entry does
    count       the first largest gap among lambda_(i+1) - lambda_i, i = 1 .. min(max_speakers, m - 1), raised to min_speakers,
                capped at m; a target >= 1 replaces it (capped at m and max_speakers)
    neighbours  r(p) = p lambda_max / largest gap (+inf for a gap that is not positive), the smallest wins, the first among equals
    sign        the entry of largest magnitude of every eigenvector, the lowest index among equals, is positive
numpy.linalg.eigh is the eigensolver for DECISIONS.  `jacobi` restates the header's eigensolver (same ordering, same rotation
formula, same stopping rule) in plain NumPy: it is the accuracy yardstick the device is held against, never the device itself."""
import numpy as np

from ahc_f64_ref import ahc

MAX_SWEEPS = 30
EPS = 2.0 ** -52


# ---- closed-form spectra ---------------------------------------------------------------------------------------------
def complete_union_spectrum(s, count):
    """`count` disjoint complete graphs K_s: eigenvalue 0 once per graph, s otherwise.  Ascending, float64 (exact)."""
    return np.sort(np.concatenate([np.zeros(count), np.full(count * (s - 1), float(s))]))


def cycle_spectrum(m):
    """The m-cycle: 2 - 2 cos(2 pi j / m), evaluated in longdouble, ascending."""
    j = np.arange(m, dtype=np.longdouble)
    return np.sort(2 - 2 * np.cos(2 * np.pi * j / np.longdouble(m)))


def complete_union_affinity(s, count, stride=None):
    """Affinities 1 inside a group of s consecutive windows, 0 across: with p = s - 1 the graph is `count` disjoint K_s."""
    m = s * count
    aff = np.zeros((stride or m, stride or m), np.float32)
    for g in range(count):
        aff[g * s:(g + 1) * s, g * s:(g + 1) * s] = 1.0
    return aff


def cycle_affinity(m, stride=None):
    """Affinity 1 between ring neighbours, 0 elsewhere: with p = 2 the graph is the m-cycle (m >= 4)."""
    aff = np.zeros((stride or m, stride or m), np.float32)
    i = np.arange(m)
    aff[i, (i + 1) % m] = 1.0
    aff[(i + 1) % m, i] = 1.0
    return aff


# ---- the definition --------------------------------------------------------------------------------------------------
def node_means(aff, n, group=None, node_stride=None):
    """-> (M float64 [m, m] with a zero diagonal, m), or None for a bad recording."""
    aff = np.asarray(aff)
    stride = aff.shape[0]
    n = int(n)
    if n < 0 or n > stride:
        return None
    up = np.triu(aff[:n, :n].astype(np.float64), 1)
    W = up + up.T
    if group is None:
        if not np.all(np.isfinite(W)):
            return None
        return W, n
    g = np.asarray(group)[:n].astype(np.int64)
    if n == 0:
        return np.zeros((0, 0)), 0
    if g.min() < 0 or g.max() >= node_stride:
        return None
    m = int(g.max()) + 1
    members = [np.flatnonzero(g == a) for a in range(m)]
    if any(len(x) == 0 for x in members):
        return None
    M = np.zeros((m, m))
    for a in range(m):
        for b in range(a + 1, m):
            block = W[np.ix_(members[a], members[b])].ravel()        # i ascending, j ascending inside it
            if not np.all(np.isfinite(block)):
                return None
            M[a, b] = M[b, a] = np.cumsum(block)[-1] / float(len(members[a]) * len(members[b]))
    return M, m


def neighbour_order(M):
    """Row a's partners b != a from the largest M[a][b] down, ties to the lower b: int [m, m - 1]."""
    m = M.shape[0]
    rows = []
    for a in range(m):
        key = -M[a].copy()
        key[a] = np.inf
        rows.append(np.argsort(key, kind="stable")[:m - 1])
    return np.array(rows, np.int64).reshape(m, max(m - 1, 0))


def graph2(order, p):
    """2 S of the top-p graph: uint8 [m, m] with entries in {0, 1, 2}."""
    m = order.shape[0]
    B = np.zeros((m, m), np.uint8)
    for a in range(m):
        B[a, order[a, :p]] = 1
    return B + B.T


def laplacian(S2):
    S = S2.astype(np.float64) / 2
    return np.diag(S.sum(1)) - S


def largest_gap(lam, max_speakers):
    """(the largest gap, the first i in 1 .. min(max_speakers, m - 1) that has it, the second largest gap or -inf)."""
    m = len(lam)
    gaps = np.diff(lam)[:min(max_speakers, m - 1)]
    k = int(np.argmax(gaps))
    rest = np.delete(gaps, k)
    return float(gaps[k]), k + 1, (float(rest.max()) if rest.size else -np.inf)


def fix_signs(V):
    """Columns of V with their entry of largest magnitude (the first among equals) made positive."""
    V = V.copy()
    for j in range(V.shape[1]):
        a = int(np.argmax(np.abs(V[:, j])))
        if V[a, j] < 0:
            V[:, j] = -V[:, j]
    return V


def candidates(neighbours):
    """An int, or (lo, hi, step) -> (lo, step, count), as Engine.spectral_embed reads it."""
    if isinstance(neighbours, (int, np.integer)):
        return int(neighbours), 1, 1
    lo, hi, step = neighbours
    return int(lo), int(step), (int(hi) - int(lo)) // int(step) + 1


def spectral(aff, n, group=None, node_stride=None, neighbours=(2, 32, 2), min_speakers=1, max_speakers=8, target=None,
             eig=np.linalg.eigh):
    """One recording.  -> dict: n_nodes, n_speakers, neighbours, ratio [count] (and what it is made of: top = lambda_max and
    gap = the largest gap of every evaluated candidate), graph (2 S, uint8 [m, m]), eigval [m],
    eigvec [m, k] (sign fixed), embed float32 [m, max_speakers], and the margins the decisions were taken with:
    margin_ratio (runner-up r / best r - 1), margin_gap (1 - second gap / largest gap on the chosen graph), margin_keep (the
    smallest (last kept - first dropped) / largest |M| over every row and evaluated candidate), margin_cut ((lambda_(k+1) -
    lambda_k) / lambda_max: the k vectors of the embedding span a space of their own only if it is positive).  Bad: {"n_nodes": -1, ...}."""
    lo, step, count = candidates(neighbours)
    bad = {"n_nodes": -1, "n_speakers": -1, "neighbours": -1, "ratio": np.full(count, np.nan)}
    nodes = node_means(aff, n, group, node_stride)
    if nodes is None:
        return bad
    M, m = nodes
    ratio, tops, gaps = np.full(count, np.nan), np.full(count, np.nan), np.full(count, np.nan)
    if m <= 1:
        return {"n_nodes": m, "n_speakers": m, "neighbours": 0, "ratio": ratio, "graph": np.zeros((m, m), np.uint8),
                "eigval": np.zeros(m), "eigvec": np.ones((m, m)), "embed": np.eye(m, max_speakers, dtype=np.float32),
                "margin_ratio": np.inf, "margin_gap": np.inf, "margin_keep": np.inf, "margin_cut": np.inf}
    order = neighbour_order(M)
    ranked = np.take_along_axis(M, order, axis=1)
    scale = max(float(np.abs(M).max()), np.finfo(np.float64).tiny)
    best, last, margin_keep, seen = None, None, np.inf, []
    for c in range(count):
        p = min(lo + c * step, m - 1)
        if p == last:
            break
        last = p
        if p < m - 1:
            margin_keep = min(margin_keep, float((ranked[:, p - 1] - ranked[:, p]).min()) / scale)
        lam = np.sort(eig(laplacian(graph2(order, p)))[0])
        gap = largest_gap(lam, max_speakers)[0]
        r = p * lam[-1] / gap if gap > 0 else np.inf
        ratio[c], tops[c], gaps[c] = r, lam[-1], gap
        seen.append(r)
        if best is None or r < best[0]:
            best = (r, p)
    p = best[1]
    S2 = graph2(order, p)
    lam, V = eig(laplacian(S2))
    idx = np.argsort(lam, kind="stable")
    lam, V = lam[idx], V[:, idx]
    gap, k, second = largest_gap(lam, max_speakers)
    k = min(max(k, min_speakers), m)
    if target is not None and int(target) >= 1:
        k = min(int(target), m, max_speakers)
    V = fix_signs(V[:, :k])
    embed = np.zeros((m, max_speakers), np.float32)
    embed[:, :k] = V.astype(np.float32)
    others = sorted(seen)
    margin_ratio = np.inf if len(others) < 2 or not np.isfinite(others[1]) else others[1] / others[0] - 1
    return {"n_nodes": m, "n_speakers": k, "neighbours": p, "ratio": ratio, "graph": S2, "eigval": lam, "eigvec": V,
            "embed": embed, "top": tops, "gap": gaps, "margin_ratio": margin_ratio, "margin_gap": (1 - second / gap) if gap > 0 else 0.0,
            "margin_keep": margin_keep, "margin_cut": np.inf if k >= m else float(lam[k] - lam[k - 1]) / float(lam[-1])}


# ---- labels from an embedding: what svk_segment_affinity + svk_ahc(target = k) compute ----------------------------------
def cosine_affinity(emb):
    """float32 [m, m]: (float)(x.y / (||x|| ||y||)) in float64, a zero norm divides by 1."""
    x = np.asarray(emb, np.float64)
    norm = np.sqrt((x * x).sum(1))
    norm[norm == 0] = 1.0
    return ((x @ x.T) / np.outer(norm, norm)).astype(np.float32)


def embedding_labels(embed, m, k):
    """int32 [m]: average-linkage clustering of the cosines of the m embedding rows down to k clusters."""
    if m == 0:
        return np.zeros(0, np.int32)
    return ahc(cosine_affinity(np.asarray(embed)[:m]), m, target=k)[0][:m]


def gather_labels(node_labels, group, n):
    """Window labels: the node labels gathered through the groups."""
    return np.asarray(node_labels)[np.asarray(group)[:n]]


# ---- the header's Jacobi, restated -----------------------------------------------------------------------------------
def round_pairs(M2, r):
    """Round r of the round-robin over M2 (even) indices: (p, q) int arrays [M2 / 2] with p < q."""
    k = np.arange(1, M2 // 2)
    a = np.concatenate([[M2 - 1], (r + k) % (M2 - 1)])
    b = np.concatenate([[r], (r - k) % (M2 - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(L):
    """-> (eigenvalues ascending [m], eigenvectors as columns [m, m] in that order, sweeps run, converged)."""
    L = np.asarray(L, np.float64)
    m = L.shape[0]
    M2 = m + (m & 1)
    H = M2 // 2
    A = np.zeros((M2, M2))
    A[:m, :m] = L
    V = np.eye(M2)
    tol = EPS * np.sqrt((L * L).sum())
    off_mask = ~np.eye(M2, dtype=bool)
    pair_of = np.zeros(M2, np.int64)
    sweeps, converged = 0, False
    for sweep in range(MAX_SWEEPS + 1):
        if np.abs(A[off_mask]).max(initial=0.0) <= tol:
            converged = True
            break
        if sweep == MAX_SWEEPS:
            break
        sweeps += 1
        for r in range(M2 - 1):
            P, Q = round_pairs(M2, r)
            apq = A[P, Q]
            live = apq != 0
            safe = np.where(live, apq, 1.0)
            with np.errstate(over="ignore"):
                theta = (A[Q, Q] - A[P, P]) / (2 * safe)
                t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            t = np.where(live, t, 0.0)
            c = np.where(live, 1 / np.sqrt(t * t + 1), 1.0)
            s = t * c
            Ap, Aq = A[:, P].copy(), A[:, Q].copy()                # columns, then rows
            A[:, P], A[:, Q] = c * Ap - s * Aq, s * Ap + c * Aq
            Ap, Aq = A[P, :].copy(), A[Q, :].copy()
            A[P, :], A[Q, :] = c[:, None] * Ap - s[:, None] * Aq, s[:, None] * Ap + c[:, None] * Aq
            pair_of[P] = pair_of[Q] = np.arange(H)
            upper = pair_of[:, None] <= pair_of[None, :]          # block (k, k'), k <= k', and its mirror image
            A = np.where(upper, A, A.T)
            A[P, Q], A[Q, P] = 0.0, 0.0                            # annihilated: set to zero outright
            Vp, Vq = V[:, P].copy(), V[:, Q].copy()
            V[:, P], V[:, Q] = c * Vp - s * Vq, s * Vp + c * Vq
    lam = np.diag(A)[:m]
    idx = np.argsort(lam, kind="stable")
    return lam[idx], V[:m, :m][:, idx], sweeps, converged


def accuracy(L, lam, V, lam_true):
    """The three error figures of an eigensolution (lam [m] ascending, V [m, k] the first k vectors) of L, in units of
    m 2^-52 lambda_max (eigenvalues against lam_true, residual) and of m 2^-52 (orthogonality)."""
    L = np.asarray(L, np.float64)
    m = L.shape[0]
    top = float(np.max(np.abs(np.asarray(lam_true, np.float64))))
    unit = m * EPS
    k = V.shape[1]
    e_val = float(np.max(np.abs(np.asarray(lam, np.longdouble) - np.asarray(lam_true, np.longdouble)))) / (unit * top)
    e_res = float(np.max(np.abs(L @ V - V * np.asarray(lam)[None, :k]))) / (unit * top) if k else 0.0
    e_orth = float(np.max(np.abs(V.T @ V - np.eye(k)))) / unit if k else 0.0
    return e_val, e_res, e_orth
