"""The reference of svk_cosine_topk_norm (include/svk.h, "top-k search on normalised scores"), built from the PLAIN entry's own bits so that the GPU
comparisons need no tolerance:

  raw_matrix   the full raw score matrix of a small problem, recovered by calling svk_cosine_topk over gallery chunks of at
               most 32 rows with k = the chunk's size (every row of the chunk is returned, so the lists ARE the matrix).  The
               contract makes those bits the ones a whole call uses: a score depends on its two rows and dim alone.
  normalise    svk_score_norm's expression in NumPy float64, every operation on its own in the written order, rounded to
               float32 once.
  topk         the k best columns of every row under the total order, in pure Python: NaN above every number, the higher
               value first, -0 == +0, the lower index among equals, -inf / -1 past the candidates.

NumPy only; `raw_matrix` is the one function that touches the device, and it calls nothing this reference is used to test."""
import numpy as np

MODES = ("z", "t", "s")
CHUNK = 32


def raw_matrix(eng, q, g):
    """float32 [nq, ng]: svk_cosine_topk's score of every (query row, gallery row), bit for bit."""
    import torch
    q, g = eng.to_device(q, torch.float32), eng.to_device(g, torch.float32)
    nq, ng = int(q.shape[0]), int(g.shape[0])
    out = np.zeros((nq, ng), dtype=np.float32)
    seen = np.zeros((nq, ng), dtype=bool)
    rows = np.arange(nq)[:, None]
    for lo in range(0, ng, CHUNK):
        n = min(CHUNK, ng - lo)
        sc, ix = eng.cosine_topk(q, g[lo:lo + n], n)
        sc, ix = sc.cpu().numpy(), ix.cpu().numpy()
        assert np.all(np.sort(ix, axis=1) == np.arange(n)[None, :]), "k = the chunk's size returns every row once"
        out[rows, lo + ix] = sc
        seen[rows, lo + ix] = True
    assert seen.all()
    return out


def tables(mode, query_moments, gallery_moments):
    """(query table or None, gallery table or None) of a mode: "t" the query side, "z" the gallery side, "s" both."""
    assert mode in MODES
    return (query_moments if mode in "ts" else None), (gallery_moments if mode in "zs" else None)


def normalise(raw, query_moments=None, gallery_moments=None):
    """float32 [nq, ng] from raw float32 [nq, ng] and float64 [n, 2] {mean, std} tables (one may be None)."""
    assert query_moments is not None or gallery_moments is not None
    x = np.asarray(raw, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if query_moments is not None:
            qm = np.asarray(query_moments, dtype=np.float64)
            a = x - qm[:, 0][:, None]
            a = a / qm[:, 1][:, None]
        if gallery_moments is not None:
            gm = np.asarray(gallery_moments, dtype=np.float64)
            b = x - gm[:, 0][None, :]
            b = b / gm[:, 1][None, :]
        if query_moments is not None and gallery_moments is not None:
            v = a + b
            v = 0.5 * v
        else:
            v = a if query_moments is not None else b
        return v.astype(np.float32)


def order_key(value):
    """The unsigned integer that sorts float32 values as the contract orders them (larger = earlier): NaN on top, -0 as +0."""
    b = int(np.asarray(value, dtype=np.float32).view(np.uint32))
    if value != value:
        return 0xFFFFFFFF
    if b == 0x80000000:
        b = 0
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def topk(values, k, exclude=None, index_base=0):
    """(float32 [nq, k], int64 [nq, k]): the k best columns of every row of float32 `values`, best first; an index is
    index_base + the column; exclude: None or one GLOBAL index per row that is no candidate."""
    values = np.asarray(values, dtype=np.float32)
    nq, ng = values.shape
    scores = np.full((nq, k), -np.inf, dtype=np.float32)
    indices = np.full((nq, k), -1, dtype=np.int64)
    for r in range(nq):
        skip = None if exclude is None else int(exclude[r]) - index_base
        cand = [(-order_key(values[r, c]), c) for c in range(ng) if c != skip]
        cand.sort()
        for j, (_, c) in enumerate(cand[:k]):
            scores[r, j] = values[r, c]
            indices[r, j] = index_base + c
    return scores, indices


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def ulps_apart(a, b):
    """How many float32 values lie between two finite float32 values of the same sign (0: the same bits)."""
    return abs(int(bits(np.float32(a))[0]) - int(bits(np.float32(b))[0]))


# ---- inputs ------------------------------------------------------------------------------------------------------------
def random_problem(nq, ng, dim, seed, sd_decades=1.0):
    """(q, g, query moments, gallery moments): N(0, 1) float32 rows; means N(0, 0.1), deviations 10^U(-d, d), d = sd_decades."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    g = rng.standard_normal((ng, dim)).astype(np.float32)

    def moments(n):
        return np.stack([0.1 * rng.standard_normal(n), 10.0 ** rng.uniform(-sd_decades, sd_decades, n)], axis=1)
    return q, g, moments(nq), moments(ng)


# The staircase: STAIR_COPIES copies of one gallery row among random rows.  Every copy has the same raw score against a query
# (a score's bits depend on its two rows alone), near 0.9 against query 0, which is that row plus a little noise.  The copies'
# column deviations are 1 and their means FALL by STAIR_STEP from copy to copy, so the normalised value s - mu_j climbs by
# half a float32 unit in the last place per copy (values in [0.5, 1): one unit is 2^-24): neighbouring copies are equal or one
# float32 apart, the best copies are the LAST ones, and inside a plateau the lower index wins.  The k-th place is decided in
# the last bit: a selection that filters with too small a margin, or orders equal values by arrival, fails here.
STAIR_COPIES, STAIR_NG, STAIR_DIM, STAIR_NQ = 72, 200, 128, 3
STAIR_STEP = {"z": 2.0 ** -25, "s": 2.0 ** -24}          # "s" halves the column term
STAIR_QUERY_MOMENTS = np.array([[-0.05, 1.0], [0.0, 1.0], [0.02, 1.0]])


def stair_rows():
    """The gallery positions of the copies, ascending: across tiles, never adjacent."""
    return np.array([2 + (STAIR_NG - 4) * j // STAIR_COPIES for j in range(STAIR_COPIES)], dtype=np.int64)


def staircase(mode):
    """(q, g, query moments, gallery moments) of the staircase for mode "z" or "s"."""
    rng = np.random.default_rng(29)
    g = rng.standard_normal((STAIR_NG, STAIR_DIM)).astype(np.float32)
    row = rng.standard_normal(STAIR_DIM).astype(np.float32)
    rows = stair_rows()
    g[rows] = row
    q = rng.standard_normal((STAIR_NQ, STAIR_DIM)).astype(np.float32)
    q[0] = row + (0.48 * rng.standard_normal(STAIR_DIM)).astype(np.float32)        # cosine about 0.9
    gm = np.stack([np.full(STAIR_NG, 0.5), np.ones(STAIR_NG)], axis=1)            # the other rows: far below the copies
    gm[rows, 0] = -STAIR_STEP[mode] * np.arange(STAIR_COPIES)
    return q, g, STAIR_QUERY_MOMENTS.copy(), gm


def stair_steps(values_row):
    """The float32 distances between neighbouring copies' normalised values, in units of the last place."""
    v = np.asarray(values_row, dtype=np.float32)[stair_rows()]
    return [ulps_apart(v[j], v[j + 1]) for j in range(STAIR_COPIES - 1)]
