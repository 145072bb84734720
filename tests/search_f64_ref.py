"""Float64 references and input makers for svk_cosine_topk's selection and merge (tests/test_search_host.py checks the
inputs on the host, tests/test_cosine_topk_paths.py runs them on the MI355X).  NumPy and nothing from the library under test.

WHY INDEX EQUALITY IS A FAIR DEMAND HERE.  On random data adjacent float64 scores lie closer than the f32 chain's error, so
tests/test_cosine_topk.py allows any swap within 2e-5.  `planted` builds inputs on which that cannot happen: for a chosen
query a, the gallery rows at chosen positions are 3 (c_j q^_a + sqrt(1 - c_j^2) r_perp) with c_j = 0.95 - 0.01 j (float64,
rounded to float32 once), so their float64 cosines against q_a are 0.95, 0.94, ... with gaps of 0.01, far above any
background row of N(0, 1) data.  `margin` measures the smallest gap among a query's best k + 1; where it is at least
4 COSINE_TOL (two neighbours may each move by COSINE_TOL: 2 x; the other 2 x is headroom) every kernel that meets the score
bar MUST return the float64 ranking `rank64`, index for index.  The condition is established by the reference alone.

THE GEOMETRY (restated from the documented plan, DESIGN.md 3.10, so that a test can aim at it): the gallery is cut into
32-row tiles, and into S = min(2048 / row blocks, tiles / 32, 1024) spans of whole tiles, span s = tiles
[tiles s / S, tiles (s + 1) / S); a row block is 128 queries; the merge's lane t owns the lists t, t + 64, t + 128, ...
The workspace holds the two 1 / norm vectors and two sections of S n_query k 4-byte entries, each rounded up to 16 bytes.
"""
import numpy as np

TILE = 32


# ---- the order contract in float64 ---------------------------------------------------------------------------------
def _candidates(row, exclude):
    cols = np.arange(row.size)
    if exclude is not None and 0 <= exclude < row.size:
        cols = cols[cols != exclude]
    return cols


def _order(scores):
    """Positions of `scores` (1-D float64) under the contract: NaN above every number, the higher score first, -0 == +0, the
    lower position among equals."""
    nan = np.isnan(scores)
    finite = np.where(nan, 0.0, scores) + 0.0            # -0.0 + 0.0 = +0.0
    return np.lexsort((np.arange(scores.size), -finite, ~nan))


def rank64(cos64, k, exclude=None):
    """int64 [nq, k]: the k best columns of every row of cos64 under the total order, -1 past the candidates.  exclude: None
    or one column per row that is no candidate (a value outside [0, n_columns) removes nothing)."""
    cos64 = np.asarray(cos64, dtype=np.float64)
    nq = cos64.shape[0]
    out = np.full((nq, k), -1, dtype=np.int64)
    for r in range(nq):
        cols = _candidates(cos64[r], None if exclude is None else int(exclude[r]))
        best = cols[_order(cos64[r, cols])[:k]]
        out[r, :best.size] = best
    return out


def margin(cos64, k, exclude=None):
    """float64 [nq]: the smallest gap between consecutive scores among every row's best min(k + 1, candidates) (+inf where
    fewer than two)."""
    cos64 = np.asarray(cos64, dtype=np.float64)
    out = np.full(cos64.shape[0], np.inf)
    for r in range(cos64.shape[0]):
        cols = _candidates(cos64[r], None if exclude is None else int(exclude[r]))
        s = cos64[r, cols]
        best = s[_order(s)[:k + 1]]
        if best.size >= 2:
            out[r] = np.min(best[:-1] - best[1:])
    return out


def cosine64(q, g):
    x, y = np.asarray(q).astype(np.float64), np.asarray(g).astype(np.float64)
    nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
    nx[nx == 0] = 1.0
    ny[ny == 0] = 1.0
    return (x @ y.T) / (nx[:, None] * ny[None, :])


# ---- planted inputs --------------------------------------------------------------------------------------------------
def planted_cosine(j):
    return 0.95 - 0.01 * j


def planted(nq, ng, dim, seed, spec):
    """(q, g, where): float32 N(0, 1) queries [nq, dim] and gallery [ng, dim]; for every query a of `spec` (a -> gallery
    positions) row spec[a][j] of g is 3 (c_j q^_a + sqrt(1 - c_j^2) r_perp), c_j = 0.95 - 0.01 j, r_perp a random unit vector
    orthogonal to q_a: built in float64, rounded once.  where[a] = the positions as int64, best first."""
    assert dim >= 2
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    g = rng.standard_normal((ng, dim)).astype(np.float32)
    where, used = {}, set()
    for a in sorted(spec):
        pos = np.asarray(spec[a], dtype=np.int64)
        assert pos.ndim == 1 and pos.size <= 40 and np.all((pos >= 0) & (pos < ng)) and 0 <= a < nq
        assert not used.intersection(pos.tolist()) and np.unique(pos).size == pos.size, "a gallery row is planted once"
        used.update(pos.tolist())
        qa = q[a].astype(np.float64)
        qa /= np.sqrt(qa @ qa)
        for j, p in enumerate(pos):
            r = rng.standard_normal(dim)
            r -= (r @ qa) * qa
            r /= np.sqrt(r @ r)
            c = planted_cosine(j)
            g[p] = (3.0 * (c * qa + np.sqrt(1.0 - c * c) * r)).astype(np.float32)
        where[a] = pos
    return q, g, where


# ---- the split of a call ---------------------------------------------------------------------------------------------
def span_rows(ng, spans):
    """[(first row, one past the last row)] of the gallery spans of a call over ng rows that the plan cuts into `spans`."""
    tiles = (ng + TILE - 1) // TILE
    return [(tiles * s // spans * TILE, min(tiles * (s + 1) // spans * TILE, ng)) for s in range(spans)]


def span_of(row, ng, spans):
    tiles = (ng + TILE - 1) // TILE
    t = row // TILE
    return next(s for s in range(spans) if tiles * s // spans <= t < tiles * (s + 1) // spans)


def spans_from_workspace(nbytes, nq, ng, k):
    """The span count of a call, recovered from its workspace size (see the module docstring).  Exact when n_query k >= 4,
    where 16 bytes of padding are less than one span's entries."""
    def up(v):
        return (v + 15) & ~15
    assert nq * k >= 4
    section = (nbytes - up(4 * nq) - up(4 * ng)) // 2
    assert section > 0 and up(4 * (section // (4 * nq * k)) * nq * k) == section
    return section // (4 * nq * k)


# ---- the planted cases, shared by the host checks and the GPU tests ----------------------------------------------------
BIG_NG, BIG_SPANS, BIG_SPAN_ROWS = 133_100, 130, 1024        # 4 160 tiles, the last one 12 rows


def _big_spec():
    ng, w = BIG_NG, BIG_SPAN_ROWS
    spec = {}
    # query 0: 40 rows in ONE span (77), scores shuffled against the index: the span's list saturates and drops 8
    spec[0] = [77 * w + 5 + 13 * ((17 * j) % 40) for j in range(40)]
    # query 1: one row in each of 40 spans, among them 0 / 64 / 128 and 1 / 65 / 129 -- the three lists of lanes 0 and 1 --
    # with the best rows in those six, so that a lane's cursor advances and its next head is in another of its lists
    others = [3 * m + 3 for m in range(34)]
    order = [129, 0, 1, 128, 65, 64] + [others[(7 * m) % 34] for m in range(34)]
    spec[1] = [s * w + (37 * j + 11) % 1000 for j, s in enumerate(order)]
    # query 2: gallery row 0, the last row (inside the ragged tile), and the last / first row on both sides of 19 span borders
    borders = [1, 2, 10, 20, 33, 40, 50, 63, 64, 65, 66, 80, 90, 100, 110, 120, 127, 128, 129]
    rows = [0, ng - 1] + [b * w - d for b in borders for d in (1, 0)]
    spec[2] = [rows[(13 * j) % 40] for j in range(40)]
    # query 3: the better the row, the higher its index: the best row arrives last, in the last span
    spec[3] = [133_000 - 3_300 * j for j in range(40)]
    # queries 127 (last of the first row block), 128 and 129 (alone in the ragged second row block): spread over 40 spans
    for a, base in ((127, 500), (128, 700), (129, 900)):
        spec[a] = [base + 3_313 * ((11 * j) % 40) for j in range(40)]
    return spec


def _small_spec(queries, ng=4200, span_rows_=1056):
    """40 rows per planted query over the 4 spans of a 4 200-row gallery; the first query takes the rows at the span borders."""
    spec = {}
    for n, a in enumerate(queries):
        rows = [3 + 26 * n + 104 * ((11 * j) % 40) for j in range(40)]
        if n == 0:
            rows[:8] = [ng - 1, 0, span_rows_ - 1, span_rows_, 2 * span_rows_ - 1, 2 * span_rows_, 3 * span_rows_ - 1, 3 * span_rows_]
        spec[a] = rows
    return spec


# name -> (n_query, n_gallery, dim, seed, spec, smallest span count the case needs)
CASES = {
    "many_lists": (130, BIG_NG, 128, 11, _big_spec(), 129),          # also run with its first 4 queries (one row block)
    "streamed": (130, 4200, 200, 12, _small_spec((0, 127, 128, 129)), 2),
    "dim130": (5, 4200, 130, 13, _small_spec((0, 4)), 2),
    "offset": (4, 4200, 128, 14, _small_spec((0, 3)), 2),
    "exhausted": (3, 38, 16, 15, {0: [(7 * j + 3) % 38 for j in range(38)]}, 1),
}

# Exact ties on the large gallery: one row copied to 50 positions in 50 spans.  The 32 lowest lie in spans 0, 1, 3, 5, ..., 57,
# 64, 65: lanes 0 and 1 of the merge each give their first list's copy, advance, and find the next one in their SECOND list
# (64, 65) against an equal score in their third (128, 129).  TIE_NAN_ROW, in span 129, is set to NaN for the second half.
TIE_SPANS = [0, 1] + list(range(3, 59, 2)) + [64, 65] + [66 + 3 * i for i in range(15)] + [127, 128, 129]
TIE_ROWS = np.array([s * BIG_SPAN_ROWS + (29 * j + 3) % 1000 for j, s in enumerate(TIE_SPANS)], dtype=np.int64)
TIE_NAN_ROW = 129 * BIG_SPAN_ROWS + 777
# chunk borders inside spans: 1 500 and 1 577 rows (one span each: the convert path when first), 48 623 and 81 400 rows
CHUNK_BOUNDS = (0, 1_500, 50_123, 51_700, BIG_NG)

_built = {}


def case(name):
    """(q, g, where, cos64 of the planted queries {a: float64 [ng]}): built once per process, read-only."""
    if name not in _built:
        nq, ng, dim, seed, spec, _ = CASES[name]
        q, g, where = planted(nq, ng, dim, seed, spec)
        rows = sorted(where)
        cos = cosine64(q[rows], g)
        cos_of = {a: cos[n] for n, a in enumerate(rows)}
        for m in (q, g, cos):
            m.setflags(write=False)
        _built[name] = (q, g, where, cos_of)
    return _built[name]


def tie_case():
    """(q [4, 128], gallery with the copies, the same with TIE_NAN_ROW set to NaN): query 0 IS the copied row, queries 1 - 3
    are those of "many_lists"."""
    if "ties" not in _built:
        q, g, _, _ = case("many_lists")
        row = np.random.default_rng(16).standard_normal(128).astype(np.float32)
        q, g = np.concatenate([row[None], q[1:4]]), g.copy()
        g[TIE_ROWS] = row
        g_nan = g.copy()
        g_nan[TIE_NAN_ROW] = np.nan
        for m in (q, g, g_nan):
            m.setflags(write=False)
        _built["ties"] = (q, g, g_nan)
    return _built["ties"]
