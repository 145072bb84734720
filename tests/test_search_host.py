"""The host side of the speaker search: `evaluation.topk_hits` against a direct loop, and the declaration of svk_cosine_topk in
the header and the binding; and the inputs of tests/test_cosine_topk_paths.py (tests/search_f64_ref.py): `rank64` against a
direct loop over the order contract, the margin of every planted case (>= 4 COSINE_TOL among a query's best k + 1 float64 scores:
the condition under which the GPU tests may demand the float64 ranking index for index), and the span count of every case,
recovered from svk_cosine_topk_workspace_bytes (no GPU)."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hits_by_loop(indices, true_columns):
    n, k = indices.shape
    hits = np.zeros(k, dtype=np.int64)
    for row in range(n):
        for r in range(k):
            if true_columns[row] >= 0 and true_columns[row] in list(indices[row, :r + 1]):
                hits[r] += 1
    return hits


@pytest.mark.parametrize("n,k,cols", [(200, 5, 12), (50, 1, 3), (7, 32, 40), (0, 4, 9), (64, 8, 4)])
def test_topk_hits(n, k, cols):
    from speaker_verification_amd.evaluation import topk_hits
    rng = np.random.default_rng(n + k)
    indices = np.full((n, k), -1, dtype=np.int64)
    for row in range(n):                                           # distinct columns, best first, -1 past the candidates
        m = min(k, cols, int(rng.integers(0, k + 1)))
        indices[row, :m] = rng.permutation(cols)[:m]
    true = rng.integers(-1, cols, n)                               # -1: the speaker is not enrolled
    got = topk_hits(indices, true)
    assert got.dtype == np.int64 and got.shape == (k,)
    np.testing.assert_array_equal(got, hits_by_loop(indices, true))
    assert np.all(np.diff(got) >= 0)


def test_topk_hits_never_counts_minus_one():
    from speaker_verification_amd.evaluation import topk_hits
    indices = np.array([[-1, -1, -1], [2, -1, -1], [0, 1, 2]], dtype=np.int64)
    np.testing.assert_array_equal(topk_hits(indices, np.array([-1, -1, -1])), [0, 0, 0])
    np.testing.assert_array_equal(topk_hits(indices, np.array([0, 2, 2])), [1, 1, 2])
    np.testing.assert_array_equal(topk_hits(indices[:, :1], np.array([0, 2, 0])), [2])
    with pytest.raises(ValueError):
        topk_hits(indices, np.array([0, 1]))


def test_header_and_binding_declare_the_search():
    from speaker_verification_amd import _lib
    header = open(os.path.join(REPO, "include", "svk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"size_t\s+svk_cosine_topk_workspace_bytes\s*\(\s*int32_t n_query, int32_t n_gallery, int32_t dim, int32_t k\)", code)
    decl = re.search(r"int\s+svk_cosine_topk\s*\((.*?)\)\s*;", code, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 14
    assert len(_lib.SIGNATURES["svk_cosine_topk"][1]) == 14 and len(_lib.SIGNATURES["svk_cosine_topk_workspace_bytes"][1]) == 4
    assert int(re.search(r"#define SVK_VERSION (\d+)", header).group(1)) == _lib.VERSION == 114


# ---- the inputs of tests/test_cosine_topk_paths.py, held to the conditions that make its demands fair -------------------
import scoring_f64_ref as SR          # noqa: E402  (tests/ is on sys.path)
import search_f64_ref as R            # noqa: E402

MARGIN = 4 * SR.COSINE_TOL


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    if not os.path.exists(os.path.join(REPO, "speaker_verification_amd", "libsvk.so")):
        entry.build()
    from speaker_verification_amd import _lib
    return _lib.load()


def spans_of_call(lib, nq, ng, dim, k=32):
    return R.spans_from_workspace(int(lib.svk_cosine_topk_workspace_bytes(nq, ng, dim, k)), nq, ng, k)


def before_by_definition(sa, ia, sb, ib):
    """The order contract, one clause at a time."""
    if np.isnan(sa) or np.isnan(sb):
        if np.isnan(sa) and np.isnan(sb):
            return ia < ib
        return bool(np.isnan(sa))
    if sa != sb:                                                   # -0.0 != +0.0 is False
        return sa > sb
    return ia < ib


def rank_by_loop(cos, k, exclude=None):
    out = np.full((cos.shape[0], k), -1, dtype=np.int64)
    for r in range(cos.shape[0]):
        left = [c for c in range(cos.shape[1]) if exclude is None or c != exclude[r]]
        for slot in range(min(k, len(left))):
            best = left[0]
            for c in left[1:]:
                if before_by_definition(cos[r, c], c, cos[r, best], best):
                    best = c
            out[r, slot] = best
            left.remove(best)
    return out


def test_rank64_against_a_direct_loop():
    rng = np.random.default_rng(5)
    cos = np.round(rng.standard_normal((6, 23)), 1)                # one decimal: many exact ties
    cos[0, [3, 9]] = np.nan
    cos[1, 4], cos[1, 11], cos[1, 17] = 0.0, -0.0, 0.0
    cos[1, [0, 1, 2]] = -1.0
    cos[2, :] = 0.5
    cos[3, 22] = np.nan
    cos[4, [5, 6]] = [-0.0, 0.0]
    exclude = np.array([3, 11, 0, -1, 23, 7])                      # a NaN, a zero, the first of equals, two outside, a plain one
    for k in (1, 5, 22, 23, 32):
        np.testing.assert_array_equal(R.rank64(cos, k), rank_by_loop(cos, k))
        np.testing.assert_array_equal(R.rank64(cos, k, exclude), rank_by_loop(cos, k, exclude))
    assert list(R.rank64(cos, 3)[0]) == [3, 9, int(np.nanargmax(cos[0]))]          # NaN first, the lower index first
    assert list(R.rank64(cos, 3, exclude)[0][:1]) == [9]
    assert list(R.rank64(cos, 4)[2]) == [0, 1, 2, 3] and list(R.rank64(cos, 32)[2][22:]) == [22] + [-1] * 9
    zeros = [c for c in R.rank64(cos, 23)[1] if cos[1, c] == 0]
    assert zeros == sorted(zeros) and {4, 11, 17} <= set(zeros)                   # -0 == +0: by index
    gaps = R.margin(cos, 5)
    assert gaps[2] == 0.0 and np.isnan(gaps[0])
    assert R.margin(np.array([[0.1, 0.9, 0.5, 0.45]]), 2)[0] == pytest.approx(0.05)  # the best 3: 0.9, 0.5, 0.45
    assert R.margin(np.array([[0.1, 0.9, 0.5, 0.45]]), 2, np.array([2]))[0] == pytest.approx(0.35)
    assert R.margin(np.array([[0.3]]), 4)[0] == np.inf


def test_planted_rows_are_what_they_claim():
    q, g, where = R.planted(3, 50, 24, 1, {2: [40, 7, 19]})
    assert q.dtype == g.dtype == np.float32 and q.shape == (3, 24) and g.shape == (50, 24)
    cos = R.cosine64(q, g)
    np.testing.assert_allclose(cos[2, where[2]], [0.95, 0.94, 0.93], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.sqrt((g[where[2]].astype(np.float64) ** 2).sum(1)), 3.0, rtol=1e-6)
    q2, g2, _ = R.planted(3, 50, 24, 1, {2: [40, 7, 19]})
    assert q2.tobytes() == q.tobytes() and g2.tobytes() == g.tobytes()
    with pytest.raises(AssertionError):
        R.planted(3, 50, 24, 1, {0: [4], 1: [4]})


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_planted_case_has_the_margin_and_reaches_its_path(lib, name):
    nq, ng, dim, _, spec, min_spans = R.CASES[name]
    q, g, where, cos_of = R.case(name)
    assert sorted(where) == sorted(spec)
    worst = np.inf
    for a, pos in where.items():
        row = cos_of[a][None]
        for k in (32, 5, 1):
            gap = float(R.margin(row, k)[0])
            worst = min(worst, gap)
            assert gap >= MARGIN, "query %d, k = %d: margin %.3g" % (a, k, gap)
            np.testing.assert_array_equal(R.rank64(row, k)[0, :min(k, pos.size)], pos[:k])
        ex = np.array([pos[0]])                                      # without its best row: the next ones, still apart
        assert float(R.margin(row, 32, ex)[0]) >= MARGIN
        np.testing.assert_array_equal(R.rank64(row, 32, ex)[0, :min(32, pos.size - 1)], pos[1:33])
        others = np.delete(cos_of[a], pos)
        print("%s, query %d: planted %.4f .. %.4f, best background row %.4f" % (name, a, cos_of[a][pos[0]], cos_of[a][pos[-1]],
                                                                                others.max() if others.size else np.nan))
    spans = spans_of_call(lib, nq, ng, dim)
    print("%s: %d x %d x %d, %d spans, smallest margin %.6f" % (name, nq, ng, dim, spans, worst))
    assert spans >= min_spans if min_spans > 1 else spans == 1
    rows = R.span_rows(ng, spans)
    assert rows[0][0] == 0 and rows[-1][1] == ng and all(rows[s][1] == rows[s + 1][0] for s in range(spans - 1))
    if min_spans > 1:                                                # every planted query has rows in at least two spans
        assert all(len({R.span_of(int(p), ng, spans) for p in pos}) >= 2 for a, pos in where.items() if a != 0 or name != "many_lists")


def test_the_large_gallery_is_cut_as_the_tests_assume(lib):
    ng, w = R.BIG_NG, R.BIG_SPAN_ROWS
    _, _, where, _ = R.case("many_lists")
    for nq in (4, 130):                                              # one and two row blocks: the same 130 spans
        assert spans_of_call(lib, nq, ng, 128) == R.BIG_SPANS >= 129
        assert spans_of_call(lib, nq, ng, 128, k=5) == R.BIG_SPANS
    assert spans_of_call(lib, 4, ng, 128, k=1) == R.BIG_SPANS
    rows = R.span_rows(ng, R.BIG_SPANS)
    assert rows[:2] == [(0, w), (w, 2 * w)] and rows[-1] == (129 * w, ng) and ng % R.TILE == 12
    span = lambda p: R.span_of(int(p), ng, R.BIG_SPANS)              # noqa: E731
    assert {span(p) for p in where[0]} == {77}                                       # one list saturates
    s1 = [span(p) for p in where[1]]
    assert len(set(s1)) == 40 and s1[:6] == [129, 0, 1, 128, 65, 64]                 # three lists of lane 0 and of lane 1
    assert {0, ng - 1} <= set(where[2].tolist()) and ng - 1 >= (ng // R.TILE) * R.TILE   # the last row is in the ragged tile
    assert sum(span(p) != span(p + 1) for p in where[2] if p + 1 < ng) == 19         # last rows of spans ...
    assert sum(p > 0 and span(p) != span(p - 1) for p in where[2]) == 19             # ... and first rows
    assert np.all(np.diff(where[3]) < 0) and len({span(p) for p in where[3]}) == 40 and span(where[3][0]) == 129
    for a in (127, 128, 129):
        assert len({span(p) for p in where[a]}) == 40
    # ties: 50 copies in 50 spans, the 32 lowest reaching into the second list of lanes 0 and 1
    t = [span(p) for p in R.TIE_ROWS]
    assert t == R.TIE_SPANS and len(set(t)) == 50 > 32 and np.all(np.diff(R.TIE_ROWS) > 0)
    assert t[30:32] == [64, 65] and {0, 1, 128, 129} <= set(t) and span(R.TIE_NAN_ROW) == 129 and R.TIE_NAN_ROW not in R.TIE_ROWS
    # chunks: borders inside spans; the short ones are one span (the convert path on a first call), the long ones many
    b = R.CHUNK_BOUNDS
    assert all(x % w not in (0, w - 1) for x in b[1:-1])
    counts = [spans_of_call(lib, 130, b[c + 1] - b[c], 128) for c in range(4)]
    assert counts[0] == counts[2] == 1 and min(counts[1], counts[3]) >= 40, counts
    cut = 30 * w + 500                                               # the two chunks of the ties between calls
    assert spans_of_call(lib, 4, cut, 128) >= 2 and spans_of_call(lib, 4, ng - cut, 128) >= 65
    assert 0 < int((R.TIE_ROWS[:32] < cut).sum()) < 32               # the 32 best copies come from both chunks


def test_one_span_where_one_span_is_meant(lib):
    for nq, ng, dim in ((3, 38, 16), (3, 30, 16), (3, 8, 16), (3, 5, 16), (3, 3, 16), (300, 40, 8), (300, 15, 8), (300, 25, 8)):
        assert spans_of_call(lib, nq, ng, dim) == 1
    assert lib.svk_cosine_topk_workspace_bytes(300, 0, 8, 32) == 0
    # the steps of the exhausted-list sequence keep the margin too (subsets of rows that are 0.01 apart)
    _, _, where, cos_of = R.case("exhausted")
    for seen in ((0, 3), (0, 8), (8, 38), (3, 38)):
        assert float(R.margin(cos_of[0][None, seen[0]:seen[1]], 32)[0]) >= MARGIN
