"""svk_cosine_topk's selection and merge, path by path, held to the float64 RANKING (not only to "no better row left out"):
more than 64 partial lists (a merge lane owns several), exact ties and NaN across spans and across calls, exhausted lists,
the grid-stride trips of the three phase-2 kernels, several row blocks x several spans, streamed fragments and 4-byte loads
together with the merge, `exclude` and a large `index_base` on a split gallery.

The inputs are those of tests/search_f64_ref.py; tests/test_search_host.py has established on the host, from the reference
alone, that every planted query's best k + 1 float64 scores are >= 4 COSINE_TOL apart and that every case is cut into the
spans it claims.  Under that condition a kernel that meets the score bar must return `rank64`, index for index.  In every
planted test: indices == rank64 for the planted queries, every score within COSINE_TOL of the float64 cosine of its index,
the other queries through check_lists (a) - (d) of tests/test_cosine_topk.py.  Everything else is compared as bytes.

On the MI355X: worst |score - float64| per planted case 4.1e-7 (many_lists, 130 spans), 4.1e-7 (streamed, 4 spans), 3.4e-7
(dim130, 4 spans), 3.3e-7 (offset, 4 spans), 1.5e-7 (exhausted, 1 span) against COSINE_TOL = 1e-5 (printed per test).

What the suite cannot see: the merge's fill of the tail when every list is exhausted.  That branch is reached only with the
accumulate flag (a split call has more than 2 048 candidates), where the slots it fills already hold -inf / -1 from the old
list, which the contract requires; test_exhausted_lists runs it and checks the tail, but a merge without the fill gives the
same bytes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scoring_f64_ref as SR                                                   # noqa: E402  (tests/ is on sys.path)
import search_f64_ref as R                                                     # noqa: E402
from test_cosine_topk import check_lists, eng, run, same_bytes                 # noqa: E402,F401  (eng: the module-scoped fixture)

TOL = SR.COSINE_TOL
NEG_INF_BITS = np.float32(-np.inf).view(np.int32)
_device, _others, _whole = {}, {}, {}


def device(eng, name):
    """(queries, gallery) of a case on the device, uploaded once."""
    if name not in _device:
        q, g = R.case(name)[:2]
        _device[name] = (eng.to_device(q), eng.to_device(g))
    return _device[name]


def others(name):
    """(the queries without planted rows, their float64 cosines): once per case, read-only."""
    if name not in _others:
        q, g, where, _ = R.case(name)
        rows = np.setdiff1d(np.arange(q.shape[0]), sorted(where))
        ref = R.cosine64(q[rows], g)
        ref.setflags(write=False)
        _others[name] = (rows, ref)
    return _others[name]


def whole(eng, name, k=32):
    """One call over the whole gallery with every query of the case: computed once, the yardstick of the byte comparisons."""
    if (name, k) not in _whole:
        _whole[name, k] = run(eng, *device(eng, name), k)
    return _whole[name, k]


def check_planted(name, scores, indices, k, base=0, exclude=None):
    """indices == rank64 and |score - float64| <= COSINE_TOL for the planted queries among the rows given; the worst error."""
    _, _, where, cos_of = R.case(name)
    worst = 0.0
    assert scores.dtype == np.float32 and indices.dtype == np.int64 and scores.shape == indices.shape and scores.shape[1] == k
    for a in sorted(where):
        if a >= scores.shape[0]:
            continue
        want = R.rank64(cos_of[a][None], k, None if exclude is None else np.array([exclude[a] - base]))[0]
        np.testing.assert_array_equal(np.where(indices[a] >= 0, indices[a] - base, -1), want, err_msg="query %d" % a)
        valid = want >= 0
        assert np.all(scores[a][~valid].view(np.int32) == NEG_INF_BITS)
        err = np.abs(scores[a][valid].astype(np.float64) - cos_of[a][want[valid]])
        assert err.max() <= TOL, "query %d: score off by %.3g" % (a, err.max())
        worst = max(worst, float(err.max()))
    return worst


def check_case(name, scores, indices, k):
    worst = check_planted(name, scores, indices, k)
    rows, ref = others(name)
    if rows.size:
        worst = max(worst, check_lists(scores[rows], indices[rows], ref, k))
    print("%s: worst |score - float64| = %.3g at k = %d (bar %.0e)" % (name, worst, k, TOL))
    return worst


def accumulate(eng, dq, dg, pieces, k, base=0, exclude=None):
    into = None
    for lo, hi in pieces:
        into = eng.cosine_topk(dq, dg[lo:hi], k, index_base=base + lo, exclude=exclude, into=into)
    return into[0].cpu().numpy(), into[1].cpu().numpy()


# ---- more than 64 lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (32, 5, 1))
def test_many_lists(eng, k):
    """4 x 133 100 x 128: 130 spans, one row block.  Query 0: 40 rows in one span; query 1: the three lists of a lane; query 2:
    both sides of span borders, row 0 and the last row; query 3: the best row arrives last."""
    dq, dg = device(eng, "many_lists")
    scores, indices = run(eng, dq[:4], dg, k)
    worst = check_planted("many_lists", scores, indices, k)
    print("many_lists, 4 queries: worst |score - float64| = %.3g at k = %d (bar %.0e)" % (worst, k, TOL))
    s32, i32 = whole(eng, "many_lists")                             # neither the batch nor k enters a list
    assert scores.tobytes() == s32[:4, :k].tobytes() and indices.tobytes() == i32[:4, :k].tobytes()


def test_two_row_blocks_times_many_spans(eng):
    """130 x 133 100 x 128: queries 128 and 129 are alone in the ragged second row block of every one of the 130 spans."""
    scores, indices = whole(eng, "many_lists")
    check_case("many_lists", scores, indices, 32)


def test_streamed_fragments_with_a_merge(eng):
    """130 x 4 200 x 200: dim > 128 streams the query fragments, the second K block is ragged, 4 spans x 2 row blocks."""
    scores, indices = whole(eng, "streamed")
    check_case("streamed", scores, indices, 32)
    for k in (5, 1):
        s, i = run(eng, *device(eng, "streamed"), k)
        assert s.tobytes() == scores[:, :k].tobytes() and i.tobytes() == indices[:, :k].tobytes()


def test_four_byte_loads_with_a_merge(eng):
    """5 x 4 200 x 130: dim % 4 != 0."""
    scores, indices = whole(eng, "dim130")
    check_case("dim130", scores, indices, 32)


def test_offset_pointers_with_a_merge(eng):
    """4 x 4 200 x 128 with both matrices 4 bytes off a 16-byte boundary: the bytes of the aligned call."""
    dq, dg = device(eng, "offset")
    aligned = whole(eng, "offset")
    check_case("offset", aligned[0], aligned[1], 32)
    fq = torch.empty(dq.numel() + 1, dtype=torch.float32, device=eng.device)
    fg = torch.empty(dg.numel() + 1, dtype=torch.float32, device=eng.device)
    oq, og = fq[1:].view(*dq.shape), fg[1:].view(*dg.shape)
    oq.copy_(dq)
    og.copy_(dg)
    assert dq.data_ptr() % 16 == 0 and dg.data_ptr() % 16 == 0 and oq.data_ptr() % 16 == 4 and og.data_ptr() % 16 == 4
    assert same_bytes(run(eng, oq, og, 32), aligned)
    assert same_bytes(run(eng, dq, og, 32), aligned)


# ---- exact ties and NaN ---------------------------------------------------------------------------------------------------
def test_ties_and_nan_across_spans(eng):
    q, g, g_nan = R.tie_case()
    ref = R.cosine64(q, g)
    assert np.all(R.margin(ref[1:], 32) >= 4 * TOL)                  # queries 1 - 3 keep their planted rows apart
    dq = eng.to_device(q)
    scores, indices = run(eng, dq, eng.to_device(g), 32)
    np.testing.assert_array_equal(indices[0], R.TIE_ROWS[:32])      # the 32 lowest of the 50 copies, ascending
    assert np.all(scores[0].view(np.int32) == scores[0].view(np.int32)[0]) and abs(float(scores[0, 0]) - 1.0) <= TOL
    np.testing.assert_array_equal(indices[1:], R.rank64(ref[1:], 32))
    assert np.abs(scores[1:].astype(np.float64) - np.take_along_axis(ref[1:], indices[1:], 1)).max() <= TOL
    dg_nan = eng.to_device(g_nan)
    scores_n, indices_n = run(eng, dq, dg_nan, 32)
    assert np.all(indices_n[:, 0] == R.TIE_NAN_ROW) and np.all(np.isnan(scores_n[:, 0]))      # NaN ranks above every number
    np.testing.assert_array_equal(indices_n[:, 1:], indices[:, :31])                          # the rest shift by one
    assert scores_n[:, 1:].tobytes() == np.ascontiguousarray(scores[:, :31]).tobytes()
    for k in (1, 5):
        s, i = run(eng, dq, dg_nan, k)
        assert s.tobytes() == scores_n[:, :k].tobytes() and i.tobytes() == indices_n[:, :k].tobytes()


def test_ties_between_calls(eng):
    """The 50 copies in two chunks, cut inside span 30, in both orders: an old and a new list meet with equal scores."""
    q, g, g_nan = R.tie_case()
    dq = eng.to_device(q)
    base = (1 << 33) + 5
    cut = 30 * R.BIG_SPAN_ROWS + 500
    pieces = [(0, cut), (cut, R.BIG_NG)]
    for gallery in (g, g_nan):
        dg = eng.to_device(gallery)
        one = run(eng, dq, dg, 32, index_base=base)
        first = 1 if gallery is g_nan else 0
        np.testing.assert_array_equal(one[1][0, first:], base + R.TIE_ROWS[:32 - first])
        assert one[1].min() > 1 << 33
        for order in (pieces, pieces[::-1]):
            assert same_bytes(accumulate(eng, dq, dg, order, 32, base=base), one)
        del dg


# ---- exhausted lists ------------------------------------------------------------------------------------------------------
def _check_partial(scores, indices, seen, cos_row, ref, exclude=None):
    """After some chunks: query 0 holds rank64 of the rows seen so far, every tail is exactly -inf / -1, every score is within
    the bar of the float64 cosine of its index."""
    cols = np.array(sorted(seen), dtype=np.int64)
    k = indices.shape[1]
    for r in range(indices.shape[0]):
        cand = cols if exclude is None else cols[cols != exclude[r]]
        n = min(k, cand.size)
        assert np.all(indices[r, n:] == -1) and np.all(scores[r, n:].view(np.int32) == NEG_INF_BITS), "query %d: the tail" % r
        assert set(indices[r, :n].tolist()) <= set(cand.tolist()) and np.unique(indices[r, :n]).size == n
        assert np.abs(scores[r, :n].astype(np.float64) - ref[r, indices[r, :n]]).max(initial=0.0) <= TOL
        if r == 0:
            local = R.rank64(cos_row[None, cand], k)[0]
            np.testing.assert_array_equal(indices[0], np.where(local >= 0, cand[np.maximum(local, 0)], -1))


def test_exhausted_lists(eng):
    """k = 32 over chunks of 3, 0, 5 and 30 rows: the merge meets old lists with empty slots and runs out of candidates."""
    q, g, where, cos_of = R.case("exhausted")
    dq, dg = device(eng, "exhausted")
    ref = R.cosine64(q, g)
    pieces = [(0, 3), (3, 3), (3, 8), (8, 38)]
    one = whole(eng, "exhausted")
    print("exhausted: worst |score - float64| = %.3g (bar %.0e)" % (check_planted("exhausted", one[0], one[1], 32), TOL))
    for order in (pieces, pieces[::-1]):
        into, seen = None, set()
        for lo, hi in order:
            into = eng.cosine_topk(dq, dg[lo:hi], 32, index_base=lo, into=into)
            seen.update(range(lo, hi))
            _check_partial(into[0].cpu().numpy(), into[1].cpu().numpy(), seen, cos_of[0], ref)
        assert same_bytes((into[0].cpu().numpy(), into[1].cpu().numpy()), one)
    # the same over the first 8 rows with one of them excluded: 7 candidates for queries 0 and 1, 8 for query 2
    exclude = np.array([int(np.argmax(cos_of[0][:8])), 2, 100], dtype=np.int64)
    one8 = run(eng, dq, dg[:8], 32, exclude=exclude)
    _check_partial(one8[0], one8[1], set(range(8)), cos_of[0], ref, exclude)
    assert (one8[1] >= 0).sum(1).tolist() == [7, 7, 8]
    dex = eng.to_device(exclude)
    for order in (pieces[:3], pieces[2::-1]):
        into, seen = None, set()
        for lo, hi in order:
            into = eng.cosine_topk(dq, dg[lo:hi], 32, index_base=lo, exclude=dex, into=into)
            seen.update(range(lo, hi))
            _check_partial(into[0].cpu().numpy(), into[1].cpu().numpy(), seen, cos_of[0], ref, exclude)
        assert same_bytes((into[0].cpu().numpy(), into[1].cpu().numpy()), one8)


# ---- chunks, exclude and index_base on the split gallery -------------------------------------------------------------------
def test_chunks_of_the_split_gallery(eng):
    """133 100 rows cut inside spans into 1 500 (one span: the convert path when it comes first), 48 623, 1 577 and 81 400."""
    dq, dg = device(eng, "many_lists")
    b = R.CHUNK_BOUNDS
    pieces = [(b[c], b[c + 1]) for c in range(len(b) - 1)]
    one = whole(eng, "many_lists")
    for order in (pieces, pieces[::-1]):
        assert same_bytes(accumulate(eng, dq, dg, order, 32), one)


def test_exclude_and_index_base_on_the_split_gallery(eng):
    dq, dg = device(eng, "many_lists")
    _, _, where, _ = R.case("many_lists")
    nq, ng, base = 130, R.BIG_NG, (1 << 33) + 7
    plain = whole(eng, "many_lists")
    shifted = run(eng, dq, dg, 32, index_base=base)
    assert shifted[0].tobytes() == plain[0].tobytes() and np.array_equal(shifted[1], plain[1] + base)
    exclude = base + ng + np.arange(nq, dtype=np.int64)               # outside the call's range ...
    for a, pos in where.items():
        exclude[a] = base + pos[0]                                    # ... but for the planted queries: their best row
    scores, indices = run(eng, dq, dg, 32, index_base=base, exclude=exclude)
    worst = check_planted("many_lists", scores, indices, 32, base=base, exclude=exclude)
    print("many_lists without the best row: worst |score - float64| = %.3g (bar %.0e)" % (worst, TOL))
    for a, pos in where.items():                                      # the list moved up by one; its scores kept their bits
        assert indices[a, 0] == base + pos[1] and scores[a, :31].tobytes() == plain[0][a, 1:].tobytes()
    rest = np.setdiff1d(np.arange(nq), sorted(where))
    assert scores[rest].tobytes() == shifted[0][rest].tobytes() and indices[rest].tobytes() == shifted[1][rest].tobytes()
    outside = exclude.copy()
    for n, (a, pos) in enumerate(where.items()):                      # the LOCAL index of the best row, base - 1, one past the end
        outside[a] = (pos[0], base - 1, base + ng)[n % 3]
    assert same_bytes(run(eng, dq, dg, 32, index_base=base, exclude=outside), shifted)
    # chunked with the exclusion: the excluded row is global, whichever chunk holds it
    b = R.CHUNK_BOUNDS
    pieces = [(b[c], b[c + 1]) for c in range(len(b) - 1)]
    dex = eng.to_device(exclude)
    assert same_bytes(accumulate(eng, dq, dg, pieces[::-1], 32, base=base, exclude=dex), (scores, indices))


# ---- the second trip of the grid-stride loops --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(eng):
    """300 queries x 40 gallery rows x 8 and their lists from one 300-row call, held to float64 once."""
    rng = np.random.default_rng(21)
    q = rng.standard_normal((300, 8)).astype(np.float32)
    g = rng.standard_normal((40, 8)).astype(np.float32)
    scores, indices = run(eng, q, g, 32)
    check_lists(scores, indices, R.cosine64(q, g), 32)
    return q, eng.to_device(g), scores, indices


def _repeat(eng, small, n):
    q, dg, scores, indices = small
    rows = np.arange(n) % 300
    return eng.to_device(q[rows]), dg, np.ascontiguousarray(scores[rows]), np.ascontiguousarray(indices[rows])


def test_grid_stride_merge(eng, small):
    """n_query = 32 num_cu + 8 with into=: the merge's workgroups 0 - 7 take a second query each."""
    grid = 32 * eng.num_cu
    dq, dg, want_s, want_i = _repeat(eng, small, grid + 8)
    got_s, got_i = accumulate(eng, dq, dg, [(0, 15), (15, 40)], 32)
    assert got_s[grid:].tobytes() == want_s[grid:].tobytes() and got_i[grid:].tobytes() == want_i[grid:].tobytes()   # the second trip
    assert got_s.tobytes() == want_s.tobytes() and got_i.tobytes() == want_i.tobytes()
    got_s, got_i = accumulate(eng, dq, dg, [(15, 40), (0, 15)], 32)
    assert got_s.tobytes() == want_s.tobytes() and got_i.tobytes() == want_i.tobytes()


def test_grid_stride_convert_and_fill(eng, small):
    """n_query 32 > 256 * 8 num_cu: the flat kernels' second trip, in the convert kernel and (n_gallery = 0) in the fill."""
    first = 256 * 8 * eng.num_cu // 32                                # the first query of the second trip
    n = first + 8
    assert n * 32 > 256 * 8 * eng.num_cu
    dq, dg, want_s, want_i = _repeat(eng, small, n)
    got_s, got_i = run(eng, dq, dg, 32)
    assert got_s[first:].tobytes() == want_s[first:].tobytes() and got_i[first:].tobytes() == want_i[first:].tobytes()
    assert got_s.tobytes() == want_s.tobytes() and got_i.tobytes() == want_i.tobytes()
    empty_s, empty_i = run(eng, dq, dg[:0], 32)
    assert empty_s.shape == (n, 32) and np.all(empty_i[first:] == -1) and np.all(empty_s[first:].view(np.int32) == NEG_INF_BITS)
    assert np.all(empty_i == -1) and np.all(empty_s.view(np.int32) == NEG_INF_BITS)
