"""The search on normalised scores without a GPU: the binding of the entries of include/svk.h's section "top-k search on
normalised scores" against the plain search's, the returns that need no device, the reference of tests/search_norm_ref.py
against an independent brute-force statement of the total order, the staircase case's
claim (equal and adjacent float32 normalised values, the k-th place decided in the last bit) established from the reference
alone, and the span counts of the GPU shapes through svk_cosine_topk_norm_workspace_bytes."""
import ctypes
import os

import numpy as np
import pytest

import search_f64_ref as S
import search_norm_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from speaker_verification_amd import _lib as binding
    if not os.path.exists(binding.LIB_PATH):
        entry.build()
    return binding.load()


# ---- the entries in the binding ----------------------------------------------------------------------------------------
def test_the_binding_is_the_plain_search_plus_two_tables():
    """(tests/test_cabi.py walks the header, the table and the library for every entry; this pins what is these entries' own)"""
    from speaker_verification_amd import _lib as binding
    assert sorted(n for n in binding.SIGNATURES if n.startswith("svk_cosine_topk_norm")) == [
        "svk_cosine_topk_norm", "svk_cosine_topk_norm_workspace_bytes"]
    # the plain entry's parameters plus the two tables, in front of the workspace
    plain, norm = binding.SIGNATURES["svk_cosine_topk"][1], binding.SIGNATURES["svk_cosine_topk_norm"][1]
    assert list(norm) == list(plain[:10]) + [ctypes.c_void_p, ctypes.c_void_p] + list(plain[10:])


def test_refusals_need_no_device(lib):
    from speaker_verification_amd import _lib as binding
    assert lib.svk_cosine_topk_norm(None, None, 1, None, 1, 4, 1, 0, None, 0, None, None, None, 0, None, None) == binding.SVK_ERR_BAD_ARG
    for shape in ((-1, 5, 4, 1), (5, -1, 4, 1), (5, 5, 0, 1), (5, 5, 4097, 1), (5, 5, 4, 0), (5, 5, 4, 33)):
        assert lib.svk_cosine_topk_norm_workspace_bytes(*shape) == 0
    assert lib.svk_cosine_topk_norm_workspace_bytes(0, 5, 4, 1) == 0 == lib.svk_cosine_topk_norm_workspace_bytes(5, 0, 4, 1)


@pytest.mark.parametrize("shape,k,spans", (((5, 7, 128), 7, 1), ((130, 33, 130), 5, 1), ((130, 4200, 128), 32, 4),
                                           ((R.STAIR_NQ, R.STAIR_NG, R.STAIR_DIM), 5, 1)))
def test_the_gpu_shapes_have_the_span_counts_claimed(lib, shape, k, spans):
    nq, ng, dim = shape
    nbytes = lib.svk_cosine_topk_norm_workspace_bytes(nq, ng, dim, k)
    assert nbytes == lib.svk_cosine_topk_workspace_bytes(nq, ng, dim, k) > 0
    assert S.spans_from_workspace(nbytes, nq, ng, k) == spans
    tiles, row_blocks = (ng + 31) // 32, (nq + 127) // 128
    assert (tiles, row_blocks) == {(5, 7, 128): (1, 1), (130, 33, 130): (2, 2), (130, 4200, 128): (132, 2),
                                   (R.STAIR_NQ, R.STAIR_NG, R.STAIR_DIM): (7, 1)}[shape]


# ---- the reference -------------------------------------------------------------------------------------------------------
def _before(sa, ia, sb, ib):
    """The contract's order in float comparisons, nothing shared with R.order_key."""
    na, nb = sa != sa, sb != sb
    if na != nb:
        return na
    if not na and sa != sb:                  # -0.0 == +0.0 here
        return sa > sb
    return ia < ib


def _brute(values, k, exclude, index_base):
    nq, ng = values.shape
    scores = np.full((nq, k), -np.inf, dtype=np.float32)
    indices = np.full((nq, k), -1, dtype=np.int64)
    for r in range(nq):
        cols = [c for c in range(ng) if exclude is None or index_base + c != exclude[r]]
        for c in cols:          # a column's rank = the candidates in front of it
            rank = sum(_before(values[r, o], o, values[r, c], c) for o in cols if o != c)
            if rank < k:
                scores[r, rank], indices[r, rank] = values[r, c], index_base + c
    return scores, indices


@pytest.mark.parametrize("seed", range(4))
def test_reference_topk_equals_a_brute_force_sort(seed):
    rng = np.random.default_rng(seed)
    pool = np.array([np.nan, 0.0, -0.0, 1.5, 1.5, -2.0, np.inf, -np.inf, 1e-40, -1e-40, 3.25], dtype=np.float32)
    values = rng.choice(np.r_[pool, rng.standard_normal(6).astype(np.float32)], (6, 23)).astype(np.float32)
    values[0, :3] = (-0.0, 0.0, -0.0)
    base = (1 << 33) + 7
    exclude = base + rng.integers(-2, 25, 6)
    for k in (1, 5, 23, 30):
        for ex in (None, exclude):
            got, want = R.topk(values, k, ex, base), _brute(values, k, ex, base)
            assert np.array_equal(R.bits(got[0]), R.bits(want[0])) and np.array_equal(got[1], want[1])
    s, i = R.topk(values[:1], 23, None, 0)
    assert np.isnan(s[0, :int(np.isnan(values[0]).sum())]).all() and list(i[0]) != sorted(i[0])
    assert R.order_key(np.float32(-0.0)) == R.order_key(np.float32(0.0)) < R.order_key(np.float32(1e-45))


def test_reference_expression_is_the_written_order():
    raw = np.array([[0.25, -0.5, 0.75]], dtype=np.float32)
    qm, gm = np.array([[0.1, 0.3]]), np.array([[0.2, 0.7], [0.0, 0.0], [np.nan, 1.0]])
    both = R.normalise(raw, qm, gm)
    x = np.float64(raw[0, 0])
    assert both[0, 0] == np.float32(0.5 * ((x - 0.1) / 0.3 + (x - 0.2) / 0.7))
    assert both[0, 1] == -np.inf and np.isnan(both[0, 2])                  # sd = 0: IEEE, nothing clamped; a NaN moment
    assert R.normalise(raw, None, gm)[0, 0] == np.float32((x - 0.2) / 0.7)
    assert R.normalise(raw, qm, None)[0, 2] == np.float32((np.float64(raw[0, 2]) - 0.1) / 0.3)
    one = np.array([[0.0, 1.0]])
    assert np.array_equal(R.normalise(raw, one, np.repeat(one, 3, 0)), raw)   # mu = 0, sd = 1 in both: the raw bits


@pytest.mark.parametrize("mode", ("z", "s"))
def test_the_staircase_holds_equal_and_adjacent_values(mode):
    """Whatever float32 the device gives the copies' raw score within 8 units of the float64 cosine: neighbouring copies are
    equal or one float32 apart, both occur, the values climb with the index, and the k-th place of k = 5 and 32 is decided
    between values at most one unit apart."""
    q, g, qm, gm = R.staircase(mode)
    rows = R.stair_rows()
    assert len(rows) == R.STAIR_COPIES >= 64 and np.all(np.diff(rows) >= 2) and len({r // 32 for r in rows}) == 7
    assert all(np.array_equal(g[r], g[rows[0]]) for r in rows)
    cos = S.cosine64(q, g)
    assert 0.85 < cos[0, rows[0]] < 0.95 and np.abs(np.delete(cos[0], rows)).max() < 0.5
    centre = np.float32(cos[0, rows[0]])
    for off in range(-8, 9):
        s = np.array([int(R.bits(centre)[0]) + off], dtype=np.uint32).view(np.float32)
        raw = cos.astype(np.float32)
        raw[0, rows] = s
        v = R.normalise(raw, *R.tables(mode, qm, gm))
        steps = R.stair_steps(v[0])
        assert set(steps) == {0, 1}, (off, sorted(set(steps)))
        assert np.all(np.diff(v[0, rows]) >= 0) and v[0, rows].min() > np.delete(v[0], rows).max() + 0.5
        for k in (5, 32):
            sc, ix = R.topk(v[:1], k + 1)
            assert set(ix[0]) <= set(rows) and R.ulps_apart(sc[0, k - 1], sc[0, k]) <= 1
            plateau = ix[0][R.bits(sc[0]) == R.bits(sc[0, 0])]
            assert list(plateau) == sorted(plateau)                     # inside the best plateau the lower index first
