"""svk_cosine_topk_norm (include/svk.h, "top-k search on normalised scores") on the MI355X against tests/search_norm_ref.py, as bytes: the reference takes
the raw scores from svk_cosine_topk's own lists, svk_score_norm's expression in NumPy float64 and the total order in pure
Python, so no comparison here has a tolerance.  Shapes: one ragged tile on the hoisted instance; the streamed instance with
4-byte loads, two row blocks and a ragged second tile; four spans and the merge; chunks accumulated in both orders with an
index_base above 2^33 and an exclusion; column deviations over six decades; the staircase (equal and adjacent float32 values,
tests/test_search_norm_host.py establishes that); NaN moments, a zero and a NaN deviation; the identity tables, where the
result is svk_cosine_topk's; and the refusals."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import search_norm_ref as R       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

_raw = {}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def raw_of(eng, name, q, g):
    """The raw matrix of a named problem: computed once, shared by the modes, read-only."""
    if name not in _raw:
        _raw[name] = R.raw_matrix(eng, q, g)
        _raw[name].setflags(write=False)
    return _raw[name]


def same(got, want, what):
    """Indices equal, scores the same bits.  A NaN equals a NaN here: the sign and payload of a NaN that an operation MAKES
    (0 / 0, inf - inf) are the processor's choice, and the reference runs on another processor; `same_as_the_matrix` compares
    those bits too, device against device."""
    sc, ix = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert sc.dtype == np.float32 and ix.dtype == np.int64 and sc.shape == want[0].shape == ix.shape
    differ = (R.bits(sc) != R.bits(want[0])) & ~(np.isnan(sc) & np.isnan(want[0]))
    bad = np.flatnonzero(differ.reshape(-1) | (ix != want[1]).reshape(-1))
    assert bad.size == 0, "%s: %d of %d entries differ, the first at flat %d: (%r, %d) against (%r, %d)" % (
        what, bad.size, sc.size, bad[0], sc.reshape(-1)[bad[0]], ix.reshape(-1)[bad[0]], want[0].reshape(-1)[bad[0]],
        want[1].reshape(-1)[bad[0]])


def same_as_the_matrix(eng, got, raw, mode, qm, gm, what, index_base=0):
    """Every returned score has the bits svk_score_norm writes at that entry of the raw matrix, NaNs included."""
    qt, gt = R.tables(mode, qm, gm)
    matrix = eng.score_norm(torch.from_numpy(np.array(raw)), qt, gt).cpu().numpy()
    sc, ix = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (ix >= index_base).all()
    at = matrix[np.arange(sc.shape[0])[:, None], ix - index_base]
    assert np.array_equal(R.bits(sc), R.bits(at)), what + ": not svk_score_norm's bits"


def run(eng, q, g, k, mode, qm, gm, **kw):
    qt, gt = R.tables(mode, qm, gm)
    return eng.cosine_topk_norm(q, g, k, query_moments=qt, gallery_moments=gt, **kw)


def want_of(raw, k, mode, qm, gm, **kw):
    return R.topk(R.normalise(raw, *R.tables(mode, qm, gm)), k, **kw)


SHAPES = {"hoisted-ragged": (5, 7, 128, (1, 3, 7)), "streamed-two-row-blocks": (130, 33, 130, (5,)),
          "four-spans": (130, 4200, 128, (32,))}


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_reference(eng, name, mode):
    nq, ng, dim, ks = SHAPES[name]
    q, g, qm, gm = R.random_problem(nq, ng, dim, seed=nq + ng)
    raw = raw_of(eng, name, q, g)
    for k in ks:
        got = run(eng, q, g, k, mode, qm, gm)
        same(got, want_of(raw, k, mode, qm, gm), "%s k %d mode %s" % (name, k, mode))
        same_as_the_matrix(eng, got, raw, mode, qm, gm, "%s k %d mode %s" % (name, k, mode))
    if mode != "t" and ng > ks[-1]:      # the ranking is not the raw score's: the normalisation sits inside the selection
        assert not torch.equal(eng.cosine_topk(q, g, ks[-1])[1], got[1])


@pytest.mark.parametrize("mode", R.MODES)
def test_chunks_accumulate_to_one_call(eng, mode):
    """Chunks of 3, 0, 5 and 30 rows in both orders, index_base above 2^33, one excluded global index per query: the bytes of
    one call.  The gallery table travels with its chunk; the exclusion and the base are global."""
    nq, ng, dim, k = 5, 38, 128, 6
    q, g, qm, gm = R.random_problem(nq, ng, dim, seed=77)
    raw = raw_of(eng, "chunks", q, g)
    base = (1 << 33) + 12345
    exclude = base + np.array([0, 2, 3, 37, 99], dtype=np.int64)          # the last one names no row
    want = want_of(raw, k, mode, qm, gm, exclude=exclude, index_base=base)
    assert not (want[1] == exclude[:, None]).any()
    same(run(eng, q, g, k, mode, qm, gm, exclude=exclude, index_base=base), want, "one call")
    bounds = [(0, 3), (3, 3), (3, 8), (8, 38)]
    for order in (bounds, bounds[::-1]):
        into = None
        for lo, hi in order:
            into = run(eng, q, g[lo:hi], k, mode, qm, gm[lo:hi], exclude=exclude, index_base=base + lo, into=into)
        same(into, want, "chunks %s" % (order,))


@pytest.mark.parametrize("mode", ("z", "s"))
def test_wide_column_deviations_rank_low_raw_scores_first(eng, mode):
    nq, ng, dim, k = 9, 300, 64, 5
    q, g, qm, gm = R.random_problem(nq, ng, dim, seed=5, sd_decades=3.0)
    assert gm[:, 1].min() < 1e-2 and gm[:, 1].max() > 1e2
    raw = raw_of(eng, "decades", q, g)
    want = want_of(raw, k, mode, qm, gm)
    same(run(eng, q, g, k, mode, qm, gm), want, "six decades, mode " + mode)
    best_raw = np.sort(raw, axis=1)[:, -k]
    winners = raw[np.arange(nq)[:, None], want[1]]
    outside = (winners < best_raw[:, None]).mean()                  # winners that the raw top-k does not hold
    assert outside > (0.5 if mode == "z" else 0.0), outside


@pytest.mark.parametrize("k", (5, 32))
@pytest.mark.parametrize("mode", ("z", "s"))
def test_staircase_ties_and_last_bit(eng, mode, k):
    q, g, qm, gm = R.staircase(mode)
    raw = raw_of(eng, "staircase", q, g)
    rows = R.stair_rows()
    assert np.unique(R.bits(raw[:, rows]), axis=1).shape[1] == 1    # the copies share their raw bits, query by query
    values = R.normalise(raw, *R.tables(mode, qm, gm))
    assert set(R.stair_steps(values[0])) == {0, 1}
    want = R.topk(values, k)
    assert R.ulps_apart(want[0][0, k - 1], R.topk(values, k + 1)[0][0, k]) <= 1
    same(run(eng, q, g, k, mode, qm, gm), want, "staircase mode %s k %d" % (mode, k))


@pytest.mark.parametrize("mode", R.MODES)
def test_nan_moments_and_degenerate_deviations(eng, mode):
    nq, ng, dim, k = 6, 40, 128, 8
    q, g, qm, gm = R.random_problem(nq, ng, dim, seed=9)
    qm[1] = np.nan                       # a query row without a finite cohort score: every score NaN, ranked by index
    qm[2, 1] = 0.0
    gm[3, 1] = 0.0                       # +-inf (or NaN at a zero difference): IEEE, nothing clamped
    gm[5, 1] = np.nan                    # NaN: above every number
    gm[7, 1] = -2.0                      # a negative deviation turns the sign
    gm[34, 0] = np.inf
    raw = raw_of(eng, "degenerate", q, g)
    want = want_of(raw, k, mode, qm, gm)
    got = run(eng, q, g, k, mode, qm, gm)
    same(got, want, "degenerate moments, mode " + mode)
    same_as_the_matrix(eng, got, raw, mode, qm, gm, "degenerate moments, mode " + mode)
    if mode != "z":
        assert np.isnan(want[0][1]).all() and list(want[1][1]) == list(range(k))
    if mode != "t":
        assert np.isnan(want[0][0, 0]) and want[1][0, 0] == 5


def test_identity_tables_give_the_plain_search(eng):
    """A cohort of +1 and -1 gives every row mean 0 and deviation 1 exactly; the S-norm of s is then 0.5 (s + s) = s."""
    nq, ng, dim, k = 130, 333, 128, 7
    q, g, _, _ = R.random_problem(nq, ng, dim, seed=3)
    pair = torch.tensor([[1.0, -1.0, -3.0]], dtype=torch.float32)        # top_k = 2 keeps +1 and -1
    qm, gm = eng.cohort_moments(pair.repeat(nq, 1), top_k=2), eng.cohort_moments(pair.repeat(ng, 1), top_k=2)
    assert np.array_equal(qm.cpu().numpy(), np.tile([0.0, 1.0], (nq, 1))) and np.array_equal(gm.cpu().numpy(), np.tile([0.0, 1.0], (ng, 1)))
    plain = eng.cosine_topk(q, g, k)
    for mode in R.MODES:
        got = run(eng, q, g, k, mode, qm, gm)
        assert torch.equal(got[1], plain[1]) and np.array_equal(R.bits(got[0].cpu().numpy()), R.bits(plain[0].cpu().numpy())), mode


def test_refusals(eng):
    from speaker_verification_amd import _lib as binding
    lib, dev = eng.lib, eng.device
    nq, ng, dim, k = 4, 9, 16, 3
    q, g = torch.randn(nq, dim, device=dev), torch.randn(ng, dim, device=dev)
    qm, gm = torch.ones(nq + 1, 2, dtype=torch.float64, device=dev), torch.ones(ng, 2, dtype=torch.float64, device=dev)
    sc, ix = torch.empty(nq, k, device=dev), torch.empty(nq, k, dtype=torch.int64, device=dev)
    nbytes = lib.svk_cosine_topk_norm_workspace_bytes(nq, ng, dim, k)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731

    def call(**kw):
        a = dict(q=p(q), nq=nq, g=p(g), ng=ng, dim=dim, k=k, base=0, ex=None, flags=0, qm=p(qm), gm=p(gm), work=p(work),
                 nbytes=nbytes, sc=p(sc), ix=p(ix))
        a.update(kw)
        eng._stream()
        return lib.svk_cosine_topk_norm(eng.ctx, a["q"], a["nq"], a["g"], a["ng"], a["dim"], a["k"], a["base"], a["ex"],
                                        a["flags"], a["qm"], a["gm"], a["work"], a["nbytes"], a["sc"], a["ix"])
    assert call() == binding.SVK_OK
    assert call(qm=None) == binding.SVK_OK and call(gm=None) == binding.SVK_OK
    bad = binding.SVK_ERR_BAD_ARG
    assert call(qm=None, gm=None) == bad and b"moment table" in lib.svk_last_error(eng.ctx)
    assert call(qm=C.c_void_p(qm.data_ptr() + 4)) == bad and b"8-byte" in lib.svk_last_error(eng.ctx)
    assert call(gm=C.c_void_p(gm.data_ptr() + 4)) == bad
    assert call(k=0) == bad and call(k=33) == bad and call(dim=0) == bad and call(nq=-1) == bad and call(ng=-1) == bad
    assert call(flags=2) == bad and call(base=-1) == bad and call(nbytes=nbytes - 1) == bad
    assert call(work=None) == bad and call(sc=None) == bad and call(q=None) == bad
    assert call(work=C.c_void_p(work.data_ptr() + 4)) == bad
    # both tables NULL is refused whatever the sizes; an empty query is no work for a well-formed call
    assert call(qm=None, gm=None, nq=0) == bad and call(nq=0) == binding.SVK_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="query_moments"):
        eng.cosine_topk_norm(q, g, k, query_moments=gm)
    with pytest.raises(binding.SvkError):
        eng.cosine_topk_norm(q, g, k)


def test_empty_gallery_and_accumulate(eng):
    q = torch.randn(3, 16)
    none, nothing = torch.zeros((0, 16)), torch.zeros((0, 2), dtype=torch.float64)
    qm = torch.ones(3, 2, dtype=torch.float64)
    sc, ix = eng.cosine_topk_norm(q, none, 2, query_moments=qm, gallery_moments=nothing)
    assert bool((sc == -np.inf).all()) and bool((ix == -1).all())
    g = torch.randn(5, 16)
    first = eng.cosine_topk_norm(q, g, 2, query_moments=qm)
    kept = (first[0].clone(), first[1].clone())
    again = eng.cosine_topk_norm(q, none, 2, query_moments=qm, gallery_moments=nothing, index_base=5, into=first)
    assert torch.equal(again[0], kept[0]) and torch.equal(again[1], kept[1])
