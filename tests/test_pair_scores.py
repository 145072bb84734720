"""svk_pair_scores against float64 NumPy: every trial within 1 float32 ulp of the reference score (exactly 0 where the
reference is 0), on both metrics, both load paths (16-byte and 4-byte) and past one sweep of the grid-stride loop."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_A, N_B = 61, 47                                   # rows of the two matrices: odd, and different
DIMS = (1, 3, 4, 127, 128, 132, 4096)
# the launch is min(ceil(n_pairs / 16), 8 * CUs) workgroups of 16 trials: 8 * 256 * 16 = 32 768 trials per sweep on the MI355X,
# so 70 001 trials take three sweeps, the last one ragged
N_PAIRS = (0, 1, 5, 257, 70_001)
METRICS = ("cosine", "l2")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


_cache = {}


def matrices(dim):
    """(a, b) float32 with a zero row each, and the float64 reference of every (row of a, row of b) pair per metric --
    computed once per dim, shared by the tests, never written to."""
    if dim not in _cache:
        rng = np.random.default_rng(100 + dim)
        a = rng.standard_normal((N_A, dim)).astype(np.float32)
        b = (rng.standard_normal((N_B, dim)) * 3 + 0.5).astype(np.float32)
        a[7] = 0
        b[5] = 0
        b[9] = a[9]                                  # an equal pair of rows: cosine 1, distance 0
        x, y = a.astype(np.float64), b.astype(np.float64)
        na, nb = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
        na[na == 0] = 1.0
        nb[nb == 0] = 1.0
        cos = np.stack([(x[i] * y).sum(1) for i in range(N_A)]) / (na[:, None] * nb[None, :])
        l2 = -np.stack([np.sqrt(((x[i] - y) ** 2).sum(1)) for i in range(N_A)])
        for m in (a, b, cos, l2):
            m.setflags(write=False)
        _cache[dim] = (a, b, {"cosine": cos, "l2": l2})
    return _cache[dim]


def assert_within_one_ulp(got, want):
    """|got - want| <= the float32 spacing at |want|; exactly 0 where want is 0."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    zero = want == 0
    assert not np.any(got[zero] != 0)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err[~zero] / ulp[~zero]).max()) if np.any(~zero) else 0.0
    print("worst error: %.3f ulp over %d trials" % (worst, got.size))
    assert worst <= 1.0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", DIMS)
def test_against_float64(eng, dim, metric):
    a, b, ref = matrices(dim)
    da, db = eng.to_device(a), eng.to_device(b)
    rng = np.random.default_rng(dim)
    for n_pairs in N_PAIRS:
        ia = rng.integers(0, N_A, n_pairs)                       # repeated indices from 257 trials on (61 x 47 pairs)
        ib = rng.integers(0, N_B, n_pairs)
        if n_pairs >= 5:
            ia[:3], ib[:3] = (7, 9, 7), (5, 9, 0)                 # zero against zero, equal rows, zero against non-zero
        bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
        got = eng.pair_scores(da, db, ia, ib, metric=metric, bad_count=bad).cpu().numpy()
        assert got.shape == (n_pairs,) and int(bad.item()) == 0
        assert_within_one_ulp(got, ref[metric][ia, ib])
        if n_pairs >= 5:
            if metric == "cosine":
                assert got[0] == 0 and got[2] == 0 and got[1] == np.float32(1.0)      # a zero row gives cosine 0
            else:
                assert got[0] == 0 and got[1] == 0


@pytest.mark.parametrize("dim", DIMS)
def test_same_matrix_same_index(eng, dim):
    """idx_a == idx_b with d_a == d_b: both sums of squares and the dot product are the same additions."""
    a, _, _ = matrices(dim)
    da = eng.to_device(a)
    idx = np.arange(N_A)
    cos = eng.pair_scores(da, da, idx, idx).cpu().numpy()
    want = np.ones(N_A, np.float32)
    want[7] = 0                                                   # the zero row
    np.testing.assert_array_equal(cos, want)
    l2 = eng.pair_scores(da, da, idx, idx, metric="l2").cpu().numpy()
    assert not l2.any()                                           # -0.0 or 0.0


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", (4, 128, 132))
def test_scalar_loads_give_the_same_bits(eng, dim, metric):
    """Matrices 4 bytes off a 16-byte boundary take the 4-byte loads (dim % 4 == 0 would otherwise take 16-byte ones)."""
    a, b, _ = matrices(dim)
    da, db = eng.to_device(a), eng.to_device(b)
    assert da.data_ptr() % 16 == 0 and db.data_ptr() % 16 == 0
    fa = torch.empty(a.size + 1, dtype=torch.float32, device=eng.device)
    fb = torch.empty(b.size + 1, dtype=torch.float32, device=eng.device)
    oa, ob = fa[1:].view(N_A, dim), fb[1:].view(N_B, dim)
    oa.copy_(da)
    ob.copy_(db)
    assert oa.data_ptr() % 16 == 4 and ob.data_ptr() % 16 == 4 and oa.is_contiguous()
    rng = np.random.default_rng(5)
    ia, ib = rng.integers(0, N_A, 999), rng.integers(0, N_B, 999)
    aligned = eng.pair_scores(da, db, ia, ib, metric=metric)
    assert torch.equal(eng.pair_scores(oa, ob, ia, ib, metric=metric).view(torch.int32), aligned.view(torch.int32))
    assert torch.equal(eng.pair_scores(oa, db, ia, ib, metric=metric).view(torch.int32), aligned.view(torch.int32))   # one off


@pytest.mark.parametrize("metric", METRICS)
def test_a_trial_alone_gives_its_bits_in_the_batch(eng, metric):
    a, b, _ = matrices(128)
    da, db = eng.to_device(a), eng.to_device(b)
    rng = np.random.default_rng(6)
    ia, ib = rng.integers(0, N_A, 40_000), rng.integers(0, N_B, 40_000)
    batch = eng.pair_scores(da, db, ia, ib, metric=metric).view(torch.int32).cpu().numpy()
    for p in (0, 1, 15, 16, 255, 32_768, 39_999):
        alone = eng.pair_scores(da, db, ia[p:p + 1], ib[p:p + 1], metric=metric).view(torch.int32).cpu().numpy()
        assert alone[0] == batch[p]
    again = eng.pair_scores(da, db, ia, ib, metric=metric).view(torch.int32).cpu().numpy()
    np.testing.assert_array_equal(again, batch)


@pytest.mark.parametrize("metric", METRICS)
def test_bad_indices(eng, metric):
    a, b, _ = matrices(132)
    da, db = eng.to_device(a), eng.to_device(b)
    rng = np.random.default_rng(7)
    n = 5000
    ia, ib = rng.integers(0, N_A, n), rng.integers(0, N_B, n)
    good = eng.pair_scores(da, db, ia, ib, metric=metric).cpu().numpy()
    ja, jb = ia.copy(), ib.copy()
    ja[[3, 100, 4097]] = (-1, N_A, 1 << 40)
    jb[[17, 4999]] = (N_B, -(1 << 62))
    jb[100] = N_B + 5                                              # both sides bad: still one trial
    ja[2000] = N_B                                                 # legal for a (47 < 61) ...
    wrong = np.zeros(n, bool)
    wrong[[3, 100, 4097, 17, 4999]] = True
    bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
    got = eng.pair_scores(da, db, ja, jb, metric=metric, bad_count=bad).cpu().numpy()
    assert int(bad.item()) == 5
    np.testing.assert_array_equal(np.isnan(got), wrong)
    same = ~wrong
    same[2000] = False
    np.testing.assert_array_equal(got[same].view(np.int32), good[same].view(np.int32))
    assert np.isnan(eng.pair_scores(da, db, ja, jb, metric=metric).cpu().numpy()).sum() == 5        # bad_count may be NULL
    kb = ib.copy()
    kb[0] = N_A - 1                                                # ... and not for b (60 >= 47)
    bad.zero_()
    assert np.isnan(eng.pair_scores(da, db, ia, kb, metric=metric, bad_count=bad).cpu().numpy()[0]) and int(bad.item()) == 1


def test_agrees_with_the_score_matrix(eng):
    """pair_scores on (i, j) against cosine_scores(a, b)[i, j]: the bar tests/test_gpu_parity.py holds that matrix to
    (test_cosine_scores: rtol = 0, atol = 1e-5)."""
    for dim in (128, 100, 7):                                         # shapes of test_cosine_scores
        rng = np.random.default_rng(dim)
        a = rng.standard_normal((N_A, dim)).astype(np.float32)
        b = rng.standard_normal((N_B, dim)).astype(np.float32)
        a[0] = 0
        full = eng.cosine_scores(a, b).cpu().numpy()
        i, j = np.meshgrid(np.arange(N_A), np.arange(N_B), indexing="ij")
        got = eng.pair_scores(a, b, i.reshape(-1), j.reshape(-1)).cpu().numpy().reshape(N_A, N_B)
        np.testing.assert_allclose(got, full, rtol=0, atol=1e-5)


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    a, b, _ = matrices(128)
    da, db = eng.to_device(a), eng.to_device(b)
    idx = eng.to_device(np.zeros(4, np.int64))
    out = torch.full((4,), -7.0, dtype=torch.float32, device=eng.device)
    p = eng._ptr

    def call(**kw):
        args = dict(a=p(da), n_a=N_A, b=p(db), n_b=N_B, dim=128, ia=p(idx), ib=p(idx), n=4, metric=0, out=p(out))
        args.update(kw)
        return eng.lib.svk_pair_scores(eng.ctx, args["a"], args["n_a"], args["b"], args["n_b"], args["dim"], args["ia"],
                                       args["ib"], args["n"], args["metric"], args["out"], None)

    def message():
        return eng.lib.svk_last_error(eng.ctx).decode()

    assert call() == _lib.SVK_OK
    for metric in (2, -1):
        assert call(metric=metric) == _lib.SVK_ERR_BAD_ARG and "metric" in message()
    for dim in (0, -3, 4097):
        assert call(dim=dim) == _lib.SVK_ERR_BAD_ARG and "dim" in message()
    assert call(n=-1) == _lib.SVK_ERR_BAD_ARG and "negative" in message()
    assert call(n_a=-1) == _lib.SVK_ERR_BAD_ARG
    for name in ("a", "b", "ia", "ib", "out"):
        assert call(**{name: None}) == _lib.SVK_ERR_BAD_ARG and "NULL" in message()
    assert call(a=C.c_void_p(da.data_ptr() + 2)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(n=0, a=None, out=None) == _lib.SVK_OK               # nothing to launch, nothing to check
    with pytest.raises(_lib.SvkError, match="dim"):
        eng.pair_scores(np.zeros((2, 4097), np.float32), np.zeros((2, 4097), np.float32), [0], [1])
    with pytest.raises(ValueError, match="metric"):
        eng.pair_scores(da, db, [0], [1], metric="dot")
    torch.cuda.synchronize()
