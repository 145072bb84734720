"""svk_plda_pair_scores against the float64 restatement (tests/plda_f64_ref.llr_pairs), trial by trial.

Shapes: dim 1, 3, 128, 130, 512 (the 4-byte and the 16-byte loads, one and several sweeps of a lane over its columns),
n_pairs 1, 15, 16, 17 (a workgroup holds 16 trials) and 1 000; d_a == d_b (one matrix, 61 rows); counts NULL and mixed {1, 2, 7}.

THE BOUND.  The reference adds 6 dim float64 terms per trial: alpha u v, -beta v^2 / 2, -gamma u^2 / 2 and three half
logarithms per direction (the kernel forms the three as one log1p, more accurate for small psi).  Both sides compute every
term with a handful of float64 roundings (a coefficient is two or three products and a division: at most 8 x 2^-53 of the
term's magnitude, the logarithms within 2 ulp of the three logarithms' magnitudes) and add them -- the kernel dim / 16 terms per
lane in order and four butterfly steps, NumPy pairwise -- which carries at most (dim / 16 + 4) 2^-53 and log2(6 dim) 2^-53 of
sum |terms|.  Together that stays below (dim + 8) 2^-52 sum |terms| for every dim >= 1 (at dim = 1:
(8 + 4.1 + 2.6) 2^-53 = 7.3 x 2^-52 against 9 x 2^-52), and the single rounding to f32 adds 2^-24 |ref|:
    |got - ref| <= 2^-24 |ref| + (dim + 8) 2^-52 sum |terms|."""
import ctypes as C

import numpy as np
import pytest

import plda_f64_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_ROWS = 61
DIMS = (1, 3, 128, 130, 512)
N_PAIRS = (1, 15, 16, 17, 1000)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


_cache = {}


def inputs(dim):
    if dim not in _cache:
        psi = ref.make_psi(dim, 500 + dim)
        rows = ref.make_rows(N_ROWS, psi, 600 + dim)
        counts = np.random.default_rng(700 + dim).choice([1, 2, 7], N_ROWS).astype(np.int32)
        for m in (psi, rows, counts):
            m.setflags(write=False)
        _cache[dim] = (psi, rows, counts)
    return _cache[dim]


def bound(dim, want, mag):
    return ref.U32 * np.abs(want) + (dim + 8) * 2.0 ** -52 * mag


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", DIMS)
def test_against_float64(eng, dim, form):
    psi, rows, counts = inputs(dim)
    d, dp = eng.to_device(rows), eng.to_device(psi)
    cnt = counts if form == "counts" else None
    dc = None if cnt is None else eng.to_device(cnt)
    rng = np.random.default_rng(dim)
    worst = 0.0
    for n_pairs in N_PAIRS:
        ia, ib = rng.integers(0, N_ROWS, n_pairs), rng.integers(0, N_ROWS, n_pairs)
        if n_pairs >= 15:
            ia[:2], ib[:2] = (5, 9), (5, 60)                        # a row against itself
        bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
        got = eng.plda_pair_scores(d, d, ia, ib, dp, counts_b=dc, bad_count=bad).cpu().numpy()
        assert got.shape == (n_pairs,) and got.dtype == np.float32 and int(bad.item()) == 0
        want, mag = ref.llr_pairs(rows, rows, ia, ib, psi, cnt)
        err = np.abs(got.astype(np.float64) - want)
        b = bound(dim, want, mag)
        worst = max(worst, float((err / b).max()))
        assert (err <= b).all(), "%d trials: %d outside the bound" % (n_pairs, int((err > b).sum()))
    print("dim %d, %s: worst error / bound = %.4f" % (dim, form, worst))


@pytest.mark.parametrize("form", ("single", "counts"))
def test_a_trial_alone_gives_its_bits_in_the_list(eng, form):
    psi, rows, counts = inputs(130)
    d, dp = eng.to_device(rows), eng.to_device(psi)
    dc = eng.to_device(counts) if form == "counts" else None
    rng = np.random.default_rng(6)
    n = 40_000                                                       # past one sweep of the grid-stride loop (32 768 trials)
    ia, ib = rng.integers(0, N_ROWS, n), rng.integers(0, N_ROWS, n)
    batch = eng.plda_pair_scores(d, d, ia, ib, dp, counts_b=dc).view(torch.int32).cpu().numpy()
    for p in (0, 1, 15, 16, 255, 32_768, 39_999):
        alone = eng.plda_pair_scores(d, d, ia[p:p + 1], ib[p:p + 1], dp, counts_b=dc).view(torch.int32).cpu().numpy()
        assert alone[0] == batch[p]
    assert np.array_equal(eng.plda_pair_scores(d, d, ia, ib, dp, counts_b=dc).view(torch.int32).cpu().numpy(), batch)
    # the same pair of rows anywhere in the list: the same bits
    first = {}
    for p in range(n):
        first.setdefault((ia[p], ib[p]), batch[p])
    assert all(first[(ia[p], ib[p])] == batch[p] for p in range(0, n, 7))


@pytest.mark.parametrize("dim", (128, 130))
def test_scalar_loads_give_the_same_bits(eng, dim):
    psi, rows, counts = inputs(dim)
    d, dp, dc = eng.to_device(rows), eng.to_device(psi), eng.to_device(counts)
    assert d.data_ptr() % 16 == 0
    flat = torch.empty(rows.size + 1, dtype=torch.float32, device=eng.device)
    off = flat[1:].view(N_ROWS, dim)
    off.copy_(d)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    rng = np.random.default_rng(5)
    ia, ib = rng.integers(0, N_ROWS, 999), rng.integers(0, N_ROWS, 999)
    aligned = eng.plda_pair_scores(d, d, ia, ib, dp, counts_b=dc).view(torch.int32)
    assert torch.equal(eng.plda_pair_scores(off, off, ia, ib, dp, counts_b=dc).view(torch.int32), aligned)
    assert torch.equal(eng.plda_pair_scores(off, d, ia, ib, dp, counts_b=dc).view(torch.int32), aligned)       # one off


def test_bad_indices_and_counts(eng):
    psi, rows, counts = inputs(130)
    d, dp = eng.to_device(rows), eng.to_device(psi)
    other = eng.to_device(rows[:47])
    rng = np.random.default_rng(7)
    n = 5000
    ia, ib = rng.integers(0, N_ROWS, n), rng.integers(0, 47, n)
    good = eng.plda_pair_scores(d, other, ia, ib, dp).cpu().numpy()
    ja, jb = ia.copy(), ib.copy()
    ja[[3, 100, 4097]] = (-1, N_ROWS, 1 << 40)
    jb[[17, 4999]] = (47, -(1 << 62))
    jb[100] = 52                                                     # both sides bad: still one trial
    ja[2000] = 47                                                    # legal for a (47 < 61) ...
    wrong = np.zeros(n, bool)
    wrong[[3, 100, 4097, 17, 4999]] = True
    bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
    got = eng.plda_pair_scores(d, other, ja, jb, dp, bad_count=bad).cpu().numpy()
    assert int(bad.item()) == 5
    np.testing.assert_array_equal(np.isnan(got), wrong)
    same = ~wrong
    same[2000] = False
    np.testing.assert_array_equal(got[same].view(np.int32), good[same].view(np.int32))
    assert np.isnan(eng.plda_pair_scores(d, other, ja, jb, dp).cpu().numpy()).sum() == 5          # bad_count may be NULL
    kb = ib.copy()
    kb[0] = N_ROWS - 1                                               # ... and not for b (60 >= 47)
    bad.zero_()
    assert np.isnan(eng.plda_pair_scores(d, other, ia, kb, dp, bad_count=bad).cpu().numpy()[0]) and int(bad.item()) == 1
    # a count < 1 gives NaN at the trials of that model and is no bad index
    c2 = counts[:47].copy()
    c2[11] = 0
    bad.zero_()
    got = eng.plda_pair_scores(d, other, ia, ib, dp, counts_b=c2, bad_count=bad).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), ib == 11)
    assert int(bad.item()) == 0 and (ib == 11).any()


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", (3, 128, 130))
def test_agrees_with_the_score_matrix(eng, dim, form):
    """Every (i, j): the trial lies within the matrix entry's bound (tests/test_plda_scores.py) of the float64 score, and so
    does the matrix entry; zero psi gives exact zeros here too."""
    psi, rows, counts = inputs(dim)
    cnt = counts if form == "counts" else None
    full = eng.plda_scores(rows, rows, psi, cnt).cpu().numpy().astype(np.float64)
    i, j = np.meshgrid(np.arange(N_ROWS), np.arange(N_ROWS), indexing="ij")
    got = eng.plda_pair_scores(rows, rows, i.reshape(-1), j.reshape(-1), psi, counts_b=cnt).cpu().numpy().reshape(N_ROWS, N_ROWS)
    want, _ = ref.llr(rows, rows, psi, cnt)
    mb = ref.matrix_bound(rows, rows, psi, cnt, want)
    assert (np.abs(full - want) <= mb).all() and (np.abs(got - want) <= mb).all()
    assert (np.abs(got - full) <= 2 * mb).all()
    zero = eng.plda_pair_scores(rows, rows, i.reshape(-1), j.reshape(-1), np.zeros(dim), counts_b=cnt).cpu().numpy()
    assert not zero.any()


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    psi, rows, counts = inputs(128)
    d, dp, dc = eng.to_device(rows), eng.to_device(psi), eng.to_device(counts)
    idx = eng.to_device(np.zeros(4, np.int64))
    out = torch.full((4,), -7.0, dtype=torch.float32, device=eng.device)
    p = eng._ptr

    def call(**kw):
        a = dict(ctx=eng.ctx, a=p(d), n_a=N_ROWS, b=p(d), n_b=N_ROWS, dim=128, psi=p(dp), cnt=p(dc), ia=p(idx), ib=p(idx), n=4,
                 out=p(out))
        a.update(kw)
        return eng.lib.svk_plda_pair_scores(a["ctx"], a["a"], a["n_a"], a["b"], a["n_b"], a["dim"], a["psi"], a["cnt"], a["ia"],
                                            a["ib"], a["n"], a["out"], None)

    def message():
        return eng.lib.svk_last_error(eng.ctx).decode()

    assert call() == _lib.SVK_OK and call(cnt=None) == _lib.SVK_OK
    assert call(ctx=None) == _lib.SVK_ERR_BAD_ARG
    for dim in (0, -3, 513):
        assert call(dim=dim) == _lib.SVK_ERR_BAD_ARG and "dim" in message()
    assert call(n=-1) == _lib.SVK_ERR_BAD_ARG and "negative" in message()
    assert call(n_a=-1) == _lib.SVK_ERR_BAD_ARG
    for name in ("a", "b", "psi", "ia", "ib", "out"):
        assert call(**{name: None}) == _lib.SVK_ERR_BAD_ARG and "NULL" in message()
    assert call(a=C.c_void_p(d.data_ptr() + 2)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(psi=C.c_void_p(dp.data_ptr() + 4)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(n=0, a=None, out=None, psi=None) == _lib.SVK_OK      # nothing to launch, nothing to check
    torch.cuda.synchronize()
    with pytest.raises(_lib.SvkError, match="dim"):
        eng.plda_pair_scores(np.zeros((2, 513), np.float32), np.zeros((2, 513), np.float32), [0], [1], np.zeros(513))
    with pytest.raises(ValueError, match="counts"):
        eng.plda_pair_scores(rows, rows, [0], [1], psi, counts_b=counts[:-1])
