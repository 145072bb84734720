"""svk_plda_scores against the float64 restatement (tests/plda_f64_ref.py): every score within a derived bound, and the bit-level
properties of the contract (include/svk.h).

THE SHAPES straddle the kernel's tiles, which are the ones the issue names: 16-row MFMA tiles, 32 rows per wave and 32
enrolled rows per LDS block, 128 test rows per workgroup, 128 columns per K block -- n_test 1, 15, 16, 17, 129 (two workgroups),
n_enroll 1, 31, 32, 33, 65, dim 1, 3, 4, 13, 128, 130 (two K blocks, the second ragged), 512.  One more shape, 17 x 131 079,
gives every workgroup two or three column blocks in a row (the launch has at most 8 workgroups per CU, 2 048 on the MI355X,
and this shape has 4 097 column blocks): the only way to reach the double-buffered walk from one block to the next.
Inputs: psi spans 0 .. 300 with every fifth entry exactly 0 (plda_f64_ref.make_psi), rows ~ N(0, 1 + psi), counts NULL or mixed
from {1, 2, 7}.

THE BOUND.  With a, b the float64 operands of the contract BEFORE their rounding (counts NULL: a = v, b = alpha(1) u, K = dim;
counts given: a = [v | v^2], b = [alpha(n) u | -beta(n) / 2], K = 2 dim) the kernel computes
    out = f32( f32sum_k( f32(a_k) f32(b_k) ) + s_i + t_j ),   s_i, t_j and the coefficients in float64.
  * each rounded operand moves its product by 2^-24 |a_k b_k| (f32(v) = v is exact, so only one operand of a first-half product
    is rounded: 2 x 2^-24 covers every product);
  * a product of two floats is exact on the matrix pipe, and the f32 sum of K terms in any order carries at most
    (K - 1) 2^-24 sum_k |a_k b_k|, one more 2^-24 for the product's own rounding if the pipe rounds it: (K - 1 + 1) 2^-24;
  * the final rounding to f32 is 2^-24 |out|, |out| = |ref| to first order;
  * the float64 pre-pass and epilogue are off by a few 2^-53 of the magnitudes of their terms: for these inputs, whose terms
    are within a factor 2^20 of sum_k |a_k b_k|, that is below 2^-30 of the first term.
  So  |out - ref| <= (K + 2) 2^-24 sum_k |a_k b_k| + 2^-24 |ref|  to first order, and the tests hold the scores to
      (K + 4) 2^-24 sum_k |a_k b_k| + 2^-24 |ref|:
  a headroom of 2 for the second-order terms (K 2^-24 of the bound itself, 3e-5 at K = 1 024), the float64 steps and the
  reference's own float64 rounding.  Derived, not tuned; each case prints its worst error / bound."""
import ctypes as C

import numpy as np
import pytest

import plda_f64_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_TEST = (1, 15, 16, 17, 129)
N_ENROLL = (1, 31, 32, 33, 65)
DIMS = (1, 3, 4, 13, 128, 130, 512)
MAX_T, MAX_E = max(N_TEST), max(N_ENROLL)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


_cache = {}


def inputs(dim):
    """(psi, test [129, dim], enroll [65, dim], counts [65]) and the float64 reference + bound of the full matrix per form --
    computed once per dim, shared by the tests, never written to.  A call on the first nt rows / ne models is held to the
    corner [:nt, :ne]: a score depends on its two rows alone."""
    if dim not in _cache:
        psi = ref.make_psi(dim, 1000 + dim)
        test, enroll = ref.make_rows(MAX_T, psi, 2000 + dim), ref.make_rows(MAX_E, psi, 3000 + dim)
        counts = np.random.default_rng(4000 + dim).choice([1, 2, 7], MAX_E).astype(np.int32)
        counts[:3] = (7, 1, 2)
        want = {}
        for form, cnt in (("single", None), ("counts", counts)):
            score, _ = ref.llr(test, enroll, psi, cnt)
            want[form] = (score, ref.matrix_bound(test, enroll, psi, cnt, score))
        for m in (psi, test, enroll, counts):
            m.setflags(write=False)
        _cache[dim] = (psi, test, enroll, counts, want)
    return _cache[dim]


def bits(t):
    return t.view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", DIMS)
def test_against_float64(eng, dim, form):
    psi, test, enroll, counts, want = inputs(dim)
    dt, de, dp = eng.to_device(test), eng.to_device(enroll), eng.to_device(psi)
    dc = eng.to_device(counts) if form == "counts" else None
    score, bound = want[form]
    worst = 0.0
    for nt in N_TEST:
        for ne in N_ENROLL:
            got = eng.plda_scores(dt[:nt], de[:ne], dp, None if dc is None else dc[:ne]).cpu().numpy()
            assert got.shape == (nt, ne) and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - score[:nt, :ne])
            worst = max(worst, float((err / bound[:nt, :ne]).max()))
            assert (err <= bound[:nt, :ne]).all(), "%d x %d: %d scores outside the bound" % (nt, ne, int((err > bound[:nt, :ne]).sum()))
    print("dim %d, %s: worst error / bound = %.4f" % (dim, form, worst))


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", (13, 128, 130))
def test_position_independence_and_reruns(eng, dim, form):
    """The 33 x 65 matrix, the same rows permuted, single rows and a 1 x 1 call: identical bits per (row, row, count)."""
    psi, test, enroll, counts, _ = inputs(dim)
    dt, de, dp = eng.to_device(test[:33]), eng.to_device(enroll), eng.to_device(psi)
    dc = eng.to_device(counts) if form == "counts" else None
    base = bits(eng.plda_scores(dt, de, dp, dc))
    assert np.array_equal(bits(eng.plda_scores(dt, de, dp, dc)), base)                       # two runs
    rng = np.random.default_rng(dim)
    pr, pc = rng.permutation(33), rng.permutation(MAX_E)
    tr, tc = torch.from_numpy(pr).to(eng.device), torch.from_numpy(pc).to(eng.device)
    perm = bits(eng.plda_scores(dt[tr].contiguous(), de[tc].contiguous(), dp, None if dc is None else dc[tc].contiguous()))
    assert np.array_equal(perm, base[np.ix_(pr, pc)])
    for i, j in ((0, 0), (32, 64), (16, 31), (7, 33)):
        one = bits(eng.plda_scores(dt[i:i + 1], de[j:j + 1], dp, None if dc is None else dc[j:j + 1]))
        assert one.shape == (1, 1) and one[0, 0] == base[i, j]
    # inside a larger problem: 129 test rows (a second workgroup) leave the first 33 rows' bits alone
    big = bits(eng.plda_scores(eng.to_device(test), de, dp, dc))
    assert np.array_equal(big[:33], base)


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", (13, 130))
def test_many_column_blocks_per_workgroup(eng, dim, form):
    """17 x 131 079: 4 097 column blocks on at most 2 048 workgroups -- each walks two or three blocks through both LDS buffers.
    The enrolled rows repeat the 65 of the small problem, so every score has a twin there: the same bits."""
    psi, test, enroll, counts, _ = inputs(dim)
    ne = 32 * 2048 * 2 + 7
    assert (ne + 31) // 32 > eng.num_cu * 8              # more column blocks than the launch has workgroups
    pick = np.random.default_rng(9).integers(0, MAX_E, ne)
    dt, dp = eng.to_device(test[:17]), eng.to_device(psi)
    de, dc = eng.to_device(enroll), eng.to_device(counts) if form == "counts" else None
    small = bits(eng.plda_scores(dt, de, dp, dc))
    tp = torch.from_numpy(pick).to(eng.device)
    got = bits(eng.plda_scores(dt, de[tp].contiguous(), dp, None if dc is None else dc[tp].contiguous()))
    assert got.shape == (17, ne) and np.array_equal(got, small[:, pick])


@pytest.mark.parametrize("form", ("single", "counts"))
def test_nan_and_inf_stay_where_they_are(eng, form):
    psi, test, enroll, counts, _ = inputs(130)
    dp = eng.to_device(psi)
    dc = eng.to_device(counts) if form == "counts" else None
    clean = eng.plda_scores(test[:33], enroll, dp, dc).cpu().numpy()
    assert np.isfinite(clean).all()
    for poison in (np.nan, np.inf):
        t2, e2 = test[:33].copy(), enroll.copy()
        t2[17, 129] = poison
        t2[2, 0] = -poison
        e2[40, 5] = poison
        got = eng.plda_scores(t2, e2, dp, dc).cpu().numpy()
        hit = np.zeros((33, MAX_E), bool)
        hit[[17, 2], :] = True
        hit[:, 40] = True
        assert not np.isfinite(got[hit]).any()
        assert np.array_equal(got[~hit].view(np.int32), clean[~hit].view(np.int32))
    if form == "counts":                                   # a count < 1 makes its column NaN, and only that
        c2 = counts.copy()
        c2[[3, 64]] = (0, -5)
        got = eng.plda_scores(test[:33], enroll, dp, c2).cpu().numpy()
        bad = np.zeros(MAX_E, bool)
        bad[[3, 64]] = True
        assert np.isnan(got[:, bad]).all() and np.array_equal(got[:, ~bad].view(np.int32), clean[:, ~bad].view(np.int32))


@pytest.mark.parametrize("dim", (3, 128, 130))
def test_zero_psi_scores_exactly_zero(eng, dim):
    _, test, enroll, counts, _ = inputs(dim)
    zero = np.zeros(dim)
    for cnt in (None, counts):
        got = eng.plda_scores(test, enroll, zero, cnt).cpu().numpy()
        assert got.shape == (MAX_T, MAX_E) and not got.any()


@pytest.mark.parametrize("form", ("single", "counts"))
@pytest.mark.parametrize("dim", (13, 128, 130))
def test_scalar_loads_give_the_same_bits(eng, dim, form):
    """Rows 4 bytes off a 16-byte boundary take the 4-byte loads; and dim % 4 != 0 (always 4-byte loads) gives the bits of the
    same rows padded with zero columns of psi = 0 to a multiple of 4 (16-byte loads): a padded column adds exactly nothing."""
    psi, test, enroll, counts, _ = inputs(dim)
    dt, de, dp = eng.to_device(test[:33]), eng.to_device(enroll), eng.to_device(psi)
    dc = eng.to_device(counts) if form == "counts" else None
    assert dt.data_ptr() % 16 == 0 and de.data_ptr() % 16 == 0
    aligned = bits(eng.plda_scores(dt, de, dp, dc))
    ft = torch.empty(dt.numel() + 1, dtype=torch.float32, device=eng.device)
    fe = torch.empty(de.numel() + 1, dtype=torch.float32, device=eng.device)
    ot, oe = ft[1:].view(33, dim), fe[1:].view(MAX_E, dim)
    ot.copy_(dt)
    oe.copy_(de)
    assert ot.data_ptr() % 16 == 4 and oe.data_ptr() % 16 == 4 and ot.is_contiguous()
    assert np.array_equal(bits(eng.plda_scores(ot, oe, dp, dc)), aligned)
    assert np.array_equal(bits(eng.plda_scores(ot, de, dp, dc)), aligned)
    if dim % 4:
        pad = 4 - dim % 4
        wide = lambda m: np.concatenate([m, np.zeros((m.shape[0], pad), np.float32)], axis=1)
        padded = bits(eng.plda_scores(wide(test[:33]), wide(enroll), np.r_[psi, np.zeros(pad)], dc))
        assert np.array_equal(padded, aligned)


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    psi, test, enroll, counts, _ = inputs(128)
    dt, de, dp, dc = eng.to_device(test), eng.to_device(enroll), eng.to_device(psi), eng.to_device(counts)
    out = torch.full((MAX_T, MAX_E), -7.0, dtype=torch.float32, device=eng.device)
    size = eng.lib.svk_plda_scores_workspace_bytes
    need = int(size(MAX_T, MAX_E, 128, 1))
    assert need > int(size(MAX_T, MAX_E, 128, 0)) >= 8 * (MAX_T + MAX_E) + 4 * MAX_E * 128
    assert need >= 8 * (MAX_T + MAX_E) + 4 * (2 * MAX_E + MAX_T) * 128
    for bad in ((0, 5, 128, 0), (5, 0, 128, 0), (-1, 5, 128, 0), (5, 5, 0, 0), (5, 5, 513, 1)):
        assert size(*bad) == 0
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    p = eng._ptr

    def call(**kw):
        a = dict(ctx=eng.ctx, t=p(dt), nt=MAX_T, e=p(de), ne=MAX_E, dim=128, psi=p(dp), cnt=p(dc), work=p(work), bytes=need,
                 out=p(out))
        a.update(kw)
        return eng.lib.svk_plda_scores(a["ctx"], a["t"], a["nt"], a["e"], a["ne"], a["dim"], a["psi"], a["cnt"], a["work"],
                                       a["bytes"], a["out"])

    def message():
        return eng.lib.svk_last_error(eng.ctx).decode()

    assert call() == _lib.SVK_OK and call(cnt=None) == _lib.SVK_OK
    assert call(ctx=None) == _lib.SVK_ERR_BAD_ARG
    for dim in (0, -3, 513):
        assert call(dim=dim) == _lib.SVK_ERR_BAD_ARG and "dim" in message()
    assert call(nt=-1) == _lib.SVK_ERR_BAD_ARG and "negative" in message()
    assert call(ne=-1) == _lib.SVK_ERR_BAD_ARG
    for name in ("t", "e", "psi", "work", "out"):
        assert call(**{name: None}) == _lib.SVK_ERR_BAD_ARG and "NULL" in message()
    assert call(t=C.c_void_p(dt.data_ptr() + 2)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(psi=C.c_void_p(dp.data_ptr() + 4)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(work=C.c_void_p(work.data_ptr() + 8)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(bytes=need - 1) == _lib.SVK_ERR_BAD_ARG and "workspace" in message()
    assert call(cnt=None, bytes=int(size(MAX_T, MAX_E, 128, 0))) == _lib.SVK_OK              # the smaller form's size is enough for it
    assert call(bytes=int(size(MAX_T, MAX_E, 128, 0))) == _lib.SVK_ERR_BAD_ARG
    for empty in (dict(nt=0), dict(ne=0)):                                                    # nothing to launch, nothing to check
        assert call(t=None, e=None, psi=None, work=None, bytes=0, out=None, **empty) == _lib.SVK_OK
    torch.cuda.synchronize()
    with pytest.raises(_lib.SvkError, match="dim"):
        eng.plda_scores(np.zeros((2, 513), np.float32), np.zeros((2, 513), np.float32), np.zeros(513))
    with pytest.raises(ValueError, match="psi"):
        eng.plda_scores(test, enroll, psi[:-1])
    with pytest.raises(ValueError, match="counts"):
        eng.plda_scores(test, enroll, psi, counts[:-1])
    assert tuple(eng.plda_scores(test[:0], enroll, psi).shape) == (0, MAX_E)
