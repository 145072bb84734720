"""svk_cosine_scores and svk_l2_dist against NumPy float64 (tests/scoring_f64_ref.py) on every kernel and branch the two
entry points can take, plus the properties that hold bit for bit from the code alone.

svk_cosine_scores dispatches to cosine_kernel (one wave per 16 test rows) or, from 2^22 pairs and 64 enrolled rows on, to
inv_norm_kernel + cosine_tiled_kernel<HOIST> (HOIST: dim <= 128, the test fragments stay in registers; otherwise they are
streamed), the latter in two register budgets (SVK_COS_WAVES=3 picks the `_w3` twins).  Both kernels load 16 bytes at a time
when dim % 4 == 0 and both matrices are 16-byte aligned, 4 bytes otherwise.

(a) test_cosine_against_float64: |got - cosine64| <= 1e-5 for four kinds of input on the smallest shapes that reach each
    branch; a planted zero row / column is exactly 0, a planted copy scores 1.  Each case prints its worst error and its worst
    err / (2^-24 absdot64).
(b) disjoint supports score exactly 0; permuting the rows permutes the bits; three runs agree bit for bit; a NaN and an Inf
    stay in their row and column.
(c) outputs past 2^31 elements, one per kernel, checked on sampled rows.
(d) svk_l2_dist against l2_64 with the bar derived in scoring_f64_ref.py.
(e) argument checks.
tests/test_gpu_parity.py::test_cosine_scores[_tiled_kernel] pin the reference's own float32 numbers and the goldens; this file
is where the score matrix is held to float64.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import scoring_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_c3d2_float64)

TOL = R.COSINE_TOL

# ---- the shapes: (n_test, n_enroll, dim) ------------------------------------------------------------------------------------
SMALL = ((1, 1, 1), (17, 33, 7), (16, 16, 64), (33, 17, 128), (40, 50, 200), (19, 21, 201), (20, 20, 4096),
         (70_000, 63, 16),        # product above 2^22 with n_enroll < 64
         (2047, 2048, 8))         # product 2^22 - 2048, just under the border
SMALL_MISALIGNED = (33, 17, 128)
HOISTED = ((2048, 2048, 128),     # exact blocks, product exactly 2^22: only the fast paths run
           (4100, 1030, 128), (3000, 1500, 7), (8200, 520, 100),
           (64, 65_536, 128),     # n_test < 128: rows_in is false for most waves
           (65_536, 64, 128))     # n_enroll == 64
TILED_MISALIGNED = (4100, 1030, 128)
STREAMED = ((2050, 2100, 200), (2050, 2100, 201), (2050, 2100, 129), (2048, 2048, 256), (2049, 2049, 4096))
SAMPLED_ROWS = 400                # 2049 x 2049 x 4096: the float64 matrix is 34 GFLOP on the CPU; 400 rows of it are checked there


def takes_tiled(shape):
    """svk_cosine_scores' own rule (csrc/scoring.hip)."""
    return shape[0] * shape[1] >= 1 << 22 and shape[1] >= 64


assert not any(takes_tiled(s) for s in SMALL) and all(takes_tiled(s) for s in HOISTED + STREAMED)
assert all(s[2] <= 128 for s in HOISTED) and all(s[2] > 128 for s in STREAMED)


def _cases():
    """(shape, kind, waves, misaligned operand): the variants of one (shape, kind) are neighbours, so that its float64
    reference is computed once and dropped when the next one comes."""
    out = []
    for shape in SMALL:
        for kind in R.KINDS:
            out.append((shape, kind, 2, None))
            if shape == SMALL_MISALIGNED:
                out += [(shape, kind, 2, "test"), (shape, kind, 2, "enroll")]
    for shape in HOISTED + STREAMED:
        for kind in R.KINDS:
            for waves in (2, 3):
                out.append((shape, kind, waves, None))
                if shape == TILED_MISALIGNED:
                    out += [(shape, kind, waves, "test"), (shape, kind, waves, "enroll")]
    return out


def _case_id(case):
    shape, kind, waves, mis = case
    return "%dx%dx%d-%s%s%s" % (shape + (kind, "-w3" if waves == 3 else "", "-misaligned_" + mis if mis else ""))


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture
def budget(monkeypatch):
    """budget(3) selects the `_w3` instances of the tiled kernel for the rest of the test (the library reads the variable on
    every call); budget(2) the default ones."""
    def pick(waves):
        if waves == 3:
            monkeypatch.setenv("SVK_COS_WAVES", "3")
        else:
            monkeypatch.delenv("SVK_COS_WAVES", raising=False)
    return pick


def off_boundary(eng, x):
    """x on the device 4 bytes past a 16-byte boundary; contiguous, so Engine.to_device keeps the pointer."""
    flat = torch.empty(x.size + 1, dtype=torch.float32, device=eng.device)
    v = flat[1:].view(*x.shape)
    v.copy_(eng.to_device(x))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def scores(eng, t, e, misaligned=None):
    dt = off_boundary(eng, t) if misaligned == "test" else eng.to_device(t)
    de = off_boundary(eng, e) if misaligned == "enroll" else eng.to_device(e)
    assert (dt.data_ptr() % 16 == 0) == (misaligned != "test") and (de.data_ptr() % 16 == 0) == (misaligned != "enroll")
    out = eng.cosine_scores(dt, de)
    assert out.dtype == torch.float32 and tuple(out.shape) == (t.shape[0], e.shape[0])
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- (a) accuracy ---------------------------------------------------------------------------------------------------------------
_last = {}


def reference(shape, kind):
    """(t, e, planted, rows, cosine64 [rows], absdot64 [rows]), read-only; rows is None (all) but for dim 4096 at 2049 rows."""
    key = (shape, kind)
    if _last.get("key") != key:
        _last.clear()
        nt, ne, dim = shape
        t, e = R.MAKERS[kind](nt, ne, dim, seed=1000 * nt + 10 * ne + dim)
        planted = R.plant(t, e)
        rows = None
        if nt * ne * dim > 1 << 33:
            must = [r for r in (0, nt - 1, planted["zero_t"], planted["copy"][0]) if r is not None]
            rest = np.random.default_rng(7).choice(nt, SAMPLED_ROWS, replace=False)
            rows = np.unique(np.concatenate([must, rest]))
        ref, cond = R.cosine64(t, e, rows), R.absdot64(t, e, rows)
        for m in (t, e, ref, cond):
            m.setflags(write=False)
        _last.update(key=key, value=(t, e, planted, rows, ref, cond))
    return _last["value"]


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_cosine_against_float64(eng, budget, case):
    shape, kind, waves, misaligned = case
    nt, ne, dim = shape
    t, e, planted, rows, ref, cond = reference(shape, kind)
    budget(waves)
    out = scores(eng, t, e, misaligned)
    if rows is not None:
        # every score on the device in float64 first, then the sampled rows against NumPy
        x, y = eng.to_device(t).double(), eng.to_device(e).double()
        nx, ny = x.norm(dim=1), y.norm(dim=1)
        nx[nx == 0] = 1.0
        ny[ny == 0] = 1.0
        dev_err = float((out.double() - (x @ y.T) / (nx[:, None] * ny[None, :])).abs().max())
        print("all %d x %d scores against torch float64 on the device: worst %.3g" % (nt, ne, dev_err))
        assert dev_err <= TOL
    got = out.cpu().numpy()
    sub = got if rows is None else got[rows]
    err = np.abs(sub.astype(np.float64) - ref)
    live = cond > 0
    ratio = float((err[live] / (R.U32 * cond[live])).max()) if live.any() else 0.0
    print("%s: worst |score - float64| = %.3g, worst err / (2^-24 absdot64) = %.3g over %d x %d"
          % (_case_id(case), err.max(), ratio, sub.shape[0], ne))
    assert not np.isnan(got).any()
    assert err.max() <= TOL
    if planted["zero_t"] is not None:
        assert np.all(got[planted["zero_t"]] == 0.0), "zero test row"
    if planted["zero_e"] is not None:
        assert np.all(got[:, planted["zero_e"]] == 0.0), "zero enrolled row"
    if planted["copy"] is not None:
        r, c = planted["copy"]
        assert abs(float(got[r, c]) - 1.0) <= TOL, "copied row scores %.9g" % got[r, c]


# ---- (b) exact properties ----------------------------------------------------------------------------------------------------------
EXACT_SHAPES = [((33, 17, 128), 2), ((4100, 1030, 128), 2), ((4100, 1030, 128), 3), ((2050, 2100, 200), 2),
                ((2050, 2100, 200), 3)]
DISJOINT_SHAPES = [((33, 17, 100), 2), ((19, 21, 201), 2), ((4100, 1030, 100), 2), ((4100, 1030, 100), 3),
                   ((2050, 2100, 201), 2), ((2050, 2100, 201), 3)]


def _shape_id(p):
    return "%dx%dx%d%s" % (p[0] + ("-w3" if p[1] == 3 else "",))


@pytest.mark.parametrize("shape,waves", DISJOINT_SHAPES, ids=[_shape_id(p) for p in DISJOINT_SHAPES])
def test_disjoint_supports_score_exactly_zero(eng, budget, shape, waves):
    """Test rows live in the even columns, enrolled rows in the odd ones: every product is 0, whatever the K order, and the
    last K block is ragged (dim 100, 201)."""
    nt, ne, dim = shape
    t, e = R.zero_mean(nt, ne, dim, seed=3)
    t[:, 1::2] = 0
    e[:, 0::2] = 0
    budget(waves)
    got = scores(eng, t, e).cpu().numpy()
    assert np.all(got == 0.0)


@pytest.mark.parametrize("shape,waves", EXACT_SHAPES, ids=[_shape_id(p) for p in EXACT_SHAPES])
def test_permuted_rows_give_permuted_bits(eng, budget, shape, waves):
    """scores(t[p], e[q])[i, j] has the bits of scores(t, e)[p[i], q[j]]: the K order depends on dim alone and a norm on its
    row alone.  Rows that contaminate one another, a stale LDS buffer or an epilogue that takes another block's norms would
    show here."""
    nt, ne, dim = shape
    t, e = R.zero_mean(nt, ne, dim, seed=4)
    rng = np.random.default_rng(5)
    p, q = rng.permutation(nt), rng.permutation(ne)
    budget(waves)
    base = scores(eng, t, e).cpu().numpy()
    perm = scores(eng, t[p], e[q]).cpu().numpy()
    assert np.array_equal(bits(perm), bits(base[p][:, q]))


@pytest.mark.parametrize("shape,waves", EXACT_SHAPES[1:], ids=[_shape_id(p) for p in EXACT_SHAPES[1:]])
def test_three_runs_agree_bit_for_bit(eng, budget, shape, waves):
    nt, ne, dim = shape
    t, e = R.zero_mean(nt, ne, dim, seed=6)
    dt, de = eng.to_device(t), eng.to_device(e)
    budget(waves)
    first = eng.cosine_scores(dt, de)
    for _ in range(2):
        assert torch.equal(eng.cosine_scores(dt, de).view(torch.int32), first.view(torch.int32))


@pytest.mark.parametrize("where", ["interior", "ragged last block"])
@pytest.mark.parametrize("shape,waves", EXACT_SHAPES, ids=[_shape_id(p) for p in EXACT_SHAPES])
def test_nan_and_inf_stay_in_their_row_and_column(eng, budget, shape, waves, where):
    """One NaN in test row r, one +inf in enrolled row c: row r and column c are NaN (inf / inf, or x times 1 / inf with an
    infinite x; sklearn's normalise-then-dot gives NaN too), every other score keeps its bits."""
    nt, ne, dim = shape
    t, e = R.zero_mean(nt, ne, dim, seed=8)
    r, c = (nt // 4, ne // 2) if where == "interior" else (nt - 1, ne - 1)
    if where != "interior":
        assert r >= nt - nt % 16 and c >= ne - ne % 16      # inside the partial last tile of either kernel
    budget(waves)
    clean = scores(eng, t, e).cpu().numpy()
    t[r, dim // 2] = np.nan
    e[c, dim - 1] = np.inf
    got = scores(eng, t, e).cpu().numpy()
    assert np.isnan(got[r]).all() and np.isnan(got[:, c]).all()
    keep = np.ones((nt, ne), dtype=bool)
    keep[r] = False
    keep[:, c] = False
    assert np.array_equal(bits(got)[keep], bits(clean)[keep])


# ---- (c) past 2^31 output elements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2_090_000, 1030, 8), (53_700_000, 40, 8)], ids=["tiled", "small"])
def test_output_past_two_to_the_31_elements(eng, shape):
    """The 64-bit index arithmetic of both epilogues.  Inputs drawn on the device; the float64 reference covers the first 130
    rows, the 260 rows around the one that holds flat element 2^31 and the last 140; every score is bounded on the device."""
    nt, ne, dim = shape
    assert nt * ne > 1 << 31 and takes_tiled(shape) == (ne >= 64)
    gen = torch.Generator(device=eng.device)
    gen.manual_seed(nt + ne)
    t = e = out = None
    try:
        try:
            t = torch.randn((nt, dim), generator=gen, dtype=torch.float32, device=eng.device)
            e = torch.randn((ne, dim), generator=gen, dtype=torch.float32, device=eng.device)
            out = eng.cosine_scores(t, e)
        except torch.cuda.OutOfMemoryError as err:
            pytest.skip("the device cannot grant the memory: %s" % err)
        mid = (1 << 31) // ne
        rows = np.concatenate([np.arange(130), np.arange(mid - 130, mid + 130), np.arange(nt - 140, nt)])
        assert 130 < mid - 130 and mid + 130 < nt - 140
        pick = torch.from_numpy(rows).to(eng.device)
        got = out[pick].cpu().numpy()
        want = R.cosine64(t[pick].cpu().numpy(), e.cpu().numpy())
        err = np.abs(got.astype(np.float64) - want)
        top = float(torch.maximum(out.max(), -out.min()))
        print("%d x %d x %d: worst |score - float64| = %.3g over %d rows, max |score| = %.9g" % (nt, ne, dim, err.max(), rows.size, top))
        assert err.max() <= TOL
        assert top <= 1.0 + TOL          # NaN fails this too
    finally:
        del t, e, out                    # 8.6 GB: back to the device before the next test
        torch.cuda.empty_cache()


# ---- (d) svk_l2_dist ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 4, 63, 64, 65, 128, 200, 4096])
def test_l2_dist_against_float64(eng, dim):
    """N(0, 1) pairs, nearly equal pairs and equal pairs; n = 32 num_cu + 5 enters the grid-stride loop (the grid is capped
    at 8 num_cu workgroups of four rows)."""
    worst = 0.0
    for n in (1, 9, 4097, 32 * eng.num_cu + 5):
        rng = np.random.default_rng(100 * dim + n)
        a = rng.standard_normal((n, dim), dtype=np.float32)
        noise = rng.standard_normal((n, dim), dtype=np.float32)
        near = (a.astype(np.float64) + 1e-4 * noise).astype(np.float32)
        da = eng.to_device(a)
        for name, b in (("normal", noise), ("nearly equal", near)):
            got = eng.l2_dist(da, b).cpu().numpy()
            want = R.l2_64(a, b)
            assert got.dtype == np.float32 and got.shape == (n,)
            err, bar = np.abs(got.astype(np.float64) - want), R.l2_bar(dim, want)
            live = want > 0              # (a nearly equal pair of dim 1 can round to an equal one: bar 0, exactly 0 wanted)
            assert live.sum() >= n - n // 100
            worst = max(worst, float((err[live] / bar[live]).max()))
            assert np.all(err <= bar), "dim %d, n %d, %s pairs: %.3g of the bar" % (dim, n, name, (err[live] / bar[live]).max())
        same = eng.l2_dist(da, da.clone()).cpu().numpy()
        assert same.shape == (n,) and np.all(same == 0.0)
    print("dim %d: worst |got - float64| / ((dim / 2 + 3) 2^-24 float64) = %.3g" % (dim, worst))


# ---- (e) arguments ----------------------------------------------------------------------------------------------------------------------
def test_cosine_arguments(eng):
    from speaker_verification_amd import _lib
    p = eng._ptr
    buf = torch.zeros(8 * 4097, dtype=torch.float32, device=eng.device)
    out = torch.full((64,), 7.0, dtype=torch.float32, device=eng.device)

    def call(nt, ne, dim, t=buf, e=buf, o=out):
        return eng.lib.svk_cosine_scores(eng.ctx, p(t), p(e), nt, ne, dim, p(o))

    def message():
        return eng.lib.svk_last_error(eng.ctx).decode()

    assert call(8, 8, 4096) == _lib.SVK_OK                      # the documented limit
    assert call(8, 8, 4097) == _lib.SVK_ERR_UNSUPPORTED and "4096" in message()
    for bad in ((8, 8, 0), (8, 8, -1), (-1, 8, 16), (8, -1, 16)):
        assert call(*bad) == _lib.SVK_ERR_BAD_ARG
    for name in ("t", "e", "o"):
        assert call(8, 8, 16, **{name: None}) == _lib.SVK_ERR_BAD_ARG and "NULL" in message()
    assert eng.lib.svk_cosine_scores(None, p(buf), p(buf), 8, 8, 16, p(out)) == _lib.SVK_ERR_BAD_ARG
    # an empty side: nothing is launched, no pointer is looked at, nothing is written
    out.fill_(7.0)
    assert call(0, 8, 16, t=None, e=None, o=None) == _lib.SVK_OK and call(8, 0, 16, t=None, e=None, o=None) == _lib.SVK_OK
    assert call(0, 8, 16) == _lib.SVK_OK and call(8, 0, 16) == _lib.SVK_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    x = torch.zeros((5, 16), dtype=torch.float32, device=eng.device)
    assert tuple(eng.cosine_scores(x[:0], x).shape) == (0, 5) and tuple(eng.cosine_scores(x, x[:0]).shape) == (5, 0)
    with pytest.raises(_lib.SvkError) as info:
        eng.cosine_scores(torch.zeros((2, 4097), device=eng.device), torch.zeros((3, 4097), device=eng.device))
    assert info.value.code == _lib.SVK_ERR_UNSUPPORTED
    with pytest.raises(_lib.SvkError) as info:
        eng.cosine_scores(x[:, :0], x[:, :0])
    assert info.value.code == _lib.SVK_ERR_BAD_ARG


def test_l2_dist_arguments(eng):
    """dim == 0 (include/svk.h): the rows are empty, every distance is 0 and the input pointers -- NULL for an empty
    tensor -- are not looked at."""
    from speaker_verification_amd import _lib
    p = eng._ptr
    a = torch.zeros((6, 0), dtype=torch.float32, device=eng.device)
    got = eng.l2_dist(a, a.clone())
    assert got.dtype == torch.float32 and tuple(got.shape) == (6,) and bool((got == 0.0).all())
    out = torch.full((6,), 7.0, dtype=torch.float32, device=eng.device)
    assert eng.lib.svk_l2_dist(eng.ctx, None, None, 6, 0, p(out)) == _lib.SVK_OK
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())
    assert eng.lib.svk_l2_dist(eng.ctx, None, None, 6, 0, None) == _lib.SVK_ERR_BAD_ARG
    assert "NULL" in eng.lib.svk_last_error(eng.ctx).decode()
    x = torch.zeros((6, 4), dtype=torch.float32, device=eng.device)
    for args in ((None, p(x), 6, 4, p(out)), (p(x), None, 6, 4, p(out)), (p(x), p(x), 6, 4, None)):
        assert eng.lib.svk_l2_dist(eng.ctx, *args) == _lib.SVK_ERR_BAD_ARG
    for n, dim in ((-1, 4), (6, -1)):
        assert eng.lib.svk_l2_dist(eng.ctx, p(x), p(x), n, dim, p(out)) == _lib.SVK_ERR_BAD_ARG
    assert eng.lib.svk_l2_dist(eng.ctx, None, None, 0, 4, None) == _lib.SVK_OK
    assert tuple(eng.l2_dist(x[:0], x[:0]).shape) == (0,)
