"""svk_embedding_project (csrc/backend.hip) against a float64 restatement: y = l2((l2(x) - mu) W) over row counts around the
16-row wave tile, full and ragged output tiles, every tile-count instance (1 to 32 tiles), dims that are no multiple of 4 or
16, the four flag values, mu and W given or NULL.

THE BOUND, un-normalised output (flag bit 1 clear).  x' is rounded to f32 once (2^-24 relative), the subtraction x' - mu once
(2^-24 of at most |x'| + |mu|), each product c_k W_kj once, and an f32 sum of dim terms in any order carries (dim - 1) 2^-24 of
the sum of the magnitudes; to first order every term is below 2^-24 sum_k (|x'_k| + |mu_k|) |W_kj|, so
    |got_j - ref_j| <= (dim + 8) 2^-24 sum_k (|x'_k| + |mu_k|) |W_kj|
with a headroom of 6 for the second-order terms and for an x' whose float64 norm was summed in another order (it can move x' by
one rounding).  NORMALISED output: y is the SAME call's un-normalised output (the contract: the same bits under both flags)
widened to float64; the kernel's float64 sum of squares, square root and division differ from NumPy's by a few 2^-53, so every
element is float32(y / ||y||) or -- when that lies within 2^-50 of a rounding boundary -- the float next to it."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backend_f64_ref import assert_f32_or_neighbour, l2_f32, project_ref, rows, unit_rows       # noqa: E402  (tests/ is on sys.path)

N_ROWS = (1, 15, 16, 17, 300)
# the issue's five shapes, then one for each tile-count instance they do not reach: 2 tiles (40, 20), 16 (300, 200), 32 (512, 300)
SHAPES = [(128, 128), (128, 50), (128, 1), (40, 13), (130, 7), (40, 20), (300, 200), (512, 300)]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.mark.parametrize("dim,out_dim", SHAPES)
def test_shapes_and_flags(eng, dim, out_dim):
    rng = np.random.default_rng(100 + dim + out_dim)
    w = (rng.standard_normal((dim, out_dim)) / np.sqrt(dim)).astype(np.float32)
    dw = eng.to_device(w)
    worst = 0.0
    for n in N_ROWS:
        x = rows(n, dim, n)
        mu = x.mean(0).astype(np.float32)
        dx = eng.to_device(x)
        for mean in (None, mu):
            for flags in (0, 1):
                got = eng.embedding_project(dx, mean=mean, w=dw, l2_in=bool(flags & 1)).cpu().numpy()
                assert got.shape == (n, out_dim) and got.dtype == np.float32
                ref, bound = project_ref(x, mean, w, flags)
                err = np.abs(got.astype(np.float64) - ref)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), "n %d flags %d mean %s: %d outside the bound" % (n, flags, mean is not None, int((err > bound).sum()))
                unit = eng.embedding_project(dx, mean=mean, w=dw, l2_in=bool(flags & 1), l2_out=True).cpu().numpy()
                assert_f32_or_neighbour(unit, unit_rows(got), "n %d flags %d" % (n, flags | 2))
    print("dim %d -> %d: worst error / bound = %.4f" % (dim, out_dim, worst))


def test_identity(eng):
    """NULL W at (128, 128): float32(x' - mu) exactly, through no matrix pipe; and at dim 130 (no 16-byte loads)."""
    for dim in (128, 130):
        x = rows(300, dim, 21)
        x[11] = 0.0
        mu = x.mean(0).astype(np.float32)
        for mean in (None, mu):
            m = np.zeros(dim, dtype=np.float32) if mean is None else mean
            for flags in (0, 1):
                want = (l2_f32(x) if flags & 1 else x) - m
                got = eng.embedding_project(x, mean=mean, l2_in=bool(flags & 1)).cpu().numpy()
                assert np.array_equal(got, want), "dim %d flags %d" % (dim, flags)
                unit = eng.embedding_project(x, mean=mean, l2_in=bool(flags & 1), l2_out=True).cpu().numpy()
                assert_f32_or_neighbour(unit, unit_rows(got), "identity dim %d flags %d" % (dim, flags | 2))


def test_row_alone_and_misaligned(eng):
    for dim, out_dim in ((128, 50), (40, 13)):
        x = rows(300, dim, 31)
        mu = x.mean(0).astype(np.float32)
        w = eng.to_device((np.random.default_rng(32).standard_normal((dim, out_dim)) / np.sqrt(dim)).astype(np.float32))
        dx = eng.to_device(x)
        for flags in range(4):
            kw = dict(mean=mu, w=w, l2_in=bool(flags & 1), l2_out=bool(flags & 2))
            got = eng.embedding_project(dx, **kw)
            assert torch.equal(eng.embedding_project(dx, **kw), got)                      # two runs: equal bits
            for r in (0, 7, 299):                                                         # a row alone: its in-batch bits
                assert torch.equal(eng.embedding_project(dx[r:r + 1], **kw)[0], got[r])
            # the same rows through a view shifted by one float (4-byte loads): the bits of the aligned one
            flat = torch.empty((x.size + 1,), dtype=torch.float32, device=eng.device)
            flat[1:] = dx.reshape(-1)
            odd = flat[1:].view(300, dim)
            assert odd.data_ptr() % 16 == 4
            assert torch.equal(eng.embedding_project(odd, **kw), got)


def test_zero_and_nan_rows(eng):
    dim, out_dim = 128, 50
    x = rows(40, dim, 41)
    mu = x.mean(0).astype(np.float32)
    x[3] = mu                                           # c = 0 -> y = 0: stays zero under bit 1
    w = (np.random.default_rng(42).standard_normal((dim, out_dim)) / np.sqrt(dim)).astype(np.float32)
    got = eng.embedding_project(x, mean=mu, w=w, l2_out=True).cpu().numpy()
    assert not got[3].any() and np.isfinite(got).all()
    assert not eng.embedding_project(x, mean=mu, l2_out=True).cpu().numpy()[3].any()          # identity path
    z = x.copy()
    z[5] = 0.0                                          # a zero row under bit 0: zeros, then -mu
    ref, bound = project_ref(z, mu, w, 1)
    got = eng.embedding_project(z, mean=mu, w=w, l2_in=True).cpu().numpy()
    assert (np.abs(got - ref) <= bound).all()
    clean = eng.embedding_project(z, mean=mu, w=w, l2_in=True, l2_out=True).cpu().numpy()
    z[18, 77] = np.nan
    for flags in range(4):
        a = eng.embedding_project(z, mean=mu, w=w, l2_in=bool(flags & 1), l2_out=bool(flags & 2)).cpu().numpy()
        assert np.isnan(a[18]).all() and np.isfinite(np.delete(a, 18, axis=0)).all()
        i = eng.embedding_project(z, mean=mu, l2_in=bool(flags & 1), l2_out=bool(flags & 2)).cpu().numpy()
        assert np.isnan(i[18, 77]) and np.isfinite(np.delete(i, 18, axis=0)).all()
    assert np.array_equal(np.delete(a, 18, axis=0), np.delete(clean, 18, axis=0))             # the other rows keep their bits


def test_bad_arguments(eng):
    from speaker_verification_amd import _lib
    x = eng.to_device(rows(8, 128, 51))
    mu = eng.to_device(np.zeros(128, dtype=np.float32))
    w = eng.to_device(np.zeros((128, 50), dtype=np.float32))
    out = torch.empty((8, 128), dtype=torch.float32, device=eng.device)
    call = lambda *a: eng.lib.svk_embedding_project(eng.ctx, *a)    # noqa: E731
    p = eng._ptr
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 2)               # noqa: E731
    OK, BAD = _lib.SVK_OK, _lib.SVK_ERR_BAD_ARG
    assert call(p(x), 8, 128, p(mu), p(w), 50, 3, p(out)) == OK
    assert call(p(x), 8, 128, None, None, 128, 0, p(out)) == OK
    assert call(None, 0, 128, None, None, 128, 0, None) == OK                           # n_rows == 0: nothing to launch
    assert eng.lib.svk_embedding_project(None, p(x), 8, 128, p(mu), p(w), 50, 0, p(out)) == BAD
    assert call(None, 8, 128, p(mu), p(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 128, p(mu), p(w), 50, 0, None) == BAD
    assert call(p(x), -1, 128, p(mu), p(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 0, p(mu), p(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 513, p(mu), p(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 128, p(mu), p(w), 0, 0, p(out)) == BAD
    assert call(p(x), 8, 128, p(mu), p(w), 129, 0, p(out)) == BAD                       # out_dim > dim
    assert call(p(x), 8, 128, p(mu), None, 50, 0, p(out)) == BAD                        # the identity wants out_dim == dim
    assert call(p(x), 8, 128, p(mu), p(w), 50, 4, p(out)) == BAD                        # an undefined flag bit
    assert call(p(x), 8, 128, None, None, 128, 0, p(x)) == BAD                          # d_out == d_emb
    assert call(off(x), 8, 128, p(mu), p(w), 50, 0, p(out)) == BAD                      # misaligned
    assert call(p(x), 8, 128, off(mu), p(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 128, p(mu), off(w), 50, 0, p(out)) == BAD
    assert call(p(x), 8, 128, p(mu), p(w), 50, 0, off(out)) == BAD
    torch.cuda.synchronize()
