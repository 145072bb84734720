"""svk_class_scatter (csrc/backend.hip) against an np.longdouble restatement: class means and the within-class scatter S_w of
CSR classes with and without a row index, both flag values, an empty and a one-row class, tile remainders (dim 40), several
chunks of rows (70 x 30), determinism, symmetry, NaN containment and the bad arguments.

THE BOUNDS (u = 2^-53; x is the row as it ENTERS, i.e. x / ||x|| under flag bit 0; m the class mean).
  * means:  |got - ref| <= (n_c + 2) u mean_i |x_i|.  A float64 sum of n_c terms in any order carries at most (n_c - 1) u sum |x|;
    the division by n_c and the row's own rounding (the normalisation) add the rest.
  * S_w:    |got_ab - ref_ab| <= (2 n_max + 8) u sum_i (|x_ia| + |m_a|)(|x_ib| + |m_b|), n_max the largest class.  A float64 mean
    of n terms carries n u |m|; each centred factor x - m carries that plus one rounding, so a product of two carries
    2 (n + 1) u (|x_a| + |m_a|)(|x_b| + |m_b|) to first order; a sum of products in any order carries n u sum |.| on top, and
    sum |d_a d_b| is far below the sum of (|x| + |m|)(|x| + |m|) that the bound is stated in (inputs are N(0, 1) + 3).
The reference is np.longdouble (64-bit mantissa on x86: 2^11 times finer than what is bounded)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backend_f64_ref import rows, scatter_ref       # noqa: E402  (tests/ is on sys.path)

LENGTHS = [1, 2, 7, 0, 300, 65]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def C_off(t, nbytes):
    """the tensor's address moved by nbytes: a misaligned pointer"""
    return ctypes.c_void_p(t.data_ptr() + nbytes)


def check(got_mean, got_sw, ref, what):
    means, sw, mean_bound, sw_bound = ref
    em = np.abs(got_mean.astype(np.longdouble) - means).astype(np.float64)
    es = np.abs(got_sw.astype(np.longdouble) - sw).astype(np.float64)
    print("%s: worst mean error / bound = %.3f, worst S_w error / bound = %.4f"
          % (what, float((em / np.maximum(mean_bound, 1e-300)).max()), float((es / sw_bound).max())))
    assert (em <= mean_bound).all(), "%s: %d class means outside the bound" % (what, int((em > mean_bound).sum()))
    assert (es <= sw_bound).all(), "%s: %d entries of S_w outside the bound" % (what, int((es > sw_bound).sum()))


def run(eng, x, start, index=None, flags=0):
    mean, sw = eng.class_scatter(x, start, row_index=index, l2_rows=bool(flags & 1))
    return mean.cpu().numpy(), sw.cpu().numpy()


@pytest.mark.parametrize("dim", [128, 40])
@pytest.mark.parametrize("shuffled", [False, True])
def test_csr_classes(eng, dim, shuffled):
    start = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    n = int(start[-1])
    x = rows(n, dim, 1)
    x[5] = 0.0                                                    # a zero row in the 7-row class
    index = np.random.default_rng(2).permutation(n).astype(np.int64) if shuffled else None
    look = index if shuffled else np.arange(n)
    groups = [look[start[s]:start[s + 1]] for s in range(len(LENGTHS))]
    dev = eng.to_device(x)
    for flags in (0, 1):
        mean, sw = run(eng, dev, start, index, flags)
        assert mean.shape == (len(LENGTHS), dim) and sw.shape == (dim, dim) and mean.dtype == sw.dtype == np.float64
        check(mean, sw, scatter_ref(x, groups, flags), "csr dim %d shuffled %d flags %d" % (dim, shuffled, flags))
        assert np.array_equal(sw, sw.T)                                           # symmetric bit for bit
        assert not mean[3].any()                                                  # the empty class: zeros
        mean2, sw2 = run(eng, dev, start, index, flags)
        assert np.array_equal(mean, mean2) and np.array_equal(sw, sw2)            # two runs: equal bits
        # the 300-row class alone: the mean bits it has inside the batch
        alone, _ = run(eng, x[groups[4]], np.array([0, 300], dtype=np.int64), None, flags)
        assert np.array_equal(alone[0], mean[4])
        # without the one-row class: S_w keeps its bits (a class of one row contributes exactly zero)
        look1 = np.concatenate(groups[1:] + [groups[0]]).astype(np.int64)         # its row now lies outside every class
        mean_wo, sw_wo = run(eng, dev, start[1:] - 1, look1, flags)
        assert np.array_equal(sw_wo, sw) and np.array_equal(mean_wo, mean[1:])
        # ... and so does it without the empty class
        keep = [0, 1, 2, 4, 5]
        start_k = np.concatenate([[0], np.cumsum([LENGTHS[c] for c in keep])]).astype(np.int64)
        mean_k, sw_k = run(eng, dev, start_k, look.astype(np.int64), flags)
        assert np.array_equal(sw_k, sw) and np.array_equal(mean_k, mean[keep])


def test_several_chunks(eng):
    """70 classes x 30 rows of dim 128: 2 100 rows are five chunks of 512 -- five partial matrices combined in order."""
    n_class, per, dim = 70, 30, 128
    x = rows(n_class * per, dim, 3)
    index = np.random.default_rng(4).permutation(n_class * per).astype(np.int64)
    start = (np.arange(n_class + 1) * per).astype(np.int64)
    groups = [index[start[s]:start[s + 1]] for s in range(n_class)]
    dev = eng.to_device(x)
    for flags in (0, 1):
        mean, sw = run(eng, dev, start, index, flags)
        check(mean, sw, scatter_ref(x, groups, flags), "70 x 30 flags %d" % flags)
        mean2, sw2 = run(eng, dev, start, index, flags)
        assert np.array_equal(sw, sw.T) and np.array_equal(sw, sw2) and np.array_equal(mean, mean2)


def test_wide_rows(eng):
    """dim 200 (13 column blocks, 91 tiles: three tile groups and the wide staging) in 8 classes x 5 rows."""
    x = rows(40, 200, 5)
    start = (np.arange(9) * 5).astype(np.int64)
    groups = [np.arange(5 * s, 5 * s + 5) for s in range(8)]
    mean, sw = run(eng, x, start, None, 1)
    check(mean, sw, scatter_ref(x, groups, 1), "dim 200")
    assert np.array_equal(sw, sw.T)


def test_nan_stays_in_its_column(eng):
    x = rows(24, 128, 6)
    x[9, 17] = np.nan                                             # class 1 (rows 8 .. 15), column 17
    start = (np.arange(4) * 8).astype(np.int64)
    mean, sw = run(eng, x, start, None, 0)
    want = np.zeros((3, 128), dtype=bool)
    want[1, 17] = True
    assert np.array_equal(np.isnan(mean), want)
    nan_sw = np.zeros((128, 128), dtype=bool)
    nan_sw[17, :] = nan_sw[:, 17] = True
    assert np.array_equal(np.isnan(sw), nan_sw)
    # flag bit 0: the row's norm is NaN and so is the whole row -> every column of that class's mean, all of S_w; the other
    # classes' means stay finite
    mean, sw = run(eng, x, start, None, 1)
    assert np.isnan(mean[1]).all() and np.isfinite(mean[[0, 2]]).all() and np.isnan(sw).all()
    # a row index outside the rows: not read, its class NaN
    index = np.arange(24, dtype=np.int64)
    index[20] = 24
    mean, sw = run(eng, rows(24, 128, 6), start, index, 0)
    assert np.isnan(mean[2]).all() and np.isfinite(mean[:2]).all() and np.isnan(sw).all()


def test_bad_arguments(eng):
    from speaker_verification_amd import _lib
    x = eng.to_device(rows(8, 128, 7))
    start = eng.to_device(np.array([0, 4, 8], dtype=np.int64))
    need = int(eng.lib.svk_class_scatter_workspace_bytes(8, 128, 2))
    assert need > 0 and need % 16 == 0
    assert eng.lib.svk_class_scatter_workspace_bytes(8, 0, 2) == 0 and eng.lib.svk_class_scatter_workspace_bytes(8, 513, 2) == 0
    assert eng.lib.svk_class_scatter_workspace_bytes(-1, 128, 2) == 0 and eng.lib.svk_class_scatter_workspace_bytes(8, 128, 0) == 0
    work = torch.empty((need + 16,), dtype=torch.uint8, device=eng.device)
    mean = torch.empty((2, 128), dtype=torch.float64, device=eng.device)
    sw = torch.full((128, 128), 7.0, dtype=torch.float64, device=eng.device)
    call = lambda *a: eng.lib.svk_class_scatter(eng.ctx, *a)        # noqa: E731
    p = eng._ptr
    OK, BAD = _lib.SVK_OK, _lib.SVK_ERR_BAD_ARG
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == OK
    assert eng.lib.svk_class_scatter(None, p(x), 8, 128, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD
    assert call(None, 8, 128, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD          # NULL rows
    assert call(p(x), 8, 128, None, None, 2, 0, p(work), need, p(mean), p(sw)) == BAD              # NULL offsets
    assert call(p(x), 8, 128, p(start), None, 2, 0, None, need, p(mean), p(sw)) == BAD             # NULL workspace
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need, None, p(sw)) == BAD             # NULL means
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need, p(mean), None) == BAD           # NULL S_w
    assert call(p(x), -1, 128, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD
    assert call(p(x), 8, 128, p(start), None, -1, 0, p(work), need, p(mean), p(sw)) == BAD
    assert call(p(x), 8, 0, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD
    assert call(p(x), 8, 513, p(start), None, 2, 0, p(work), 1 << 30, p(mean), p(sw)) == BAD
    assert call(p(x), 8, 128, p(start), None, 2, 2, p(work), need, p(mean), p(sw)) == BAD          # an undefined flag bit
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need - 16, p(mean), p(sw)) == BAD     # a short workspace
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work[8:]), need, p(mean), p(sw)) == BAD      # workspace off 16 bytes
    assert call(C_off(x, 2), 8, 128, p(start), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD   # rows off 4 bytes
    assert call(p(x), 8, 128, C_off(start, 4), None, 2, 0, p(work), need, p(mean), p(sw)) == BAD   # offsets off 8 bytes
    index = eng.to_device(np.arange(9, dtype=np.int64))
    assert call(p(x), 8, 128, p(start), p(index), 2, 0, p(work), need, p(mean), p(sw)) == OK
    assert call(p(x), 8, 128, p(start), C_off(index, 4), 2, 0, p(work), need, p(mean), p(sw)) == BAD  # row index off 8 bytes
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need, C_off(mean, 4), p(sw)) == BAD
    assert call(p(x), 8, 128, p(start), None, 2, 0, p(work), need, p(mean), C_off(sw, 4)) == BAD
    # n_class == 0: a zero S_w and nothing else (no offsets, means or workspace needed)
    assert call(p(x), 8, 128, None, None, 0, 0, None, 0, None, p(sw)) == OK
    torch.cuda.synchronize()
    assert not sw.cpu().numpy().any()

