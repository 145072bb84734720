"""svk_embedding_pool (csrc/pool.hip) against a float64 NumPy restatement: CSR and uniform segments, a row index, the four flag
values, an empty segment, a zero row, a NaN row, determinism; and pipeline.enroll_mean on top of it.

THE BOUND.  Inputs are N(0, 1) + 3, so the terms of every sum share a sign-dominant offset and no sum cancels: |sum| is of
the order of sum |x|.  Adding n float64 numbers in any order has an error of at most (n - 1) u sum |x| with u = 2^-53, so the
kernel's float64 sum and the reference's differ by at most ~2 n u |sum| -- for n = 300 that is 2^-43 |sum|, 2^20 times below one
float32 rounding (2^-24).  The division by the count, the row norms (sums of squares: no cancellation at all), the square
roots and the divisions by them add a few u each.  The float64 value the kernel rounds is therefore within ~2^-40 relative
of ref64, and rounding to float32 is monotonic: the result is float32(ref64), or -- when ref64 lies within 2^-40 of a rounding
boundary -- the float next to it.  Every output must be one of those two."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backend_f64_ref import assert_f32_or_neighbour, pool_ref, rows       # noqa: E402  (tests/ is on sys.path)

LENGTHS = [1, 2, 7, 0, 300]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.mark.parametrize("dim", [128, 40])
@pytest.mark.parametrize("shuffled", [False, True])
def test_csr_segments(eng, dim, shuffled):
    start = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    n = int(start[-1])
    x = rows(n, dim, 1)
    x[4] = 0.0                                                    # a zero row in the 7-row segment
    index = np.random.default_rng(2).permutation(n).astype(np.int64) if shuffled else None
    look = index if shuffled else np.arange(n)
    groups = [look[start[s]:start[s + 1]] for s in range(len(LENGTHS))]
    dev = eng.to_device(x)
    for flags in range(4):
        empty = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        got = eng.embedding_pool(dev, seg_start=start, row_index=index, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2),
                                 empty_count=empty)
        again = eng.embedding_pool(dev, seg_start=start, row_index=index, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2))
        assert tuple(got.shape) == (len(LENGTHS), dim) and int(empty) == 1 and torch.equal(got, again)
        got = got.cpu().numpy()
        assert not got[3].any()                                                   # the empty segment: zeros
        assert_f32_or_neighbour(got, pool_ref(x, groups, flags), "csr dim %d shuffled %d flags %d" % (dim, shuffled, flags))
        # the 300-row segment pooled alone: the bits it has inside the batch
        long_rows = groups[4]
        alone = eng.embedding_pool(eng.to_device(x[long_rows]), rows_per_seg=300, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2))
        assert np.array_equal(alone.cpu().numpy()[0], got[4])


@pytest.mark.parametrize("dim", [128, 40])
@pytest.mark.parametrize("shuffled", [False, True])
def test_uniform_segments(eng, dim, shuffled):
    K, n_seg = 4, 37                                    # 37 segments: more than one workgroup of 8 (dim 128) or 16 (dim 40)
    x = rows(K * n_seg, dim, 3)
    index = np.random.default_rng(4).permutation(K * n_seg).astype(np.int64) if shuffled else None
    look = index if shuffled else np.arange(K * n_seg)
    groups = [look[K * s:K * s + K] for s in range(n_seg)]
    dev = eng.to_device(x)
    for flags in range(4):
        got = eng.embedding_pool(dev, rows_per_seg=K, row_index=index, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2))
        assert_f32_or_neighbour(got.cpu().numpy(), pool_ref(x, groups, flags), "uniform dim %d shuffled %d flags %d" % (dim, shuffled, flags))
    # the same rows through a misaligned view (row 1 of a dim 40 or 128 matrix is 16-byte aligned; shift by one float instead)
    flat = torch.empty((x.size + 1,), dtype=torch.float32, device=eng.device)
    flat[1:] = dev.reshape(-1)
    odd = flat[1:].view(K * n_seg, dim)
    assert odd.data_ptr() % 16 == 4
    assert torch.equal(eng.embedding_pool(odd, rows_per_seg=K, l2_rows=True, l2_mean=True),
                       eng.embedding_pool(dev, rows_per_seg=K, l2_rows=True, l2_mean=True))


def test_zero_row_and_nan_row(eng):
    x = rows(12, 128, 5)
    x[1] = 0.0                                          # segment 0: a zero row enters as zeros under bit 0
    x[6, 17] = np.nan                                   # segment 1: NaN
    groups = [np.arange(4 * s, 4 * s + 4) for s in range(3)]
    for flags in range(4):
        got = eng.embedding_pool(x, rows_per_seg=4, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2)).cpu().numpy()
        ref = pool_ref(x, groups, flags)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()                      # NaN stays in its own segment
        assert np.isnan(got[1, 17]) and (np.isnan(got[1]).all() if flags else np.isnan(got[1]).sum() == 1)
        assert_f32_or_neighbour(got[[0, 2]], ref[[0, 2]], "zero / NaN rows, flags %d" % flags)
    # an all-zero segment: the zero mean stays zero under bit 1
    z = np.zeros((4, 128), dtype=np.float32)
    assert not eng.embedding_pool(z, rows_per_seg=4, l2_rows=True, l2_mean=True).cpu().numpy().any()


def test_bad_arguments(eng):
    from speaker_verification_amd import _lib
    x = eng.to_device(rows(8, 128, 6))
    out = torch.empty((2, 128), dtype=torch.float32, device=eng.device)
    call = lambda *a: eng.lib.svk_embedding_pool(eng.ctx, *a)       # noqa: E731
    p = eng._ptr
    assert call(p(x), 8, 128, 2, 4, None, None, 0, p(out), None) == _lib.SVK_OK
    assert call(p(x), 8, 128, 0, 4, None, None, 0, None, None) == _lib.SVK_OK               # n_seg == 0: nothing to launch
    assert call(p(x), 8, 128, 2, 0, None, None, 0, p(out), None) == _lib.SVK_ERR_BAD_ARG    # rows_per_seg < 1
    assert call(p(x), 8, 128, 3, 4, None, None, 0, p(out), None) == _lib.SVK_ERR_BAD_ARG    # 3 x 4 rows > 8
    assert call(p(x), 8, 0, 2, 4, None, None, 0, p(out), None) == _lib.SVK_ERR_BAD_ARG
    assert call(p(x), 8, 4097, 2, 4, None, None, 0, p(out), None) == _lib.SVK_ERR_BAD_ARG
    assert call(p(x), 8, 128, 2, 4, None, None, 4, p(out), None) == _lib.SVK_ERR_BAD_ARG    # an undefined flag bit
    assert call(p(x), 8, 128, 2, 4, None, None, 0, None, None) == _lib.SVK_ERR_BAD_ARG      # NULL output
    assert call(p(x), -1, 128, 2, 4, None, None, 0, p(out), None) == _lib.SVK_ERR_BAD_ARG
    torch.cuda.synchronize()


def test_wide_rows(eng):
    """dim 300 (75 quads over a team of 64 threads: two chunks per thread, the second partly empty), dim 4096 (sixteen chunks) and
    dim 301 (no 16-byte loads, a ragged last quad)."""
    for dim in (300, 4096, 301):
        x = rows(9, dim, 7)
        groups = [np.arange(3 * s, 3 * s + 3) for s in range(3)]
        got = eng.embedding_pool(x, rows_per_seg=3, l2_rows=True, l2_mean=True).cpu().numpy()
        assert_f32_or_neighbour(got, pool_ref(x, groups, 3), "dim %d" % dim)


def test_enroll_mean(eng):
    from speaker_verification_amd.pipeline import enroll_mean
    rng = np.random.default_rng(8)
    ids = rng.permutation(np.repeat(np.array(["id3", "id1", "id7", "id2"]), [5, 1, 70, 3]))
    x = rows(len(ids), 128, 9)
    for l2 in (True, False):
        uniq, models = enroll_mean(x, ids, l2=l2)
        assert list(uniq) == sorted(set(ids)) and tuple(models.shape) == (4, 128) and models.is_cuda
        groups = [np.nonzero(ids == sid)[0] for sid in uniq]
        assert_f32_or_neighbour(models.cpu().numpy(), pool_ref(x, groups, int(l2)), "enroll_mean l2 %d" % l2)
