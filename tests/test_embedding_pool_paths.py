"""svk_embedding_pool (csrc/pool.hip) on the instances with four and sixteen column chunks per thread (dim 257 - 1 024, and
above), and at the dims where the instance changes (256|257, 1 024|1 028).  CSR lengths [1, 2, 5, 0, 64, 65, 130] behind a
shuffled row index: an empty segment, the 64-row block exactly full, crossed once (65) and twice (130), and the remainders of
the 2-row load batches (1, 5, 65 rows: a last batch of one) next to full ones.  Every output is float32(ref64) or its neighbour
(test_embedding_pool.py derives the rule; tests/backend_f64_ref.py holds it), for the four flag values."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from backend_f64_ref import POOL_DIMS, POOL_LENGTHS, assert_f32_or_neighbour, csr, groups_of, pool_ref, rows       # noqa: E402


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def pool(eng, x, flags, **kw):
    return eng.embedding_pool(x, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2), **kw)


@pytest.mark.parametrize("dim", POOL_DIMS)
def test_wide_instances(eng, dim):
    start = csr(POOL_LENGTHS)
    n = int(start[-1])
    assert n == 267
    x = rows(n, dim, dim)
    index = np.random.default_rng(dim + 1).permutation(n).astype(np.int64)
    groups = groups_of(start, index)
    dev = eng.to_device(x)
    flat = torch.empty((x.size + 1,), dtype=torch.float32, device=eng.device)
    flat[1:] = dev.reshape(-1)
    odd = flat[1:].view(n, dim)
    assert dev.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4
    if dim == 257:          # 65 quads on a team of 64 threads, as dim 260 has
        padded = np.zeros((n, 260), dtype=np.float32)
        padded[:, :257] = x
    for flags in range(4):
        empty = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        got = pool(eng, dev, flags, seg_start=start, row_index=index, empty_count=empty)
        assert tuple(got.shape) == (len(POOL_LENGTHS), dim) and got.dtype == torch.float32 and int(empty) == 1
        assert torch.equal(pool(eng, dev, flags, seg_start=start, row_index=index), got), "a second run differs"
        assert torch.equal(pool(eng, odd, flags, seg_start=start, row_index=index), got), "the rows 4 bytes off give other bits"
        got = got.cpu().numpy()
        assert not got[3].view(np.uint32).any(), "the empty segment is not +0.0"
        assert_f32_or_neighbour(got, pool_ref(x, groups, flags), "dim %d flags %d" % (dim, flags))
        alone = pool(eng, x[groups[6]], flags, rows_per_seg=130).cpu().numpy()
        assert np.array_equal(alone[0].view(np.uint32), got[6].view(np.uint32)), "the 130-row segment alone has other bits"
        if dim == 257:
            wide = pool(eng, padded, flags, seg_start=start, row_index=index).cpu().numpy()
            assert np.array_equal(wide[:, :257].view(np.uint32), got.view(np.uint32)), "zero-padded to 260: other bits"
            assert not wide[:, 257:].any()
