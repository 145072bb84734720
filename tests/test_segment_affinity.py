"""svk_segment_affinity (csrc/cluster.hip): the cosines of every pair of live rows of every recording against float64.

THE BOUND.  The kernel forms x.y, x.x and y.y in float64 (a product of two float32 values is exact there, so each is a sum of
dim exact terms with one rounding per addition), two square roots, one product and one division.  A float64 sum of dim terms
in any order is off by at most (dim - 1) u sum |terms| with u = 2^-53, and sum |x_k y_k| <= ||x|| ||y|| (Cauchy-Schwarz), so the
dot product contributes at most (dim - 1) u to the cosine in ABSOLUTE terms; the norms are sums of non-negative terms (relative
error (dim - 1) u each, halved by the square root), and the roots, the product and the division add u each: the float64 value
the kernel rounds lies within (dim + 8) 2^-53 of the exact cosine.  The reference here is the same expression in np.longdouble
(a 64-bit significand on x86-64: its own error is (dim + 8) eps_ld / 2, 2^11 times smaller; where longdouble is float64 the same
formula doubles the allowance, which is then the reference's own error).  Rounding to float32 is monotonic, so every output is
float32(ref) or -- when ref lies within that distance of a rounding boundary -- the float next to it.  The test accepts exactly
those: got == float32(ref), or got is its neighbour AND ref is within (dim + 8) (2^-53 + eps_ld / 2) of the midpoint between
the two."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STRIDE = 40
N_SEG = [0, 1, 2, 17, STRIDE]
SENTINEL = -7.5


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def cosine_ref(x):
    """Extended-precision cosines of the rows of one recording; a zero norm divides by 1."""
    x = x.astype(np.longdouble)
    nrm = np.sqrt((x * x).sum(1))
    nrm = np.where(nrm == 0, 1.0, nrm)
    return (x @ x.T) / (nrm[:, None] * nrm[None, :])


def assert_f32_or_boundary_neighbour(got, ref64, dim, what):
    want = ref64.astype(np.float32)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    ld = np.longdouble
    tol = (dim + 8) * (ld(2.0) ** -53 + np.finfo(ld).eps / 2)
    with np.errstate(invalid="ignore"):
        near_up = (got == up) & (np.abs(ref64 - (want.astype(ld) + up.astype(ld)) / 2) <= tol)
        near_down = (got == down) & (np.abs(ref64 - (want.astype(ld) + down.astype(ld)) / 2) <= tol)
    ok = same | near_up | near_down
    print("%s: %d values, %d equal float32(ref64), %d boundary neighbours" % (what, got.size, int(same.sum()), int((ok & ~same).sum())))
    assert ok.all(), "%s: %d values are neither float32(ref64) nor its neighbour at a rounding boundary" % (what, int((~ok).sum()))


def batch(dim, seed):
    """[len(N_SEG), STRIDE, dim]: mixed-sign rows (cosines of every size), a zero row and a duplicated row in the full recording."""
    x = np.random.default_rng(seed).standard_normal((len(N_SEG), STRIDE, dim)).astype(np.float32)
    x[:, 1::3] += 1.5
    x[4, 5] = 0.0
    x[4, 9] = x[4, 8]
    return x


def run(eng, x, n_seg, out=None):
    if out is None:
        out = torch.full((x.shape[0], x.shape[1], x.shape[1]), SENTINEL, dtype=torch.float32, device=eng.device)
    return eng.segment_affinity(x, np.asarray(n_seg, np.int32), out=out).cpu().numpy()


def check_batch(got, x, n_seg, dim, what):
    for r, n in enumerate(n_seg):
        assert_f32_or_boundary_neighbour(got[r, :n, :n], cosine_ref(x[r, :n]), dim, "%s rec %d" % (what, r))
        assert np.array_equal(got[r].view(np.uint32), got[r].T.copy().view(np.uint32))            # symmetric bit for bit
        dead = np.ones((x.shape[1], x.shape[1]), bool)
        dead[:n, :n] = False
        assert (got[r][dead] == SENTINEL).all()                                                   # dead entries are not written


@pytest.fixture(scope="module")
def batch128(eng):
    x = batch(128, 1)
    return x, run(eng, x, N_SEG)


def test_affinity_against_float64_vector_path(batch128):
    x, got = batch128
    check_batch(got, x, N_SEG, 128, "dim 128")
    full = got[4]
    assert (full[5, :] == 0).all() and (full[:, 5] == 0).all()            # a zero row scores exactly 0, never NaN
    assert full[8, 9] == 1.0 and full[0, 0] == 1.0


@pytest.mark.parametrize("dim", [40, 3])
def test_affinity_against_float64_other_dims(eng, dim):
    x = batch(dim, 10 + dim)
    check_batch(run(eng, x, N_SEG), x, N_SEG, dim, "dim %d" % dim)


@pytest.mark.parametrize("dim", [128, 40, 3])
def test_affinity_load_paths_give_the_same_bits(eng, dim):
    """A base pointer that is only 4-byte aligned takes the 4-byte loads whatever dim is."""
    x = batch(dim, 20 + dim)
    aligned = run(eng, x, N_SEG)
    flat = torch.empty((x.size + 1,), dtype=torch.float32, device=eng.device)
    shifted = flat[1:].view(x.shape)
    shifted.copy_(torch.from_numpy(x))
    assert shifted.data_ptr() % 16 == 4
    out = torch.full((len(N_SEG), STRIDE, STRIDE), SENTINEL, dtype=torch.float32, device=eng.device)
    eng._stream()
    rc = eng.lib.svk_segment_affinity(eng.ctx, shifted.data_ptr(), len(N_SEG), STRIDE, dim,
                                      torch.tensor(N_SEG, dtype=torch.int32, device=eng.device).data_ptr(), out.data_ptr())
    assert rc == 0
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), aligned.view(np.uint32))
    check_batch(got, x, N_SEG, dim, "dim %d, 4-byte loads" % dim)


def test_affinity_nan_row_stays_in_its_row_and_column(eng, batch128):
    x, clean = batch128
    y = x.copy()
    y[4, 11, 77] = np.nan
    y[3, 30, 0] = np.nan                      # a dead row of recording 3 (17 live rows): never read
    got = run(eng, y, N_SEG)
    hit = np.zeros((STRIDE, STRIDE), bool)
    hit[11, :] = hit[:, 11] = True
    assert np.isnan(got[4][hit]).all()
    assert np.array_equal(got[4][~hit].view(np.uint32), clean[4][~hit].view(np.uint32))
    for r in range(4):
        assert np.array_equal(got[r].view(np.uint32), clean[r].view(np.uint32))


def test_affinity_alone_equals_batch_and_runs_are_identical(eng, batch128):
    x, got = batch128
    again = run(eng, x, N_SEG)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    # recording 3 alone, in another slot geometry: a tighter stride and no neighbours
    alone = run(eng, np.ascontiguousarray(x[3:4, :24]), [17])
    assert np.array_equal(alone[0, :17, :17].view(np.uint32), got[3, :17, :17].view(np.uint32))
    # and the last rows of the full recording as the FIRST rows of a short one: the bits depend on the two rows alone
    moved = run(eng, np.ascontiguousarray(x[4:5, 20:]), [20])
    assert np.array_equal(moved[0, :20, :20].view(np.uint32), got[4, 20:, 20:].view(np.uint32))


def test_affinity_arguments(eng):
    from speaker_verification_amd._lib import SvkError
    lib = eng.lib
    assert lib.svk_segment_affinity(None, None, 1, 4, 8, None, None) == -1
    assert lib.svk_segment_affinity(eng.ctx, None, 1, 4, 8, None, None) == -1
    assert lib.svk_segment_affinity(eng.ctx, None, -1, 4, 8, None, None) == -1
    assert lib.svk_segment_affinity(eng.ctx, None, 0, 4, 8, None, None) == 0             # looks at no pointer
    for dim in (0, 513):
        with pytest.raises((SvkError, RuntimeError)) as err:
            eng.segment_affinity(np.zeros((1, 4, dim), np.float32), [4])
        assert getattr(err.value, "code", -1) == -1
    # a count outside [0, stride] is clamped, not followed
    x = batch(8, 3)[:1]
    got = run(eng, x, [STRIDE + 100])
    assert_f32_or_boundary_neighbour(got[0], cosine_ref(x[0]), 8, "clamped count")
