"""svk_cohort_moments against tests/snorm_f64_ref.py: the selection exactly (d_used and d_kth equal the reference's m and v*
to the bit), the moments within the header's bounds (A from the order of additions: ref.additions), the special cases
exactly, and the same bits across load widths, batch positions, runs and every top_k >= n_cohort.

Every shape carries rows of every kind of ref.KINDS (row i of shape number s is kind (i + s) % 8), so that a one-row matrix
still meets them all over the shapes; the kinds that are special cases have tests of their own as well."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_f64_ref as ref  # noqa: E402

LD, L = ref.LD, ref.ROW_LDS_MAX
W = ref.WAVE_ROW_MAX            # W | W + 1: a wave's row | a workgroup's;  L | L + 1: a row kept in LDS | re-read in every pass
COHORTS = [1, 2, 63, 64, 65, 255, 256, 257, 1211, W, W + 1, L, L + 1, L + 257]
ROWS = [1, 3, 17, 130]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def top_ks(n):
    return sorted({k for k in (0, 1, 2, 300, n - 1, n, n + 5) if k >= 0})


def matrix(n_rows, n, shape_no, seed):
    rng = np.random.default_rng(seed)
    kinds = [ref.KINDS[(i + shape_no) % len(ref.KINDS)] for i in range(n_rows)]
    return np.stack([ref.make_row(rng, n, kind) for kind in kinds]), kinds


def run(eng, view, top_k):
    mom, used, kth = eng.cohort_moments(view, top_k, want_used=True, want_kth=True)
    return mom.cpu().numpy(), used.cpu().numpy(), kth.cpu().numpy()


def vec_layout(eng, mat):
    """Rows a multiple of four floats apart from a 16-byte aligned base: the 16-byte loads."""
    view = ref.place_rows(eng, mat, (mat.shape[1] + 3) // 4 * 4, 0)
    assert view.data_ptr() % 16 == 0
    return view


def scalar_layout(eng, mat):
    view = ref.place_rows(eng, mat, mat.shape[1] + 3, 1)
    assert view.data_ptr() % 16 == 4
    return view


def check_rows(mat, top_k, mom, used, kth, what):
    """Selection exact, moments within the header's bounds, special cases exact -> the widest ratio error / bound seen."""
    n = mat.shape[1]
    worst = 0.0
    for i in range(mat.shape[0]):
        m, vstar, r = ref.row_reference(mat[i], top_k)
        tag = "%s, row %d" % (what, i)
        assert int(used[i]) == m, tag
        assert kth[i].tobytes() == np.float32(vstar).tobytes() or (m == 0 and np.isnan(kth[i])), tag
        mean, sd = mom[i]
        if m == 0:
            assert np.isnan(mean) and np.isnan(sd), tag
            continue
        if r["sum_d2"] == 0:                                  # all selected values equal: the value, +0.0, exactly
            assert mean == np.float64(vstar) and sd == 0.0 and not np.signbit(sd), tag
            assert not (mean == 0 and np.signbit(mean)), tag
            continue
        dm, dv = ref.moment_bounds(r, n)
        e_mean, e_var = abs(LD(mean) - r["mean"]), abs(LD(sd) * LD(sd) - r["var"])
        assert e_mean <= dm and e_var <= dv and sd >= 0, "%s: mean off by %.3g (bound %.3g), std^2 by %.3g (bound %.3g)" % (
            tag, e_mean, dm, e_var, dv)
        worst = max(worst, float(e_mean / dm), float(e_var / dv))
    return worst


@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("n", COHORTS)
def test_selection_exact_moments_within_bounds_same_bits_everywhere(eng, n, n_rows):
    shape_no = COHORTS.index(n) * len(ROWS) + ROWS.index(n_rows)
    mat, kinds = matrix(n_rows, n, shape_no, 7000 + shape_no)
    vec, scalar = vec_layout(eng, mat), scalar_layout(eng, mat)
    alone_at = n_rows // 2
    alone = vec_layout(eng, mat[alone_at:alone_at + 1])
    worst, whole = 0.0, None
    for top_k in top_ks(n):
        mom, used, kth = run(eng, vec, top_k)
        worst = max(worst, check_rows(mat, top_k, mom, used, kth, "n = %d, top_k = %d (%s)" % (n, top_k, kinds)))
        bits = (mom.tobytes(), used.tobytes(), kth.tobytes())
        again, other = run(eng, vec, top_k), run(eng, scalar, top_k)
        assert tuple(a.tobytes() for a in again) == bits                      # a second run
        assert tuple(a.tobytes() for a in other) == bits                      # 4-byte loads, rows n + 3 apart, base 4 off 16
        one = run(eng, alone, top_k)                                          # the row alone: the bits it has in the batch
        assert one[0].tobytes() == mom[alone_at:alone_at + 1].tobytes()
        assert one[1][0] == used[alone_at] and one[2].tobytes() == kth[alone_at:alone_at + 1].tobytes()
        if top_k == 0:
            whole = bits
        elif top_k >= n:
            assert bits == whole                                              # top_k >= n_cohort: top_k = 0's bits
    print("n_cohort %d x %d rows: worst error / bound = %.3f" % (n, n_rows, worst))


@pytest.mark.parametrize("n", [1, 63, 257, 1211, W + 1, L + 1])
def test_special_rows(eng, n):
    rng = np.random.default_rng(n)
    kinds = ["all_equal", "zeros", "no_finite", "few_finite", "all_equal"]
    mat = np.stack([ref.make_row(rng, n, kind) for kind in kinds])
    mat[4] = np.float32(-0.0)
    value = mat[0, 0]
    for top_k in (0, 1, 300):
        mom, used, kth = run(eng, vec_layout(eng, mat), top_k)
        check_rows(mat, top_k, mom, used, kth, "n = %d, top_k = %d" % (n, top_k))
        full = n if top_k == 0 else min(top_k, n)
        assert mom[0, 0] == np.float64(value) and mom[0, 1].tobytes() == np.float64(0.0).tobytes() and used[0] == full
        for i in (1, 4):                                      # zeros of either sign: +0.0 everywhere
            assert mom[i].tobytes() == np.zeros(2).tobytes() and kth[i].tobytes() == np.float32(0.0).tobytes() and used[i] == full
        assert np.isnan(mom[2]).all() and used[2] == 0 and np.isnan(kth[2])
        finite = int(np.isfinite(mat[3]).sum())
        assert finite == min(3, n) and used[3] == (finite if top_k == 0 else min(top_k, finite))   # fewer candidates than top_k


@pytest.mark.parametrize("n", [257, 1211, W + 1, L + 1])
def test_permuting_a_tie_heavy_row_moves_no_selection_bit(eng, n):
    rng = np.random.default_rng(3 * n)
    row = ref.tie_heavy_row(rng, n)
    mat = np.stack([row] + [row[rng.permutation(n)] for _ in range(6)])
    for top_k in (2, 300, n // 2, n - 1):
        mom, used, kth = run(eng, vec_layout(eng, mat), top_k)
        check_rows(mat, top_k, mom, used, kth, "n = %d, top_k = %d" % (n, top_k))
        assert np.all(used == used[0]) and kth.tobytes() == np.repeat(kth[:1], len(kth)).tobytes()
        m, _, r = ref.row_reference(row, top_k)
        if r["sum_d2"] == 0:
            assert mom.tobytes() == np.tile(mom[:1], (len(mom), 1)).tobytes()
            continue
        dm, dv = ref.moment_bounds(r, n)
        assert np.all(np.abs(mom[:, 0].astype(LD) - LD(mom[0, 0])) <= dm)
        assert np.all(np.abs(mom[:, 1].astype(LD) ** 2 - LD(mom[0, 1]) ** 2) <= dv)


def test_optional_outputs_and_empty_input(eng):
    mat = np.random.default_rng(5).standard_normal((9, 70)).astype(np.float32)
    both = eng.cohort_moments(mat, 10, want_used=True, want_kth=True)
    only = eng.cohort_moments(mat, 10)
    assert isinstance(only, torch.Tensor) and only.dtype == torch.float64 and tuple(only.shape) == (9, 2)
    assert torch.equal(only, both[0])
    used_only = eng.cohort_moments(mat, 10, want_used=True)
    assert used_only[2] is None and torch.equal(used_only[1], both[1]) and torch.equal(used_only[0], only)
    empty = eng.cohort_moments(torch.zeros((0, 70), dtype=torch.float32, device=eng.device), 10)
    assert tuple(empty.shape) == (0, 2)


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    lib, n_rows, n = eng.lib, 6, 100
    sc = vec_layout(eng, np.random.default_rng(1).standard_normal((n_rows, n)).astype(np.float32))
    mom = torch.empty((n_rows, 2), dtype=torch.float64, device=eng.device)
    used = torch.empty((n_rows + 1,), dtype=torch.int32, device=eng.device)
    kth = torch.empty((n_rows + 1,), dtype=torch.float32, device=eng.device)

    def call(**kw):
        a = dict(ctx=eng.ctx, scores=sc.data_ptr(), n_rows=n_rows, n=n, stride=n, top_k=10, mom=mom.data_ptr(),
                 used=used.data_ptr(), kth=kth.data_ptr())
        a.update(kw)
        return lib.svk_cohort_moments(a["ctx"], a["scores"], a["n_rows"], a["n"], a["stride"], a["top_k"], a["mom"], a["used"],
                                      a["kth"])

    eng._stream()
    assert call() == _lib.SVK_OK
    assert call(used=None, kth=None) == _lib.SVK_OK
    assert call(n_rows=0, scores=None, mom=None) == _lib.SVK_OK              # nothing to launch: no pointer is looked at
    cases = dict(null_ctx=dict(ctx=None), null_scores=dict(scores=None), null_moments=dict(mom=None), negative_rows=dict(n_rows=-1),
                 no_cohort=dict(n=0), negative_cohort=dict(n=-3), negative_top_k=dict(top_k=-1), short_stride=dict(stride=n - 1),
                 scores_2_bytes_off=dict(scores=sc.data_ptr() + 2), moments_4_bytes_off=dict(mom=mom.data_ptr() + 4),
                 used_2_bytes_off=dict(used=used.data_ptr() + 2), kth_1_byte_off=dict(kth=kth.data_ptr() + 1))
    for name, kw in cases.items():
        assert call(**kw) == _lib.SVK_ERR_BAD_ARG, name
    assert call() == _lib.SVK_OK
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.cohort_moments(np.zeros((3,), dtype=np.float32))
