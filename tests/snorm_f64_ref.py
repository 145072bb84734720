"""NumPy restatement of svk_cohort_moments / svk_score_norm (include/svk.h "score normalisation"), the reference of the score
normalisation tests.

The selection is stated twice: `select_threshold` is the header's rule (everything strictly above the m-th largest candidate
v*, then copies of v* up to m), `select_sorted` is np.sort(finite)[-m:]; tests/test_score_norm_host.py holds them equal as
multisets on tie-heavy rows, so the GPU tests may use either.  The moments and the three norm expressions are np.longdouble;
`moment_bounds` and `norm_bound` are the header's accuracy expressions, with A from `additions(n_cohort)`."""
import numpy as np

LD = np.longdouble
WAVE_ROW_MAX = 2048            # csrc/snorm.hip: a row of up to this many columns is one wave's, a 256-thread workgroup's above
ROW_LDS_MAX = 16384            # csrc/snorm.hip: the columns of a row kept in LDS


def team_size(n_cohort):
    return 64 if n_cohort <= WAVE_ROW_MAX else 256


def additions(n_cohort):
    """A of the header: the additions on the longest path of a row's sums."""
    t = team_size(n_cohort)
    return -(-n_cohort // t) + 6 + (4 if t == 256 else 0) + 1


def candidates(row):
    """The finite values of a row as float32, -0.0 as +0.0."""
    row = np.asarray(row, dtype=np.float32).reshape(-1)
    return row[np.isfinite(row)] + np.float32(0.0)


def used_count(n_candidates, top_k):
    return n_candidates if top_k == 0 else min(int(top_k), n_candidates)


def select_threshold(row, top_k):
    """-> (m, v*, the selected multiset float32 [m]) by the header's rule; v* is NaN when m == 0."""
    cand = candidates(row)
    m = used_count(cand.size, top_k)
    if m == 0:
        return 0, np.float32(np.nan), cand[:0]
    vstar = np.partition(cand, cand.size - m)[cand.size - m]
    above = cand[cand > vstar]
    assert above.size < m <= above.size + int((cand == vstar).sum())
    return m, vstar, np.concatenate([above, np.full(m - above.size, vstar, dtype=np.float32)])


def select_sorted(row, top_k):
    """-> (m, v*, np.sort(finite)[-m:])."""
    cand = candidates(row)
    m = used_count(cand.size, top_k)
    if m == 0:
        return 0, np.float32(np.nan), cand[:0]
    top = np.sort(cand)[cand.size - m:]
    return m, top[0], top


def moments_longdouble(selected):
    """-> dict of the exact (longdouble) mean and variance of the multiset and the sums the bounds scale with."""
    x = np.asarray(selected).astype(LD)
    m = x.size
    mean = x.sum() / m
    d = x - mean
    return {"m": m, "mean": mean, "var": (d * d).sum() / m, "sum_abs": np.abs(x).sum(), "sum_d2": (d * d).sum(),
            "sum_abs_d": np.abs(d).sum()}


def moment_bounds(ref, n_cohort):
    """-> (bound on |mean - ref mean|, bound on |std^2 - ref var|): the header's expressions."""
    a, m, u2 = additions(n_cohort), ref["m"], LD(2.0) ** -52
    dm = (a + 2) * u2 * ref["sum_abs"] / m
    dv = (a + 4) * u2 * ref["sum_d2"] / m + 2 * dm * ref["sum_abs_d"] / m + dm * dm + LD(2.0) ** -51 * ref["var"]
    return dm, dv


def row_reference(row, top_k):
    """Everything svk_cohort_moments returns for one row -> (m, v*, ref dict or None)."""
    m, vstar, sel = select_threshold(row, top_k)
    return m, vstar, (moments_longdouble(sel) if m else None)


def norm_longdouble(scores, row_moments=None, col_moments=None):
    """The header's expression in longdouble -> (ref [n_rows, n_cols], |t_r| + |t_c|).  A table left out is None."""
    s = np.asarray(scores, dtype=np.float32).astype(LD)
    quot = []
    with np.errstate(all="ignore"):
        if row_moments is not None:
            rm = np.asarray(row_moments, dtype=np.float64).astype(LD)
            quot.append((s - rm[:, None, 0]) / rm[:, None, 1])
        if col_moments is not None:
            cm = np.asarray(col_moments, dtype=np.float64).astype(LD)
            quot.append((s - cm[None, :, 0]) / cm[None, :, 1])
        assert quot, "give the row table, the column table or both"
        if len(quot) == 2:
            return LD(0.5) * (quot[0] + quot[1]), np.abs(quot[0]) + np.abs(quot[1])
        return quot[0], np.abs(quot[0])


def norm_bound(ref, abs_quot):
    return LD(2.0) ** -24 * np.abs(ref) + 4 * LD(2.0) ** -52 * abs_quot


def tie_heavy_row(rng, n, levels=5):
    """n scores on `levels` distinct values: ties at v* for most top_k."""
    return rng.choice(rng.standard_normal(levels).astype(np.float32), size=n)


KINDS = ("gaussian", "five_values", "all_equal", "zeros", "non_finite_mixed", "no_finite", "few_finite", "wide_range")


def make_row(rng, n, kind):
    """One test row float32 [n] of the named kind."""
    if kind == "gaussian":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "five_values":
        return tie_heavy_row(rng, n)
    if kind == "all_equal":
        return np.full(n, np.float32(rng.standard_normal() * 3), dtype=np.float32)
    if kind == "zeros":
        return np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    if kind == "wide_range":
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 4, n)).astype(np.float32)
    row = rng.standard_normal(n).astype(np.float32)
    junk = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), n)
    if kind == "non_finite_mixed":
        return np.where(rng.random(n) < 0.2, junk, row)
    if kind == "no_finite":
        return junk
    assert kind == "few_finite"
    keep = np.zeros(n, dtype=bool)
    keep[rng.choice(n, size=min(3, n), replace=False)] = True
    return np.where(keep, row, junk)


def place_rows(eng, mat, stride, offset):
    """The matrix on the device, rows `stride` floats apart, the first `offset` floats into a fresh (256-byte aligned) buffer."""
    import torch
    n_rows, n_cols = mat.shape
    buf = torch.zeros((offset + n_rows * stride + 4,), dtype=torch.float32, device=eng.device)
    view = torch.as_strided(buf, (n_rows, n_cols), (stride, 1), storage_offset=offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(mat)))
    return view
