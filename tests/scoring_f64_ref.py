"""Float64 references and input makers for the two oldest entries of csrc/scoring.hip, svk_cosine_scores and svk_l2_dist
(tests/test_scoring_float64.py).  NumPy float64 and nothing from the library under test; oracle/scoring_ref.py restates the
reference's own float32 arithmetic and is not used here.

Every reference starts from the float32 rows the kernel is given: input rounding is never counted as kernel error.

THE BARS.
  cosine   |got - cosine64| <= 1e-5, the project's own bar (README, tests/test_gpu_parity.py), now against float64.  Each case
           also reports err / (2^-24 absdot64): absdot64 = sum_k |t_k| |e_k| / (||t|| ||e||) is what one float32 rounding of
           every partial sum can move a score by, so the ratio is the length of the rounding chain the kernel behaves like.
  l2       |got - l2_64| <= (dim / 2 + 3) 2^-24 l2_64: fl(a - b) rounds once; the squares are non-negative, so ANY order of
           adding dim of them is off by at most about (dim + 1) 2^-24 relative; the square root halves that and rounds once
           more.  The bar follows from the operation, not from the kernel's order of additions.
"""
import numpy as np

U32 = 2.0 ** -24                   # float32 unit roundoff
COSINE_TOL = 1e-5
KINDS = ("zero_mean", "one_signed", "near_duplicate", "scaled")


def _norms(x):
    n = np.sqrt((x * x).sum(1))
    n[n == 0] = 1.0                # sklearn normalize(): a zero norm divides by 1
    return n


def cosine64(t, e, rows=None):
    """[n_test, n_enroll] float64 cosine of float32 rows; `rows` (an index array) keeps that subset of the test rows only."""
    t = np.asarray(t)
    x = (t if rows is None else t[rows]).astype(np.float64)
    y = np.asarray(e).astype(np.float64)
    return (x @ y.T) / (_norms(x)[:, None] * _norms(y)[None, :])


def absdot64(t, e, rows=None):
    """(|t| @ |e|.T) / (nt * ne): the condition term of a score, same subset rule as cosine64."""
    t = np.asarray(t)
    x = (t if rows is None else t[rows]).astype(np.float64)
    y = np.asarray(e).astype(np.float64)
    return (np.abs(x) @ np.abs(y).T) / (_norms(x)[:, None] * _norms(y)[None, :])


def l2_64(a, b):
    d = np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)
    return np.sqrt(np.einsum("ij,ij->i", d, d))


def l2_bar(dim, want):
    return (dim / 2.0 + 3.0) * U32 * want


# ---- input makers: (test [nt, dim], enroll [ne, dim]) float32, seeded ---------------------------------------------------
def _normal(rng, n, dim):
    return rng.standard_normal((n, dim), dtype=np.float32)


def zero_mean(nt, ne, dim, seed):
    rng = np.random.default_rng(seed)
    return _normal(rng, nt, dim), _normal(rng, ne, dim)


def one_signed(nt, ne, dim, seed):
    t, e = zero_mean(nt, ne, dim, seed)
    return np.abs(t), np.abs(e)


def near_duplicate(nt, ne, dim, seed):
    """Test row i = enrolled row i mod ne + 1e-3 N(0, 1): every test row has a score near 1."""
    rng = np.random.default_rng(seed)
    e = _normal(rng, ne, dim)
    t = e[np.arange(nt) % ne] + np.float32(1e-3) * _normal(rng, nt, dim)
    return t, e


def scaled(nt, ne, dim, seed):
    """Zero-mean rows, each times its own power of two in 2^-40 .. 2^40 (exact in float32; squares stay below 2^80 dim 20)."""
    rng = np.random.default_rng(seed)
    t, e = _normal(rng, nt, dim), _normal(rng, ne, dim)
    t *= np.exp2(rng.integers(-40, 41, (nt, 1))).astype(np.float32)
    e *= np.exp2(rng.integers(-40, 41, (ne, 1))).astype(np.float32)
    return t, e


MAKERS = {"zero_mean": zero_mean, "one_signed": one_signed, "near_duplicate": near_duplicate, "scaled": scaled}


def plant(t, e):
    """In place: a zero row in each operand and an enrolled row copied from a test row, where the shape has room.
    -> dict(zero_t, zero_e, copy=(test row, enrolled row)), None for what did not fit."""
    nt, ne = t.shape[0], e.shape[0]
    where = {"zero_t": None, "zero_e": None, "copy": None}
    if nt > 2:
        where["zero_t"] = nt // 2
        t[nt // 2] = 0
    if ne > 2:
        where["zero_e"] = ne // 3
        e[ne // 3] = 0
    if ne > 1 or nt * ne == 1:
        src = min(1, nt - 1)
        e[ne - 1] = t[src]
        where["copy"] = (src, ne - 1)
    return where
