"""backend.solve and the save / load round trip of EmbeddingBackend: pure NumPy float64 on the host, no GPU.

The statistics are the float64 NumPy class means and within-class scatter of a small labelled set, 12 classes x 9 rows, dim 24
(96 within-class degrees of freedom for 24 dimensions: S_w has full rank).  THE BOUND: every identity below is one or two
symmetric eigendecompositions (`eigh`, backward stable: errors of a few dim eps ||A||) of a matrix conditioned by
shrinkage = 1e-3 followed by products with V lambda^-1/2, so the residual of W^T S W = I is of the order of dim eps cond(S):
with the condition number the test prints (about 30 for S_w here, below 1e3 for S_t) that is 1e-12 or less, and the tests
ask for 1e-9 dim."""
import numpy as np
import pytest

from speaker_verification_amd import backend

N_CLASS, PER, DIM = 12, 9, 24
TOL = 1e-9 * DIM
SHRINK = 1e-3


@pytest.fixture(scope="module")
def stats():
    rng = np.random.default_rng(11)
    centres = 2.0 * rng.standard_normal((N_CLASS, DIM))
    x = np.repeat(centres, PER, axis=0) + rng.standard_normal((N_CLASS * PER, DIM)) * rng.uniform(0.5, 2.0, DIM) + 3.0
    ids = np.repeat(np.arange(N_CLASS), PER)
    counts = np.full(N_CLASS, PER)
    mean = np.stack([x[ids == c].mean(0) for c in range(N_CLASS)])
    d = x - mean[ids]
    sw = d.T @ d
    n = x.shape[0]
    g = x.mean(0)
    s_w = sw / n
    s_w = s_w + SHRINK * np.trace(s_w) / DIM * np.eye(DIM)
    s_b = ((mean - g).T * counts) @ (mean - g) / n
    print("cond(S_w + shrinkage) = %.1f, cond(S_t) = %.1f" % (np.linalg.cond(s_w), np.linalg.cond(s_w + s_b)))
    return {"x": x, "class_mean": mean, "counts": counts, "sw": sw, "s_w": s_w, "s_b": s_b, "g": g}


def test_center(stats):
    mean, w = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "center")
    assert w is None and np.abs(mean - stats["g"]).max() <= 1e-13 * np.abs(stats["g"]).max()


def test_whiten_identity(stats):
    mean, w = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "whiten", shrinkage=SHRINK)
    assert w.shape == (DIM, DIM) and w.dtype == np.float64
    s_t = stats["s_w"] + stats["s_b"]
    assert np.abs(w.T @ s_t @ w - np.eye(DIM)).max() <= TOL
    _, w8 = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "whiten", out_dim=8, shrinkage=SHRINK)
    assert np.array_equal(w8, w[:, :8])                         # truncation keeps the leading columns
    # leading = the largest eigenvalues of S_t: the projected variances w_j^T S_t w_j are all 1, the raw ones descend
    lam = 1.0 / (w * w).sum(0)
    assert (np.diff(lam) <= 0).all()


def test_wccn_identity(stats):
    _, w = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "wccn", shrinkage=SHRINK)
    assert w.shape == (DIM, DIM)
    assert np.abs(w @ w.T @ stats["s_w"] - np.eye(DIM)).max() <= TOL


def test_lda_identities_and_eigenvalues(stats):
    mean, w = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "lda", shrinkage=SHRINK)
    assert w.shape == (DIM, N_CLASS - 1)                        # the default: min(dim, n_class - 1)
    assert np.abs(w.T @ stats["s_w"] @ w - np.eye(N_CLASS - 1)).max() <= TOL
    proj_b = w.T @ stats["s_b"] @ w
    lead = np.diag(proj_b)
    assert np.abs(proj_b - np.diag(lead)).max() <= TOL * lead.max() and (np.diff(lead) <= 0).all()
    try:
        from scipy.linalg import eigh
    except ImportError:
        eigh = None
    if eigh is not None:
        ref = np.sort(eigh(stats["s_b"], stats["s_w"], eigvals_only=True))[::-1][:N_CLASS - 1]
        np.testing.assert_allclose(np.sort(lead)[::-1], ref, rtol=1e-8, atol=0)
    _, w5 = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "lda", out_dim=5, shrinkage=SHRINK)
    assert np.array_equal(w5, w[:, :5])
    # the projected classes separate: between-class variance along the first direction exceeds the within-class one (= 1)
    assert lead[0] > 1.0


def test_value_errors(stats):
    cm, counts, sw = stats["class_mean"], stats["counts"], stats["sw"]
    bad = cm.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        backend.solve(bad, counts, sw, "lda", shrinkage=SHRINK)
    bad_sw = sw.copy()
    bad_sw[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        backend.solve(cm, counts, bad_sw, "wccn", shrinkage=SHRINK)
    # two rows per class: 12 within-class degrees of freedom in 24 dimensions -> S_w is singular without shrinkage
    x2 = stats["x"].reshape(N_CLASS, PER, DIM)[:, :2]
    m2 = x2.mean(1)
    d2 = (x2 - m2[:, None]).reshape(-1, DIM)
    for method in ("lda", "wccn"):
        with pytest.raises(ValueError, match="singular"):
            backend.solve(m2, np.full(N_CLASS, 2), d2.T @ d2, method, shrinkage=0.0)
        backend.solve(m2, np.full(N_CLASS, 2), d2.T @ d2, method, shrinkage=SHRINK)       # ... and regular with it
    for method, out_dim in (("lda", 0), ("lda", N_CLASS), ("whiten", DIM + 1), ("wccn", DIM - 1), ("center", 3)):
        with pytest.raises(ValueError, match="out_dim"):
            backend.solve(cm, counts, sw, method, out_dim=out_dim, shrinkage=SHRINK)
    with pytest.raises(ValueError, match="method"):
        backend.solve(cm, counts, sw, "plda")
    with pytest.raises(ValueError):
        backend.solve(cm, counts[:-1], sw, "lda")
    with pytest.raises(ValueError):
        backend.solve(cm, np.zeros(N_CLASS), sw, "center")


def test_empty_class_carries_no_weight(stats):
    cm = np.concatenate([stats["class_mean"], np.full((1, DIM), np.nan)])      # an empty class: its mean is never read
    counts = np.r_[stats["counts"], 0]
    a = backend.solve(cm, counts, stats["sw"], "lda", shrinkage=SHRINK)
    b = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "lda", shrinkage=SHRINK)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_save_load_round_trip(stats, tmp_path):
    mean, w = backend.solve(stats["class_mean"], stats["counts"], stats["sw"], "lda", out_dim=7, shrinkage=SHRINK)
    b = backend.EmbeddingBackend(mean, w, l2_in=False, l2_out=True, method="lda", shrinkage=SHRINK)
    path = str(tmp_path / "backend.npz")
    b.save(path)
    r = backend.EmbeddingBackend.load(path)
    assert np.array_equal(r.mean, mean) and np.array_equal(r.w, w) and r.mean.dtype == r.w.dtype == np.float64
    assert (r.l2_in, r.l2_out, r.method, r.shrinkage, r.dim, r.out_dim) == (False, True, "lda", SHRINK, DIM, 7)
    c = backend.EmbeddingBackend(mean, None, l2_in=True, l2_out=False, method="center")
    c.save(path)
    r = backend.EmbeddingBackend.load(path)
    assert r.w is None and np.array_equal(r.mean, mean) and (r.l2_in, r.l2_out, r.method, r.out_dim) == (True, False, "center", DIM)
    with pytest.raises(RuntimeError):
        backend.EmbeddingBackend().save(path)
