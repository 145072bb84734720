"""plda.solve_plda, plda.coefficients and the save / load round trip of Plda: pure NumPy float64 on the host, no GPU.

The statistics are the float64 NumPy class means and within-class scatter of a seeded labelled set: 60 classes of 2 .. 8 rows,
dim 24 (N - C is about 240 within-class degrees of freedom for 24 dimensions: W has full rank).  THE BOUNDS: as in
tests/test_backend_host.py every identity is two symmetric eigendecompositions (backward stable, errors of a few dim eps ||A||)
of matrices conditioned by the data (cond(W) is printed, below 1e2) followed by products with P = V lambda^-1/2: residuals of
the order of dim eps cond(W), 1e-12 or less, and the tests ask for 1e-9.  The closed-form LLR against the joint-Gaussian form:
both are float64 evaluations of one quantity whose terms are a few hundred at most in size with psi up to 300 (the joint
covariance has condition number below 1e4), so they agree to about 1e-12 relative and the test asks for 1e-10."""
import numpy as np
import pytest

from speaker_verification_amd import plda

import plda_f64_ref as ref

N_CLASS, DIM = 60, 24


@pytest.fixture(scope="module")
def stats():
    rng = np.random.default_rng(21)
    sizes = rng.integers(2, 9, N_CLASS)
    sizes[:2] = (2, 8)
    ids = np.repeat(np.arange(N_CLASS), sizes)
    spread = rng.uniform(0.2, 3.0, DIM)
    centres = rng.standard_normal((N_CLASS, DIM)) * spread
    mix = 0.3 * rng.standard_normal((DIM, DIM)) / np.sqrt(DIM) + np.eye(DIM)
    x = (centres[ids] + rng.standard_normal((ids.size, DIM))) @ mix + 1.5
    mean = np.stack([x[ids == c].mean(0) for c in range(N_CLASS)])
    d = x - mean[ids]
    sw = d.T @ d
    n = float(ids.size)
    w = sw / (n - N_CLASS)
    g = x.mean(0)
    m_b = ((mean - g).T * sizes) @ (mean - g) / (N_CLASS - 1)
    n0 = (n - (sizes.astype(np.float64) ** 2).sum() / n) / (N_CLASS - 1)
    print("N = %d, n0 = %.4f, cond(W) = %.1f" % (ids.size, n0, np.linalg.cond(w)))
    return {"class_mean": mean, "counts": sizes, "sw": sw, "w": w, "m_b": m_b, "n0": n0, "g": g}


def test_solve_identities(stats):
    mean, v, psi = plda.solve_plda(stats["class_mean"], stats["counts"], stats["sw"])
    assert v.shape == (DIM, DIM) and psi.shape == (DIM,) and v.dtype == psi.dtype == mean.dtype == np.float64   # min(dim, C - 1)
    assert np.abs(mean - stats["g"]).max() <= 1e-13 * np.abs(stats["g"]).max()
    assert np.abs(v.T @ stats["w"] @ v - np.eye(DIM)).max() <= 1e-9
    proj = v.T @ stats["m_b"] @ v
    lead = np.diag(proj)
    assert np.abs(proj - np.diag(lead)).max() <= 1e-9 * lead.max()
    assert (np.diff(psi) <= 0).all() and (psi >= 0).all() and psi[0] > 0
    pos = psi > 0
    np.testing.assert_allclose(lead[pos], 1.0 + stats["n0"] * psi[pos], rtol=1e-9, atol=0)
    assert (lead[~pos] <= 1.0 + 1e-9).all()
    # an independent generalised-eigenvalue computation: the eigenvalues of W^-1 M_b (non-symmetric solver)
    lam = np.sort(np.linalg.eigvals(np.linalg.solve(stats["w"], stats["m_b"])).real)[::-1]
    want = np.maximum((lam - 1.0) / stats["n0"], 0.0)
    np.testing.assert_allclose(psi[pos], want[pos], rtol=1e-8, atol=0)
    # truncation keeps the leading directions
    _, v5, psi5 = plda.solve_plda(stats["class_mean"], stats["counts"], stats["sw"], out_dim=5)
    assert np.array_equal(v5, v[:, :5]) and np.array_equal(psi5, psi[:5])
    # shrinkage: W + s tr(W) / dim I is what gets whitened
    _, vs, _ = plda.solve_plda(stats["class_mean"], stats["counts"], stats["sw"], shrinkage=1e-2)
    ws = stats["w"] + 1e-2 * np.trace(stats["w"]) / DIM * np.eye(DIM)
    assert np.abs(vs.T @ ws @ vs - np.eye(DIM)).max() <= 1e-9


@pytest.mark.parametrize("n", [1, 2, 5, 40])
def test_closed_form_against_joint_gaussians(n):
    rng = np.random.default_rng(100 + n)
    psi = ref.make_psi(12, 3)
    assert (psi == 0).sum() >= 2 and psi.max() == 300.0
    worst = 0.0
    for trial in range(8):
        same = trial % 2 == 0
        y = rng.standard_normal(12) * np.sqrt(psi)
        u = y + rng.standard_normal(12) / np.sqrt(n)
        v = (y if same else rng.standard_normal(12) * np.sqrt(psi)) + rng.standard_normal(12)
        want = ref.llr_joint(u, n, v, psi)
        got = ref.llr(v[None], u[None], psi, counts=[n])[0][0, 0]
        worst = max(worst, abs(got - want) / abs(want))
        # the library's host coefficients (log1p form) give the same score
        alpha, beta, gamma, c = plda.coefficients(psi, n)
        lib = (alpha * u * v - 0.5 * beta * v * v - 0.5 * gamma * u * u).sum() + c
        worst = max(worst, abs(lib - want) / abs(want))
    print("n = %d: worst relative difference %.2e" % (n, worst))
    assert worst <= 1e-10


def test_zero_psi_contributes_nothing():
    alpha, beta, gamma, c = plda.coefficients(np.zeros(7), 3)
    assert not alpha.any() and not beta.any() and not gamma.any() and c == 0.0
    psi = ref.make_psi(10, 5)
    keep = psi > 0
    rng = np.random.default_rng(1)
    u, v = rng.standard_normal((2, 10))
    full = ref.llr(v[None], u[None], psi, counts=[4])[0][0, 0]
    cut = ref.llr(v[None, keep], u[None, keep], psi[keep], counts=[4])[0][0, 0]
    assert abs(full - cut) <= 1e-13 * abs(full)


def test_value_errors(stats):
    cm, counts, sw = stats["class_mean"], stats["counts"], stats["sw"]
    bad = cm.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="finite"):
        plda.solve_plda(bad, counts, sw)
    bad_sw = sw.copy()
    bad_sw[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        plda.solve_plda(cm, counts, bad_sw)
    one = np.zeros_like(counts)
    one[4] = 5
    with pytest.raises(ValueError, match="2 non-empty classes"):
        plda.solve_plda(cm, one, sw)
    with pytest.raises(ValueError, match="more than one row"):
        plda.solve_plda(cm, np.ones_like(counts), np.zeros_like(sw))          # N == C
    for out_dim in (0, DIM + 1, -2):
        with pytest.raises(ValueError, match="out_dim"):
            plda.solve_plda(cm, counts, sw, out_dim=out_dim)
    with pytest.raises(ValueError, match="out_dim"):
        plda.solve_plda(cm[:5], counts[:5], sw, out_dim=5)                    # 5 classes: at most 4
    with pytest.raises(ValueError, match="singular"):
        plda.solve_plda(cm, counts, np.zeros_like(sw))
    with pytest.raises(ValueError, match="shrinkage"):
        plda.solve_plda(cm, counts, sw, shrinkage=-1.0)
    with pytest.raises(ValueError):
        plda.solve_plda(cm, counts[:-1], sw)
    with pytest.raises(ValueError, match="psi"):
        plda.coefficients([1.0, -0.5], 1)
    with pytest.raises(ValueError, match="psi"):
        plda.Plda(mean=np.zeros(2), v=np.eye(2), psi=[1.0, np.nan])
    with pytest.raises(ValueError, match="at least one"):
        plda.coefficients([1.0], 0)
    with pytest.raises(ValueError):
        plda.Plda(mean=np.zeros(3), v=np.eye(2), psi=[1.0, 0.5])


def test_empty_class_carries_no_weight(stats):
    cm = np.concatenate([stats["class_mean"], np.full((1, DIM), np.nan)])      # an empty class: its mean is never read
    counts = np.r_[stats["counts"], 0]
    a = plda.solve_plda(cm, counts, stats["sw"], shrinkage=1e-3)
    b = plda.solve_plda(stats["class_mean"], stats["counts"], stats["sw"], shrinkage=1e-3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_save_load_round_trip(stats, tmp_path):
    mean, v, psi = plda.solve_plda(stats["class_mean"], stats["counts"], stats["sw"], out_dim=7, shrinkage=1e-3)
    p = plda.Plda(mean, v, psi, l2_in=False, shrinkage=1e-3)
    path = str(tmp_path / "plda.npz")
    p.save(path)
    r = plda.Plda.load(path)
    assert np.array_equal(r.mean, mean) and np.array_equal(r.v, v) and np.array_equal(r.psi, psi)
    assert r.mean.dtype == r.v.dtype == r.psi.dtype == np.float64
    assert (r.l2_in, r.shrinkage, r.dim, r.out_dim) == (False, 1e-3, DIM, 7)
    with pytest.raises(RuntimeError):
        plda.Plda().save(path)
