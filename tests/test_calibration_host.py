"""calibration.py on the host: the Newton iteration over a NumPy float64 restatement of svk_calibration_stats
(tests/calibration_f64_ref.py), the thresholds, save / load.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_f64_ref as ref  # noqa: E402

from speaker_verification_amd.calibration import Calibration, bayes_threshold, cllr, logit  # noqa: E402

N_TAR, N_NON = 700, 5000


def dev_set(n_sys, seed):
    """700 targets ~ N(2, 1), 5 000 non-targets ~ N(-1, 1.5), shuffled; systems beyond the first are noisy affine copies."""
    rng = np.random.default_rng(seed)
    base = np.r_[rng.normal(2.0, 1.0, N_TAR), rng.normal(-1.0, 1.5, N_NON)]
    labels = np.r_[np.ones(N_TAR, dtype=np.uint8), np.zeros(N_NON, dtype=np.uint8)]
    order = rng.permutation(base.size)
    base, labels = base[order], labels[order]
    planes = [base]
    for d in range(1, n_sys):
        planes.append(rng.uniform(0.5, 2.0) * base + rng.uniform(-1.0, 1.0) + rng.normal(0.0, 0.5 + 0.1 * d, base.size))
    return np.stack(planes).astype(np.float32), labels


@pytest.mark.parametrize("p_target", [0.01, 0.5])
@pytest.mark.parametrize("n_sys", [1, 3, 8])
def test_newton_converges_on_the_numpy_provider(n_sys, p_target):
    scores, labels = dev_set(n_sys, 100 + n_sys)
    cal = Calibration(p_target=p_target).fit(scores, labels, stats=ref.stats_float64)
    assert cal.converged_ and 1 <= cal.n_iter_ <= 30
    assert cal.weights_.shape == (n_sys + 1,) and cal.weights_.dtype == np.float64 and np.isfinite(cal.weights_).all()
    cw = (p_target / N_TAR, (1 - p_target) / N_NON)
    l_tar, l_non, grad, hess, counts = ref.stats_float64(scores, labels, cal.weights_, logit(p_target), cw)
    assert counts == (N_TAR, N_NON, 0)
    assert np.max(np.abs(grad)) <= 1e-10
    assert cal.objective_ == pytest.approx(cw[0] * l_tar + cw[1] * l_non, rel=1e-14)
    assert np.linalg.eigvalsh(hess).min() > 0                                   # a minimum
    # the zero start's objective is that of llr = 0: the prior's entropy; the fit is below it
    assert cal.objective_ < -(p_target * math.log(p_target) + (1 - p_target) * math.log1p(-p_target))
    after = ref.z_float64(scores, cal.weights_).astype(np.float32)
    cllr_after = cllr(after, labels, stats=ref.stats_float64)
    for d in range(n_sys):                                                      # no raw system read as LLRs is better
        assert cllr_after <= cllr(scores[d], labels, stats=ref.stats_float64)


def test_fit_recovers_a_known_affine_map():
    """Scores made from true LLRs by s = (llr - b) / a: the fit returns (a, b) within sampling error.  For equal-variance
    Gaussian classes N(+-m, 2 m) the score IS its own LLR.  The bar is 5 standard deviations of the estimate, from the
    sandwich covariance H^-1 (sum_p c_p^2 r_p^2 x_p x_p^T) H^-1 of the weighted M-estimator at the solution."""
    rng = np.random.default_rng(7)
    m, n_tar, n_non = 2.0, 4000, 40000
    llr = np.r_[rng.normal(m, math.sqrt(2 * m), n_tar), rng.normal(-m, math.sqrt(2 * m), n_non)]
    labels = np.r_[np.ones(n_tar, dtype=np.uint8), np.zeros(n_non, dtype=np.uint8)]
    a, b = 7.5, -1.25
    scores = ((llr - b) / a).astype(np.float32)
    p = 0.1
    cal = Calibration(p_target=p).fit(scores, labels, stats=ref.stats_float64)
    assert cal.converged_
    cw = (p / n_tar, (1 - p) / n_non)
    _, _, grad, hess, _ = ref.stats_float64(scores, labels, cal.weights_, logit(p), cw)
    z = ref.z_float64(scores, cal.weights_, logit(p))
    sig = 1.0 / (1.0 + np.exp(-z))
    r = np.where(labels != 0, -(1.0 - sig) * cw[0], sig * cw[1])
    x = np.stack([scores.astype(np.float64), np.ones_like(z)])
    meat = (x * r * r) @ x.T
    cov = np.linalg.solve(hess, np.linalg.solve(hess, meat).T)
    sd = np.sqrt(np.diag(cov))
    assert sd[0] < 0.05 * a and sd[1] < 0.25                                      # the bar means something
    assert abs(cal.weights_[0] - a) <= 5 * sd[0]
    assert abs(cal.weights_[1] - b) <= 5 * sd[1]


def test_separable_scores_end_unconverged_and_finite():
    rng = np.random.default_rng(3)
    scores = np.r_[rng.uniform(0.5, 2.0, 300), rng.uniform(-2.0, -0.5, 900)].astype(np.float32)
    labels = np.r_[np.ones(300, dtype=np.uint8), np.zeros(900, dtype=np.uint8)]
    cal = Calibration(p_target=0.05, max_iter=100).fit(scores, labels, stats=ref.stats_float64)
    assert cal.converged_ is False
    assert cal.n_iter_ == 100
    assert np.isfinite(cal.weights_).all() and np.isfinite(cal.objective_)
    assert cal.weights_[0] > 10                                                    # the slope runs away, as it must


def test_single_class_and_non_finite_scores_raise():
    scores, labels = dev_set(1, 5)
    with pytest.raises(ValueError, match="both classes"):
        Calibration().fit(scores, np.ones_like(labels), stats=ref.stats_float64)
    with pytest.raises(ValueError, match="both classes"):
        Calibration().fit(scores, np.zeros_like(labels), stats=ref.stats_float64)
    bad = scores.copy()
    bad[0, 17] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        Calibration().fit(bad, labels, stats=ref.stats_float64)
    with pytest.raises(ValueError):
        cllr(bad[0], labels, stats=ref.stats_float64)
    with pytest.raises(ValueError):
        Calibration(p_target=1.0)
    with pytest.raises(RuntimeError, match="not fitted"):
        Calibration().save("unused.npz")


def test_sequence_of_systems_is_the_stacked_matrix():
    scores, labels = dev_set(3, 11)
    one = Calibration(p_target=0.5).fit(scores, labels, stats=ref.stats_float64)
    two = Calibration(p_target=0.5).fit([scores[0], scores[1], scores[2]], labels, stats=ref.stats_float64)
    np.testing.assert_array_equal(one.weights_, two.weights_)
    assert one.n_sys == 3


def test_save_load_round_trip(tmp_path):
    scores, labels = dev_set(3, 21)
    cal = Calibration(p_target=0.05, max_iter=50, tol=1e-11).fit(scores, labels, stats=ref.stats_float64)
    path = str(tmp_path / "cal.npz")
    cal.save(path)
    back = Calibration.load(path)
    np.testing.assert_array_equal(back.weights_, cal.weights_)
    assert (back.p_target, back.max_iter, back.tol) == (0.05, 50, 1e-11)
    assert (back.n_iter_, back.converged_, back.objective_) == (cal.n_iter_, cal.converged_, cal.objective_)
    assert back.n_sys == 3


def test_bayes_threshold_known_answers():
    assert bayes_threshold(0.5) == 0.0
    assert bayes_threshold(0.01) == pytest.approx(math.log(99.0), rel=1e-15)
    assert bayes_threshold(0.05) == pytest.approx(math.log(19.0), rel=1e-15)
    assert bayes_threshold(0.01, c_miss=10, c_fa=1) == pytest.approx(math.log(9.9), rel=1e-15)
    assert bayes_threshold(0.5, c_miss=1, c_fa=4) == pytest.approx(math.log(4.0), rel=1e-15)
    assert bayes_threshold(0.2) == pytest.approx(-logit(0.2), rel=1e-15)
    for bad in ((0.0, 1, 1), (1.0, 1, 1), (0.5, 0, 1), (0.5, 1, -1)):
        with pytest.raises(ValueError):
            bayes_threshold(*bad)


def test_cllr_known_answers():
    labels = np.array([1, 0, 1, 0], dtype=np.uint8)
    assert cllr(np.zeros(4, dtype=np.float32), labels, stats=ref.stats_float64) == pytest.approx(1.0, rel=1e-15)
    good = np.array([30, -30, 30, -30], dtype=np.float32)
    assert cllr(good, labels, stats=ref.stats_float64) == pytest.approx(math.log1p(math.exp(-30.0)) / math.log(2.0), rel=1e-12)
    assert cllr(-good, labels, stats=ref.stats_float64) == pytest.approx(30.0 / math.log(2.0), rel=1e-12)


def test_float64_provider_agrees_with_the_longdouble_reference():
    scores, labels = dev_set(3, 31)
    w, tau, cw = np.array([0.7, -0.2, 0.4, -1.5]), logit(0.01), (0.01 / N_TAR, 0.99 / N_NON)
    l_tar, l_non, grad, hess, counts = ref.stats_float64(scores, labels, w, tau, cw)
    values, abs_sums, counts_ld = ref.stats_longdouble(scores, labels, w, tau, cw)
    flat = np.r_[l_tar, l_non, grad, hess[np.triu_indices(4)]]
    assert counts == counts_ld
    assert np.all(np.abs(flat - values) <= 64 * 2.0 ** -52 * abs_sums)            # NumPy's pairwise sums: log2(n) + the terms
    # extreme z: the exact limits, nothing non-finite
    for z in (800.0, -800.0, 1e30):
        got = ref.stats_float64(np.array([z, z], dtype=np.float32), np.array([1, 0]), (1.0, 0.0), 0.0, (1.0, 1.0))
        assert np.isfinite(got[0]) and np.isfinite(got[1]) and np.isfinite(got[2]).all() and np.isfinite(got[3]).all()
        assert (got[0], got[1]) == ((0.0, float(np.float32(z))) if z > 0 else (-z, 0.0))


def test_symbol_table_lists_the_calibration_entries():
    """header <-> binding <-> dlsym is tests/test_cabi.py's; here only that the binding names the three entries with the
    argument counts of include/svk.h."""
    from speaker_verification_amd import _lib
    assert len(_lib.SIGNATURES["svk_calibration_stats"][1]) == 14
    assert len(_lib.SIGNATURES["svk_calibration_apply"][1]) == 7
    assert len(_lib.SIGNATURES["svk_calibration_stats_workspace_bytes"][1]) == 2
    assert ref.additions(1) == 4 + 6 + 4 + 1 + 16 and ref.additions(3_000_007) == 4 * 2 + 6 + 4 + 92 + 16
