"""svk_calibration_stats against the np.longdouble restatement (tests/calibration_f64_ref.py) with the bound of include/svk.h:

    |dev - ref| <= (A + 8) 2^-52 sum_p |term_p|      for every output

A = the additions on the longest path of the summation order the header states for that n (`calibration_f64_ref.additions`
computes it from n), 8 for exp, log1p, the division and the products of a term.  Plus: bit identity of runs and of the 16-byte /
4-byte load paths, labels other than 0 / 1, |z| = 800, non-finite scores, a single class, the value-only flag, every rejected
argument."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_f64_ref as ref  # noqa: E402

EPS = 2.0 ** -52
TERM_ULPS = 8
SIZES, SYSTEMS, problem, place = ref.SIZES, ref.SYSTEMS, ref.problem, ref.place


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def flat(result):
    l_tar, l_non, grad, hess, counts = result
    if grad is None:
        return np.array([l_tar, l_non]), counts
    return np.r_[l_tar, l_non, grad, hess[np.triu_indices(grad.size)]], counts


@pytest.mark.parametrize("n_sys", SYSTEMS)
@pytest.mark.parametrize("n", SIZES)
def test_against_longdouble_on_every_layout(eng, n, n_sys):
    scores, labels, weights, tau, cw = problem(n, n_sys, 1000 * n_sys + n % 997)
    want, abs_sums, want_counts = ref.stats_longdouble(scores, labels, weights, tau, cw)
    bound = (ref.additions(n) + TERM_ULPS) * EPS * abs_sums
    lab = eng.to_device(labels)
    lab_odd = eng.to_device(np.r_[np.uint8(0), labels])[1:]                    # 1 byte into its buffer: the 1-byte label loads
    layouts = {"stride n": (place(eng, scores, n, 0), lab), "stride n + 3": (place(eng, scores, n + 3, 0), lab),
               "base + 4 bytes": (place(eng, scores, n, 1), lab), "labels + 1 byte": (place(eng, scores, n, 0), lab_odd)}
    assert layouts["stride n"][0].data_ptr() % 16 == 0 and layouts["base + 4 bytes"][0].data_ptr() % 16 == 4
    first = None
    for name, (sc, lb) in layouts.items():
        got, counts = flat(eng.calibration_stats(sc, lb, weights, tau, cw))
        assert counts == want_counts and counts[2] == 0, name
        err = np.abs(got.astype(ref.LD) - want)
        print("n = %d, n_sys = %d, %s: max err / bound = %.3f" % (n, n_sys, name, float(np.max(err / np.maximum(bound, 1e-300)))))
        assert np.all(err <= bound), (name, float(np.max(err / np.maximum(bound, 1e-300))))
        if first is None:
            first = got
            again, _ = flat(eng.calibration_stats(sc, lb, weights, tau, cw))
            assert again.tobytes() == got.tobytes()                             # two runs: the same bits
        assert got.tobytes() == first.tobytes(), name                           # 16-byte and 4-byte loads: the same bits
    value, counts = flat(eng.calibration_stats(layouts["stride n"][0], lab, weights, tau, cw, value_only=True))
    assert value.tobytes() == first[:2].tobytes() and counts == want_counts


def test_empty_list_returns_zeros(eng):
    for n_sys in SYSTEMS:
        sc = torch.zeros((n_sys, 0), dtype=torch.float32, device=eng.device)
        got, counts = flat(eng.calibration_stats(sc, np.zeros(0, dtype=np.uint8), np.ones(n_sys + 1), 0.5, (1.0, 2.0)))
        assert got.shape == (2 + (n_sys + 1) + (n_sys + 1) * (n_sys + 2) // 2,) and not got.any() and counts == (0, 0, 0)
        assert eng.lib.svk_calibration_stats_workspace_bytes(0, n_sys) == 0


def test_any_non_zero_label_is_a_target(eng):
    scores, labels, weights, tau, cw = problem(10_007, 2, 5)
    assert (labels == 7).any() and (labels == 1).any()
    a, ca = flat(eng.calibration_stats(scores, labels, weights, tau, cw))
    b, cb = flat(eng.calibration_stats(scores, (labels != 0).astype(np.uint8), weights, tau, cw))
    assert a.tobytes() == b.tobytes() and ca == cb == (int((labels != 0).sum()), int((labels == 0).sum()), 0)


def test_extreme_z_gives_the_exact_limits(eng):
    """|z| = 800 (exp(-800) underflows to 0) and far beyond: softplus = max(z, 0), sigma = 0 or 1, the Hessian term 0."""
    for big in (800.0, 1e30):
        scores = np.array([big, -big, big, -big], dtype=np.float32)
        labels = np.array([1, 1, 0, 0], dtype=np.uint8)
        b = float(np.float32(big))
        got, counts = flat(eng.calibration_stats(scores, labels, (1.0, 0.0), 0.0, (0.5, 0.25)))
        assert np.isfinite(got).all() and counts == (2, 2, 0)
        # target at -big: softplus(big) = big, r = -1; non-target at +big: softplus(big) = big, r = +1; the other two add 0
        np.testing.assert_array_equal(got, [b, b, 0.5 * -1.0 * -b + 0.25 * 1.0 * b, -0.5 + 0.25, 0.0, 0.0, 0.0])
    # 745.2 > |z| > 708: e is subnormal-small but not 0; still finite, and the longdouble reference agrees
    scores = np.array([740.0, -740.0, 30.0, -30.0], dtype=np.float32)
    got, _ = flat(eng.calibration_stats(scores, labels, (1.0, 0.0), 0.0, (0.5, 0.25)))
    want, abs_sums, _ = ref.stats_longdouble(scores, labels, (1.0, 0.0), 0.0, (0.5, 0.25))
    assert np.isfinite(got).all() and np.all(np.abs(got.astype(ref.LD) - want) <= (ref.additions(4) + TERM_ULPS) * EPS * abs_sums)


@pytest.mark.parametrize("n_sys", [1, 3])
def test_non_finite_scores_are_skipped_and_counted(eng, n_sys):
    n = 20_011
    scores, labels, weights, tau, cw = problem(n, n_sys, 77)
    rng = np.random.default_rng(8)
    bad = rng.choice(n, size=300, replace=False)
    scores[rng.integers(0, n_sys, 300), bad] = np.tile(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 100)
    scores[0, [0, n - 1]] = np.nan                                             # the first trial and the ragged tail
    n_bad = int((~np.isfinite(scores).all(axis=0)).sum())
    want, abs_sums, want_counts = ref.stats_longdouble(scores, labels, weights, tau, cw)
    assert want_counts[2] == n_bad >= 300
    for sc in (place(eng, scores, n, 0), place(eng, scores, n + 3, 1)):
        got, counts = flat(eng.calibration_stats(sc, labels, weights, tau, cw))
        assert counts == want_counts and sum(counts) == n
        assert np.isfinite(got).all()
        assert np.all(np.abs(got.astype(ref.LD) - want) <= (ref.additions(n) + TERM_ULPS) * EPS * abs_sums)
    value, counts = flat(eng.calibration_stats(scores, labels, weights, tau, cw, value_only=True))
    assert value.tobytes() == got[:2].tobytes() and counts == want_counts


def test_single_class_leaves_the_other_sum_exactly_zero(eng):
    scores, labels, weights, tau, cw = problem(5_003, 2, 9)
    got, counts = flat(eng.calibration_stats(scores, np.ones_like(labels), weights, tau, cw))
    assert counts == (5_003, 0, 0) and got[1] == 0.0 and got[0] > 0.0
    got, counts = flat(eng.calibration_stats(scores, np.zeros_like(labels), weights, tau, cw))
    assert counts == (0, 5_003, 0) and got[0] == 0.0 and got[1] > 0.0


def test_cllr_is_one_value_only_call(eng):
    from speaker_verification_amd.calibration import cllr
    scores, labels, _, _, _ = problem(30_001, 1, 12)
    l_tar, l_non, _, _, (n_tar, n_non, _) = ref.stats_float64(scores, labels, (1.0, 0.0), 0.0, (1.0, 1.0), value_only=True)
    want = (l_tar / n_tar + l_non / n_non) / (2 * math.log(2))
    assert cllr(scores[0], labels, engine=eng) == pytest.approx(want, rel=1e-13)
    assert cllr(np.zeros(4, dtype=np.float32), [1, 0, 1, 0], engine=eng) == pytest.approx(1.0, rel=1e-15)


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    lib, n, n_sys = eng.lib, 1000, 2
    scores, labels, weights, tau, cw = problem(n, n_sys, 3)
    sc, lb = place(eng, scores, n, 0), eng.to_device(labels)
    work = torch.empty((int(lib.svk_calibration_stats_workspace_bytes(n, n_sys)) + 16,), dtype=torch.uint8, device=eng.device)
    assert work.numel() > 16 and work.data_ptr() % 16 == 0
    out, count = (C.c_double * 16)(), (C.c_int64 * 3)()
    dp = C.POINTER(C.c_double)

    def call(**kw):
        a = dict(ctx=eng.ctx, scores=sc.data_ptr(), n_sys=n_sys, stride=n, labels=lb.data_ptr(), n=n, weights=weights, tau=tau,
                 cw=np.array(cw), flags=0, work=work.data_ptr(), work_bytes=work.numel() - 16, out=out, count=count)
        a.update(kw)
        w = None if a["weights"] is None else np.ascontiguousarray(a["weights"], dtype=np.float64).ctypes.data_as(dp)
        c = None if a["cw"] is None else np.ascontiguousarray(a["cw"], dtype=np.float64).ctypes.data_as(dp)
        return lib.svk_calibration_stats(a["ctx"], a["scores"], a["n_sys"], a["stride"], a["labels"], a["n"], w, a["tau"], c,
                                         a["flags"], a["work"], a["work_bytes"], a["out"], a["count"])

    eng._stream()
    assert call() == _lib.SVK_OK and count[0] + count[1] == n
    bad_w = [weights.copy() for _ in range(3)]
    bad_w[0][0], bad_w[1][n_sys], bad_w[2][1] = np.nan, np.inf, -np.inf
    cases = dict(null_ctx=dict(ctx=None), null_scores=dict(scores=None), null_labels=dict(labels=None), null_work=dict(work=None),
                 null_weights=dict(weights=None), null_cw=dict(cw=None), null_out=dict(out=None), null_count=dict(count=None),
                 negative_n=dict(n=-1), no_system=dict(n_sys=0), nine_systems=dict(n_sys=9), short_stride=dict(stride=n - 1),
                 scores_2_bytes_off=dict(scores=sc.data_ptr() + 2), work_8_bytes_off=dict(work=work.data_ptr() + 8),
                 nan_weight=dict(weights=bad_w[0]), inf_offset=dict(weights=bad_w[1]), neg_inf_weight=dict(weights=bad_w[2]),
                 nan_tau=dict(tau=float("nan")), inf_tau=dict(tau=float("inf")), nan_cw=dict(cw=np.array([np.nan, 1.0])),
                 inf_cw=dict(cw=np.array([1.0, np.inf])), flag_bit_1=dict(flags=2), flag_high_bit=dict(flags=1 | 1 << 20),
                 short_work=dict(work_bytes=int(lib.svk_calibration_stats_workspace_bytes(n, n_sys)) - 1))
    for name, kw in cases.items():
        assert call(**kw) == _lib.SVK_ERR_BAD_ARG, name
    assert b"workspace" in lib.svk_last_error(eng.ctx)
    for args in ((-1, 1), (10, 0), (10, 9), (0, 1)):
        assert lib.svk_calibration_stats_workspace_bytes(*args) == 0
    assert call() == _lib.SVK_OK                                                 # the handle is still good
    with pytest.raises(ValueError):
        eng.calibration_stats(scores, labels[:-1], weights, tau, cw)
    with pytest.raises(ValueError):
        eng.calibration_stats(scores, labels, weights[:-1], tau, cw)
