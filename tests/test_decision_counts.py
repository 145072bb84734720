"""svk_decision_counts: accepted targets / non-targets at given thresholds, exact against NumPy."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def want_counts(scores, labels, thresholds):
    lab = labels != 0
    with np.errstate(invalid="ignore"):
        acc = [((scores >= np.float32(t)) & lab, (scores >= np.float32(t)) & ~lab) for t in thresholds]
    return np.array([[a.sum(), b.sum()] for a, b in acc], dtype=np.int64), (int(lab.sum()), int((~lab).sum()))


def data(n, seed, nan_every=0):
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    if n > 1:
        labels[rng.random(n) < 0.1] = 7                            # any non-zero label is a target
    scores = np.round(rng.standard_normal(n) + labels.astype(bool), 2).astype(np.float32)   # ties
    if nan_every:
        scores[::nan_every] = np.nan
    return scores, labels


@pytest.mark.parametrize("n", [1, 255, 100_003])
def test_exact_against_numpy(eng, n):
    scores, labels = data(n, 30 + n)
    finite = np.unique(scores)
    present = float(finite[finite.size // 2])
    between = float((finite[0].astype(np.float64) + finite[min(1, finite.size - 1)]) / 2) if n > 1 else 0.123
    four = [-np.inf, present, between, np.inf]
    sixteen = four + list(np.linspace(-2.5, 3.0, 12))
    for thresholds in ([present], [-np.inf], [np.inf], four, four[:2], sixteen[:5], sixteen):   # 1, 2, 4, 5, 16: every kernel width
        got, totals = eng.decision_counts(scores, labels, thresholds)
        want, want_totals = want_counts(scores, labels, thresholds)
        assert got.dtype == np.int64 and got.shape == (len(thresholds), 2)
        np.testing.assert_array_equal(got, want)
        assert totals == want_totals
    got, totals = eng.decision_counts(scores, labels, four)
    assert tuple(got[0]) == totals and tuple(got[3]) == (0, 0)       # -inf accepts every pair, +inf none


@pytest.mark.parametrize("n", [255, 100_003])
def test_nan_scores_are_never_accepted(eng, n):
    scores, labels = data(n, 40 + n, nan_every=7)
    thresholds = [-np.inf, 0.0, 0.5, np.inf]
    got, totals = eng.decision_counts(scores, labels, thresholds)
    want, want_totals = want_counts(scores, labels, thresholds)
    np.testing.assert_array_equal(got, want)
    assert totals == want_totals == (int((labels != 0).sum()), int((labels == 0).sum()))          # NaN pairs count here only
    n_nan = int(np.isnan(scores).sum())
    assert n_nan > 0 and int(got[0].sum()) == n - n_nan


def test_unaligned_buffers_and_device_tensors(eng):
    """Views 4 bytes (scores) and 1 byte (labels) into their buffers take the 4-byte / 1-byte loads."""
    scores, labels = data(10_007, 50)
    sc, lb = eng.to_device(scores), eng.to_device(labels)
    thresholds = [-0.25, 0.75, 1.5]
    want, want_totals = want_counts(scores[1:], labels[1:], thresholds)
    assert sc[1:].data_ptr() % 16 == 4
    got, totals = eng.decision_counts(sc[1:], lb[1:], thresholds)
    np.testing.assert_array_equal(got, want)
    assert totals == want_totals
    want, want_totals = want_counts(scores[4:], labels[4:], thresholds)        # aligned scores, labels too: the wide loads
    got, totals = eng.decision_counts(sc[4:], lb[4:], thresholds)
    np.testing.assert_array_equal(got, want)
    assert totals == want_totals


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    scores, labels = data(100, 60)
    for thresholds in ([], [0.0] * 17, [np.nan]):
        with pytest.raises(_lib.SvkError) as err:
            eng.decision_counts(scores, labels, thresholds)
        assert err.value.code == _lib.SVK_ERR_BAD_ARG and "threshold" in err.value.message
    with pytest.raises(ValueError):
        eng.decision_counts(scores, labels[:-1], [0.0])
    got, totals = eng.decision_counts(scores[:0], labels[:0], [0.0])            # an empty set: zeros
    assert not got.any() and totals == (0, 0)
