"""svk_calibration_apply against np.longdouble:  |out - ref| <= 2^-24 |ref| + (n_sys + 1) 2^-52 sum |terms|  (the one rounding to
float32, and n_sys + 1 float64 roundings of products and sums on the way), on the shapes and layouts of the statistics test."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_f64_ref as ref  # noqa: E402

SIZES, SYSTEMS, problem, place = ref.SIZES, ref.SYSTEMS, ref.problem, ref.place


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def check(out, scores, weights):
    want, abs_sums = ref.apply_longdouble(scores, weights)
    bound = 2.0 ** -24 * np.abs(want) + (scores.shape[0] + 1) * 2.0 ** -52 * abs_sums
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (scores.shape[1],)
    assert np.all(np.abs(got.astype(ref.LD) - want) <= bound)
    return got


@pytest.mark.parametrize("n_sys", SYSTEMS)
@pytest.mark.parametrize("n", SIZES)
def test_against_longdouble_on_every_layout(eng, n, n_sys):
    scores, _, weights, _, _ = problem(n, n_sys, 2000 * n_sys + n % 991)
    first = check(eng.calibration_apply(place(eng, scores, n, 0), weights), scores, weights)
    # what the header states to the bit: float64 products and sums in order, rounded once
    np.testing.assert_array_equal(first, ref.z_float64(scores, weights).astype(np.float32))
    for stride, offset in ((n + 3, 0), (n, 1)):
        got = check(eng.calibration_apply(place(eng, scores, stride, offset), weights), scores, weights)
        assert got.tobytes() == first.tobytes()                                 # 16-byte and 4-byte loads: the same bits
    odd = torch.zeros((n + 5,), dtype=torch.float32, device=eng.device)[1:n + 1]   # a 4-byte aligned output
    assert odd.data_ptr() % 16 == 4
    assert eng.calibration_apply(place(eng, scores, n, 0), weights, out=odd).cpu().numpy().tobytes() == first.tobytes()


@pytest.mark.parametrize("n", [1, 257, 100_003])
def test_in_place_for_one_system(eng, n):
    scores, _, weights, _, _ = problem(n, 1, 31 + n)
    for offset in (0, 1):
        sc = place(eng, scores, n, offset)
        out = eng.calibration_apply(sc, weights, out=sc.reshape(-1))
        assert out.data_ptr() == sc.data_ptr()
        got = check(out, scores, weights)
        np.testing.assert_array_equal(got, ref.z_float64(scores, weights).astype(np.float32))


def test_non_finite_scores_follow_ieee_and_empty_lists_launch_nothing(eng):
    scores = np.array([[1.0, np.nan, np.inf, -np.inf, 2.0]], dtype=np.float32)
    got = eng.calibration_apply(scores, (2.0, 0.5)).cpu().numpy()
    np.testing.assert_array_equal(got, np.array([2.5, np.nan, np.inf, -np.inf, 4.5], dtype=np.float32))
    out = eng.calibration_apply(torch.zeros((3, 0), dtype=torch.float32, device=eng.device), np.ones(4))
    assert out.shape == (0,)


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    lib, n = eng.lib, 100
    scores, _, weights, _, _ = problem(n, 2, 4)
    sc = place(eng, scores, n, 0)
    out = torch.empty((n + 4,), dtype=torch.float32, device=eng.device)
    dp = C.POINTER(C.c_double)

    def call(**kw):
        a = dict(ctx=eng.ctx, scores=sc.data_ptr(), n_sys=2, stride=n, n=n, weights=weights, out=out.data_ptr())
        a.update(kw)
        w = None if a["weights"] is None else np.ascontiguousarray(a["weights"], dtype=np.float64).ctypes.data_as(dp)
        return lib.svk_calibration_apply(a["ctx"], a["scores"], a["n_sys"], a["stride"], a["n"], w, a["out"])

    eng._stream()
    assert call() == _lib.SVK_OK
    nan_w, inf_w = weights.copy(), weights.copy()
    nan_w[1], inf_w[2] = np.nan, np.inf
    cases = dict(null_ctx=dict(ctx=None), null_scores=dict(scores=None), null_out=dict(out=None), null_weights=dict(weights=None),
                 negative_n=dict(n=-1), no_system=dict(n_sys=0), nine_systems=dict(n_sys=9), short_stride=dict(stride=n - 1),
                 scores_2_bytes_off=dict(scores=sc.data_ptr() + 2), out_1_byte_off=dict(out=out.data_ptr() + 1),
                 nan_weight=dict(weights=nan_w), inf_offset=dict(weights=inf_w))
    for name, kw in cases.items():
        assert call(**kw) == _lib.SVK_ERR_BAD_ARG, name
    assert call() == _lib.SVK_OK
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.calibration_apply(scores, weights[:-1])
