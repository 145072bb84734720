"""svk_score_norm and svk_score_norm_pairs against np.longdouble:  |out - ref| <= 2^-24 |ref| + 4 * 2^-52 (|t_r| + |t_c|)  (the one
rounding to float32, and the float64 roundings of the differences, the quotients, their sum and the half on the way), for the
three normalisations, in place, on strided and 4-byte aligned layouts, and the trial-list form against the matrix form."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import snorm_f64_ref as ref  # noqa: E402

LD = ref.LD
SHAPES = [(1, 1), (17, 65), (130, 1211)]
MODES = {"s": (True, True), "t": (True, False), "z": (False, True)}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def problem(n_rows, n_cols, seed):
    """PLDA-like scores and moment tables as svk_cohort_moments writes them: means of either sign, std in [0.05, 20]."""
    rng = np.random.default_rng(seed)
    scores = (rng.standard_normal((n_rows, n_cols)) * 10.0 ** rng.uniform(-1, 2, (n_rows, 1))).astype(np.float32)
    def table(n):
        return np.stack([rng.standard_normal(n) * 5, 10.0 ** rng.uniform(-1.3, 1.3, n)], axis=1)
    return scores, table(n_rows), table(n_cols)


def check(out, scores, rm, cm):
    want, quot = ref.norm_longdouble(scores, rm, cm)
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == scores.shape
    assert np.all(np.abs(got.astype(LD) - want) <= ref.norm_bound(want, quot))
    return got


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", SHAPES)
def test_against_longdouble_on_every_layout_and_in_place(eng, shape, mode):
    n_rows, n_cols = shape
    scores, rm, cm = problem(n_rows, n_cols, 10 * n_cols + len(mode) + ord(mode))
    rm, cm = (rm if MODES[mode][0] else None), (cm if MODES[mode][1] else None)
    padded = (n_cols + 3) // 4 * 4
    first = check(eng.score_norm(ref.place_rows(eng, scores, padded, 0), rm, cm), scores, rm, cm)
    for stride, offset in ((n_cols + 3, 0), (n_cols + 3, 1), (padded, 1), (n_cols, 0)):
        got = eng.score_norm(ref.place_rows(eng, scores, stride, offset), rm, cm)
        assert got.cpu().numpy().tobytes() == first.tobytes()                  # 16-byte and 4-byte loads: the same bits
    odd = ref.place_rows(eng, np.zeros_like(scores), n_cols + 1, 1)            # a strided, 4-byte aligned output
    assert eng.score_norm(ref.place_rows(eng, scores, padded, 0), rm, cm, out=odd).data_ptr() == odd.data_ptr()
    assert odd.cpu().numpy().tobytes() == first.tobytes()
    for stride, offset in ((padded, 0), (n_cols + 3, 1)):                       # in place, both load widths
        sc = ref.place_rows(eng, scores, stride, offset)
        out = eng.score_norm(sc, rm, cm, out=sc)
        assert out.data_ptr() == sc.data_ptr() and out.cpu().numpy().tobytes() == first.tobytes()


def test_zero_and_nan_std_and_nan_scores_follow_ieee(eng):
    scores = np.array([[1.0, np.nan, np.inf, -2.0], [3.0, 3.0, -np.inf, 0.0]], dtype=np.float32)
    rm = np.array([[1.0, 0.0], [2.0, np.nan]])
    cm = np.array([[0.0, 1.0], [1.0, 2.0], [0.0, 1.0], [-2.0, 0.0]])
    with np.errstate(all="ignore"):
        s = scores.astype(np.float64)
        t_r = (s - rm[:, None, 0]) / rm[:, None, 1]
        t_c = (s - cm[None, :, 0]) / cm[None, :, 1]
        want = {"t": t_r, "z": t_c, "s": 0.5 * (t_r + t_c)}
    assert np.isnan(want["t"][0, 0]) and want["t"][0, 3] == -np.inf and want["z"][1, 3] == np.inf      # 0/0, -3/0, 2/0
    for mode, (use_r, use_c) in MODES.items():
        got = eng.score_norm(scores, rm if use_r else None, cm if use_c else None).cpu().numpy()
        np.testing.assert_array_equal(got, want[mode].astype(np.float32))       # NaNs in the same places, infinities by sign
    out = eng.score_norm(torch.zeros((0, 4), dtype=torch.float32, device=eng.device), None, cm)
    assert tuple(out.shape) == (0, 4)
    out = eng.score_norm_pairs(torch.zeros((0,), dtype=torch.float32, device=eng.device), rm, [], None, None)
    assert tuple(out.shape) == (0,)


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("n", [1, 257, 100_003])
def test_pairs_equal_the_matrix_entries(eng, n, mode):
    n_a, n_b = 130, 65
    scores, ma, mb = problem(n_a, n_b, 77)
    use_a, use_b = MODES[mode]
    rng = np.random.default_rng(n)
    ia, ib = rng.integers(0, n_a, n), rng.integers(0, n_b, n)
    matrix = eng.score_norm(scores, ma if use_a else None, mb if use_b else None).cpu().numpy()
    trial = torch.from_numpy(scores[ia, ib]).to(eng.device)
    args = (ma if use_a else None, ia if use_a else None, mb if use_b else None, ib if use_b else None)
    bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    got = eng.score_norm_pairs(trial, *args, bad_count=bad)
    assert got.cpu().numpy().tobytes() == matrix[ia, ib].tobytes() and int(bad.item()) == 0
    want, quot = ref.norm_longdouble(scores, ma if use_a else None, mb if use_b else None)
    assert np.all(np.abs(got.cpu().numpy().astype(LD) - want[ia, ib]) <= ref.norm_bound(want[ia, ib], quot[ia, ib]))
    # a 4-byte aligned list, and in place
    buf = torch.zeros((n + 5,), dtype=torch.float32, device=eng.device)
    odd = buf[1:n + 1]
    odd.copy_(trial)
    assert odd.data_ptr() % 16 == 4
    out = eng.score_norm_pairs(odd, *args, out=odd)
    assert out.data_ptr() == odd.data_ptr() and out.cpu().numpy().tobytes() == matrix[ia, ib].tobytes()


def test_bad_indices_give_nan_and_are_counted(eng):
    n_a, n_b, n = 130, 65, 1000
    scores, ma, mb = problem(n_a, n_b, 78)
    rng = np.random.default_rng(9)
    ia, ib = rng.integers(0, n_a, n), rng.integers(0, n_b, n)
    trial = scores[ia, ib]
    want = eng.score_norm_pairs(trial, ma, ia, mb, ib).cpu().numpy()
    bad_a, bad_b = ia.copy(), ib.copy()
    bad_a[[3, 500]] = (-1, n_a)
    bad_b[[3, 998, 999]] = (n_b, -7, 1 << 40)
    bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    got = eng.score_norm_pairs(trial, ma, bad_a, mb, bad_b, bad_count=bad).cpu().numpy()
    hit = np.zeros(n, dtype=bool)
    hit[[3, 500, 998, 999]] = True
    assert int(bad.item()) == 4 and np.isnan(got[hit]).all()
    assert got[~hit].tobytes() == want[~hit].tobytes()
    # a table that is not given is not indexed: its bad indices do not matter
    bad.zero_()
    only_a = eng.score_norm_pairs(trial, ma, ia, None, None, bad_count=bad).cpu().numpy()
    assert int(bad.item()) == 0 and not np.isnan(only_a).any()
    got = eng.score_norm_pairs(trial, ma, bad_a, mb, bad_b).cpu().numpy()        # no counter: still NaN
    assert np.isnan(got[hit]).all()


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    lib, n_rows, n_cols = eng.lib, 6, 100
    scores, rm, cm = problem(n_rows, n_cols, 4)
    sc = ref.place_rows(eng, scores, n_cols, 0)
    out = torch.empty((n_rows * n_cols + 4,), dtype=torch.float32, device=eng.device)
    rm, cm = eng.to_device(rm), eng.to_device(cm)
    idx = torch.zeros((n_rows * n_cols,), dtype=torch.int64, device=eng.device)
    bad = torch.zeros((2,), dtype=torch.int32, device=eng.device)

    def matrix(**kw):
        a = dict(ctx=eng.ctx, scores=sc.data_ptr(), n_rows=n_rows, n_cols=n_cols, stride=n_cols, rm=rm.data_ptr(), cm=cm.data_ptr(),
                 out=out.data_ptr(), out_stride=n_cols)
        a.update(kw)
        return lib.svk_score_norm(a["ctx"], a["scores"], a["n_rows"], a["n_cols"], a["stride"], a["rm"], a["cm"], a["out"],
                                  a["out_stride"])

    def pairs(**kw):
        a = dict(ctx=eng.ctx, scores=sc.data_ptr(), n=n_rows * n_cols, ma=rm.data_ptr(), n_a=n_rows, mb=cm.data_ptr(), n_b=n_cols,
                 ia=idx.data_ptr(), ib=idx.data_ptr(), out=out.data_ptr(), bad=bad.data_ptr())
        a.update(kw)
        return lib.svk_score_norm_pairs(a["ctx"], a["scores"], a["n"], a["ma"], a["n_a"], a["mb"], a["n_b"], a["ia"], a["ib"],
                                        a["out"], a["bad"])

    eng._stream()
    assert matrix() == _lib.SVK_OK and matrix(rm=None) == _lib.SVK_OK and matrix(cm=None) == _lib.SVK_OK
    assert matrix(n_rows=0, scores=None, out=None) == _lib.SVK_OK and matrix(n_cols=0, scores=None, out=None) == _lib.SVK_OK
    cases = dict(null_ctx=dict(ctx=None), null_scores=dict(scores=None), null_out=dict(out=None), no_table=dict(rm=None, cm=None),
                 negative_rows=dict(n_rows=-1), negative_cols=dict(n_cols=-1), short_stride=dict(stride=n_cols - 1),
                 short_out_stride=dict(out_stride=n_cols - 1), in_place_with_another_stride=dict(out=sc.data_ptr(), out_stride=n_cols + 4), scores_2_bytes_off=dict(scores=sc.data_ptr() + 2),
                 out_1_byte_off=dict(out=out.data_ptr() + 1), rows_4_bytes_off=dict(rm=rm.data_ptr() + 4),
                 cols_4_bytes_off=dict(cm=cm.data_ptr() + 4))
    for name, kw in cases.items():
        assert matrix(**kw) == _lib.SVK_ERR_BAD_ARG, name
    assert matrix() == _lib.SVK_OK

    assert pairs() == _lib.SVK_OK and pairs(bad=None) == _lib.SVK_OK
    assert pairs(ma=None, ia=None) == _lib.SVK_OK and pairs(mb=None, ib=None) == _lib.SVK_OK
    assert pairs(n=0, scores=None, out=None) == _lib.SVK_OK
    cases = dict(null_ctx=dict(ctx=None), null_scores=dict(scores=None), null_out=dict(out=None), no_table=dict(ma=None, mb=None),
                 table_a_without_indices=dict(ia=None), table_b_without_indices=dict(ib=None), negative_n=dict(n=-1),
                 negative_n_a=dict(n_a=-1), negative_n_b=dict(n_b=-1), scores_2_bytes_off=dict(scores=sc.data_ptr() + 2),
                 out_1_byte_off=dict(out=out.data_ptr() + 1), table_4_bytes_off=dict(ma=rm.data_ptr() + 4),
                 indices_4_bytes_off=dict(ib=idx.data_ptr() + 4), counter_2_bytes_off=dict(bad=bad.data_ptr() + 2))
    for name, kw in cases.items():
        assert pairs(**kw) == _lib.SVK_ERR_BAD_ARG, name
    assert pairs() == _lib.SVK_OK
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.score_norm(scores, rm[:-1], None)
    with pytest.raises(ValueError):
        eng.score_norm_pairs(scores.reshape(-1), rm, idx[:5], None, None)
