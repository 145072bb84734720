"""The memory contract of include/svk.h (Conventions) for the evaluation entries: svk_roc_eer, svk_roc_k, svk_roc_dcf,
svk_decision_counts, svk_top1, svk_calibration_stats, svk_calibration_apply, svk_cohort_moments, svk_score_norm and
svk_score_norm_pairs, called directly on guarded arenas (tests/memory_contract.py) in the environments A, B and C; the
properties P1-P4 as tests/test_memory_contract_scoring.py states them, and P5: where the header allows d_out == d_scores, the
in-place result equals the out-of-place result byte for byte.  Host results (h_out, h_count, ...) are compared as bits with what
the Engine wrapper returns for the same call on ordinary buffers, and must not be written past their documented length."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f64bits(values):
    return np.asarray(list(values), dtype=np.float64).view(np.uint64)


def _host(ctype, n, sentinel, extra=4):
    """A host result array of n entries with `extra` sentinel entries behind them."""
    return (ctype * (n + extra))(*([sentinel] * (n + extra)))


def _host_tail_kept(arr, n, sentinel, what):
    assert list(arr[n:]) == [sentinel] * (len(arr) - n), what + ": the host result was written past its %d entries" % n


# ---- svk_roc_eer, svk_roc_dcf, svk_roc_k -------------------------------------------------------------------------------------
def _roc_case(n, ties, k=1):
    """Scores (heavy ties: multiples of 1/2; or continuous) and labels with both classes in every split of n // k."""
    s = M.randn(n + int(ties), n)
    if ties:
        s = torch.round(s * 2.0) / 2.0
    lb = (torch.rand((n,), generator=_gen(n)) < 0.3).to(torch.uint8)
    step = n // k
    for j in range(k):
        lb[j * step], lb[j * step + 1] = 1, 0
    s[0] = -0.0 if n > 2 else s[0]
    return s, lb


OPS = ((0.01, 1.0, 1.0), (0.05, 10.0, 1.0))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("ties", (True, False), ids=("heavy-ties", "continuous"))
@pytest.mark.parametrize("n", (2, 2049, 100003))
def test_roc_eer_and_dcf(eng, n, ties, placed):
    s, lb = _roc_case(n, ties)
    eer, auc = eng.roc_eer(s, lb)
    dcf = eng.roc_dcf(s, lb, OPS)
    want_dcf = [dcf["eer"], dcf["auc"], dcf["positives"], dcf["points"], dcf["eer_threshold"]]
    for o in range(len(OPS)):
        want_dcf += [dcf[name][o] for name in ("min_dcf", "threshold", "p_miss", "p_fa")]
    ops = (C.c_double * (3 * len(OPS)))(*[v for op in OPS for v in op])
    seen = []
    for env in M.ENV_NAMES:
        what = "n %d ties %s, %s, environment %s" % (n, ties, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, dl = c.input("d_scores", s), c.input("d_labels", lb)
        nbytes = eng.lib.svk_roc_workspace_bytes(n)
        work, out = c.workspace(nbytes), _host(C.c_double, 4, -5.0)
        c.call(eng.lib.svk_roc_eer, ds, dl, n, work, nbytes, out)
        _host_tail_kept(out, 4, -5.0, "svk_roc_eer " + what)
        M.same_bits(_f64bits(out[:2]), _f64bits((eer, auc)), "svk_roc_eer " + what)
        seen.append(list(out[:4]))

        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, dl = c.input("d_scores", s), c.input("d_labels", lb)
        nbytes = eng.lib.svk_roc_dcf_workspace_bytes(n)
        n_out = 5 + 4 * len(OPS)
        work, out = c.workspace(nbytes), _host(C.c_double, n_out, -5.0)
        c.call(eng.lib.svk_roc_dcf, ds, dl, n, ops, len(OPS), work, nbytes, out)
        _host_tail_kept(out, n_out, -5.0, "svk_roc_dcf " + what)
        M.same_bits(_f64bits(out[:n_out]), _f64bits(want_dcf), "svk_roc_dcf " + what)
        M.same_bits(_f64bits(out[:4]), _f64bits(seen[-1]), "svk_roc_dcf's first four against svk_roc_eer, " + what)
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("ties", (True, False), ids=("heavy-ties", "continuous"))
@pytest.mark.parametrize("n,k", ((2, 1), (6, 3), (2049, 3), (100003, 3)))
def test_roc_k_curve_planes(eng, n, k, ties, placed):
    """k = 3: the splits' bases are not 16-byte aligned (683 and 33 334 pairs per split) and the last n - 3 step pairs are
    ignored.  n = 2 allows one split only (a split needs two pairs); n = 6 is the smallest three-split call.  Plane entries at
    and past a split's curve points are not written."""
    s, lb = _roc_case(n, ties, k)
    step = n // k
    ref = eng.roc_k(s, lb, k=k, curve=True)
    for env in M.ENV_NAMES:
        what = "svk_roc_k n %d k %d ties %s, %s, environment %s" % (n, k, ties, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, dl = c.input("d_scores", s), c.input("d_labels", lb)
        nbytes = eng.lib.svk_roc_k_workspace_bytes(n, k)
        work, out = c.workspace(nbytes), _host(C.c_double, 4 * k, -5.0)
        planes = c.output("d_curve", torch.int32, (2, k, step + 1))
        c.call(eng.lib.svk_roc_k, ds, dl, n, k, work, nbytes, planes, out)
        _host_tail_kept(out, 4 * k, -5.0, what)
        got = planes.bits()
        for j in range(k):
            length = int(out[4 * j + 3])
            assert 2 <= length <= step + 1
            M.same_bits(_f64bits(out[4 * j:4 * j + 2]), _f64bits(ref[j][:2]), what + ": split %d eer, auc" % j)
            for p in (0, 1):
                cnt = got[p, j, :length].astype(np.float64)
                M.same_bits((cnt / cnt[-1]).view(np.uint64), ref[j][2 + p].view(np.uint64), what + ": split %d plane %d" % (j, p))
                M.keeps_prefill(planes, got[p, j, length:], what + ": split %d plane %d past its %d points" % (j, p, length))
        # without the planes: the same host results
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, dl = c.input("d_scores", s), c.input("d_labels", lb)
        work, out2 = c.workspace(nbytes), _host(C.c_double, 4 * k, -5.0)
        c.call(eng.lib.svk_roc_k, ds, dl, n, k, work, nbytes, None, out2)
        assert list(out2) == list(out), what + ": d_curve == NULL changes the host results"


# ---- svk_decision_counts, svk_top1 ------------------------------------------------------------------------------------------
def _thresholds(n_thr):
    return np.concatenate(([-np.inf], np.linspace(-1.5, 1.5, n_thr - 1))).astype(np.float32)[:n_thr] if n_thr > 1 else \
        np.array([0.25], dtype=np.float32)


def _decision_direct(eng, env, placed, s, lb, thr):
    n, n_thr = s.numel(), thr.size
    c = M.Contract(eng, env, scalar=placed == "scalar")
    ds, dl = c.input("d_scores", s), c.input("d_labels", lb)
    out = _host(C.c_int64, 2 * n_thr + 2, -5)
    c.call(eng.lib.svk_decision_counts, ds, dl, n, thr.ctypes.data_as(C.POINTER(C.c_float)), n_thr, out)
    _host_tail_kept(out, 2 * n_thr + 2, -5, "svk_decision_counts")
    return list(out[:2 * n_thr + 2])


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n_thr", (1, 4, 16))
@pytest.mark.parametrize("n", (1, 5, 4099))
def test_decision_counts(eng, n, n_thr, placed):
    s = torch.round(M.randn(n + n_thr, n) * 4.0) / 4.0
    if n > 1:
        s[1] = NAN                                                   # never accepted, counted in its class only
    lb = (torch.rand((n,), generator=_gen(n)) < 0.4).to(torch.uint8)
    thr = _thresholds(n_thr)
    accepted, totals = eng.decision_counts(s, lb, thr)
    want = [int(v) for v in accepted.reshape(-1)] + [int(totals[0]), int(totals[1])]
    for env in M.ENV_NAMES:
        assert _decision_direct(eng, env, placed, s, lb, thr) == want, "svk_decision_counts n %d with %d thresholds, %s, " \
            "environment %s" % (n, n_thr, placed, env)


def test_decision_counts_and_top1_on_a_handle_whose_workspace_is_regrown(eng):
    """svk_decision_counts keeps its counters in ctx->work, svk_top1 its hit counter in the handle's fixed scratch; neither can
    be guarded.  On a FRESH handle, whose workspace starts empty: each call (svk_decision_counts makes the handle allocate 4
    KiB), a svk_cosine_scores call that makes it free that block and allocate 32 KiB, each call again -- the same counts and
    bytes, equal to the long-lived handle's.  For svk_top1 this shows that its counter starts from zero at every call."""
    from speaker_verification_amd.engine import Engine
    s = torch.round(M.randn(3, 4099) * 4.0) / 4.0
    lb = (torch.rand((4099,), generator=_gen(4)) < 0.4).to(torch.uint8)
    thr = _thresholds(16)
    sc, tr = M.randn(5, 300, 65), torch.arange(300, dtype=torch.int32) % 65
    want, want_top = _decision_direct(eng, "B", "vector", s, lb, thr), _top1_direct(eng, "B", "vector", sc, tr)
    fresh = Engine(eng.device_index)
    assert _decision_direct(fresh, "B", "vector", s, lb, thr) == want
    first_top = _top1_direct(fresh, "B", "vector", sc, tr)
    fresh.cosine_scores(M.randn(1, 1024, 8), M.randn(2, 8192, 8))
    assert _decision_direct(fresh, "A", "vector", s, lb, thr) == want
    again_top = _top1_direct(fresh, "A", "vector", sc, tr)
    for got in (first_top, again_top):
        M.same_bits(got[0], want_top[0], "d_argmax")
        M.same_bits(got[1], want_top[1], "d_labels")
        assert got[2] == want_top[2]


def _top1_direct(eng, env, placed, sc, tr):
    n_rows, n_cols = sc.shape
    c = M.Contract(eng, env, scalar=placed == "scalar")
    ds, dt = c.input("d_scores", sc), c.input("d_true", tr)
    amax, lab = c.output("d_argmax", torch.int32, (n_rows,)), c.output("d_labels", torch.uint8, (n_rows, n_cols))
    correct = _host(C.c_int64, 1, -5)
    c.call(eng.lib.svk_top1, ds, n_rows, n_cols, dt, amax, lab, correct)
    _host_tail_kept(correct, 1, -5, "svk_top1")
    return amax.bits(), lab.bits(), int(correct[0])


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n_rows,n_cols", ((37, 1), (5, 64), (300, 65)))
def test_top1(eng, n_rows, n_cols, placed):
    sc = M.randn(n_rows + n_cols, n_rows, n_cols)
    sc[n_rows // 2, n_cols // 2] = NAN                               # a NaN is the maximum
    tr = torch.argmax(torch.nan_to_num(sc, nan=INF), dim=1).to(torch.int32)
    tr[::3] = -1                                                     # not enrolled: an all-zero label row
    tr[1::5] = (tr[1::5] + 1) % n_cols
    amax, correct, labels = eng.top1(sc, tr, want_labels=True)
    for env in M.ENV_NAMES:
        what = "svk_top1 %dx%d, %s, environment %s" % (n_rows, n_cols, placed, env)
        got = _top1_direct(eng, env, placed, sc, tr)
        M.same_bits(got[0], M.bits(amax), what + ": d_argmax")
        M.same_bits(got[1], M.bits(labels), what + ": d_labels")
        assert got[2] == correct, what + ": h_correct"


# ---- svk_calibration_stats, svk_calibration_apply ---------------------------------------------------------------------------
def _calibration_case(eng, n_sys, n):
    """Scores as planes n + 3 apart (one system: n), labels, weights; the wrapper gets a device view of the same layout."""
    s = M.randn(n_sys * 7 + n % 97, n_sys, n) * 2.0
    if n >= 5:
        s[n_sys - 1, 3], s[0, n - 1] = NAN, -INF                     # skipped trials (the statistics); IEEE results (apply)
    lb = (torch.rand((n,), generator=_gen(n + n_sys)) < 0.35).to(torch.uint8)
    w = np.linspace(0.5, 1.5, n_sys + 1)
    stride = n + 3 if n_sys > 1 else n
    dev = torch.full((n_sys, stride), 123.0, dtype=torch.float32, device=eng.device)[:, :n]
    dev.copy_(s)
    return s, lb, w, stride, dev


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 5, 1027, 300001))
@pytest.mark.parametrize("n_sys", (1, 2, 8))
def test_calibration_stats(eng, n_sys, n, placed):
    s, lb, w, stride, dev = _calibration_case(eng, n_sys, n)
    tau, cw = -1.25, np.array([0.7, 0.3])
    dim = n_sys + 1
    n_full = 2 + dim + dim * (dim + 1) // 2
    l_tar, l_non, grad, hess, counts = eng.calibration_stats(dev, lb, w, tau, cw)
    want = [l_tar, l_non] + list(grad) + list(hess[np.triu_indices(dim)])
    value = eng.calibration_stats(dev, lb, w, tau, cw, value_only=True)
    M.same_bits(_f64bits(value[:2]), _f64bits(want[:2]), "value only: L_tar, L_non of the full call")
    assert n < 5 or counts[2] == 2
    nbytes = eng.lib.svk_calibration_stats_workspace_bytes(n, n_sys)
    dp = C.POINTER(C.c_double)
    for env in M.ENV_NAMES:
        for flags, n_out in ((0, n_full), (1, 2)):
            what = "svk_calibration_stats n_sys %d n %d flags %d, %s, environment %s" % (n_sys, n, flags, placed, env)
            c = M.Contract(eng, env, scalar=placed == "scalar")
            ds, dl, work = c.input("d_scores", s, stride=stride), c.input("d_labels", lb), c.workspace(nbytes)
            out, count = _host(C.c_double, n_out, -5.0), _host(C.c_int64, 3, -5)
            c.call(eng.lib.svk_calibration_stats, ds, n_sys, stride, dl, n, w.ctypes.data_as(dp), tau, cw.ctypes.data_as(dp),
                   flags, work, nbytes, out, count)
            _host_tail_kept(out, n_out, -5.0, what)
            _host_tail_kept(count, 3, -5, what)
            M.same_bits(_f64bits(out[:n_out]), _f64bits(want[:n_out]), what)
            assert tuple(count[:3]) == counts, what + ": h_count"


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 5, 1027, 300001))
@pytest.mark.parametrize("n_sys", (1, 2, 8))
def test_calibration_apply(eng, n_sys, n, placed):
    s, _, w, stride, dev = _calibration_case(eng, n_sys, n)
    ref = M.bits(eng.calibration_apply(dev, w))
    dp = C.POINTER(C.c_double)
    for env in M.ENV_NAMES:
        what = "svk_calibration_apply n_sys %d n %d, %s, environment %s" % (n_sys, n, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, out = c.input("d_scores", s, stride=stride), c.output("d_out", torch.float32, (n,))
        c.call(eng.lib.svk_calibration_apply, ds, n_sys, stride, n, w.ctypes.data_as(dp), out)
        M.same_bits(out.bits(), ref, what)
        if n_sys == 1:               # P5: in place
            c = M.Contract(eng, env, scalar=placed == "scalar")
            both = c.output("d_scores == d_out", torch.float32, (n,), prefill=s[0])
            c.call(eng.lib.svk_calibration_apply, both, 1, n, n, w.ctypes.data_as(dp), both)
            M.same_bits(both.bits(), ref, what + ", in place")


# ---- svk_cohort_moments ----------------------------------------------------------------------------------------------------
def _strided_on_device(eng, t, stride):
    """`t` [rows, cols] on the device with its rows `stride` apart: the view the wrapper takes as it is."""
    dev = torch.full((t.shape[0], stride), 123.0, dtype=torch.float32, device=eng.device)[:, :t.shape[1]]
    dev.copy_(t)
    return dev


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("pad", (0, 3), ids=("stride-n", "stride-n+3"))
@pytest.mark.parametrize("top_k", (0, 20))
@pytest.mark.parametrize("n_cohort", (63, 2049, 16385))
def test_cohort_moments(eng, n_cohort, top_k, pad, placed):
    n_rows, stride = 6, n_cohort + pad                               # four rows share a workgroup below 2 049: two groups
    s = M.randn(n_cohort + top_k, n_rows, n_cohort)
    s[1] = torch.round(s[1] * 2.0) / 2.0                             # ties around the k-th value
    s[2, ::7], s[2, 5], s[2, 6] = NAN, INF, -INF                     # never candidates
    s[3] = 0.25                                                      # all equal: the case of its own
    s[4] = NAN                                                       # no candidate: NaN, NaN
    ref = tuple(M.bits(t) for t in eng.cohort_moments(_strided_on_device(eng, s, stride), top_k, want_used=True, want_kth=True))
    for env in M.ENV_NAMES:
        what = "svk_cohort_moments cohort %d top_k %d stride %d, %s, environment %s" % (n_cohort, top_k, stride, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds = c.input("d_scores", s, stride=stride)
        mom, used, kth = (c.output("d_moments", torch.float64, (n_rows, 2)), c.output("d_used", torch.int32, (n_rows,)),
                          c.output("d_kth", torch.float32, (n_rows,)))
        c.call(eng.lib.svk_cohort_moments, ds, n_rows, n_cohort, stride, top_k, mom, used, kth)
        for got, want, name in zip((mom, used, kth), ref, ("d_moments", "d_used", "d_kth")):
            M.same_bits(got.bits(), want, what + ": " + name)
        c = M.Contract(eng, env, scalar=placed == "scalar")       # the optional outputs left out: the same moments
        ds, mom = c.input("d_scores", s, stride=stride), c.output("d_moments", torch.float64, (n_rows, 2))
        c.call(eng.lib.svk_cohort_moments, ds, n_rows, n_cohort, stride, top_k, mom, None, None)
        M.same_bits(mom.bits(), ref[0], what + ": d_moments alone")


# ---- svk_score_norm, svk_score_norm_pairs ---------------------------------------------------------------------------------
def _moments(seed, n):
    g = _gen(seed)
    return torch.stack((torch.randn((n,), generator=g, dtype=torch.float64),
                        torch.rand((n,), generator=g, dtype=torch.float64) + 0.5), dim=1)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("pad", (0, 3), ids=("stride-n", "stride-n+3"))
@pytest.mark.parametrize("tables", ("rows", "columns", "both"))
@pytest.mark.parametrize("n_rows,n_cols", ((3, 1027), (130, 5)))
def test_score_norm(eng, n_rows, n_cols, tables, pad, placed):
    s = M.randn(n_rows, n_rows, n_cols)
    s[n_rows - 1, n_cols - 1] = INF
    rm = _moments(1, n_rows) if tables != "columns" else None
    cm = _moments(2, n_cols) if tables != "rows" else None
    if cm is not None:
        cm[1, 1] = 0.0                                               # a zero std: what IEEE arithmetic gives
    stride = n_cols + pad
    ref = M.bits(eng.score_norm(s, rm, cm))
    for env in M.ENV_NAMES:
        what = "svk_score_norm %dx%d %s stride %d, %s, environment %s" % (n_rows, n_cols, tables, stride, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, dr, dc = c.input("d_scores", s, stride=stride), c.input("d_row_moments", rm), c.input("d_col_moments", cm)
        out = c.output("d_out", torch.float32, (n_rows, n_cols), stride=stride)
        c.call(eng.lib.svk_score_norm, ds, n_rows, n_cols, stride, dr, dc, out, stride)
        M.same_bits(out.bits(), ref, what)
        c = M.Contract(eng, env, scalar=placed == "scalar")       # P5: in place; the padding between rows keeps its prefill
        dr, dc = c.input("d_row_moments", rm), c.input("d_col_moments", cm)
        both = c.output("d_scores == d_out", torch.float32, (n_rows, n_cols), stride=stride, prefill=s)
        c.call(eng.lib.svk_score_norm, both, n_rows, n_cols, stride, dr, dc, both, stride)
        M.same_bits(both.bits(), ref, what + ", in place")


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("tables", ("a", "b", "both"))
@pytest.mark.parametrize("n", (1, 5, 1027))
def test_score_norm_pairs(eng, n, tables, placed):
    n_a, n_b = 3, 130
    g = _gen(n)
    s = M.randn(n + 1, n)
    ma, mb = (_moments(3, n_a) if tables != "b" else None), (_moments(4, n_b) if tables != "a" else None)
    ia = torch.randint(0, n_a, (n,), generator=g) if ma is not None else None
    ib = torch.randint(0, n_b, (n,), generator=g) if mb is not None else None
    bad = 0
    if n >= 5:                       # one index outside its table: NaN there, counted, nothing read
        (ia if ia is not None else ib)[2] = 130 if ia is None else n_a
        bad = 1
    ref = M.bits(eng.score_norm_pairs(s, ma, ia, mb, ib))
    for env in M.ENV_NAMES:
        what = "svk_score_norm_pairs n %d tables %s, %s, environment %s" % (n, tables, placed, env)
        for in_place in (False, True):
            c = M.Contract(eng, env, scalar=placed == "scalar")
            da, db, xa, xb = c.input("d_mom_a", ma), c.input("d_mom_b", mb), c.input("d_idx_a", ia), c.input("d_idx_b", ib)
            cnt = c.counter("d_bad_count")
            if in_place:
                ds = out = c.output("d_scores == d_out", torch.float32, (n,), prefill=s)
            else:
                ds, out = c.input("d_scores", s), c.output("d_out", torch.float32, (n,))
            c.call(eng.lib.svk_score_norm_pairs, ds, n, da, n_a if ma is not None else 0, db, n_b if mb is not None else 0,
                   xa, xb, out, cnt)
            M.same_bits(out.bits(), ref, what + (", in place" if in_place else ""))
            M.counter_is(cnt, bad, what + ": d_bad_count")
