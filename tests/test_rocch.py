"""svk_rocch: the ROC convex hull on the device against the Python-integer reference of tests/rocch_ref.py -- the vertices
exactly, their scores bit for bit, svk_roc_dcf's values bit for bit -- on the smallest shapes at which each stage can go wrong
(rocch_ref.gpu_cases: one thread's chain, the LDS levels, the tile boundary, the first global merge with a one-point right
hull, many tiles, a hull that keeps every point across tiles), and the values derived from the hull."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rocch_ref as R                    # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

OPS = R.OPS
DCF_KEYS = ("eer", "auc", "positives", "points", "eer_threshold", "min_dcf", "threshold", "p_miss", "p_fa")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def f64bits(res, keys):
    """The dict's values under `keys` as the bits of their doubles: -0.0 differs from +0.0, as "bit for bit" asks."""
    flat = [v for k in keys for v in (res[k] if isinstance(res[k], list) else [res[k]])]
    return np.asarray(flat, dtype=np.float64).view(np.uint64).tolist()


def same_result(a, b):
    keys = DCF_KEYS + ("min_cllr", "rocch_eer")
    return f64bits(a, keys) == f64bits(b, keys) and np.array_equal(a["vertices"], b["vertices"]) \
        and np.array_equal(a["vertex_scores"].view(np.uint32), b["vertex_scores"].view(np.uint32))


@pytest.mark.parametrize("name", list(R.gpu_cases()))
def test_against_the_reference(eng, name):
    lab, sc = R.gpu_cases()[name]
    pts, vals, keep = R.reference(name)
    res = eng.rocch(sc, lab, OPS)
    want = np.array([pts[i] for i in keep], dtype=np.int64)
    print(name, "points", len(pts), "vertices", len(keep), "device", len(res["vertices"]))
    assert res["vertices"].dtype == np.int64 and np.array_equal(res["vertices"], want)
    want_sc = np.array([np.inf] + [vals[i] for i in keep[1:]], dtype=np.float32)
    assert np.array_equal(res["vertex_scores"].view(np.uint32), want_sc.view(np.uint32))
    # svk_roc_dcf's values, bit for bit, with and without operating points
    dcf = eng.roc_dcf(sc, lab, OPS)
    assert f64bits(res, DCF_KEYS) == f64bits(dcf, DCF_KEYS) and res["points"] == len(pts) - 1
    none = eng.rocch(sc, lab)
    assert none["min_dcf"] == [] and np.array_equal(none["vertices"], want)
    assert f64bits(none, DCF_KEYS[:5]) == f64bits(dcf, DCF_KEYS[:5])
    # a second run, and the trials stored sorted instead of shuffled
    assert same_result(eng.rocch(sc, lab, OPS), res)
    order = np.argsort(-sc.astype(np.float64), kind="stable")
    assert same_result(eng.rocch(sc[order], lab[order], OPS), res)
    assert same_result(eng.rocch(sc[order[::-1]], lab[order[::-1]], OPS), res)
    # the derived values
    v = [tuple(int(x) for x in row) for row in want]
    K = len(v) - 1
    ref = R.min_cllr(v)
    print(name, "min_cllr", res["min_cllr"], "reference", ref, "rocch_eer", res["rocch_eer"], "eer", res["eer"])
    assert abs(res["min_cllr"] - ref) <= (K + 4) * 2.0 ** -52 * ref and res["min_cllr"] <= 1.0
    assert abs(res["rocch_eer"] - float(R.rocch_eer(v))) <= 4 * 2.0 ** -52
    assert res["rocch_eer"] <= res["eer"]
    # per operating point the cheapest hull vertex costs what the cheapest point costs (exact rationals from the integers)
    N, P = v[-1]
    for p, c_miss, c_fa in OPS:
        a, b = Fraction(c_miss) * Fraction(p), Fraction(c_fa) * (1 - Fraction(p))
        den = a.denominator * b.denominator
        ai, bi = int(a * den), int(b * den)                                          # the cost times den N P, an integer
        cost = lambda q: ai * (P - q[1]) * N + bi * q[0] * P                         # noqa: E731
        assert min(cost(q) for q in v) == min(cost(q) for q in pts)


def test_calibration_entry_points(eng):
    from speaker_verification_amd import calibration as cal
    lab, sc = R.gpu_cases()["farey_8"]
    res = eng.rocch(sc, lab)
    assert cal.min_cllr(sc, lab, engine=eng) == res["min_cllr"] and cal.rocch_eer(sc, lab, engine=eng) == res["rocch_eer"]
    lab, sc = R.gpu_cases()["inverted"]
    assert cal.min_cllr(sc, lab, engine=eng) == 1.0


def _direct(eng, sc, lab, capacity, work_bytes=None, n_op=1):
    s, l = eng.to_device(sc, torch.float32), eng.to_device(lab, torch.uint8)
    need = int(eng.lib.svk_rocch_workspace_bytes(s.numel()))
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    planes = torch.full((3, max(capacity, 1)), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    ops = (C.c_double * 3)(0.01, 1, 1)
    out = (C.c_double * 10)(*([-7.0] * 10))
    eng._stream()
    rc = eng.lib.svk_rocch(eng.ctx, eng._ptr(s), eng._ptr(l), s.numel(), ops, n_op, eng._ptr(work),
                           need if work_bytes is None else work_bytes, eng._ptr(planes[0]), eng._ptr(planes[1]),
                           eng._ptr(planes[2]), capacity, out)
    torch.cuda.synchronize()
    return rc, list(out), planes.cpu().numpy(), eng.lib.svk_last_error(eng.ctx) or b""


def test_refusals(eng):
    from speaker_verification_amd import _lib
    lab, sc = R.gpu_cases()["points_2049"]
    x = sc.copy()
    x[77] = np.nan
    with pytest.raises(_lib.SvkError, match="non-finite"):
        eng.rocch(x, lab, OPS)
    for one in (np.zeros_like(lab), np.ones_like(lab)):
        with pytest.raises(_lib.SvkError, match="one class"):
            eng.rocch(sc, one, OPS)
    with pytest.raises(_lib.SvkError, match="at least two"):
        eng.rocch(sc[:1], lab[:1], OPS)
    with pytest.raises(_lib.SvkError, match="operating points"):
        eng.rocch(sc, lab, [(0.01, 1, 1)] * 9)
    count = len(R.reference("points_2049")[2])
    need = int(eng.lib.svk_rocch_workspace_bytes(sc.size))
    rc, out, planes, err = _direct(eng, sc, lab, count, work_bytes=need - 1)
    assert rc == _lib.SVK_ERR_BAD_ARG and b"svk_rocch_workspace_bytes" in err and out == [-7.0] * 10
    assert (planes == 0x5A5A5A5A).all()
    # capacity one below the count: the count is named, the planes and h_out stay as they were
    rc, out, planes, err = _direct(eng, sc, lab, count - 1)
    assert rc == _lib.SVK_ERR_BAD_ARG and (b"%d vertices" % count) in err and out == [-7.0] * 10
    assert (planes == 0x5A5A5A5A).all()
    rc, out, planes, err = _direct(eng, sc, lab, count)
    assert rc == 0 and out[9] == count and out[0] == eng.roc_eer(sc, lab)[0]
    assert planes[0].view(np.uint32).tolist() == [R.reference("points_2049")[0][i][0] for i in R.reference("points_2049")[2]]
    rc, _, _, err = _direct(eng, sc, lab, 0)
    assert rc == _lib.SVK_ERR_BAD_ARG and b"capacity" in err
