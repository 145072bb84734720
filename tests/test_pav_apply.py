"""svk_pav_apply: the output bits against tests/rocch_ref.py's step map, on every path the entry takes -- the table in LDS and
(above 4 096 bins) in global memory, 16-byte loads between a scalar head and tail when scores and output are equally placed,
scalar ones otherwise, in place and out of place -- with scores on, one ulp above and one ulp below every kind of edge."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rocch_ref as R                    # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 4099)
BINS = (1, 2, 33, 3177, 4096, 4097)      # 4 096 is the LDS table's bound (include/svk.h, "the PAV map")
# (floats past a 256-byte boundary of the scores, of the output); None: in place
PLACED = {"aligned": (0, 0), "aligned-in-place": (0, None), "one-past": (1, 1), "one-past-in-place": (1, None),
          "scores-one-past": (1, 0), "two-and-three-past": (2, 3)}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def table(n_bins):
    """Descending distinct edges with 0.0 among them (from two bins on), LLRs of every kind, a +inf and a -inf included."""
    rng = np.random.default_rng(n_bins)
    edges = np.sort(np.unique(np.r_[rng.standard_normal(4 * n_bins).astype(np.float32), np.float32(0.0)]))[::-1]
    zero = int(np.flatnonzero(edges == 0)[0])
    lo = min(max(0, zero - n_bins // 2), edges.size - n_bins)
    edges = edges[lo:lo + n_bins].copy()
    assert edges.size == n_bins and (n_bins == 1 or 0.0 in edges) and (np.diff(edges) < 0).all()
    llr = rng.standard_normal(n_bins).astype(np.float32) * 10
    llr[0], llr[-1] = (np.inf, -np.inf) if n_bins > 1 else (1.5, 1.5)
    return edges, llr


def scores_for(edges, n, seed):
    """n scores drawn from: every edge, one ulp above and below it, -0.0 and +0.0, beyond both ends, +-inf, NaN, others."""
    rng = np.random.default_rng(seed)
    up, down = np.nextafter(edges, np.float32(np.inf)), np.nextafter(edges, np.float32(-np.inf))
    special = np.array([-0.0, 0.0, edges[0] + 1, edges[-1] - 1, np.inf, -np.inf, np.nan, 3e38, -3e38], np.float32)
    pool = np.r_[edges, up, down, special, rng.standard_normal(16).astype(np.float32)]
    head = np.r_[edges[:1], down[:1], special[6:7], special[:1], up[-1:], special[1:6], special[7:], up[:1], edges[-1:], down[-1:]]
    return np.ascontiguousarray(rng.permutation(np.r_[head, rng.choice(pool, n)].astype(np.float32)[:n]))      # the head always takes part


def placed(eng, host, floats_past):
    """`host` on the device, `floats_past` floats behind a 256-byte boundary; the floats around it hold a pattern."""
    buf = torch.full((host.size + 128,), 777.0, dtype=torch.float32, device=eng.device)
    at = (-(buf.data_ptr() // 4)) % 64 + floats_past
    view = buf[at:at + host.size]
    assert view.data_ptr() % 256 == 4 * floats_past
    view.copy_(torch.from_numpy(host.copy()))
    return buf, view


@pytest.mark.parametrize("where", list(PLACED))
@pytest.mark.parametrize("n_bins", BINS)
def test_bits_of_the_step_map(eng, n_bins, where):
    edges, llr = table(n_bins)
    d_edges, d_llr = eng.to_device(edges), eng.to_device(llr)
    s_off, o_off = PLACED[where]
    for n in SIZES:
        sc = scores_for(edges, n, 1000 * n_bins + n)
        want = R.pav_apply(sc, edges, llr)
        if n_bins <= 33:                                  # the counting form against the definition's loop
            by_loop = [s.view(np.uint32) if k is None else llr[k].view(np.uint32) for s, k in ((s, R.pav_map(s, edges)) for s in sc)]
            assert np.array_equal(np.array(by_loop, np.uint32), want)
        sbuf, sview = placed(eng, sc, s_off)
        if o_off is None:
            obuf, oview = sbuf, sview
        else:
            obuf, oview = placed(eng, np.full(n, 555.0, np.float32), o_off)
        got = eng.pav_apply(sview, d_edges, d_llr, out=oview)
        assert got.data_ptr() == oview.data_ptr()
        torch.cuda.synchronize()
        what = "n_bins %d, %s, n %d" % (n_bins, where, n)
        assert np.array_equal(oview.cpu().numpy().view(np.uint32), want), what
        rest = obuf.cpu().numpy().copy()
        at = (oview.data_ptr() - obuf.data_ptr()) // 4
        rest[at:at + n] = 777.0
        assert (rest == 777.0).all(), what + ": written outside the output"
        if o_off is not None:
            assert np.array_equal(sview.cpu().numpy().view(np.uint32), sc.view(np.uint32)), what + ": the scores changed"
    # a fresh output from the wrapper
    sc = scores_for(edges, 4099, 5)
    assert np.array_equal(eng.pav_apply(sc, edges, llr).cpu().numpy().view(np.uint32), R.pav_apply(sc, edges, llr))


def test_signed_zero_against_an_edge_of_zero(eng):
    edges, llr = np.array([1.0, 0.0, -1.0], np.float32), np.array([3.0, 2.0, 1.0], np.float32)
    sc = np.array([-0.0, 0.0, -1e-45, 1e-45, np.nan], np.float32)
    got = eng.pav_apply(sc, edges, llr).cpu().numpy()
    assert got[:4].tolist() == [2.0, 2.0, 1.0, 2.0] and got[4:].view(np.uint32) == sc[4:].view(np.uint32)


def test_refusals(eng):
    from speaker_verification_amd import _lib
    t = torch.zeros(8, dtype=torch.float32, device=eng.device)
    p = eng._ptr(t)
    eng._stream()
    call = lambda *a: eng.lib.svk_pav_apply(eng.ctx, *a)                 # noqa: E731
    assert call(p, 8, p, p, 0, p) == _lib.SVK_ERR_BAD_ARG and b"n_bins" in eng.lib.svk_last_error(eng.ctx)
    assert call(p, 8, p, p, -3, p) == _lib.SVK_ERR_BAD_ARG
    for args in ((None, 8, p, p, 1, p), (p, 8, None, p, 1, p), (p, 8, p, None, 1, p), (p, 8, p, p, 1, None)):
        assert call(*args) == _lib.SVK_ERR_BAD_ARG and b"NULL" in eng.lib.svk_last_error(eng.ctx)
    assert call(p, -1, p, p, 1, p) == _lib.SVK_ERR_BAD_ARG
    assert call(None, 0, p, p, 1, None) == 0                             # n == 0 launches nothing
    with pytest.raises(ValueError):
        eng.pav_apply(t, np.zeros(0, np.float32), np.zeros(0, np.float32))
    torch.cuda.synchronize()
    assert not t.any()
