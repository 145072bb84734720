"""The memory contract of include/svk.h (Conventions) for the scoring entries: svk_cosine_scores, svk_l2_dist, svk_pair_scores,
svk_plda_pair_scores, svk_plda_scores and svk_cosine_topk, called directly on guarded arenas (tests/memory_contract.py) in the
environments A, B and C.  After every call: every guard of every input, output and workspace is intact and every input is
byte-identical (P1); every output byte equals, in all three environments, what the Engine wrapper gives for the same call on
ordinary torch.empty buffers -- the wrapper path is held to float64 elsewhere, so every comparison here is on bytes (P2); the
workspace is exactly svk_*_workspace_bytes long (P3); counters preset to 7 end at 7 plus the exact count (P4).  `placed`:
"vector" puts every buffer on a 256-byte boundary, "scalar" one element past it (the 4-byte load paths; the workspace 16 bytes
past it), "out+4" only the output (svk_cosine_scores: 16-byte loads with row segments that start 4 bytes off)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


# ---- svk_cosine_scores -----------------------------------------------------------------------------------------------------
_COSINE = {}


def _cosine_case(eng, nt, ne, dim):
    """(test rows, enrolled rows, the wrapper's score bits), made once per shape and left unchanged."""
    key = (nt, ne, dim)
    if key not in _COSINE:
        t, e = M.randn(100 + dim, nt, dim), M.randn(200 + dim, ne, dim)
        e[ne // 2] = 0.0                                             # a zero row: scores exactly 0, never NaN
        _COSINE[key] = (t, e, M.bits(eng.cosine_scores(t, e)))
    return _COSINE[key]


def _cosine_direct(eng, env, placed, t, e):
    nt, ne, dim = t.shape[0], e.shape[0], t.shape[1]
    c = M.Contract(eng, env, scalar=placed != "vector")
    same = 0 if placed == "out+4" else None
    dt, de = c.input("d_test", t, off=same), c.input("d_enroll", e, off=same)
    out = c.output("d_out", torch.float32, (nt, ne))
    c.call(eng.lib.svk_cosine_scores, dt, de, nt, ne, dim, out)
    return out.bits()


@pytest.mark.parametrize("placed", ("vector", "out+4", "scalar"))
@pytest.mark.parametrize("nt,ne,dim", ((17, 33, 128), (17, 33, 130), (65537, 65, 128), (65537, 65, 132)),
                         ids=("wave-128", "wave-130", "tiled-hoisted-128", "tiled-streamed-132"))
def test_cosine_scores(eng, nt, ne, dim, placed):
    t, e, ref = _cosine_case(eng, nt, ne, dim)
    for env in M.ENV_NAMES:
        M.same_bits(_cosine_direct(eng, env, placed, t, e), ref, "svk_cosine_scores %dx%d dim %d, %s, environment %s"
                    % (nt, ne, dim, placed, env))


def test_cosine_scores_handle_workspace_regrown(eng):
    """ctx->work (the enrolled rows' 1 / norms) cannot be guarded.  On a FRESH handle, whose workspace starts empty: a call that
    makes it allocate 4 KiB (260 bytes asked), one that makes it free that block and allocate 32 KiB, the first again -- the
    same bytes, equal to what the session's long-lived handle gives."""
    from speaker_verification_amd.engine import Engine
    t, e, ref = _cosine_case(eng, 65537, 65, 128)
    fresh = Engine(eng.device_index)
    M.same_bits(_cosine_direct(fresh, "B", "vector", t, e), ref, "the first call of a fresh handle")
    big_t, big_e = M.randn(7, 1024, 8), M.randn(8, 8192, 8)
    big = _cosine_direct(fresh, "B", "vector", big_t, big_e)
    M.same_bits(big, M.bits(eng.cosine_scores(big_t, big_e)), "the call that regrows the handle's workspace")
    M.same_bits(_cosine_direct(fresh, "B", "vector", t, e), ref, "after the handle's workspace was regrown")
    M.same_bits(_cosine_direct(fresh, "A", "vector", big_t, big_e), big, "the larger call again")


# ---- svk_l2_dist, svk_pair_scores, svk_plda_pair_scores ----------------------------------------------------------------------
N_A, N_B = 19, 23


def _trial_case(dim, n):
    g = torch.Generator().manual_seed(1000 * dim + n)
    a, b = M.randn(3 * dim + n, N_A, dim), M.randn(5 * dim + n, N_B, dim)
    ia, ib = torch.randint(0, N_A, (n,), generator=g), torch.randint(0, N_B, (n,), generator=g)
    ia[-1], ib[0] = N_A - 1, N_B - 1                                 # the last rows: flush against the guards
    psi = torch.rand((dim,), generator=g, dtype=torch.float64) * 4.0
    psi[0] = 0.0
    counts = torch.randint(1, 6, (N_B,), generator=g, dtype=torch.int32)
    return a, b, ia, ib, psi, counts


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n", (1, 17, 1000))
@pytest.mark.parametrize("dim", (1, 13, 128))
def test_l2_dist(eng, dim, n, placed):
    a, b = M.randn(dim + n, n, dim), M.randn(2 * dim + n, n, dim)
    b[n // 2] = a[n // 2]
    ref = M.bits(eng.l2_dist(a, b))
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        da, db, out = c.input("d_a", a), c.input("d_b", b), c.output("d_out", torch.float32, (n,))
        c.call(eng.lib.svk_l2_dist, da, db, n, dim, out)
        M.same_bits(out.bits(), ref, "svk_l2_dist n %d dim %d, %s, environment %s" % (n, dim, placed, env))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("bad", (False, True), ids=("in-range", "one-out-of-range"))
@pytest.mark.parametrize("n", (1, 17, 1000))
@pytest.mark.parametrize("dim", (1, 13, 128))
def test_pair_scores(eng, dim, n, bad, placed):
    a, b, ia, ib, _, _ = _trial_case(dim, n)
    if bad:
        ia = ia.clone()
        ia[n // 2] = N_A                                             # one past the last row: must not be followed
    for metric, code in (("cosine", 0), ("l2", 1)):
        ref = M.bits(eng.pair_scores(a, b, ia, ib, metric))
        assert bool(np.isnan(ref.view(np.float32)[n // 2])) == bad
        for env in M.ENV_NAMES:
            c = M.Contract(eng, env, scalar=placed == "scalar")
            da, db, xa, xb = c.input("d_a", a), c.input("d_b", b), c.input("d_idx_a", ia), c.input("d_idx_b", ib)
            out, cnt = c.output("d_out", torch.float32, (n,)), c.counter("d_bad_count")
            c.call(eng.lib.svk_pair_scores, da, N_A, db, N_B, dim, xa, xb, n, code, out, cnt)
            what = "svk_pair_scores %s n %d dim %d, %s, environment %s" % (metric, n, dim, placed, env)
            M.same_bits(out.bits(), ref, what)
            M.counter_is(cnt, int(bad), what)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("bad", (False, True), ids=("in-range", "one-out-of-range"))
@pytest.mark.parametrize("n", (1, 17, 1000))
@pytest.mark.parametrize("dim", (1, 13, 128))
def test_plda_pair_scores(eng, dim, n, bad, placed):
    a, b, ia, ib, psi, counts = _trial_case(dim, n)
    if bad:
        ib = ib.clone()
        ib[n // 2] = -1
    for cnt_b in (None, counts):
        ref = M.bits(eng.plda_pair_scores(a, b, ia, ib, psi, counts_b=cnt_b))
        for env in M.ENV_NAMES:
            c = M.Contract(eng, env, scalar=placed == "scalar")
            da, db, xa, xb = c.input("d_a", a), c.input("d_b", b), c.input("d_idx_a", ia), c.input("d_idx_b", ib)
            dp, dc = c.input("d_psi", psi), c.input("d_count_b", cnt_b)
            out, cnt = c.output("d_out", torch.float32, (n,)), c.counter("d_bad_count")
            c.call(eng.lib.svk_plda_pair_scores, da, N_A, db, N_B, dim, dp, dc, xa, xb, n, out, cnt)
            what = "svk_plda_pair_scores counts %s n %d dim %d, %s, environment %s" % (cnt_b is not None, n, dim, placed, env)
            M.same_bits(out.bits(), ref, what)
            M.counter_is(cnt, int(bad), what)


# ---- svk_plda_scores -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("with_counts", (False, True), ids=("counts-NULL", "counts-given"))
@pytest.mark.parametrize("nt,ne,dim", ((17, 33, 130), (129, 65, 128)))
def test_plda_scores(eng, nt, ne, dim, with_counts, placed):
    g = torch.Generator().manual_seed(nt + dim)
    t, e = M.randn(nt, nt, dim), M.randn(ne, ne, dim)
    psi = torch.rand((dim,), generator=g, dtype=torch.float64) * 4.0
    counts = torch.randint(1, 6, (ne,), generator=g, dtype=torch.int32) if with_counts else None
    ref = M.bits(eng.plda_scores(t, e, psi, counts))
    nbytes = eng.lib.svk_plda_scores_workspace_bytes(nt, ne, dim, int(with_counts))
    assert nbytes > 0
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dt, de, dp, dc = c.input("d_test", t), c.input("d_enroll", e), c.input("d_psi", psi), c.input("d_enroll_count", counts)
        work, out = c.workspace(nbytes), c.output("d_out", torch.float32, (nt, ne))
        c.call(eng.lib.svk_plda_scores, dt, nt, de, ne, dim, dp, dc, work, nbytes, out)
        M.same_bits(out.bits(), ref, "svk_plda_scores %dx%d dim %d, %s, environment %s" % (nt, ne, dim, placed, env))


# ---- svk_cosine_topk -------------------------------------------------------------------------------------------------------
def _topk_direct(eng, env, placed, q, g, k, base, exclude, flags, lists):
    """One svk_cosine_topk call on arenas -> (score bits, index bits).  lists: the (scores, indices) the outputs hold on
    entry (the accumulate flag), or None: the environment's prefill."""
    nq, ng, dim = q.shape[0], g.shape[0], q.shape[1]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    dq, dg, dx = c.input("d_query", q), c.input("d_gallery", g), c.input("d_exclude", exclude)
    nbytes = eng.lib.svk_cosine_topk_workspace_bytes(nq, ng, dim, k)
    work = c.workspace(nbytes)
    sc = c.output("d_top_score", torch.float32, (nq, k), prefill=None if lists is None else lists[0])
    ix = c.output("d_top_index", torch.int64, (nq, k), prefill=None if lists is None else lists[1])
    c.call(eng.lib.svk_cosine_topk, dq, nq, dg, ng, dim, k, base, dx, flags, work, nbytes, sc, ix)
    return sc, ix


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("nq,ng,dim,k", ((129, 333, 128, 32), (4, 40000, 128, 5), (33, 31, 7, 32)),
                         ids=("one-span", "spans-and-merge", "fewer-candidates-than-k"))
def test_cosine_topk(eng, nq, ng, dim, k, placed):
    q, g = M.randn(nq, nq, dim), M.randn(ng, ng, dim)
    g[ng // 3] = g[ng // 3 + 1]                                      # a tie: the lower index first
    exclude = torch.arange(nq, dtype=torch.int64) % ng
    for ex in (None, exclude):
        ref = tuple(M.bits(t) for t in eng.cosine_topk(q, g, k, exclude=ex))
        for env in M.ENV_NAMES:
            what = "svk_cosine_topk (%d, %d, %d, k %d) exclude %s, %s, environment %s" % (nq, ng, dim, k, ex is not None, placed, env)
            sc, ix = _topk_direct(eng, env, placed, q, g, k, 0, ex, 0, None)
            M.same_bits(sc.bits(), ref[0], what + ": scores")
            M.same_bits(ix.bits(), ref[1], what + ": indices")
            # the accumulate flag over two chunks, the second first: one call over the whole gallery, bit for bit
            h = ng // 2 + 1
            s1, i1 = _topk_direct(eng, env, placed, q, g[h:], k, h, ex, 0, None)
            s2, i2 = _topk_direct(eng, env, placed, q, g[:h], k, 0, ex, 1, (s1.tensor, i1.tensor))
            M.same_bits(s2.bits(), ref[0], what + ": scores accumulated over two chunks")
            M.same_bits(i2.bits(), ref[1], what + ": indices accumulated over two chunks")


@pytest.mark.parametrize("placed", M.PLACED)
def test_cosine_topk_accumulate_keeps_the_lists_of_an_empty_chunk(eng, placed):
    """n_gallery == 0 with the accumulate flag leaves the lists as they are: every slot keeps its prefill; without the flag
    every slot is written with -1 / -inf."""
    q, none = M.randn(1, 5, 16), torch.zeros((0, 16), dtype=torch.float32)
    for env in M.ENV_NAMES:
        sc, ix = _topk_direct(eng, env, placed, q, none, 3, 0, None, 1, None)
        M.keeps_prefill(sc, sc.bits(), "d_top_score")
        M.keeps_prefill(ix, ix.bits(), "d_top_index")
        sc, ix = _topk_direct(eng, env, placed, q, none, 3, 0, None, 0, None)
        assert np.all(sc.bits().view(np.float32) == -np.inf) and np.all(ix.bits().view(np.int64) == -1)
