"""svk_cosine_topk: the k best gallery rows of every query against float64 NumPy, the total order on exact ties and NaN, and
the independence of the result from chunking, batch, alignment and run.

A list is held to four properties rather than to the float64 index set (adjacent float64 scores among a row's best 32 lie
closer than the f32 chain's error in 0.4 - 5 % of the gaps, so an exact set comparison would fail a correct kernel):
  (a) distinct indices in range, -1 / -inf exactly in the slots past min(k, candidates);
  (b) every returned score within 1e-5 of the float64 cosine of the returned index (the bar of test_gpu_parity.py::
      test_cosine_scores);
  (c) sorted under the total order by the kernel's own scores, ascending index among equal scores;
  (d) every candidate NOT returned has a float64 score <= the smallest float64 score among the returned + 2e-5.
Worst |score - float64| observed on the MI355X over the cases of test_against_float64: 2.3e-6 at dim = 4096, 3.0e-7 at dim <= 200
(printed per case)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-5
SET_TOL = 2e-5
SHAPES = ((300, 1000, 128),      # three row blocks, the last one ragged
          (129, 1000, 200),      # dim > 128: the streamed-fragment path
          (17, 333, 4096),
          (33, 257, 7),          # 4-byte loads
          (5, 40, 1),
          (1, 1, 128),
          (4, 40_000, 128),      # the gallery splits across workgroups and goes through the merge
          (300, 31, 128))        # n_gallery < k = 32
CASES = [(s, k) for n, s in enumerate(SHAPES) for k in ((1, 5, 32) if n in (0, 6) else (32,))]


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


_cache = {}


def cosine64(q, g):
    x, y = q.astype(np.float64), g.astype(np.float64)
    nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
    nx[nx == 0] = 1.0
    ny[ny == 0] = 1.0
    return (x @ y.T) / (nx[:, None] * ny[None, :])


def matrices(shape):
    """(q, g, float64 cosine [nq, ng]): q = N(0, 1), g = 3 N(0, 1) + 0.5, a zero row in each and a gallery row copied from a
    query where the shape has room -- computed once per shape, shared by the tests, never written to."""
    if shape not in _cache:
        nq, ng, dim = shape
        rng = np.random.default_rng(1000 * nq + ng + dim)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        g = (rng.standard_normal((ng, dim)) * 3 + 0.5).astype(np.float32)
        if nq > 2:
            q[nq // 2] = 0
        if ng > 2:
            g[ng // 3] = 0
            g[ng - 2] = q[min(1, nq - 1)]
        ref = cosine64(q, g)
        for m in (q, g, ref):
            m.setflags(write=False)
        _cache[shape] = (q, g, ref)
    return _cache[shape]


def check_lists(scores, indices, ref, k, excluded=None):
    """(a) - (d) of the module docstring for every query row; returns the worst |score - float64|."""
    nq, ng = ref.shape
    assert scores.dtype == np.float32 and indices.dtype == np.int64 and scores.shape == indices.shape == (nq, k)
    ref = ref.copy()
    cand = np.full(nq, ng)
    if excluded is not None:
        inside = (excluded >= 0) & (excluded < ng)
        ref[np.nonzero(inside)[0], excluded[inside]] = -np.inf
        cand = cand - inside
    worst = 0.0
    for r in range(nq):
        valid = int(min(k, cand[r]))
        idx, sc = indices[r], scores[r]
        assert np.all(idx[valid:] == -1) and np.all(np.isneginf(sc[valid:])), "row %d: slots past the candidates" % r   # (a)
        idx, sc = idx[:valid], sc[:valid]
        assert np.all((idx >= 0) & (idx < ng)) and np.unique(idx).size == valid, "row %d: indices" % r
        if excluded is not None:
            assert excluded[r] not in idx, "row %d returned its excluded row" % r
        want = ref[r, idx]
        err = np.abs(sc.astype(np.float64) - want)
        worst = max(worst, float(err.max()) if valid else 0.0)
        assert np.all(err <= SCORE_TOL), "row %d: score off by %.3g" % (r, err.max())                                 # (b)
        assert np.all((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (idx[:-1] < idx[1:]))), "row %d: order" % r          # (c)
        if valid < cand[r]:
            rest = ref[r].copy()
            rest[idx] = -np.inf
            assert rest.max() <= want.min() + SET_TOL, "row %d: a better row was left out by %.3g" % (r, rest.max() - want.min())  # (d)
    return worst


def run(eng, q, g, k, **kw):
    s, i = eng.cosine_topk(q, g, k, **kw)
    return s.cpu().numpy(), i.cpu().numpy()


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("shape,k", CASES)
def test_against_float64(eng, shape, k):
    q, g, ref = matrices(shape)
    scores, indices = run(eng, q, g, k)
    worst = check_lists(scores, indices, ref, k)
    print("worst |score - float64| = %.3g over %d x %d, k = %d" % (worst, shape[0], min(k, shape[1]), k))


def test_scalar_loads_give_the_same_bits(eng):
    """Matrices 4 bytes off a 16-byte boundary take the 4-byte loads."""
    shape = SHAPES[0]
    q, g, _ = matrices(shape)
    dq, dg = eng.to_device(q), eng.to_device(g)
    assert dq.data_ptr() % 16 == 0 and dg.data_ptr() % 16 == 0
    fq = torch.empty(q.size + 1, dtype=torch.float32, device=eng.device)
    fg = torch.empty(g.size + 1, dtype=torch.float32, device=eng.device)
    oq, og = fq[1:].view(*q.shape), fg[1:].view(*g.shape)
    oq.copy_(dq)
    og.copy_(dg)
    assert oq.data_ptr() % 16 == 4 and og.data_ptr() % 16 == 4 and oq.is_contiguous()
    aligned = run(eng, dq, dg, 32)
    assert same_bytes(run(eng, oq, og, 32), aligned)
    assert same_bytes(run(eng, dq, og, 32), aligned)          # one off


def test_exact_ties_and_nan(eng):
    rng = np.random.default_rng(2)
    g = rng.standard_normal((200, 128)).astype(np.float32)
    copies = np.sort(rng.choice(200, 50, replace=False))
    row = rng.standard_normal(128).astype(np.float32)
    g[copies] = row
    q = np.stack([row, rng.standard_normal(128).astype(np.float32)])
    scores, indices = run(eng, q, g, 32)
    np.testing.assert_array_equal(indices[0], copies[:32])     # the 32 lowest indices of the copies, ascending
    assert np.all(scores[0].view(np.int32) == scores[0].view(np.int32)[0]) and abs(float(scores[0, 0]) - 1.0) <= SCORE_TOL
    check_lists(scores, indices, cosine64(q, g), 32)
    nan_at = int(np.setdiff1d(np.arange(200), copies)[40])       # a row that is no copy
    g[nan_at] = np.nan
    scores_n, indices_n = run(eng, q, g, 32)
    assert np.all(indices_n[:, 0] == nan_at) and np.all(np.isnan(scores_n[:, 0]))     # NaN ranks above every number
    np.testing.assert_array_equal(indices_n[0, 1:], copies[:31])
    assert not np.isnan(scores_n[:, 1:]).any()
    for k in (1, 5):                                           # the k-th score is the NaN (k = 1) or a number
        s, i = run(eng, q, g, k)
        np.testing.assert_array_equal(i, indices_n[:, :k])
        assert s.tobytes() == scores_n[:, :k].tobytes()


def test_independent_of_chunking(eng):
    q, g, _ = matrices(SHAPES[0])
    dq, dg = eng.to_device(q), eng.to_device(g)
    base = 1 << 33
    whole = run(eng, dq, dg, 32, index_base=base)
    assert whole[1].min() >= base and whole[1].max() < base + 1000        # indices above 2^32
    sizes = (1, 37, 500, 462)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    assert bounds[-1] == 1000
    chunks = [(int(bounds[c]), int(bounds[c + 1])) for c in range(len(sizes))]
    for order in (chunks, chunks[::-1]):
        into = None
        for lo, hi in order:
            into = eng.cosine_topk(dq, dg[lo:hi], 32, index_base=base + lo, into=into)
        assert same_bytes((into[0].cpu().numpy(), into[1].cpu().numpy()), whole)
    # an empty chunk leaves the lists as they are; without the flag it empties them
    kept = eng.cosine_topk(dq, dg[:0], 32, index_base=base, into=into)
    assert same_bytes((kept[0].cpu().numpy(), kept[1].cpu().numpy()), whole)
    s, i = run(eng, dq, dg[:0], 32)
    assert np.all(i == -1) and np.all(np.isneginf(s))


def test_split_gallery_is_independent_of_chunking(eng):
    """The same on the shape whose single call splits the gallery into spans: two chunks take other splits."""
    q, g, _ = matrices(SHAPES[6])
    dq, dg = eng.to_device(q), eng.to_device(g)
    whole = run(eng, dq, dg, 32)
    into = eng.cosine_topk(dq, dg[25_001:], 32, index_base=25_001)
    into = eng.cosine_topk(dq, dg[:25_001], 32, into=into)
    assert same_bytes((into[0].cpu().numpy(), into[1].cpu().numpy()), whole)


def test_independent_of_the_batch_and_the_run(eng):
    q, g, _ = matrices(SHAPES[0])
    dq, dg = eng.to_device(q), eng.to_device(g)
    batch = run(eng, dq, dg, 32)
    for r in (0, 127, 128, 299):
        alone = run(eng, dq[r:r + 1], dg, 32)
        assert alone[0].tobytes() == batch[0][r:r + 1].tobytes() and alone[1].tobytes() == batch[1][r:r + 1].tobytes()
    assert same_bytes(run(eng, dq, dg, 32), batch)
    for k in (1, 5):                                           # k does not enter a score's bits either
        s, i = run(eng, dq, dg, k)
        assert s.tobytes() == batch[0][:, :k].tobytes() and i.tobytes() == batch[1][:, :k].tobytes()


def test_exclude(eng):
    q, _, _ = matrices((300, 1000, 128))
    dq = eng.to_device(q)
    ref = cosine64(q, q)
    own = np.arange(300)
    scores, indices = run(eng, dq, dq, 32, exclude=own)
    assert not np.any(indices == own[:, None])
    check_lists(scores, indices, ref, 32, excluded=own)
    plain = run(eng, dq, dq, 32)
    assert np.all(plain[1][own != 150, 0] == own[own != 150])               # without it every non-zero row finds itself first
    assert same_bytes(run(eng, dq, dq, 32, exclude=own + 300), plain)      # outside the range: nothing changes
    assert same_bytes(run(eng, dq, dq, 32, exclude=own - 1000), plain)
    shifted = run(eng, dq, dq, 32, exclude=own + 5000, index_base=5000)     # the exclusion is a GLOBAL index
    assert shifted[0].tobytes() == scores.tobytes() and np.array_equal(shifted[1], indices + 5000)
    full = run(eng, dq[:40], dq[:40], 32, exclude=own[:40])                 # 39 candidates for 32 slots, then for 40
    check_lists(full[0], full[1], ref[:40, :40], 32, excluded=own[:40])
    few = run(eng, dq[:20], dq[:20], 32, exclude=own[:20])                  # 19 candidates: 13 empty slots
    check_lists(few[0], few[1], ref[:20, :20], 32, excluded=own[:20])


def test_argument_errors(eng):
    from speaker_verification_amd import _lib
    q, g, _ = matrices(SHAPES[0])
    dq, dg = eng.to_device(q), eng.to_device(g)
    nq, ng, dim, k = 300, 1000, 128, 32
    size = eng.lib.svk_cosine_topk_workspace_bytes
    need = int(size(nq, ng, dim, k))
    assert need > 0
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=eng.device)
    indices = torch.empty((nq, k), dtype=torch.int64, device=eng.device)
    p = eng._ptr

    def call(ctx=eng.ctx, **kw):
        a = dict(q=p(dq), nq=nq, g=p(dg), ng=ng, dim=dim, k=k, base=0, ex=None, flags=0, work=p(work), bytes=need,
                 s=p(scores), i=p(indices))
        a.update(kw)
        return eng.lib.svk_cosine_topk(ctx, a["q"], a["nq"], a["g"], a["ng"], a["dim"], a["k"], a["base"], a["ex"], a["flags"],
                                       a["work"], a["bytes"], a["s"], a["i"])

    def message():
        return eng.lib.svk_last_error(eng.ctx).decode()

    assert call() == _lib.SVK_OK
    assert call(ctx=None) == _lib.SVK_ERR_BAD_ARG
    for name in ("q", "g", "work", "s", "i"):
        assert call(**{name: None}) == _lib.SVK_ERR_BAD_ARG and "NULL" in message()
    for name in ("nq", "ng"):
        assert call(**{name: -1}) == _lib.SVK_ERR_BAD_ARG and "negative" in message()
    for bad in (0, -3, 4097):
        assert call(dim=bad) == _lib.SVK_ERR_BAD_ARG and "dim" in message()
        assert size(nq, ng, bad, k) == 0
    for bad in (0, -1, 33):
        assert call(k=bad) == _lib.SVK_ERR_BAD_ARG and "k must" in message()
        assert size(nq, ng, dim, bad) == 0
    for bad in (2, 4, 3, -1, 1 << 30):
        assert call(flags=bad) == _lib.SVK_ERR_BAD_ARG and "flag" in message()
    assert size(-1, ng, dim, k) == 0 and size(nq, -1, dim, k) == 0
    assert call(q=C.c_void_p(dq.data_ptr() + 2)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(g=C.c_void_p(dg.data_ptr() + 1)) == _lib.SVK_ERR_BAD_ARG and "aligned" in message()
    assert call(bytes=need - 1) == _lib.SVK_ERR_BAD_ARG and "workspace" in message()
    assert call(base=-1) == _lib.SVK_ERR_BAD_ARG and "index_base" in message()
    assert call(nq=0, q=None, work=None, s=None, i=None) == _lib.SVK_OK          # nothing to launch, nothing to check
    assert call(ng=0, flags=1, g=None, work=None) == _lib.SVK_OK
    with pytest.raises(_lib.SvkError, match="k must"):
        eng.cosine_topk(dq, dg, 33)
    with pytest.raises(ValueError, match="exclude"):
        eng.cosine_topk(dq, dg, 5, exclude=np.arange(7))
    with pytest.raises(ValueError, match="into"):
        eng.cosine_topk(dq, dg, 5, into=(scores, indices))
    torch.cuda.synchronize()


def test_pipeline_search_and_rank_speakers(eng):
    from speaker_verification_amd import evaluation
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline
    q, g, ref = matrices(SHAPES[0])
    dq, dg = eng.to_device(q), eng.to_device(g)
    pipe = VerificationPipeline(C3D2(4, 1), use_vad=False)
    want = run(eng, dq, dg, 5)
    for gallery, chunk in ((g, 100), (g, None), (dg, 333), (dg, None)):       # host / device gallery, chunked or whole
        got = pipe.search(dq, gallery, k=5, chunk_rows=chunk)
        assert same_bytes((got[0].cpu().numpy(), got[1].cpu().numpy()), want)
    me = pipe.search(q, q, k=3, exclude_self=True, chunk_rows=64)
    alone = run(eng, dq, dq, 3, exclude=np.arange(300))
    assert same_bytes((me[0].cpu().numpy(), me[1].cpu().numpy()), alone)
    with pytest.raises(ValueError, match="exclude_self"):
        pipe.search(q, g, exclude_self=True)

    ids = ["spk%04d" % j for j in range(1000)]
    threshold = float(np.median(want[0]))
    ranked = evaluation.rank_speakers(q, g, ids, k=5, threshold=threshold)
    assert ranked["scores"].tobytes() == want[0].tobytes() and np.array_equal(ranked["indices"], want[1])
    below = want[0] < np.float32(threshold)
    assert below.any() and not below.all()
    for r in range(300):
        assert ranked["ids"][r] == [None if below[r, j] else ids[want[1][r, j]] for j in range(5)]
    free = evaluation.rank_speakers(q, g[:3], ids[:3], k=5)                   # no threshold: only the empty slots are None
    assert all(row[3:] == [None, None] and None not in row[:3] for row in free["ids"])
    # rank-k accuracy against the float64 ranking: the copied query row finds its copy first
    hits = evaluation.topk_hits(want[1], np.argmax(ref, axis=1))
    assert hits.shape == (5,) and np.all(np.diff(hits) >= 0) and want[1][1, 0] == 998
