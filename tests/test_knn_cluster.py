"""svk_knn_cluster (include/svk.h, "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists") on hand-made k-NN lists: every output exactly equal to the plain-Python reference
of tests/knn_cluster_ref.py, gave_up == 0 and two runs byte-identical in every case -- partial waves and workgroups, every k
and list_stride path, the deepest union-find (a 5 000-row path from every direction), the threshold's edge cases, the
shared-neighbour count at its boundary, every kind of bad slot, min_size, random lists in both modes, and the refusals."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import knn_cluster_ref as R       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

HOSTILE = np.array([-2, -(1 << 63), (1 << 63) - 1], dtype=np.int64)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def run(eng, index, score, k, threshold, min_shared=0, mutual=True, min_size=1):
    """One case: the device's four outputs against the reference, twice.  -> the reference's (labels, root, sizes, counts)."""
    index, score = np.ascontiguousarray(index, dtype=np.int64), np.ascontiguousarray(score, dtype=np.float32)
    want = R.cluster(index, score, k, threshold, min_shared, mutual, min_size)
    args = dict(k=k, threshold=threshold, min_shared=min_shared, mutual=mutual, min_size=min_size)
    first = [t.cpu().numpy() for t in eng.knn_cluster(torch.from_numpy(score), torch.from_numpy(index), **args)]
    again = [t.cpu().numpy() for t in eng.knn_cluster(torch.from_numpy(score), torch.from_numpy(index), **args)]
    what = "n %d k %d stride %d threshold %r min_shared %d mutual %s min_size %d" % (
        index.shape[0], k, index.shape[1], threshold, min_shared, mutual, min_size)
    assert first[3][3] == 0, what + ": gave_up"
    for name, got, rerun, ref in zip(("labels", "root", "sizes", "counts"), first, again, want):
        assert got.dtype == np.int32 and got.shape == ref.shape, what + ": " + name
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, "%s: %s differs from the reference in %d places, the first at %d (%d against %d)" % (
            what, name, bad.size, bad[0], got[bad[0]], ref[bad[0]])
        assert got.tobytes() == rerun.tobytes(), what + ": " + name + " differs between two runs"
    return want


def local_lists(seed, n, k, stride):
    """Neighbours drawn from the 40 rows on either side (modulo n: at small n the wrap brings the row itself and repeats in,
    so bad slots occur at every size), 3 % of the slots empty or hostile, scores from five values around 0.5.  The slots
    behind k hold rows and scores that would change every answer if they were read."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([np.arange(-40, 0), np.arange(1, 41)])
    index = (np.arange(n)[:, None] + rng.permuted(np.broadcast_to(offsets, (n, 80)), axis=1)[:, :stride]) % n
    index = index.astype(np.int64)
    hit = rng.random((n, stride)) < 0.03
    index[hit] = rng.choice(np.concatenate([HOSTILE, [-1, -1, n]]), int(hit.sum()))
    score = rng.choice(np.array([0.25, np.nextafter(np.float32(0.5), np.float32(0)), 0.5, 0.5, 0.75], dtype=np.float32), (n, stride))
    score[:, k:] = 1.0
    return index, score


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257, 5000))
def test_shapes(eng, n):
    for k in (1, 5, 31, 32):
        for stride in sorted({k, 32}):
            index, score = local_lists(1000 * n + k, n, k, stride)
            want = run(eng, index, score, k, 0.5, min_shared=1 if k > 1 else 0, mutual=True)
            if n >= 63 and k >= 31:
                assert 1 <= want[3][0] < n and want[3][2] > 0            # the case joins something and holds bad slots
    index, score = local_lists(n, n, 5, 8)
    run(eng, index, score, 5, 0.5, min_shared=0, mutual=False)


def test_a_narrower_k_is_a_narrower_search(eng):
    index, score = local_lists(3, 500, 32, 32)
    for k in (1, 10, 31):
        wide = [t.cpu().numpy() for t in eng.knn_cluster(score, index, k=k, threshold=0.5, min_shared=1)]
        narrow = [t.cpu().numpy() for t in eng.knn_cluster(score[:, :k].copy(), index[:, :k].copy(), threshold=0.5, min_shared=1)]
        assert all(np.array_equal(a, b) for a, b in zip(wide, narrow))
    assert not np.array_equal(eng.knn_cluster(score, index, k=10, threshold=0.5)[1].cpu().numpy(),
                              eng.knn_cluster(score, index, k=32, threshold=0.5)[1].cpu().numpy())


# ---- topologies --------------------------------------------------------------------------------------------------------------
def _path(order):
    """Row order[p] lists order[p - 1] and order[p + 1]: one path through every row in the order given."""
    n = order.size
    index = np.full((n, 2), -1, dtype=np.int64)
    index[order[1:], 0] = order[:-1]
    index[order[:-1], 1] = order[1:]
    return index, np.ones((n, 2), dtype=np.float32)


@pytest.mark.parametrize("direction", ("forward", "reversed", "permuted"))
def test_a_path_of_5000_rows(eng, direction):
    n = 5000
    order = {"forward": np.arange(n), "reversed": np.arange(n)[::-1].copy(),
             "permuted": np.random.default_rng(11).permutation(n)}[direction]
    index, score = _path(order)
    for mutual in (True, False):
        labels, root, sizes, counts = run(eng, index, score, 2, 0.5, mutual=mutual)
        assert not root.any() and list(counts) == [1, 0, 0, 0] and sizes[0] == n
    # cut in the middle: two components, each rooted at its own minimum
    cut = index.copy()
    cut[order[n // 2], 0] = -1
    labels, root, sizes, counts = run(eng, cut, score, 2, 0.5, mutual=False)
    assert counts[0] == 1 and sizes[0] == n                     # one direction still holds the arc
    labels, root, sizes, counts = run(eng, cut, score, 2, 0.5, mutual=True)
    assert counts[0] == 2 and sorted(set(root)) == sorted({int(order[:n // 2].min()), int(order[n // 2:].min())})


def test_a_star(eng):
    n, centre = 40, 7
    leaves = np.array([i for i in range(n) if i != centre])
    index = np.full((n, 32), -1, dtype=np.int64)
    index[centre] = leaves[:32]                                  # the centre's list holds 32 of its 39 leaves
    index[leaves, 0] = centre
    score = np.ones((n, 32), dtype=np.float32)
    labels, root, sizes, counts = run(eng, index, score, 32, 0.5, mutual=True)
    assert counts[0] == 1 + 7 and sizes[0] == 33 and set(root[leaves[:32]]) == {0} and list(root[leaves[32:]]) == list(leaves[32:])
    labels, root, sizes, counts = run(eng, index, score, 32, 0.5, mutual=False)
    assert list(counts) == [1, 0, 0, 0] and not root.any()
    run(eng, index, score, 32, 0.5, mutual=True, min_size=2)


def test_two_cliques_and_a_one_way_arc(eng):
    index = np.full((12, 6), -1, dtype=np.int64)
    for i in range(12):
        index[i, :5] = [j for j in range(6 * (i // 6), 6 * (i // 6) + 6) if j != i]
    index[2, 5] = 8
    score = np.ones((12, 6), dtype=np.float32)
    labels, root, sizes, counts = run(eng, index, score, 6, 0.5, mutual=True)
    assert list(root) == [0] * 6 + [6] * 6 and list(labels) == [0] * 6 + [1] * 6
    labels, root, sizes, counts = run(eng, index, score, 6, 0.5, mutual=False)
    assert not root.any() and sizes[0] == 12
    labels, root, sizes, counts = run(eng, index, score, 5, 0.5, mutual=False)      # the arc lies behind k
    assert counts[0] == 2


def test_fully_connected_lists(eng):
    n = 33
    index = np.array([[j for j in range(n) if j != i] for i in range(n)], dtype=np.int64)
    score = np.ones((n, 32), dtype=np.float32)
    for min_shared in (0, 31, 32):
        labels, root, sizes, counts = run(eng, index, score, 32, 0.5, min_shared=min_shared)
        assert counts[0] == (1 if min_shared <= 31 else n)       # two rows share the other 31


# ---- the threshold -------------------------------------------------------------------------------------------------------------
def test_threshold_cases(eng):
    half = np.float32(0.5)
    below = np.nextafter(half, np.float32(0))
    pairs = [(half, half), (below, half), (half, below), (below, below), (np.nan, half), (np.nan, np.nan), (1.0, 1.0),
             (0.0, 0.0), (-0.0, -0.0), (-0.0, 0.0), (-1e-45, 0.0), (-np.inf, -np.inf), (np.inf, np.inf)]
    n = 2 * len(pairs)
    index = (np.arange(n) ^ 1).reshape(n, 1).astype(np.int64)    # rows 2 p and 2 p + 1 list each other
    score = np.array(pairs, dtype=np.float32).reshape(n, 1)
    joined = {}
    for threshold in (0.5, 0.0, -0.0, -np.inf, np.inf):
        for mutual in (True, False):
            root = run(eng, index, score, 1, threshold, mutual=mutual)[1]
            joined[threshold if threshold else str(threshold), mutual] = [bool(root[2 * p + 1] == 2 * p) for p in range(len(pairs))]
    t, f = True, False
    assert joined[0.5, True] == [t, f, f, f, f, f, t, f, f, f, f, f, t]              # equal is kept, one ulp below is dropped
    assert joined[0.5, False] == [t, t, t, f, t, f, t, f, f, f, f, f, t]             # a NaN score gives no arc
    assert joined["0.0", True] == joined["-0.0", True] == [t, t, t, t, f, f, t, t, t, t, f, f, t]   # -0 >= +0 and +0 >= -0
    assert joined[-np.inf, True] == joined[-np.inf, False] == [t] * len(pairs)       # the score test is off, NaN included
    assert joined[np.inf, True] == [f] * 12 + [t]


# ---- shared neighbours -----------------------------------------------------------------------------------------------------------
def test_min_shared_at_its_boundary(eng):
    index = np.full((12, 6), -1, dtype=np.int64)
    index[0, :5] = [1, 2, 3, 4, 5]
    index[1, :5] = [0, 2, 3, 4, 6]                              # N(0) & N(1) = {2, 3, 4}
    index[7, :3] = [8, 9, 9]                                     # a repeated neighbour counts once: N(7) & N(8) = {9}
    index[8, :3] = [7, 9, 10]
    score = np.ones((12, 6), dtype=np.float32)
    for mutual in (True, False):
        for min_shared, pair01, pair78 in ((0, True, True), (1, True, True), (2, True, False), (3, True, False), (4, False, False)):
            root = run(eng, index, score, 6, 0.5, min_shared=min_shared, mutual=mutual)[1]
            assert (root[1] == 0) == pair01 and (root[8] == 7) == pair78, (mutual, min_shared)


# ---- bad slots -------------------------------------------------------------------------------------------------------------------
def test_every_kind_of_bad_slot(eng):
    n = 10
    index = np.array([[1, -1, 2, -1, 3, -1, -1, -1],
                      [0, -2, 0, 1, n, 2, (1 << 63) - 1, 2],       # -2, a repeat, itself, n, 2^63 - 1, a repeat: 6 bad
                      [1, 0, -(1 << 63), n + 1, 2, 2, 3, 3],       # 5 bad
                      [3, 3, 3, 3, 3, 3, 3, 2],                    # 7 bad, then a good one
                      [-1] * 8, [-2] * 8, [n] * 8, [(1 << 63) - 1] * 8, [8] * 8, [8, 8, 8, 8, 9, 9, 9, 8]], dtype=np.int64)
    score = np.ones((n, 8), dtype=np.float32)
    for mutual in (True, False):
        labels, root, sizes, counts = run(eng, index, score, 8, 0.5, mutual=mutual)
        assert counts[2] == 0 + 6 + 5 + 7 + 0 + 8 + 8 + 8 + 8 + 7
    assert list(run(eng, index, score, 8, 0.5, mutual=False)[1]) == [0, 0, 0, 0, 4, 5, 6, 7, 8, 8]
    assert list(run(eng, index, score, 8, 0.5, mutual=True)[1]) == [0, 0, 0, 0, 4, 5, 6, 7, 8, 9]
    assert run(eng, index, score, 4, 0.5)[3][2] == 0 + 3 + 2 + 4 + 0 + 4 + 4 + 4 + 4 + 3


# ---- min_size ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size", (1, 2, 26))
def test_min_size(eng, min_size):
    """Cliques of 1, 2, 25, 26, 1, 30, 2 and 27 rows, scattered over the rows by a permutation."""
    blocks = (1, 2, 25, 26, 1, 30, 2, 27)
    n = sum(blocks)
    place = np.random.default_rng(4).permutation(n)
    index = np.full((n, 32), -1, dtype=np.int64)
    first = 0
    for size in blocks:
        rows = place[first:first + size]
        for r in rows:
            index[r, :size - 1] = rows[rows != r]
        first += size
    labels, root, sizes, counts = run(eng, index, np.ones((n, 32), dtype=np.float32), 32, 0.5, min_size=min_size)
    kept = [b for b in blocks if b >= min_size]
    C = len(kept)
    assert counts[0] == C and counts[1] == n - sum(kept) == int((labels == -1).sum())
    assert sizes[:C].sum() + counts[1] == n and not sizes[C:].any() and sorted(sizes[:C]) == sorted(kept)
    assert np.array_equal(np.unique(labels[labels >= 0]), np.arange(C))                  # dense
    smallest = [int(np.flatnonzero(labels == c).min()) for c in range(C)]
    assert smallest == sorted(smallest) and all(root[s] == s for s in smallest)         # in order of the smallest member
    assert all(int((labels == c).sum()) == sizes[c] for c in range(C))


# ---- random lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutual", (True, False))
def test_random_lists(eng, mutual):
    n, k = 3000, 6
    rng = np.random.default_rng(17)
    index = rng.integers(0, n, (n, k)).astype(np.int64)
    back = rng.random((n, k)) < 0.3                              # return some arcs, or the mutual graph is all but empty
    index[index[:, 0][back[:, 0]], 1] = np.flatnonzero(back[:, 0])
    hit = rng.random((n, k)) < 0.05
    index[hit] = rng.choice(np.concatenate([HOSTILE, [-1, n, n + 1]]), int(hit.sum()))
    own = rng.random((n, k)) < 0.01
    index[own] = np.broadcast_to(np.arange(n)[:, None], (n, k))[own]
    score = rng.choice(np.array([0.25, 0.5, 0.75, 0.75, np.nan], dtype=np.float32), (n, k))
    labels, root, sizes, counts = run(eng, index, score, k, 0.5, mutual=mutual)
    assert counts[2] > 100 and (100 < counts[0] < n if mutual else counts[0] < n // 4 and sizes[:counts[0]].max() > n // 2)
    run(eng, index, score, k, 0.5, min_shared=1, mutual=mutual, min_size=3)
    run(eng, index, score, k, -np.inf, mutual=mutual, min_size=2)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_empty_corpus(eng):
    from speaker_verification_amd import _lib as binding
    lib, n, k = eng.lib, 6, 3
    index = torch.full((n, k), -1, dtype=torch.int64, device=eng.device)
    score = torch.zeros((n, k), dtype=torch.float32, device=eng.device)
    out = [torch.full((n + 1,), 7, dtype=torch.int32, device=eng.device) for _ in range(4)]
    nbytes = lib.svk_knn_cluster_workspace_bytes(n, k)
    work = torch.empty((nbytes + 16,), dtype=torch.uint8, device=eng.device)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                             # noqa: E731

    def call(**kw):
        a = dict(score=p(score), index=p(index), n=n, k=k, stride=k, threshold=0.5, min_shared=0, min_size=1, flags=1,
                 work=p(work), nbytes=nbytes, labels=p(out[0]), root=p(out[1]), sizes=p(out[2]), counts=p(out[3]))
        a.update(kw)
        eng._stream()
        return lib.svk_knn_cluster(eng.ctx, a["score"], a["index"], a["n"], a["k"], a["stride"], a["threshold"], a["min_shared"],
                                   a["min_size"], a["flags"], a["work"], a["nbytes"], a["labels"], a["root"], a["sizes"], a["counts"])

    for bad in (dict(n=-1), dict(n=1 << 31), dict(k=0), dict(k=33, stride=33), dict(stride=k - 1), dict(min_shared=-1),
                dict(min_shared=33), dict(min_size=0), dict(threshold=float("nan")), dict(flags=2), dict(flags=3), dict(flags=-1),
                dict(score=None), dict(index=None), dict(labels=None), dict(root=None), dict(sizes=None), dict(counts=None),
                dict(work=None), dict(nbytes=nbytes - 1), dict(work=p(work, 8)), dict(index=p(index, 4)), dict(score=p(score, 2)),
                dict(labels=p(out[0], 2)), dict(root=p(out[1], 1)), dict(sizes=p(out[2], 2)), dict(counts=p(out[3], 2))):
        assert call(**bad) == binding.SVK_ERR_BAD_ARG, bad
        assert b"bad argument" in lib.svk_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)                                        # a refused call writes nothing
    # n == 0: nothing but the counts is touched, and the other buffers may be NULL
    assert call(n=0, score=None, index=None, labels=None, root=None, sizes=None, work=None, nbytes=0) == 0
    assert call(n=0, counts=None) == binding.SVK_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert out[3][:5].tolist() == [0, 0, 0, 0, 7] and all(bool((t == 7).all()) for t in out[:3])
    got = eng.knn_cluster(score[:0], index[:0], k=3, threshold=0.5)
    assert [tuple(t.shape) for t in got] == [(0,), (0,), (0,), (4,)] and got[3].tolist() == [0, 0, 0, 0]
    # all slots empty: n singletons; the outputs' element behind the last stays as it was
    assert call() == 0
    torch.cuda.synchronize()
    assert out[0].tolist() == list(range(n)) + [7] and out[1].tolist() == list(range(n)) + [7]
    assert out[2].tolist() == [1] * n + [7] and out[3][:5].tolist() == [n, 0, 0, 0, 7]
