"""The memory contract of include/svk.h (Conventions) for the back-end entries: svk_class_scatter, svk_embedding_project,
svk_embedding_pool and svk_c3d2_head, called directly on guarded arenas (tests/memory_contract.py) in the environments A, B and
C; the properties P1-P4 as tests/test_memory_contract_scoring.py states them.  Every comparison is on bytes, against the Engine
wrapper's result for the same call on ordinary buffers."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _csr(lengths):
    start = [0]
    for n in lengths:
        start.append(start[-1] + n)
    return torch.tensor(start, dtype=torch.int64)


# ---- svk_class_scatter -----------------------------------------------------------------------------------------------------
# 1 030 classes of 0 - 3 rows: eff_scan_kernel carries across its blocks of 1 024, so a misread entry of the effective offsets
# shows.  600 one-row classes and two of 3 rows: two chunk slots, the second without an effective row -- its partials keep the
# workspace's fill, which scatter_reduce_kernel must not read.
_MANY = tuple(int(n) for n in torch.randint(0, 4, (1030,), generator=torch.Generator().manual_seed(1030)))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("flags", (0, 1))
@pytest.mark.parametrize("lengths,dim,permute", (((1, 2, 7, 0, 300, 65), 40, True), ((1, 2, 7, 0, 300, 65), 128, True),
                                                 ((5,) * 8, 200, False), (_MANY, 40, True), ((1,) * 600 + (3, 3), 128, True)),
                         ids=("ragged-40", "ragged-128", "8x5-200", "1030-classes-40", "surplus-slot-128"))
def test_class_scatter(eng, lengths, dim, permute, flags, placed):
    start = _csr(lengths)
    n_class, n_rows = len(lengths), int(start[-1]) + 3              # three rows outside every class: ignored
    x = M.randn(dim + n_rows, n_rows, dim)
    index = torch.randperm(n_rows, generator=torch.Generator().manual_seed(dim)) if permute else None
    ref = tuple(M.bits(t) for t in eng.class_scatter(x, start, row_index=index, l2_rows=bool(flags)))
    nbytes = eng.lib.svk_class_scatter_workspace_bytes(n_rows, dim, n_class)
    assert nbytes > 0
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dx, ds, di = c.input("d_emb", x), c.input("d_seg_start", start), c.input("d_row_index", index)
        work = c.workspace(nbytes)
        mean, sw = c.output("d_class_mean", torch.float64, (n_class, dim)), c.output("d_sw", torch.float64, (dim, dim))
        c.call(eng.lib.svk_class_scatter, dx, n_rows, dim, ds, di, n_class, flags, work, nbytes, mean, sw)
        what = "svk_class_scatter %s dim %d flags %d, %s, environment %s" % (
            lengths if n_class <= 8 else "%d classes" % n_class, dim, flags, placed, env)
        M.same_bits(mean.bits(), ref[0], what + ": d_class_mean")
        M.same_bits(sw.bits(), ref[1], what + ": d_sw")


# ---- svk_embedding_project -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
@pytest.mark.parametrize("n,dim,out_dim", ((17, 130, 7), (300, 128, 50), (33, 128, None)), ids=("17x130-7", "300x128-50", "identity-128"))
def test_embedding_project(eng, n, dim, out_dim, flags, placed):
    x, mu = M.randn(n + dim, n, dim), M.randn(dim, dim) * 0.1
    x[n // 2] = 0.0                                                  # a zero row: zeros in, the norm divides by nothing
    w = M.randn(out_dim, dim, out_dim) if out_dim is not None else None
    cols = out_dim if out_dim is not None else dim
    ref = M.bits(eng.embedding_project(x, mean=mu, w=w, l2_in=bool(flags & 1), l2_out=bool(flags & 2)))
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dx, dm, dw = c.input("d_emb", x), c.input("d_mean", mu), c.input("d_w", w)
        out = c.output("d_out", torch.float32, (n, cols))
        c.call(eng.lib.svk_embedding_project, dx, n, dim, dm, dw, cols, flags, out)
        M.same_bits(out.bits(), ref, "svk_embedding_project %d rows %d -> %s flags %d, %s, environment %s"
                    % (n, dim, out_dim, flags, placed, env))


# ---- svk_embedding_pool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("flags", (0, 1, 2, 3))
@pytest.mark.parametrize("form", ("uniform-3", "csr-with-an-empty-segment"))
@pytest.mark.parametrize("dim", (13, 128, 260, 4096))
def test_embedding_pool(eng, dim, form, flags, placed):
    n_rows = 15
    x = M.randn(dim, n_rows, dim)
    x[4] = 0.0
    if form == "uniform-3":
        K, start, index, n_seg, empty = 3, None, None, 5, 0
        ref = M.bits(eng.embedding_pool(x, rows_per_seg=K, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2)))
    else:
        K, start, n_seg, empty = 0, _csr((2, 0, 7, 6)), 4, 1
        index = torch.randperm(n_rows, generator=torch.Generator().manual_seed(dim))
        ref = M.bits(eng.embedding_pool(x, seg_start=start, row_index=index, l2_rows=bool(flags & 1), l2_mean=bool(flags & 2)))
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dx, ds, di = c.input("d_emb", x), c.input("d_seg_start", start), c.input("d_row_index", index)
        out, cnt = c.output("d_out", torch.float32, (n_seg, dim)), c.counter("d_empty_count")
        c.call(eng.lib.svk_embedding_pool, dx, n_rows, dim, n_seg, K, ds, di, flags, out, cnt)
        what = "svk_embedding_pool dim %d %s flags %d, %s, environment %s" % (dim, form, flags, placed, env)
        M.same_bits(out.bits(), ref, what)
        M.counter_is(cnt, empty, what + ": d_empty_count")


# ---- svk_c3d2_head ---------------------------------------------------------------------------------------------------------
def _head_direct(eng, env, placed, x, w6, b6, slope, want_probs, k, true_idx):
    """One svk_c3d2_head call on arenas -> (probs bits | None, top-k bits | None, hits | None).  d_emb and d_w6 are 16-byte
    aligned by the ABI: the scalar placement puts them 16 bytes past the boundary."""
    n, n_labels = x.shape[0], w6.shape[0]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    dx, dw, db = c.input("d_emb", x, off=16), c.input("d_w6", w6, off=16), c.input("d_b6", b6)
    dt = c.input("d_true", true_idx)
    probs = c.output("d_probs", torch.float32, (n, n_labels)) if want_probs else None
    top = c.output("d_topk", torch.int32, (n, k)) if k else None
    hits = (C.c_int64 * 8)(*([-5] * 8))
    c.call(eng.lib.svk_c3d2_head, dx, n, n_labels, slope, dw, db, probs, k or 0, top, dt, hits if dt is not None else None)
    kept = k if dt is not None else 0
    assert list(hits[kept:]) == [-5] * (8 - kept), "h_hits was written past its k entries"
    return (probs.bits() if probs else None, top.bits() if top else None, list(hits[:k]) if dt is not None else None)


def _head_case(eng, n, n_labels):
    x, w6, b6 = M.randn(n, n, 128), M.randn(n_labels, n_labels, 128) * 0.2, M.randn(n_labels + 1, n_labels)
    true_idx = (torch.arange(n, dtype=torch.int32) * 7) % n_labels
    top1 = eng.c3d2_head(x, (w6.to(eng.device), b6.to(eng.device), 0.25), probs=False, k=1)[1].cpu()[:, 0]
    true_idx[::2] = top1[::2]                                        # every other row is a hit at rank 1
    true_idx[0] = -1                                                 # no label: never counts
    return x, w6, b6, 0.25, true_idx


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("k", (1, 5))
@pytest.mark.parametrize("n_labels", (1, 17, 1211))
@pytest.mark.parametrize("n", (1, 17, 33))
def test_c3d2_head(eng, n, n_labels, k, placed):
    k = min(k, n_labels)             # k <= n_labels is the ABI's rule: one label has a top-1 only
    x, w6, b6, slope, true_idx = _head_case(eng, n, n_labels)
    tables = (w6.to(eng.device), b6.to(eng.device), slope)
    for want_probs, want_top in ((True, False), (False, True), (True, True)):
        p, top, hits = eng.c3d2_head(x, tables, probs=want_probs, k=k if want_top else None, true_idx=true_idx if want_top else None)
        for env in M.ENV_NAMES:
            got = _head_direct(eng, env, placed, x, w6, b6, slope, want_probs, k if want_top else None, true_idx if want_top else None)
            what = "svk_c3d2_head n %d labels %d k %d probs %s top-k %s, %s, environment %s" % (n, n_labels, k, want_probs, want_top, placed, env)
            if want_probs:
                M.same_bits(got[0], M.bits(p), what + ": d_probs")
            if want_top:
                M.same_bits(got[1], M.bits(top), what + ": d_topk")
                assert got[2] == hits, what + ": h_hits"


def test_c3d2_head_counters_start_from_zero_at_every_call(eng):
    """The hit counters live in the handle's fixed scratch (ctx->scratch), which cannot be guarded and is never reallocated:
    what can go wrong is a call that does not zero them, or another entry that disturbs them.  On a fresh handle: a head call,
    svk_top1 (its counter is the neighbouring scratch slot) and a svk_cosine_scores call that allocates the handle's
    workspace, the head call again -- the same bytes and hit counts, equal to the long-lived handle's."""
    from speaker_verification_amd.engine import Engine
    x, w6, b6, slope, true_idx = _head_case(eng, 33, 1211)
    want = _head_direct(eng, "B", "vector", x, w6, b6, slope, True, 5, true_idx)
    fresh = Engine(eng.device_index)
    first = _head_direct(fresh, "B", "vector", x, w6, b6, slope, True, 5, true_idx)
    fresh.top1(M.randn(3, 300, 65), torch.arange(300, dtype=torch.int32) % 65)
    fresh.cosine_scores(M.randn(1, 1024, 8), M.randn(2, 8192, 8))
    again = _head_direct(fresh, "A", "vector", x, w6, b6, slope, True, 5, true_idx)
    for got, name in ((first, "the first call of a fresh handle"), (again, "after other entries used the handle")):
        M.same_bits(got[0], want[0], name + ": d_probs")
        M.same_bits(got[1], want[1], name + ": d_topk")
        assert got[2] == want[2] and sum(got[2]) > 0, name + ": h_hits"
