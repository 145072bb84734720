"""The memory contract of include/svk.h (Conventions) for the entry of its section "top-k search on normalised scores", svk_cosine_topk_norm
(csrc/search.hip): called directly on guarded arenas (tests/memory_contract.py) in the environments A, B and C, placed for the
vector paths and for the scalar ones (the moment tables one float64 past a 256-byte boundary: the alignment the header asks
for and no more).  The guards stay intact -- the tables are read in their [n][2] extent only, each flush against its trailing
guard --, the inputs byte-identical, and the results are the same bits in all three environments and equal the Engine
wrapper's on ordinary tensors, so nothing in the workspace or in the outputs is read before it is written; with the
accumulate flag the lists on entry are inputs, and two chunks give the bytes of one call."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

MODES = ("z", "t", "s")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _moments(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([0.1 * torch.randn(n, generator=g, dtype=torch.float64),
                        0.2 + torch.rand(n, generator=g, dtype=torch.float64)], dim=1)


def _direct(eng, env, placed, q, g, k, base, exclude, flags, qm, gm, lists):
    """One svk_cosine_topk_norm call on arenas -> (score arena, index arena).  lists: the (scores, indices) the outputs hold
    on entry (the accumulate flag), or None: the environment's prefill."""
    nq, ng, dim = q.shape[0], g.shape[0], q.shape[1]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    dq, dg, dx = c.input("d_query", q), c.input("d_gallery", g), c.input("d_exclude", exclude)
    dqm, dgm = c.input("d_query_moments", qm), c.input("d_gallery_moments", gm)
    nbytes = eng.lib.svk_cosine_topk_norm_workspace_bytes(nq, ng, dim, k)
    work = c.workspace(nbytes)
    sc = c.output("d_top_score", torch.float32, (nq, k), prefill=None if lists is None else lists[0])
    ix = c.output("d_top_index", torch.int64, (nq, k), prefill=None if lists is None else lists[1])
    c.call(eng.lib.svk_cosine_topk_norm, dq, nq, dg, ng, dim, k, base, dx, flags, dqm, dgm, work, nbytes, sc, ix)
    return sc, ix


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nq,ng,dim,k", ((129, 333, 128, 32), (4, 4200, 128, 5), (33, 31, 130, 32)),
                         ids=("one-span", "spans-and-merge", "streamed-fewer-candidates-than-k"))
def test_cosine_topk_norm(eng, nq, ng, dim, k, mode, placed):
    q, g = M.randn(nq, nq, dim), M.randn(ng, ng, dim)
    qm_all, gm_all = _moments(nq, nq), _moments(ng + 1, ng)
    gm_all[ng // 3] = gm_all[ng // 3 + 1]
    g[ng // 3] = g[ng // 3 + 1]                                      # a tie of normalised scores: the lower index first
    qm, gm = (qm_all if mode in "ts" else None), (gm_all if mode in "zs" else None)
    exclude = torch.arange(nq, dtype=torch.int64) % ng
    h = ng // 2 + 1
    for ex in (None, exclude):
        ref = tuple(M.bits(t) for t in eng.cosine_topk_norm(q, g, k, query_moments=qm, gallery_moments=gm, exclude=ex))
        for env in M.ENV_NAMES:
            what = "svk_cosine_topk_norm (%d, %d, %d, k %d) mode %s exclude %s, %s, environment %s" % (
                nq, ng, dim, k, mode, ex is not None, placed, env)
            sc, ix = _direct(eng, env, placed, q, g, k, 0, ex, 0, qm, gm, None)
            M.same_bits(sc.bits(), ref[0], what + ": scores")
            M.same_bits(ix.bits(), ref[1], what + ": indices")
            # the accumulate flag over two chunks, the second first, each with its own rows of the gallery table
            lo_gm, hi_gm = (None, None) if gm is None else (gm[:h], gm[h:])
            s1, i1 = _direct(eng, env, placed, q, g[h:], k, h, ex, 0, qm, hi_gm, None)
            s2, i2 = _direct(eng, env, placed, q, g[:h], k, 0, ex, 1, qm, lo_gm, (s1.tensor, i1.tensor))
            M.same_bits(s2.bits(), ref[0], what + ": scores accumulated over two chunks")
            M.same_bits(i2.bits(), ref[1], what + ": indices accumulated over two chunks")


@pytest.mark.parametrize("placed", M.PLACED)
def test_accumulate_keeps_the_lists_of_an_empty_chunk(eng, placed):
    """n_gallery == 0 with the accumulate flag leaves the lists as they are: every slot keeps its prefill; without the flag
    every slot is written with -1 / -inf.  Neither reads a table."""
    q, none = M.randn(1, 5, 16), torch.zeros((0, 16), dtype=torch.float32)
    qm, nothing = _moments(2, 5), torch.zeros((0, 2), dtype=torch.float64)
    for env in M.ENV_NAMES:
        sc, ix = _direct(eng, env, placed, q, none, 3, 0, None, 1, qm, nothing, None)
        M.keeps_prefill(sc, sc.bits(), "d_top_score")
        M.keeps_prefill(ix, ix.bits(), "d_top_index")
        sc, ix = _direct(eng, env, placed, q, none, 3, 0, None, 0, qm, nothing, None)
        assert np.all(sc.bits().view(np.float32) == -np.inf) and np.all(ix.bits().view(np.int64) == -1)
