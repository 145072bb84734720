"""The memory contract of include/svk.h (Conventions) for the entry of its section "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists", svk_knn_cluster
(csrc/knn_cluster.hip): called directly on guarded arenas (tests/memory_contract.py) in the
environments A, B and C, placed on 256-byte boundaries and one element past them (the alignment the header asks for and no
more; the workspace 16 bytes past).  The lists are strided where list_stride > k: the slots behind k hold the payload pattern
(0, -1 / NaN, another finite number) and are not read.  The guards stay intact, the inputs byte-identical, and the four
outputs are the same bytes in all three environments and equal the Engine wrapper's on ordinary tensors, so nothing in the
workspace or in the outputs is read before it is written."""
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


def _lists(n, k):
    """Real lists: the self-search's shape (distinct neighbours near the row), a few empty and hostile slots, scores on
    both sides of 0.5."""
    rng = np.random.default_rng(100 * n + k)
    offsets = np.concatenate([np.arange(-20, 0), np.arange(1, 21)])
    index = ((np.arange(n)[:, None] + rng.permuted(np.broadcast_to(offsets, (n, 40)), axis=1)[:, :k]) % n).astype(np.int64)
    hit = rng.random((n, k)) < 0.05
    index[hit] = rng.choice(np.array([-1, -2, n, (1 << 63) - 1], dtype=np.int64), int(hit.sum()))
    score = rng.choice(np.array([0.25, 0.5, 0.75, np.nan], dtype=np.float32), (n, k))
    return torch.from_numpy(score), torch.from_numpy(index)


def _direct(eng, env, placed, score, index, stride, threshold, min_shared, min_size, flags):
    n, k = index.shape
    c = M.Contract(eng, env, scalar=placed == "scalar")
    ds, di = c.input("d_nbr_score", score, stride=stride), c.input("d_nbr_index", index, stride=stride)
    nbytes = eng.lib.svk_knn_cluster_workspace_bytes(n, k)
    work = c.workspace(nbytes)
    outs = [c.output(name, torch.int32, (m,)) for name, m in (("d_labels", n), ("d_root", n), ("d_sizes", n), ("d_counts", 4))]
    c.call(eng.lib.svk_knn_cluster, ds, di, n, k, stride, threshold, min_shared, min_size, flags, work, nbytes, *outs)
    return outs


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("n,k,stride", ((129, 32, 32), (1000, 5, 8), (65, 1, 1)))
def test_knn_cluster(eng, n, k, stride, placed):
    score, index = _lists(n, k)
    for mutual, min_shared, min_size, threshold in ((True, 0, 1, 0.5), (True, 2, 3, 0.5), (False, 1, 2, 0.5), (False, 0, 1, -np.inf)):
        if k == 1 and min_shared:
            continue
        ref = [M.bits(t) for t in eng.knn_cluster(score, index, threshold=threshold, min_shared=min_shared, mutual=mutual,
                                                  min_size=min_size)]
        assert ref[3][3] == 0 and ref[3][2] > 0
        for env in M.ENV_NAMES:
            what = "svk_knn_cluster (%d, k %d, stride %d) mutual %s min_shared %d min_size %d threshold %r, %s, environment %s" % (
                n, k, stride, mutual, min_shared, min_size, threshold, placed, env)
            outs = _direct(eng, env, placed, score, index, stride, threshold, min_shared, min_size, int(mutual))
            for name, out, want in zip(("labels", "root", "sizes", "counts"), outs, ref):
                M.same_bits(out.bits(), want, what + ": " + name)
