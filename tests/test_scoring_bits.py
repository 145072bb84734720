"""The bits of the scoring kernels (csrc/scoring.hip, search.hip, plda.hip, backend.hip), pinned for refactors: the SHA-256 of
every entry's output bytes on one seeded input per case against tests/golden/scoring_bits.json.

The golden pins ONE compiler and ONE architecture (hipcc of the ROCm release the digests were recorded with, gfx950): a change
that leaves the source's arithmetic and its order alone leaves these digests alone, and a deliberate change of the arithmetic
order or a compiler that contracts or reorders differently must re-record the file -- run this module once on the commit BEFORE
such a change with SVK_SCORING_BITS_RECORD=1 to see that it reproduces the committed file, and once after it to write the new
one.  What the numbers should be is the business of tests/test_scoring_float64.py, test_pair_scores.py, test_cosine_topk.py,
test_plda_scores.py, test_plda_pair_scores.py and test_embedding_project.py; this file only says they are still the same.

The cases are the smallest shapes that reach each branch (the cosine shapes are rows of test_scoring_float64.py's table):
cosine_scores  small kernel with 16-byte and 4-byte loads; tiled with the fragments hoisted, ragged both ways; tiled, streamed
l2_dist        dim % 4 == 0 and not
pair_scores    both metrics at dim 128 and 7, two indices out of range (NaN there, and bad_count == 2)
cosine_topk    one span; four spans; streamed (dim > 128) at k = 32; a self-search with `exclude`; two chunks through `into=`
plda_scores / plda_pair_scores   dim 128 and 150, without and with enrolment counts
embedding_project   centre + LDA + both norms (128 -> 64); centring alone at dim 130
Inputs are N(0, 1) float32 from np.random.default_rng; psi is sorted, descending, rng.random(dim) ** 3 * 100; counts lie in
[1, 8)."""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scoring_bits.json")
RECORD = bool(os.environ.get("SVK_SCORING_BITS_RECORD"))
SEED = 20261019
ROWS, TRIALS = 500, 3000


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def _normal(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


def _psi(rng, dim):
    return np.sort(rng.random(dim) ** 3 * 100)[::-1].copy()


def _trials(rng, n_a, n_b):
    """Two index lists of TRIALS entries, one entry of each outside its matrix."""
    ia, ib = rng.integers(0, n_a, TRIALS), rng.integers(0, n_b, TRIALS)
    ia[1234], ib[77] = n_a, -1
    return ia.astype(np.int64), ib.astype(np.int64)


def _cosine(eng, rng, nt, ne, dim):
    return _sha(eng.cosine_scores(_normal(rng, nt, dim), _normal(rng, ne, dim)))


def _l2(eng, rng, n, dim):
    return _sha(eng.l2_dist(_normal(rng, n, dim), _normal(rng, n, dim)))


def _pair(eng, rng, dim, metric):
    a, b = _normal(rng, ROWS, dim), _normal(rng, ROWS, dim)
    ia, ib = _trials(rng, ROWS, ROWS)
    bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
    out = eng.pair_scores(a, b, ia, ib, metric=metric, bad_count=bad)
    assert int(bad.item()) == 2
    return _sha(out)


def _topk(eng, rng, n, ng, dim, k, how="whole"):
    g = eng.to_device(_normal(rng, ng, dim))
    q = eng.to_device(_normal(rng, n, dim))
    if how == "exclude":            # an ng x ng self-search cut to its first n queries
        return _sha(*eng.cosine_topk(g[:n], g, k, exclude=np.arange(n)))
    if how == "into":
        half = ng // 2
        part = eng.cosine_topk(q, g[:half], k)
        return _sha(*eng.cosine_topk(q, g[half:], k, index_base=half, into=part))
    return _sha(*eng.cosine_topk(q, g, k))


def _plda(eng, rng, nt, ns, dim, counts):
    t, e, psi = _normal(rng, nt, dim), _normal(rng, ns, dim), _psi(rng, dim)
    cnt = rng.integers(1, 8, ns).astype(np.int32)
    return _sha(eng.plda_scores(t, e, psi, counts=cnt if counts else None))


def _plda_pair(eng, rng, dim, counts):
    a, b, psi = _normal(rng, ROWS, dim), _normal(rng, ROWS, dim), _psi(rng, dim)
    cnt = rng.integers(1, 8, ROWS).astype(np.int32)
    ia, ib = _trials(rng, ROWS, ROWS)
    bad = torch.zeros(1, dtype=torch.int32, device=eng.device)
    out = eng.plda_pair_scores(a, b, ia, ib, psi, counts_b=cnt if counts else None, bad_count=bad)
    assert int(bad.item()) == 2
    return _sha(out)


def _project(eng, rng, n, dim, out_dim):
    x, mean = _normal(rng, n, dim), _normal(rng, dim)
    if out_dim == dim:
        return _sha(eng.embedding_project(x, mean=mean))
    return _sha(eng.embedding_project(x, mean=mean, w=_normal(rng, dim, out_dim), l2_in=True, l2_out=True))


CASES = [("cosine_scores-33x17x128", _cosine, (33, 17, 128)),
         ("cosine_scores-19x21x201", _cosine, (19, 21, 201)),
         ("cosine_scores-4100x1030x128", _cosine, (4100, 1030, 128)),
         ("cosine_scores-2050x2100x200", _cosine, (2050, 2100, 200)),
         ("cosine_scores-2050x2100x201", _cosine, (2050, 2100, 201)),
         ("l2_dist-1000x128", _l2, (1000, 128)),
         ("l2_dist-37x7", _l2, (37, 7)),
         ("pair_scores-128-cosine", _pair, (128, "cosine")),
         ("pair_scores-128-l2", _pair, (128, "l2")),
         ("pair_scores-7-cosine", _pair, (7, "cosine")),
         ("pair_scores-7-l2", _pair, (7, "l2")),
         ("cosine_topk-300x1000x128-k5", _topk, (300, 1000, 128, 5)),
         ("cosine_topk-300x5000x128-k5", _topk, (300, 5000, 128, 5)),
         ("cosine_topk-300x5000x200-k32", _topk, (300, 5000, 200, 32)),
         ("cosine_topk-300x5000x128-k5-exclude", _topk, (300, 5000, 128, 5, "exclude")),
         ("cosine_topk-300x5000x128-k5-into", _topk, (300, 5000, 128, 5, "into")),
         ("plda_scores-300x70x128", _plda, (300, 70, 128, False)),
         ("plda_scores-300x70x128-counts", _plda, (300, 70, 128, True)),
         ("plda_scores-300x70x150", _plda, (300, 70, 150, False)),
         ("plda_scores-300x70x150-counts", _plda, (300, 70, 150, True)),
         ("plda_pair_scores-128", _plda_pair, (128, False)),
         ("plda_pair_scores-128-counts", _plda_pair, (128, True)),
         ("plda_pair_scores-150", _plda_pair, (150, False)),
         ("plda_pair_scores-150-counts", _plda_pair, (150, True)),
         ("embedding_project-1000x128to64", _project, (1000, 128, 64)),
         ("embedding_project-1000x130", _project, (1000, 130, 130))]


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(CASES)), ids=[c[0] for c in CASES])
def test_output_bits_are_the_recorded_ones(eng, index):
    """The entry's output bytes hash to the recorded digest.  A case's inputs depend on its position in CASES alone."""
    name, run, args = CASES[index]
    got = run(eng, np.random.default_rng([SEED, index]), *args)
    if RECORD:
        gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        gold.setdefault("digests", {})[name] = got
        gold["hip_runtime"] = torch.version.hip
        gold["arch"] = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
        with open(GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")
    gold = json.load(open(GOLDEN))["digests"]
    assert RECORD or set(gold) == set(c[0] for c in CASES)
    assert got == gold[name], "%s: other bits than recorded" % name
