"""Trial lists on the host: read_trials, make_trials, get_min_dcf against the brute-force definition, and the argument checks
of svk_pair_scores / svk_roc_dcf / svk_decision_counts that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "speaker_verification_amd", "libsvk.so")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    if not os.path.exists(LIB):
        entry.build()
    from speaker_verification_amd import _lib
    return _lib.load()


# ---- read_trials ------------------------------------------------------------------------------------------------
def test_read_trials_well_formed(tmp_path):
    from speaker_verification_amd.evaluation import read_trials
    lines = ["1 id10270/x/00001.wav id10270/y/00002.wav\n", "0 id10270/x/00001.wav id10300/z/00001.wav\n",
             "1 id10300/z/00001.wav id10300/z/00004.wav\n"]
    labels, ia, ib, names = read_trials(lines)
    assert labels.dtype == np.uint8 and ia.dtype == np.int64 and ib.dtype == np.int64
    np.testing.assert_array_equal(labels, [1, 0, 1])
    assert names == ["id10270/x/00001.wav", "id10270/y/00002.wav", "id10300/z/00001.wav", "id10300/z/00004.wav"]
    np.testing.assert_array_equal(ia, [0, 0, 2])                     # a repeated name maps to one index
    np.testing.assert_array_equal(ib, [1, 2, 3])
    path = tmp_path / "trials.txt"
    path.write_text("".join(lines))
    again = read_trials(str(path))
    for x, y in zip(again[:3], (labels, ia, ib)):
        np.testing.assert_array_equal(x, y)
    assert again[3] == names


def test_read_trials_comments_and_blank_lines():
    from speaker_verification_amd.evaluation import read_trials
    labels, ia, ib, names = read_trials(["# VoxCeleb-style list", "", "1 a b", "   ", "  # indented comment", "0\tb\tc  "])
    np.testing.assert_array_equal(labels, [1, 0])
    np.testing.assert_array_equal(ia, [0, 1])
    np.testing.assert_array_equal(ib, [1, 2])
    assert names == ["a", "b", "c"]
    empty = read_trials([])
    assert empty[0].size == 0 and empty[1].dtype == np.int64 and empty[3] == []


def test_read_trials_errors_name_the_line():
    from speaker_verification_amd.evaluation import read_trials
    with pytest.raises(ValueError, match="line 3"):
        read_trials(["1 a b", "# comment", "1 a"])                   # malformed: two fields
    with pytest.raises(ValueError, match="line 2"):
        read_trials(["1 a b", "0 a b c"])                            # four fields
    with pytest.raises(ValueError, match="line 4.*label"):
        read_trials(["1 a b", "", "0 a c", "2 a b"])
    with pytest.raises(ValueError, match="line 1.*label"):
        read_trials(["yes a b"])


# ---- make_trials ------------------------------------------------------------------------------------------------
def check_trials(ids, labels, ia, ib, n_target, n_nontarget):
    ids = np.asarray(ids)
    assert labels.dtype == np.uint8 and ia.dtype == np.int64 and ib.dtype == np.int64
    assert labels.size == ia.size == ib.size == n_target + n_nontarget
    assert int(labels.sum()) == n_target
    np.testing.assert_array_equal(labels, (ids[ia] == ids[ib]).astype(np.uint8))     # the labels are what the ids say
    assert not np.any(ia == ib)                                                      # no self pairs
    unordered = {(min(i, j), max(i, j)) for i, j in zip(ia.tolist(), ib.tolist())}
    assert len(unordered) == labels.size                                             # no pair twice, in either order
    assert ia.min() >= 0 and max(ia.max(), ib.max()) < ids.size


def test_make_trials():
    from speaker_verification_amd.evaluation import make_trials
    ids = np.repeat(np.arange(7), [1, 2, 3, 4, 5, 6, 7])                             # 28 utterances; one speaker alone
    have_t = sum(k * (k - 1) // 2 for k in range(1, 8))                              # 56
    have_n = 28 * 27 // 2 - have_t
    for n_t, n_n in ((10, 30), (have_t, have_n), (0, 5), (5, 0), (0, 0)):
        labels, ia, ib = make_trials(ids, n_t, n_n, seed=4)
        if n_t + n_n:
            check_trials(ids, labels, ia, ib, n_t, n_n)
        else:
            assert labels.size == ia.size == ib.size == 0
    a = make_trials(ids, 20, 40, seed=9)
    b = make_trials(ids, 20, 40, seed=9)
    c = make_trials(ids, 20, 40, seed=10)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))                           # same seed, same list
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    names = np.array(["id%05d" % s for s in ids])                                    # string ids work the same
    assert all(np.array_equal(x, y) for x, y in zip(a, make_trials(names, 20, 40, seed=9)))
    with pytest.raises(ValueError, match="target"):
        make_trials(ids, have_t + 1, 0, seed=1)
    with pytest.raises(ValueError):
        make_trials(ids, 0, have_n + 1, seed=1)
    with pytest.raises(ValueError):
        make_trials(np.arange(10), 1, 0, seed=1)                                     # every speaker once: no target pair


def test_make_trials_large_corpus_draws_by_rejection():
    """More candidate pairs than are worth listing (3 000 utterances: 4.5e6 pairs): the rejection path."""
    from speaker_verification_amd.evaluation import make_trials
    ids = np.random.default_rng(2).integers(0, 40, 3000)
    labels, ia, ib = make_trials(ids, 300, 700, seed=12)
    check_trials(ids, labels, ia, ib, 300, 700)


# ---- get_min_dcf ------------------------------------------------------------------------------------------------
def brute_force_dcf(labels, scores, p_target, c_miss, c_fa):
    """The definition, from direct counts: every distinct score and +inf as threshold, highest first; accept when
    score >= threshold.  Returns (thresholds, costs, p_miss, p_fa) over all candidates."""
    labels = np.asarray(labels).astype(bool)
    scores = np.asarray(scores)
    thresholds = np.r_[np.inf, np.unique(scores)[::-1].astype(np.float64)]
    P, N = int(labels.sum()), int((~labels).sum())
    p_miss = np.array([np.sum(labels & ~(scores >= t)) / P for t in thresholds])
    p_fa = np.array([np.sum(~labels & (scores >= t)) / N for t in thresholds])
    cost = c_miss * p_target * p_miss + c_fa * (1 - p_target) * p_fa
    return thresholds, cost, p_miss, p_fa


def test_get_min_dcf_against_the_definition():
    from speaker_verification_amd.evaluation import get_min_dcf
    rng = np.random.default_rng(21)
    labels = (rng.random(500) < 0.3).astype(np.uint8)
    scores = (np.floor((rng.standard_normal(500) + 1.2 * labels) * 2).clip(-8, 7) / 4).astype(np.float32)   # 16 levels
    assert np.unique(scores).size <= 16
    for p, cm, cf in ((0.01, 1, 1), (0.05, 1, 1), (0.5, 1, 1), (0.001, 10, 1), (0.3, 2, 5)):
        thresholds, cost, p_miss, p_fa = brute_force_dcf(labels, scores, p, cm, cf)
        norm = min(cm * p, cf * (1 - p))
        min_dcf, thr, miss, fa = get_min_dcf(labels, scores, p, cm, cf)
        assert min_dcf == pytest.approx(cost.min() / norm, rel=1e-13)
        at = np.nonzero(thresholds == thr)[0]
        assert at.size == 1                                              # a score of the input, or +inf
        assert cost[at[0]] == pytest.approx(cost.min(), rel=1e-13)       # ... at which the cost is the minimum
        assert miss == pytest.approx(p_miss[at[0]], abs=1e-15) and fa == p_fa[at[0]]
    with pytest.raises(ValueError):
        get_min_dcf(labels, scores, 0.0)
    with pytest.raises(ValueError):
        get_min_dcf(labels, scores, 1.0)
    with pytest.raises(ValueError):
        get_min_dcf(labels, scores, 0.5, c_miss=0)


def dyadic_case(seed=22):
    """128 pairs, 64 targets and 64 non-targets, p_target = 0.5, costs 1: every rate is k / 64 and every cost a multiple of
    1 / 128, so all arithmetic is exact.  In descending score order the pairs alternate non-target, target: after every
    target the rates are equal (cost 0.5, the origin's), after every non-target the false accepts lead by one (cost above
    0.5).  The minimum is therefore reached at 65 points, the origin first, and the tie rule must return the origin.  The
    pairs are stored in a shuffled order."""
    rank = np.arange(128)
    labels = (rank % 2).astype(np.uint8)
    scores = ((127 - rank) / 32.0 - 2.0).astype(np.float32)
    order = np.random.default_rng(seed).permutation(128)
    return labels[order], scores[order]


def test_get_min_dcf_exact_case_ties_go_to_the_origin():
    from speaker_verification_amd.evaluation import get_min_dcf
    labels, scores = dyadic_case()
    thresholds, cost, p_miss, p_fa = brute_force_dcf(labels, scores, 0.5, 1, 1)
    assert cost.min() == 0.5 and int(np.sum(cost == 0.5)) == 65 and cost[0] == 0.5
    assert get_min_dcf(labels, scores, 0.5, 1, 1) == (1.0, float("inf"), 1.0, 0.0)
    # one swap makes a target outrank its neighbour: a unique minimum below the origin's cost, all still exact
    s2 = scores.copy()
    i, j = np.nonzero(scores == scores.max())[0][0], np.nonzero(scores == np.sort(scores)[-2])[0][0]
    s2[i], s2[j] = scores[j], scores[i]
    thresholds, cost, p_miss, p_fa = brute_force_dcf(labels, s2, 0.5, 1, 1)
    at = int(np.argmin(cost))
    assert at == 1 and cost[1] == 0.5 - 1 / 128
    assert get_min_dcf(labels, s2, 0.5, 1, 1) == (cost[1] / 0.5, thresholds[1], p_miss[1], p_fa[1])


# ---- the C entries without a GPU ----------------------------------------------------------------------------------
def test_new_entries_reject_a_null_context(lib):
    from speaker_verification_amd import _lib
    out = (C.c_double * 13)(*([-7.0] * 13))
    ops = (C.c_double * 6)(0.01, 1, 1, 0.05, 1, 1)
    assert lib.svk_roc_dcf(None, None, None, 100, ops, 2, None, 0, out) == _lib.SVK_ERR_BAD_ARG
    assert list(out) == [-7.0] * 13
    counts = (C.c_int64 * 4)(*([-7] * 4))
    thr = (C.c_float * 1)(0.5)
    assert lib.svk_decision_counts(None, None, None, 100, thr, 1, counts) == _lib.SVK_ERR_BAD_ARG
    assert list(counts) == [-7] * 4
    assert lib.svk_pair_scores(None, None, 4, None, 4, 128, None, None, 4, 0, None, None) == _lib.SVK_ERR_BAD_ARG
    assert lib.svk_last_error(None) == b"null context"


def test_dcf_workspace_bytes(lib):
    for n in (2, 3, 100, 5000, 100_003, 2_000_000, 148642 * 1211, (1 << 31) + 12345, (1 << 32) - 1):   # test_device_evaluation's
        assert lib.svk_roc_dcf_workspace_bytes(n) >= lib.svk_roc_workspace_bytes(n) > 0
    for n in (1, 0, -5):
        assert lib.svk_roc_dcf_workspace_bytes(n) == 0
