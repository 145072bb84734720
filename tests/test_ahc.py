"""svk_ahc (csrc/cluster.hip) against tests/ahc_f64_ref.py, the naive form of the definition: labels, cluster counts, merge pairs
and merge similarities must be EQUAL -- the similarities as float64 bit patterns -- on both instances (matrix in LDS, matrix in the
workspace) within one call, under every stop rule, with ties at most steps."""
import numpy as np
import pytest

import ahc_f64_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


@pytest.fixture(scope="module")
def limits(eng):
    L, top = eng.ahc_limits()
    assert L >= 66 and top >= 2048
    return L, top


def sizes(L):
    return [0, 1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 3]


def symmetric(rng, n, kind):
    """One recording's f32 matrix [n, n]; only the part above the diagonal matters."""
    if kind == "random":
        a = rng.uniform(-1, 1, (n, n))
    elif kind == "ties":                    # multiples of 1/8: most steps choose among equals, and averages tie again
        a = rng.integers(-8, 9, (n, n)) / 8.0
    else:                                   # 1 - 4 groups that are clear to the eye
        groups = rng.integers(0, int(rng.integers(1, 5)), n)
        a = np.where(groups[:, None] == groups[None, :], 0.8, -0.2) + rng.uniform(-0.1, 0.1, (n, n))
    a = np.triu(a, 1)
    return (a + a.T).astype(np.float32)


def make_batch(L, kind, seed, below=0.0):
    """Every size of `sizes(L)` in one padded batch; the part below the diagonal and the dead rows hold `below`."""
    ns = sizes(L)
    stride = max(ns)
    rng = np.random.default_rng(seed)
    aff = np.full((len(ns), stride, stride), below, np.float32)
    for r, n in enumerate(ns):
        m = symmetric(rng, n, kind)
        iu = np.triu_indices(n, 1)
        aff[r][iu] = m[iu]
        if below == 0.0:
            aff[r, :n, :n] = m
    return aff, np.array(ns, np.int32)


def run(eng, aff, n_seg, **kw):
    bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    labels, count, pair, sim = eng.ahc(aff, n_seg, want_merges=True, bad_count=bad, **kw)
    return labels.cpu().numpy(), count.cpu().numpy(), pair.cpu().numpy(), sim.cpu().numpy(), int(bad.item())


def assert_equal_ref(got, aff, n_seg, what, **kw):
    want = ref.ahc_batch(aff, n_seg, kw["threshold"], kw.get("min_clusters", 1), kw.get("max_clusters"), kw.get("target"))
    for r in range(len(n_seg)):
        tag = "%s, recording %d (n = %d)" % (what, r, n_seg[r])
        assert np.array_equal(got[2][r], want[2][r]), tag + ": merge pairs"
        assert np.array_equal(got[3][r].view(np.uint64), want[3][r].view(np.uint64)), tag + ": merge similarities (bits)"
        assert got[1][r] == want[1][r], tag + ": cluster count"
        assert np.array_equal(got[0][r], want[0][r]), tag + ": labels"


STOP_RULES = {
    "threshold": dict(threshold=0.25),
    "min2": dict(threshold=-5.0, min_clusters=2),                   # everything reaches it: stops at two clusters
    "min2_unreached": dict(threshold=5.0, min_clusters=2),          # a threshold nothing reaches: no merge at all
    "max3": dict(threshold=5.0, max_clusters=3),                    # forced merges down to three
}


@pytest.fixture(scope="module")
def batches(limits):
    return {kind: make_batch(limits[0], kind, seed) for seed, kind in enumerate(("random", "ties", "blocks"))}


@pytest.mark.parametrize("rule", sorted(STOP_RULES))
@pytest.mark.parametrize("kind", ["random", "ties", "blocks"])
def test_ahc_equals_the_definition(eng, batches, kind, rule):
    aff, n_seg = batches[kind]
    kw = STOP_RULES[rule]
    got = run(eng, aff, n_seg, **kw)
    assert got[4] == 0
    assert_equal_ref(got, aff, n_seg, "%s / %s" % (kind, rule), **kw)
    if rule == "max3":
        assert list(got[1]) == [min(n, 3) for n in n_seg]
    if rule == "min2_unreached":
        assert list(got[1]) == list(n_seg)
    if rule == "min2":
        assert list(got[1]) == [min(n, 2) for n in n_seg]


def test_ahc_blocks_are_found(eng, limits):
    """Three groups that are clear to the eye come back as three clusters under a threshold between the two levels."""
    n = 50
    groups = np.arange(n) % 3
    a = np.where(groups[:, None] == groups[None, :], 0.8, -0.2).astype(np.float32)
    labels, count, _, _, bad = run(eng, a[None], [n], threshold=0.3)
    assert bad == 0 and count[0] == 3 and np.array_equal(labels[0], groups)


def test_ahc_target_per_recording(eng, batches):
    aff, n_seg = batches["ties"]
    target = np.array([1, 5, 1, 7, 4, 0, 2, 3, 1, 2, 6], np.int32)      # 5 > n = 1 and 7 > n = 3 merge nothing; 0 = not set
    kw = dict(threshold=0.5, min_clusters=2, max_clusters=9, target=target)
    got = run(eng, aff, n_seg, **kw)
    assert_equal_ref(got, aff, n_seg, "targets", **kw)
    for r, n in enumerate(n_seg):
        if target[r] >= 1:
            assert got[1][r] == min(n, target[r])


def test_ahc_alone_equals_batch_and_runs_are_identical(eng, batches, limits):
    aff, n_seg = batches["random"]
    kw = STOP_RULES["threshold"]
    first, again = run(eng, aff, n_seg, **kw), run(eng, aff, n_seg, **kw)
    for a, b in zip(first[:4], again[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # 63 and L: in LDS both times, in the batch beside a workspace recording and alone with a stride of their own;
    # 2 L + 3: in the workspace both times
    for r in (4, 8, 10):
        n = int(n_seg[r])
        alone = run(eng, np.ascontiguousarray(aff[r:r + 1, :n, :n]), [n], **kw)      # another stride, no neighbours
        assert np.array_equal(alone[0][0], first[0][r, :n]) and alone[1][0] == first[1][r]
        steps = n - int(first[1][r])
        assert np.array_equal(alone[2][0, :steps], first[2][r, :steps])
        assert np.array_equal(alone[3][0, :steps].view(np.uint64), first[3][r, :steps].view(np.uint64))


def test_ahc_rejects_non_finite_and_bad_counts(eng, batches):
    aff, n_seg = batches["blocks"]
    kw = STOP_RULES["threshold"]
    clean = run(eng, aff, n_seg, **kw)
    bad_aff, bad_n = aff.copy(), n_seg.copy()
    bad_aff[4, 3, 40] = np.inf               # above the diagonal of a live row: recording 4 (n = 63) is not clustered
    bad_aff[10, 100, 200] = np.nan           # recording 10 (the workspace instance)
    bad_n[6] = aff.shape[1] + 1              # a count out of range
    bad_n[2] = -1
    got = run(eng, bad_aff, bad_n, **kw)
    assert got[4] == 4
    for r in (4, 10):
        assert got[1][r] == -1 and (got[0][r, :n_seg[r]] == -1).all()
    for r in (2, 6):
        assert got[1][r] == -1 and (got[0][r] == -1).all()
    for r in (2, 4, 6, 10):
        assert (got[2][r] == -1).all() and np.isnan(got[3][r]).all()
    assert_equal_ref(got, bad_aff, bad_n, "with bad recordings", **kw)
    for r in (0, 1, 3, 5, 7, 8, 9):          # the neighbours are unaffected
        for a, b in zip(got[:4], clean[:4]):
            assert np.array_equal(a[r:r + 1].view(np.uint8), b[r:r + 1].view(np.uint8))


def test_ahc_ignores_what_lies_below_the_diagonal_and_in_dead_rows(eng, limits):
    aff, n_seg = make_batch(limits[0], "random", 0)
    poisoned, _ = make_batch(limits[0], "random", 0, below=np.nan)
    assert np.isnan(poisoned).any()
    kw = STOP_RULES["max3"]
    clean, got = run(eng, aff, n_seg, **kw), run(eng, poisoned, n_seg, **kw)
    assert got[4] == 0
    for a, b in zip(got[:4], clean[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_ahc_dead_labels_are_not_written(eng):
    aff = symmetric(np.random.default_rng(5), 12, "random")[None]
    held = torch.full((1, 12), 77, dtype=torch.int32, device=eng.device)
    labels, count = eng.ahc(aff, [7], threshold=0.0, labels_out=held)
    assert (labels.cpu().numpy()[0, 7:] == 77).all() and (labels.cpu().numpy()[0, :7] >= 0).all()


def test_ahc_arguments(eng, limits):
    from speaker_verification_amd._lib import SvkError
    L, top = limits
    lib = eng.lib
    assert lib.svk_ahc_workspace_bytes(10, L) == 0                       # every recording fits the LDS instance
    assert lib.svk_ahc_workspace_bytes(3, L + 1) == 3 * 8 * (L + 1) ** 2
    assert lib.svk_ahc_limits(None) == -1
    null = [None] * 5
    assert lib.svk_ahc(None, None, 1, 4, None, 0.0, 1, 2, None, None, 0, *null) == -1
    assert lib.svk_ahc(eng.ctx, None, 1, 4, None, 0.0, 1, 2, None, None, 0, *null) == -1       # NULL buffers
    assert lib.svk_ahc(eng.ctx, None, -1, 4, None, 0.0, 1, 2, None, None, 0, *null) == -1
    assert lib.svk_ahc(eng.ctx, None, 0, 4, None, 0.0, 1, 2, None, None, 0, *null) == 0        # looks at no pointer
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    ns, lab, cnt = dev(np.array([2], np.int32)), dev(np.zeros((1, top + 1), np.int32)), dev(np.zeros(1, np.int32))
    small = dev(np.zeros((1, 4, 4), np.float32))
    # seg_stride above limits[1] (rejected before any buffer is read: the matrix need not exist)
    assert lib.svk_ahc(eng.ctx, small.data_ptr(), 1, top + 1, ns.data_ptr(), 0.0, 1, 2, None, None, 0, lab.data_ptr(), cnt.data_ptr(),
                       None, None, None) == -1
    # a short workspace
    big = dev(np.zeros((1, L + 1, L + 1), np.float32))
    work = torch.empty((lib.svk_ahc_workspace_bytes(1, L + 1),), dtype=torch.uint8, device=eng.device)
    args = (big.data_ptr(), 1, L + 1, ns.data_ptr(), 0.0, 1, 2, None)
    outs = (lab.data_ptr(), cnt.data_ptr(), None, None, None)
    assert lib.svk_ahc(eng.ctx, *args, work.data_ptr(), work.numel() - 1, *outs) == -1
    assert lib.svk_ahc(eng.ctx, *args, None, 0, *outs) == -1
    assert lib.svk_ahc(eng.ctx, *args, work.data_ptr(), work.numel(), *outs) == 0
    # the stop rule
    for kw in (dict(min_clusters=0), dict(min_clusters=3, max_clusters=2), dict(threshold=float("nan"))):
        with pytest.raises(SvkError) as err:
            eng.ahc(small, [2], **kw)
        assert err.value.code == -1
