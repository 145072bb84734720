"""svk_spectral_embed (csrc/spectral.hip) against its definition, tests/spectral_f64_ref.py.

Everything up to the Laplacian is exact, so graphs, node counts and neighbour counts must be EQUAL.  The eigensolver is the one
place that rounds: its eigenvalues, residuals and orthogonality are held to 4 x what the NumPy restatement of the same Jacobi
iteration shows on the same matrix, plus one unit of m 2^-52 lambda_max (m 2^-52 for orthogonality) -- the device may contract to
FMA and order a rotation's additions differently, which moves the error by a small factor, while an indexing or rotation bug
moves it by ten orders of magnitude.  Decisions (speaker count, neighbour count, labels) are compared on inputs whose margins
tests/test_spectral_host.py has checked on the CPU."""
import numpy as np
import pytest

import spectral_cases as cases
import spectral_f64_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = ("embed", "n_nodes", "n_speakers", "neighbours", "eigval", "eigvec", "graph", "ratio")


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def run(eng, aff, n_seg, **kw):
    bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    out = eng.spectral_embed(aff, n_seg, want_spectrum=True, want_graph=True, bad_count=bad, **kw)
    got = {name: t.cpu().numpy() for name, t in zip(NAMES, out)}
    got["bad"] = int(bad.item())
    return got


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in NAMES)


@pytest.fixture(scope="module")
def ties():
    return cases.ties_batch()


@pytest.fixture(scope="module")
def blocks():
    return cases.blocks_batch()


@pytest.fixture(scope="module")
def blocks_ref(blocks):
    """The reference of the block batch under every set of bounds the tests use, computed once."""
    aff, n_seg, _ = blocks
    return {name: cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP, **kw) for name, kw in BOUNDS.items()}


TARGET, BOUNDS = cases.TARGET, cases.BOUNDS


# ---- exact logic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3, cases.STRIDE - 1, cases.STRIDE + 5])
def test_graphs_of_tied_affinities_equal_the_definition(eng, ties, p):
    aff, n_seg = ties
    got = run(eng, aff, n_seg, neighbours=p)
    assert got["bad"] == 0
    for r, n in enumerate(n_seg):
        want = ref.spectral(aff[r], n, neighbours=p)
        assert got["n_nodes"][r] == n and got["neighbours"][r] == want["neighbours"] == (min(p, n - 1) if n > 1 else 0)
        assert np.array_equal(got["graph"][r, :n, :n], want["graph"]), "recording %d (n = %d)" % (r, n)
        assert not got["graph"][r, n:].any() and not got["graph"][r, :, n:].any()


@pytest.mark.parametrize("p", [1, 3, cases.GROUPED_NODES - 1, cases.GROUPED_NODES + 5])
def test_graphs_of_grouped_windows_equal_the_definition(eng, p):
    aff, n_seg, group = cases.grouped_ties_batch()
    got = run(eng, aff, n_seg, group=group, neighbours=p)
    assert got["bad"] == 0 and got["graph"].shape[1] == cases.GROUPED_NODES
    for r, n in enumerate(n_seg):
        want = ref.spectral(aff[r], n, group[r], cases.GROUPED_NODES, neighbours=p)
        m = want["n_nodes"]
        assert got["n_nodes"][r] == m == min(n, cases.GROUPED_NODES) and got["neighbours"][r] == want["neighbours"]
        assert np.array_equal(got["graph"][r, :m, :m], want["graph"]), "recording %d (n = %d, m = %d)" % (r, n, m)


def test_dead_rows_and_the_lower_triangle_are_never_read(eng, ties, blocks):
    for clean, poisoned, kw in ((ties, cases.ties_batch(below=np.nan), dict(neighbours=3)),
                                (blocks, cases.blocks_batch(below=np.nan), dict(neighbours=cases.SWEEP))):
        assert np.isnan(poisoned[0]).any()
        a, b = run(eng, clean[0], clean[1], **kw), run(eng, poisoned[0], poisoned[1], **kw)
        assert a["bad"] == b["bad"] == 0 and same_bits(a, b)


# ---- accuracy ----------------------------------------------------------------------------------------------------------
_YARDSTICK = {}


def yardstick(L):
    """The Jacobi restatement on L, once per matrix: (eigenvalues, eigenvectors, sweeps)."""
    key = L.tobytes()
    if key not in _YARDSTICK:
        lam, V, sweeps, converged = ref.jacobi(L)
        assert converged
        _YARDSTICK[key] = (lam, V, sweeps)
    return _YARDSTICK[key]


def held_to_the_yardstick(L, lam, V, lam_true, tag):
    """The device's three error figures against 4 x the Jacobi restatement's + 1 unit; prints both."""
    k = V.shape[1]
    y_lam, y_V, sweeps = yardstick(L)
    yard = ref.accuracy(L, y_lam, y_V[:, :k], lam_true)
    dev = ref.accuracy(L, lam, V, lam_true)
    print("%s: device %.3f / %.3f / %.3f units (eigenvalues / residual / orthogonality), yardstick %.3f / %.3f / %.3f in %d sweeps"
          % ((tag,) + dev + yard + (sweeps,)))
    for d, y, what in zip(dev, yard, ("eigenvalues", "residual", "orthogonality")):
        assert d <= 4 * y + 1, "%s: %s %.3g units against a yardstick of %.3g" % (tag, what, d, y)
    return yard


@pytest.mark.parametrize("case", cases.known_spectra(), ids=lambda c: c[0])
def test_known_spectra(eng, case):
    name, aff, p, exact = case
    m = aff.shape[0]
    got = run(eng, aff[None], [m], neighbours=p, max_speakers=8)
    want = ref.spectral(aff, m, neighbours=p)
    assert got["bad"] == 0 and got["n_nodes"][0] == m and got["neighbours"][0] == p
    assert np.array_equal(got["graph"][0], want["graph"])
    k = int(got["n_speakers"][0])
    assert k == want["n_speakers"]
    lam = got["eigval"][0]
    assert (np.diff(lam) >= 0).all()
    held_to_the_yardstick(ref.laplacian(want["graph"]), lam, got["eigvec"][0, :k].T, exact, name)


def test_block_spectra_against_eigh(eng, blocks, blocks_ref):
    aff, n_seg, _ = blocks
    got = run(eng, aff, n_seg, neighbours=cases.SWEEP)
    assert got["bad"] == 0
    for r, want in enumerate(blocks_ref["free"]):
        m = int(n_seg[r])
        if m < 2:
            continue
        assert np.array_equal(got["graph"][r, :m, :m], want["graph"])
        k = int(got["n_speakers"][r])
        held_to_the_yardstick(ref.laplacian(want["graph"]), got["eigval"][r, :m], got["eigvec"][r, :k, :m].T, want["eigval"],
                              "blocks, %d nodes" % m)


# ---- decisions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", sorted(BOUNDS))
def test_decisions_equal_the_definition(eng, blocks, blocks_ref, bounds):
    aff, n_seg, _ = blocks
    kw = BOUNDS[bounds]
    got = run(eng, aff, n_seg, neighbours=cases.SWEEP, **kw)
    assert got["bad"] == 0
    K = kw.get("max_speakers", 8)
    assert got["embed"].shape == (len(n_seg), cases.STRIDE, K)
    emb_aff = eng.segment_affinity(torch.from_numpy(got["embed"]), got["n_nodes"])
    labels = eng.ahc(emb_aff, got["n_nodes"], target=got["n_speakers"])[0].cpu().numpy()
    for r, want in enumerate(blocks_ref[bounds]):
        m, tag = int(n_seg[r]), "%s, recording %d (%d nodes)" % (bounds, r, n_seg[r])
        assert got["n_nodes"][r] == m and got["neighbours"][r] == want["neighbours"], tag
        assert got["n_speakers"][r] == want["n_speakers"], tag
        assert np.array_equal(np.isnan(got["ratio"][r]), np.isnan(want["ratio"])), tag
        assert not got["embed"][r, m:].any() and not got["embed"][r, :, want["n_speakers"]:].any(), tag
        if m < 2:
            assert np.array_equal(got["embed"][r, :m], want["embed"]), tag
            continue
        # r = p lambda_max / gap with every eigenvalue within e of the truth: |dr| <= r (e / lambda_max + 2 e / gap).  e, in units
        # of m 2^-52 lambda_max of the candidate's graph: the device's bar (4 x the yardstick's eigenvalue figure on the chosen
        # graph + 1) and one more unit for the reference's own eigensolver
        y_lam = yardstick(ref.laplacian(want["graph"]))[0]
        units = 4 * np.max(np.abs(y_lam - want["eigval"])) / (m * ref.EPS * want["eigval"][-1]) + 2
        live = ~np.isnan(want["ratio"])
        r_ref, r_dev, top, gap = want["ratio"][live], got["ratio"][r][live], want["top"][live], want["gap"][live]
        bar = r_ref * units * m * ref.EPS * (1 + 2 * top / gap)
        print("%s: ratios off by at most %.3g of a bar of %.3g" % (tag, np.max(np.abs(r_dev - r_ref) / bar), 1.0))
        assert np.all(np.abs(r_dev - r_ref) <= bar), "%s: ratios off by %s against %s" % (tag, np.abs(r_dev - r_ref), bar)
        assert np.array_equal(labels[r, :m], ref.embedding_labels(want["embed"], m, want["n_speakers"])), tag
        assert (labels[r, m:] == -1).all()
    if "min_speakers" in kw and "target" not in kw:
        assert (got["n_speakers"][n_seg >= 3] >= 3).all()
    if "max_speakers" in kw:
        assert (got["n_speakers"] <= 2).all()
    if "target" in kw:
        fixed = TARGET >= 1
        assert np.array_equal(got["n_speakers"][fixed], np.minimum(TARGET, n_seg)[fixed])
        assert np.array_equal(got["ratio"].view(np.uint64), run(eng, aff, n_seg, neighbours=cases.SWEEP,
                                                                 **{k: v for k, v in kw.items() if k != "target"})["ratio"].view(np.uint64))


def test_tight_speakers_converge_and_decide_as_the_definition(eng):
    """Nearly complete graphs with heaps of equal eigenvalues (tests/spectral_cases.py tight_batch): no recording runs out of
    sweeps, and count and neighbours are the reference's."""
    aff, n_seg = cases.tight_batch()
    got = run(eng, aff, n_seg, neighbours=cases.SWEEP)
    assert got["bad"] == 0
    want = cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP)
    assert got["neighbours"].tolist() == [w["neighbours"] for w in want]
    assert got["n_speakers"].tolist() == [w["n_speakers"] for w in want]
    for r, w in enumerate(want):
        m = int(n_seg[r])
        assert np.array_equal(got["graph"][r, :m, :m], w["graph"])
        held_to_the_yardstick(ref.laplacian(w["graph"]), got["eigval"][r, :m], got["eigvec"][r, :w["n_speakers"], :m].T, w["eigval"],
                              "tight, %d nodes" % m)


def test_speaker_counts_of_the_blocks_are_found(eng, blocks):
    aff, n_seg, who = blocks
    got = run(eng, aff, n_seg, neighbours=cases.SWEEP)
    assert got["n_speakers"].tolist() == [cases.BLOCK_SPEAKERS[int(n)] for n in n_seg]
    labels = eng.ahc(eng.segment_affinity(torch.from_numpy(got["embed"]), got["n_nodes"]), got["n_nodes"],
                     target=got["n_speakers"])[0].cpu().numpy()
    for r, n in enumerate(n_seg):
        assert np.array_equal(labels[r, :n], who[r])


# ---- bits --------------------------------------------------------------------------------------------------------------
def test_runs_are_identical_and_a_recording_alone_equals_the_batch(eng, blocks):
    aff, n_seg, _ = blocks
    kw = dict(neighbours=cases.SWEEP)
    first, again = run(eng, aff, n_seg, **kw), run(eng, aff, n_seg, **kw)
    assert same_bits(first, again)

    def same_recording(a, ra, b, rb, m):
        k = int(a["n_speakers"][ra])
        for name in ("n_nodes", "n_speakers", "neighbours", "ratio"):
            assert np.array_equal(a[name][ra:ra + 1].view(np.uint8), b[name][rb:rb + 1].view(np.uint8)), name
        assert np.array_equal(a["embed"][ra, :m].view(np.uint32), b["embed"][rb, :m].view(np.uint32))
        assert np.array_equal(a["eigval"][ra, :m].view(np.uint64), b["eigval"][rb, :m].view(np.uint64))
        assert np.array_equal(a["eigvec"][ra, :k, :m].view(np.uint64), b["eigvec"][rb, :k, :m].view(np.uint64))
        assert np.array_equal(a["graph"][ra, :m, :m], b["graph"][rb, :m, :m])

    for r, n in enumerate(n_seg):
        n = int(n)
        same_recording(run(eng, aff[r:r + 1], [n], **kw), 0, first, r, n)                                    # no neighbours
        if n >= 1:                                                                                         # another stride,
            same_recording(run(eng, np.ascontiguousarray(aff[r:r + 1, :n, :n]), [n], **kw), 0, first, r, n)  # another LDS size
    order = np.array([11, 3, 9, 10, 4, 8, 6], np.int64)                                                    # another n_rec, other slots
    moved = run(eng, aff[order], n_seg[order], **kw)
    for slot, r in enumerate(order):
        same_recording(moved, slot, first, int(r), int(n_seg[r]))


# ---- bad inputs and arguments ------------------------------------------------------------------------------------------
def assert_bad(got, rows, clean, others):
    assert got["bad"] == len(rows)
    for r in rows:
        assert got["n_nodes"][r] == got["n_speakers"][r] == got["neighbours"][r] == -1
        assert not got["embed"][r].any() and np.isnan(got["ratio"][r]).all()
    for r in others:
        for name in NAMES:
            assert np.array_equal(got[name][r:r + 1].view(np.uint8), clean[name][r:r + 1].view(np.uint8)), (r, name)


def test_bad_recordings_are_marked_and_their_neighbours_untouched(eng, blocks):
    aff, n_seg, _ = blocks
    kw = dict(neighbours=cases.SWEEP)
    clean = run(eng, aff, n_seg, **kw)
    everyone = set(range(len(n_seg)))
    for row, change in ((7, ("nan", 3, 40)), (8, ("inf", 0, 63)), (5, ("n", cases.STRIDE + 1)), (9, ("n", -1))):
        bad_aff, bad_n = aff.copy(), n_seg.copy()
        if change[0] == "n":
            bad_n[row] = change[1]
        else:
            bad_aff[row, change[1], change[2]] = np.nan if change[0] == "nan" else np.inf            # above the diagonal
        assert_bad(run(eng, bad_aff, bad_n, **kw), [row], clean, everyone - {row})
        assert ref.spectral(bad_aff[row], bad_n[row], neighbours=cases.SWEEP)["n_nodes"] == -1
    # one of each in one batch
    bad_aff, bad_n = aff.copy(), n_seg.copy()
    bad_aff[7, 3, 40], bad_n[5], bad_n[9] = np.nan, cases.STRIDE + 1, -1
    assert_bad(run(eng, bad_aff, bad_n, **kw), [5, 7, 9], clean, everyone - {5, 7, 9})


def test_bad_groups_are_marked(eng):
    aff, n_seg, group = cases.grouped_ties_batch()
    kw = dict(neighbours=3)
    clean = run(eng, aff, n_seg, group=group, **kw)
    assert clean["bad"] == 0
    everyone = set(range(len(n_seg)))
    hole = group[8].copy()
    hole[hole == 5] = 127                                                             # node 5 is left without a member
    assert n_seg[8] > cases.GROUPED_NODES and hole[:n_seg[8]].max() == 127
    high, negative = group[4].copy(), group[5].copy()
    high[7], negative[0] = cases.GROUPED_NODES, -1                                    # labels out of range
    for row, labels in ((4, high), (5, negative), (8, hole)):
        g2 = group.copy()
        g2[row] = labels
        assert_bad(run(eng, aff, n_seg, group=g2, **kw), [row], clean, everyone - {row})
        assert ref.spectral(aff[row], n_seg[row], g2[row], cases.GROUPED_NODES, neighbours=3)["n_nodes"] == -1


def test_arguments(eng):
    lib = eng.lib
    nodes, top, spk = eng.spectral_limits()
    assert (nodes, top, spk) == (128, 2048, 16)
    assert lib.svk_spectral_limits(None) == -1
    # per recording: V^T of c x c float64, c = max(2, node_stride rounded up to even), and int32 [seg_stride rounded up to 4]
    assert lib.svk_spectral_workspace_bytes(3, 300, 128) == 3 * (8 * 128 * 128 + 4 * 300)
    assert lib.svk_spectral_workspace_bytes(2, 17, 17) == 2 * (8 * 18 * 18 + 4 * 20)
    assert lib.svk_spectral_workspace_bytes(1, 0, 0) == 8 * 2 * 2
    assert lib.svk_spectral_workspace_bytes(0, 8, 8) == 0 and lib.svk_spectral_workspace_bytes(1, top + 1, 8) == 0
    assert lib.svk_spectral_workspace_bytes(1, 8, nodes + 1) == 0 and lib.svk_spectral_workspace_bytes(-1, 8, 8) == 0
    dev = lambda a: torch.from_numpy(a).to(eng.device)
    n = 8
    aff, ns = dev(np.zeros((1, n, n), np.float32)), dev(np.array([n], np.int32))
    grp = dev(np.zeros((1, n), np.int32))
    emb = dev(np.zeros((1, nodes, spk), np.float32))
    ints = [dev(np.zeros(1, np.int32)) for _ in range(3)]
    work = torch.empty((lib.svk_spectral_workspace_bytes(1, n, n),), dtype=torch.uint8, device=eng.device)

    def call(ctx=eng.ctx, aff=aff, n_rec=1, stride=n, ns=ns, group=None, node_stride=n, lo=2, step=2, count=3, lo_spk=1, hi_spk=8,
             work_ptr=work.data_ptr(), work_bytes=work.numel(), emb=emb, counts=ints):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.svk_spectral_embed(ctx, ptr(aff), n_rec, stride, ptr(ns), ptr(group), node_stride, lo, step, count, lo_spk, hi_spk,
                                      None, work_ptr, work_bytes, ptr(emb), *[ptr(t) for t in counts], None, None, None, None, None)

    assert call() == 0
    assert call(ctx=None) == -1
    for missing in ("aff", "ns", "emb"):
        assert call(**{missing: None}) == -1, missing
    assert call(counts=[ints[0], None, ints[2]]) == -1
    assert call(n_rec=-1) == -1 and call(stride=-1) == -1 and call(node_stride=-1) == -1
    assert call(node_stride=nodes + 1) == -1 and call(stride=top + 1, group=grp) == -1
    assert call(node_stride=n - 1) == -1                                   # without groups every window is a node
    assert call(node_stride=n - 1, group=grp) == 0                         # with groups the stride may exceed the nodes
    assert call(lo=0) == -1 and call(step=0) == -1 and call(count=0) == -1
    assert call(lo_spk=0) == -1 and call(lo_spk=3, hi_spk=2) == -1 and call(hi_spk=spk + 1) == -1 and call(hi_spk=spk) == 0
    assert call(work_bytes=work.numel() - 1) == -1 and call(work_ptr=None, work_bytes=0) == -1
    assert call(work_ptr=work.data_ptr() + 8, work_bytes=work.numel()) == -1                      # misaligned workspace
    assert lib.svk_spectral_embed(eng.ctx, aff.data_ptr() + 2, 1, n, ns.data_ptr(), None, n, 2, 2, 3, 1, 8, None, work.data_ptr(),
                                  work.numel(), emb.data_ptr(), *[t.data_ptr() for t in ints], None, None, None, None, None) == -1
    # n_rec == 0 looks at no pointer
    assert lib.svk_spectral_embed(eng.ctx, None, 0, n, None, None, n, 2, 2, 3, 1, 8, None, None, 0, *[None] * 9) == 0
    eng.synchronize()
    with pytest.raises(ValueError):
        eng.spectral_embed(aff, [n], neighbours=(4, 2, 1))
