"""The ROC convex hull without a GPU: the reference of tests/rocch_ref.py against an independent statement of the same object
(pool adjacent violators), the device's merge predicate restated in Python against the chain, the teeth of the GPU case list
(every mutant of the hull rule differs on some case), the vertex bound, the names of the entries of include/svk.h's sections
"the ROC convex hull" and "the PAV map" in the binding, the returns that need no device, and PavCalibration's host logic
through injected hull vertices.  All integers: every comparison is exact."""
import ctypes
import os

import numpy as np
import pytest

import rocch_ref as R

CASES = list(R.gpu_cases())
SMALL = [c for c in CASES if c != "n300000"]          # (what the mutants and the PAV tables run on: they die, or hold, earlier)


def vertices_of(name):
    pts, _, keep = R.reference(name)
    return [pts[i] for i in keep]


# ---- the reference -----------------------------------------------------------------------------------------------------------
def test_the_cases_are_what_the_issue_counted():
    count = lambda name: (len(R.gpu_cases()[name][0]), len(R.reference(name)[0]), len(R.reference(name)[2]))      # noqa: E731
    assert count("farey_8") == (370, 46, 46) and count("farey_72") == (229558, 3178, 3178)
    assert count("flat_then_arc") == (7200, 7201, 3) and count("n5000_16_levels")[1] == 16
    assert count("n300000") == (300000, 299410, 112)
    assert [count("points_%d" % p)[1] for p in (2047, 2048, 2049, 4097)] == [2047, 2048, 2049, 4097]
    assert vertices_of("all_equal")[1:] == [R.reference("all_equal")[0][-1]] and len(R.reference("all_equal")[0]) == 2
    assert vertices_of("separated") == [(0, 0), (0, 40), (60, 40)] and vertices_of("inverted") == [(0, 0), (40, 60)]
    assert R.min_cllr(vertices_of("inverted")) == 1.0 and R.min_cllr(vertices_of("separated")) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_chain_edges_are_the_pav_blocks(name):
    pts, _, keep = R.reference(name)
    assert keep == R.pav_pool(pts)                    # the same boundaries, hence the same counts in every block


@pytest.mark.parametrize("leaf", (2, 8, 2048))
def test_merge_predicate_equals_the_chain(leaf):
    """v(u) by bisection, as the kernel's routine finds it."""
    for name in CASES:
        pts, _, keep = R.reference(name)
        assert R.hull_merge(pts, leaf) == keep, name


@pytest.mark.parametrize("leaf", (2, 8, 2048))
def test_bisection_finds_the_first_index_of_the_definition(leaf):
    """The same merges with v(u) as the definition states it, the first i from the left: the predicate is monotone along B."""
    for name in CASES:
        pts, _, keep = R.reference(name)
        assert R.hull_merge(pts, leaf, bisect=False) == keep, name


MUTANTS = {
    "pop on > 0": lambda lab, sc: [p for p in _mutant_points(lab, sc, pop_collinear=False)],
    "ties not pooled": lambda lab, sc: _mutant_points(lab, sc, pool_ties=False),
    "origin left out": lambda lab, sc: _mutant_points(lab, sc, origin=False),
    "right test strict": lambda lab, sc: _mutant_merge(lab, sc),
}


def _mutant_points(lab, sc, pool_ties=True, origin=True, pop_collinear=True):
    pts, _ = R.roc_points(lab, sc, pool_ties, origin)
    return [pts[i] for i in R.hull_chain(pts, pop_collinear)]


def _mutant_merge(lab, sc):
    pts, _ = R.roc_points(lab, sc)
    return [pts[i] for i in R.hull_merge(pts, 8, right_strict=True)]


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_of_the_rule_differs_on_some_case(mutant):
    caught = [name for name in SMALL if MUTANTS[mutant](*R.gpu_cases()[name]) != vertices_of(name)]
    print("MUTANT %s: caught by %s" % (mutant, caught))
    assert caught, mutant


# ---- the entries in the binding and the library ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from speaker_verification_amd import _lib as binding
    if not os.path.exists(binding.LIB_PATH):
        entry.build()
    return binding.load()


def test_the_five_entries_are_bound():
    """(tests/test_cabi.py walks the header, the table and the library for every entry; this pins the names)"""
    from speaker_verification_amd import _lib as binding
    assert sorted(n for n in binding.SIGNATURES if n.startswith(("svk_rocch", "svk_pav"))) == [
        "svk_pav_apply", "svk_rocch", "svk_rocch_level_counts_offset", "svk_rocch_max_vertices", "svk_rocch_workspace_bytes"]


def test_refusals_need_no_device(lib):
    from speaker_verification_amd import _lib as binding
    out = (ctypes.c_double * 6)()
    assert lib.svk_rocch(None, None, None, 2, None, 0, None, 0, None, None, None, 1, out) == binding.SVK_ERR_BAD_ARG
    assert lib.svk_pav_apply(None, None, 0, None, None, 1, None) == binding.SVK_ERR_BAD_ARG
    assert lib.svk_rocch_workspace_bytes(1) == 0 and lib.svk_rocch_max_vertices(0) == 0
    assert lib.svk_rocch_level_counts_offset(1) == 0
    for n in (2, 1000, 300000):
        assert lib.svk_rocch_workspace_bytes(n) > lib.svk_roc_dcf_workspace_bytes(n) + 16 * n
        tiles = (n + 1 + 2047) // 2048                       # room for every level's counts: below 2 tiles + 64 of them
        assert lib.svk_roc_dcf_workspace_bytes(n) + 16 * n < lib.svk_rocch_level_counts_offset(n) \
            <= lib.svk_rocch_workspace_bytes(n) - 4 * (2 * tiles + 64)


def test_vertex_bound(lib):
    for name in CASES:
        n = len(R.gpu_cases()[name][0])
        assert lib.svk_rocch_max_vertices(n) >= len(R.reference(name)[2]), name
    assert [lib.svk_rocch_max_vertices(n) for n in (1, 2, 3)] == [2, 3, 4]             # K <= n: nothing tighter exists there
    top = lib.svk_rocch_max_vertices(2 ** 32 - 1)
    assert 1.04 * (2.0 ** 32) ** (2 / 3) < top < 1.1 * (2.0 ** 32) ** (2 / 3)          # ~ 2.7e6 vertices, 33 MB of planes
    # the bound is the count argument of the header, restated: all vectors of weight <= S cost S (S + 1) (S + 2) / 3
    for n in (2, 3, 8, 9, 370, 229558, 2 ** 32 - 1):
        s = 1
        while s * (s + 1) * (s + 2) // 3 < n:
            s += 1
        assert lib.svk_rocch_max_vertices(n) == min(s * (s + 3) // 2, n) + 1
    # any int64 is taken: beyond the 2^32 - 1 trials svk_rocch accepts the bound stays that of 2^32 - 1
    for n in (2 ** 32, 2 ** 62, 2 ** 63 - 1):
        assert lib.svk_rocch_max_vertices(n) == top
    assert lib.svk_rocch_max_vertices(-5) == 0


# ---- the derived values and PavCalibration on the host -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_derived_values_of_the_package(name):
    from speaker_verification_amd import calibration as cal
    v = vertices_of(name)
    got, want = cal.min_cllr_of(np.array(v)), R.min_cllr(v)
    assert abs(got - want) <= (len(v) - 1 + 4) * 2.0 ** -52 * want and 0.0 <= got <= 1.0
    assert abs(cal.rocch_eer_of(np.array(v)) - float(R.rocch_eer(v))) <= 4 * 2.0 ** -52
    pts = R.reference(name)[0]
    assert cal.hull_chain(pts) == R.reference(name)[2]


@pytest.mark.parametrize("laplace", (False, True))
@pytest.mark.parametrize("name", SMALL)
def test_pav_table_through_injected_vertices(name, laplace):
    from speaker_verification_amd.calibration import PavCalibration
    lab, sc = R.gpu_cases()[name]
    pts, vals, keep = R.reference(name)
    hull = (np.array([pts[i] for i in keep]), np.array([np.inf] + [vals[i] for i in keep[1:]], np.float32))
    pav = PavCalibration(laplace=laplace).fit(hull=hull)
    edges, llr = R.pav_table(lab, sc, laplace)
    assert pav.n_sys == 1 and pav.edges_.dtype == pav.llr_.dtype == np.float32
    assert np.array_equal(pav.edges_.view(np.uint32), edges.view(np.uint32))
    assert np.array_equal(pav.llr_.view(np.uint32), llr.view(np.uint32))
    assert (np.diff(pav.edges_) < 0).all() and (np.diff(pav.llr_.astype(np.float64)) < 0).all()      # a monotone step map
    values = np.where(sc == 0, np.float32(0), sc)
    assert np.isin(pav.edges_, values).all() and pav.edges_[-1] == values.min()
    if laplace:
        assert np.isfinite(pav.llr_).all()
    else:
        assert len(edges) == len(keep) - 1


def test_pav_save_load_round_trip(tmp_path):
    from speaker_verification_amd.calibration import PavCalibration
    pts, vals, keep = R.reference("farey_8")
    hull = (np.array([pts[i] for i in keep]), np.array([np.inf] + [vals[i] for i in keep[1:]], np.float32))
    for laplace in (False, True):
        pav = PavCalibration(laplace=laplace).fit(hull=hull)
        path = str(tmp_path / ("pav%d.npz" % laplace))
        pav.save(path)
        back = PavCalibration.load(path)
        assert back.laplace == laplace and back.n_sys == 1
        assert np.array_equal(back.edges_.view(np.uint32), pav.edges_.view(np.uint32))
        assert np.array_equal(back.llr_.view(np.uint32), pav.llr_.view(np.uint32))
    with pytest.raises(RuntimeError, match="not fitted"):
        PavCalibration().save(str(tmp_path / "x.npz"))
    with pytest.raises(RuntimeError, match="not fitted"):
        PavCalibration().apply(np.zeros(3, np.float32))
