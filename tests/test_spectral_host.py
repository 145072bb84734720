"""What svk_spectral_embed's tests rest on, checked without a GPU: the NumPy definition (tests/spectral_f64_ref.py) against spectra
known in closed form, its decisions on the block inputs, the margin conditions of EVERY input the GPU tests use (a decision
that hinges on the last bits of an eigenvalue would compare two eigensolvers, not the kernel with its definition), and the
argument rules of Diarizer.diarize that need no engine."""
import types

import numpy as np
import pytest

import spectral_cases as cases
import spectral_f64_ref as ref
from speaker_verification_amd import diarization as dz


@pytest.fixture(scope="module")
def blocks():
    return cases.blocks_batch()


# A backward-stable symmetric eigensolver moves every eigenvalue by a modest multiple of m 2^-52 ||L||_2; 4 units of
# m 2^-52 lambda_max is the allowance the device gets over its yardstick, asked here of the yardsticks themselves.
@pytest.mark.parametrize("case", cases.known_spectra(), ids=lambda c: c[0])
def test_reference_and_jacobi_restatement_give_the_exact_spectra(case):
    name, aff, p, exact = case
    m = aff.shape[0]
    out = ref.spectral(aff, m, neighbours=p)
    L = ref.laplacian(out["graph"])
    assert out["neighbours"] == p and (np.diag(L) == p).all(), "every node of these graphs has degree p"
    k = out["n_speakers"]
    e_val, e_res, e_orth = ref.accuracy(L, out["eigval"], out["eigvec"], exact)
    assert max(e_val, e_res, e_orth) <= 4.0, "numpy.linalg.eigh: %s" % ((e_val, e_res, e_orth),)
    lam, V, sweeps, converged = ref.jacobi(L)
    assert converged and sweeps <= 12
    e_val, e_res, e_orth = ref.accuracy(L, lam, V[:, :k], exact)
    assert max(e_val, e_res, e_orth) <= 4.0, "Jacobi restatement: %s" % ((e_val, e_res, e_orth),)
    assert out["margin_keep"] > cases.MARGIN and out["margin_gap"] > cases.MARGIN and out["margin_cut"] > cases.MARGIN


def test_closed_forms():
    assert ref.complete_union_spectrum(4, 2).tolist() == [0, 0, 4, 4, 4, 4, 4, 4]
    c6 = ref.cycle_spectrum(6).astype(np.float64)
    assert np.allclose(c6, [0, 1, 1, 3, 3, 4], atol=1e-15)
    assert ref.cycle_spectrum(128).dtype == np.longdouble


def test_round_robin_meets_every_pair_once():
    for M2 in (2, 4, 16, 128):
        seen = set()
        for r in range(M2 - 1):
            P, Q = ref.round_pairs(M2, r)
            assert (P < Q).all() and len(set(P) | set(Q)) == M2
            seen |= set(zip(P.tolist(), Q.tolist()))
        assert len(seen) == M2 * (M2 - 1) // 2


def test_reference_graph_ties_and_node_means():
    M = np.array([[0, .5, .5, .5], [.5, 0, .25, 1], [.5, .25, 0, 0], [.5, 1, 0, 0]])
    order = ref.neighbour_order(M)
    assert order.tolist() == [[1, 2, 3], [3, 0, 2], [0, 1, 3], [1, 0, 2]]           # equals go to the lower index
    assert ref.graph2(order, 1).tolist() == [[0, 1, 1, 0], [1, 0, 0, 2], [1, 0, 0, 0], [0, 2, 0, 0]]
    aff = np.array([[9, 1, 2, 3], [9, 9, 4, 5], [9, 9, 9, 6], [9, 9, 9, 9]], np.float32)      # 9: never read
    M, m = ref.node_means(aff, 4, np.array([0, 1, 0, 1]), 8)
    assert m == 2 and M[0, 1] == M[1, 0] == (1 + 3 + 4 + 6) / 4.0 and M[0, 0] == 0
    assert ref.node_means(aff, 4, np.array([0, 2, 0, 2]), 8) is None                # node 1 has no member
    assert ref.node_means(aff, 4, np.array([0, 8, 0, 1]), 8) is None                # a label out of range
    assert ref.node_means(aff, 5) is None
    aff[0, 3] = np.nan
    assert ref.node_means(aff, 4) is None and ref.node_means(aff, 3) is not None
    assert ref.node_means(aff, 4, np.array([0, 1, 1, 0]), 8) is not None            # 0 and 3 share a node: not read


def test_reference_recovers_count_and_labels_on_the_block_inputs(blocks):
    aff, n_seg, who = blocks
    for r, out in enumerate(cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP)):
        n = int(n_seg[r])
        assert out["n_nodes"] == n and out["n_speakers"] == cases.BLOCK_SPEAKERS[n], "recording %d" % r
        assert np.array_equal(ref.embedding_labels(out["embed"], n, out["n_speakers"]), who[r]), "recording %d" % r
    assert sorted(set(cases.BLOCK_SPEAKERS.values())) == [0, 1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("bounds", sorted(cases.BOUNDS))
def test_every_decision_input_keeps_its_margins(blocks, bounds):
    aff, n_seg, _ = blocks
    bounds = cases.BOUNDS[bounds]
    outs = cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP, **bounds)
    free = cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP)
    for r, out in enumerate(outs):
        for what in ("margin_ratio", "margin_gap", "margin_keep", "margin_cut"):
            assert out[what] > cases.MARGIN, "recording %d (n = %d): %s = %g" % (r, n_seg[r], what, out[what])
    if "min_speakers" in bounds and "target" not in bounds:       # each bound binds somewhere
        assert any(o["n_speakers"] == 3 and f["n_speakers"] < 3 for o, f in zip(outs, free))
    if "max_speakers" in bounds:
        assert any(o["n_speakers"] < f["n_speakers"] for o, f in zip(outs, free))


def test_jacobi_restatement_converges_where_eigenvalues_pile_up():
    """Nearly complete graphs of two tight speakers: every candidate of the sweep converges well inside the sweep limit, and
    the decisions on these inputs keep their margins too (the GPU test compares them)."""
    aff, n_seg = cases.tight_batch()
    worst = 0
    for r, n in enumerate(n_seg):
        order = ref.neighbour_order(ref.node_means(aff[r], n)[0])
        for p in list(range(2, n - 1, 2)) + [n - 1]:
            lam, _, sweeps, converged = ref.jacobi(ref.laplacian(ref.graph2(order, p)))
            assert converged, "recording %d, p = %d" % (r, p)
            worst = max(worst, sweeps)
    assert worst <= ref.MAX_SWEEPS // 2, worst
    for r, out in enumerate(cases.reference_batch(aff, n_seg, neighbours=cases.SWEEP)):
        for what in ("margin_ratio", "margin_gap", "margin_keep", "margin_cut"):
            assert out[what] > cases.MARGIN, "recording %d (n = %d): %s = %g" % (r, n_seg[r], what, out[what])


def test_exact_logic_inputs_are_exact():
    """Multiples of 1/8: the node means of the grouped batch are sums of at most 300^2 of them (exact in any order) and one
    division, so the graph comparison is one of integers."""
    aff, n_seg, group = cases.grouped_ties_batch()
    assert np.array_equal(aff * 8, np.round(aff * 8))
    assert [int(group[r, :n].max()) + 1 if n else 0 for r, n in enumerate(n_seg)] == [min(n, cases.GROUPED_NODES) for n in n_seg]
    assert (group[-1] >= 0).all() and len(np.unique(group[-1])) == cases.GROUPED_NODES


# ---- Diarizer.diarize: the rules that need no engine ---------------------------------------------------------------------
def fake_pipeline():
    return types.SimpleNamespace(plda=None, calibration=None, score_norm=None, backend=None)


def test_diarize_method_rules():
    d = dz.Diarizer(fake_pipeline())
    pcm = np.zeros((1, 16000), np.int16)
    with pytest.raises(ValueError, match="unknown method"):
        d.diarize(pcm, num_speakers=2, method="kmeans")
    with pytest.raises(ValueError, match="threshold"):
        d.diarize(pcm, threshold=0.3, method="spectral")
    with pytest.raises(ValueError, match="threshold"):
        d.diarize(pcm, method="ahc")
    # spectral needs neither: the argument check passes (and the fake pipeline has no engine to go on with)
    dz.Diarizer._arguments("spectral", None, None)
    dz.Diarizer._arguments("spectral", None, 3)
    with pytest.raises(AttributeError, match="eng"):
        d.diarize(pcm, method="spectral")
    assert dz.Diarizer.NEIGHBOURS == (2, 32, 2) and dz.Diarizer.MAX_SPEAKERS == 8
