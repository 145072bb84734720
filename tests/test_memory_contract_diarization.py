"""The memory contract of include/svk.h (Conventions) for the diarization entries: svk_window_crops, svk_segment_affinity, svk_ahc
and svk_spectral_embed, called directly on guarded arenas (tests/memory_contract.py) in the environments A, B and C; the
properties P1-P4 as tests/test_memory_contract_scoring.py states them.  What the header calls untouched keeps its prefill: the
dead rows and columns of d_aff, the labels past d_n_seg, the embedding rows past the node count and everything of d_eigval,
d_eigvec and d_graph outside the chosen graph's block.  What the header says is never read -- affinities on or below the
diagonal or in dead rows, group labels of dead rows -- holds the environment's payload pattern (0, NaN / -1, another finite
number) instead of data.  Cases: two recordings of stride 40 with 40 and 17 live rows at dim 13 and 128, a recording whose
count exceeds the stride (clamped by the affinity, rejected by the clustering entries), and one recording of 130 rows for
svk_ahc's workspace instance."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu
STRIDE = 40
CASES = {"two-recordings": (40, 17), "count-above-the-stride": (41,)}


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _embeddings(n_rec, stride, dim, seed=0):
    """Rows around three speaker centres per recording, so that the clusterings have something to find."""
    g = torch.Generator().manual_seed(100 * dim + n_rec + seed)
    centres = torch.randn((n_rec, 3, dim), generator=g)
    who = torch.randint(0, 3, (n_rec, stride), generator=g)
    x = torch.gather(centres, 1, who[:, :, None].expand(-1, -1, dim)) + 0.4 * torch.randn((n_rec, stride, dim), generator=g)
    x[0, 1] = 0.0                                                    # a zero row: scores exactly 0
    return x.to(torch.float32)


def _live(n_seg, stride):
    """[n_rec, stride] bool: the live rows (a count outside [0, stride] clamped, as svk_segment_affinity reads it)."""
    n = torch.tensor(n_seg).clamp(0, stride)
    return torch.arange(stride)[None, :] < n[:, None]


# ---- svk_window_crops ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("frames,bad", (((150 + 75 * 39, 150 + 75 * 15 + 7), 0), ((150 + 75 * 45, 79, 100, -3), 1)),
                         ids=("40-and-17-windows", "more-windows-than-max_windows"))
def test_window_crops(eng, frames, bad, placed):
    n_rec, K, n_crops = len(frames), STRIDE, 20
    nf = torch.tensor(frames, dtype=torch.int32)
    ref = tuple(M.bits(t) for t in eng.window_crops(nf, K))
    assert list(ref[1]) == ([40, 17] if not bad else [40, 0, 1, 0])
    for env in M.ENV_NAMES:
        for want_spans in (True, False):
            what = "svk_window_crops %s spans %s, %s, environment %s" % (frames, want_spans, placed, env)
            c = M.Contract(eng, env, scalar=placed == "scalar")
            dn = c.input("d_n_frames", nf)
            idx, nwin = c.output("d_crop_idx", torch.int32, (n_rec, K, n_crops)), c.output("d_n_windows", torch.int32, (n_rec,))
            spans = c.output("d_window_span", torch.int32, (n_rec, K, 2)) if want_spans else None
            cnt = c.counter("d_bad_count")
            c.call(eng.lib.svk_window_crops, dn, n_rec, 150, 75, 80, n_crops, K, idx, nwin, spans, cnt)
            M.same_bits(idx.bits(), ref[0], what + ": d_crop_idx")
            M.same_bits(nwin.bits(), ref[1], what + ": d_n_windows")
            if want_spans:
                M.same_bits(spans.bits(), ref[2], what + ": d_window_span")
            M.counter_is(cnt, bad, what + ": d_bad_count")


# ---- svk_segment_affinity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("dim", (13, 128))
@pytest.mark.parametrize("case", tuple(CASES))
def test_segment_affinity(eng, case, dim, placed):
    n_seg = CASES[case]
    n_rec = len(n_seg)
    x, ns = _embeddings(n_rec, STRIDE, dim), torch.tensor(n_seg, dtype=torch.int32)
    ref = M.bits(eng.segment_affinity(x, ns))
    live = _live(n_seg, STRIDE)
    block = (live[:, :, None] & live[:, None, :]).numpy()
    for env in M.ENV_NAMES:
        what = "svk_segment_affinity %s dim %d, %s, environment %s" % (n_seg, dim, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        # rows past d_n_seg are not read: they hold the payload pattern
        dx = c.input_where("d_emb", x, live[:, :, None].expand(-1, -1, dim))
        dn, aff = c.input("d_n_seg", ns), c.output("d_aff", torch.float32, (n_rec, STRIDE, STRIDE))
        c.call(eng.lib.svk_segment_affinity, dx, n_rec, STRIDE, dim, dn, aff)
        got = aff.bits()
        M.same_bits(got[block], ref[block], what + ": live entries")
        M.keeps_prefill(aff, got[~block], what + ": entries of dead rows and columns")


# ---- svk_ahc ---------------------------------------------------------------------------------------------------------------
def _read_by_clustering(n_seg, stride):
    """[n_rec, stride, stride] bool: entries ABOVE the diagonal of live rows -- all svk_ahc and svk_spectral_embed may read.  A
    recording whose count is outside [0, stride] is rejected on its count: nothing of it is read."""
    n = torch.tensor(n_seg)
    n = torch.where((n < 0) | (n > stride), torch.zeros_like(n), n)
    live = torch.arange(stride)[None, :] < n[:, None]
    upper = torch.triu(torch.ones((stride, stride), dtype=torch.bool), diagonal=1)
    return live[:, :, None] & live[:, None, :] & upper[None]


def _ahc_direct(eng, env, placed, aff, n_seg, threshold, target, want_merges):
    n_rec, stride = aff.shape[0], aff.shape[1]
    c = M.Contract(eng, env, scalar=placed == "scalar")
    da = c.input_where("d_aff", aff, _read_by_clustering(n_seg, stride))
    dn, dt = c.input("d_n_seg", torch.tensor(n_seg, dtype=torch.int32)), c.input("d_target", target)
    nbytes = eng.lib.svk_ahc_workspace_bytes(n_rec, stride)
    work = c.workspace(nbytes)
    labels, count = c.output("d_labels", torch.int32, (n_rec, stride)), c.output("d_n_clusters", torch.int32, (n_rec,))
    pair = c.output("d_merge_pair", torch.int32, (n_rec, stride, 2)) if want_merges else None
    sim = c.output("d_merge_sim", torch.float64, (n_rec, stride)) if want_merges else None
    cnt = c.counter("d_bad_count")
    c.call(eng.lib.svk_ahc, da, n_rec, stride, dn, threshold, 1, 0x7fffffff, dt, work, nbytes, labels, count, pair, sim, cnt)
    return labels, count, pair, sim, cnt, nbytes


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("dim", (13, 128))
@pytest.mark.parametrize("case", tuple(CASES) + ("workspace-instance",))
def test_ahc(eng, case, dim, placed):
    n_seg, stride = (CASES[case], STRIDE) if case in CASES else ((130,), 132)
    n_rec = len(n_seg)
    aff = eng.segment_affinity(_embeddings(n_rec, stride, dim), torch.tensor(n_seg, dtype=torch.int32)).cpu()
    rejected = [n > stride for n in n_seg]
    written = _live([stride if r else n for n, r in zip(n_seg, rejected)], stride).numpy()    # a rejected recording: all -1
    target = torch.tensor([0, 3][:n_rec], dtype=torch.int32)
    for tg, want_merges in ((None, True), (target, False)):
        ref = eng.ahc(aff, torch.tensor(n_seg, dtype=torch.int32), threshold=0.5, target=tg, want_merges=want_merges)
        for env in M.ENV_NAMES:
            what = "svk_ahc %s stride %d dim %d target %s, %s, environment %s" % (n_seg, stride, dim, tg is not None, placed, env)
            labels, count, pair, sim, bad, nbytes = _ahc_direct(eng, env, placed, aff, n_seg, 0.5, tg, want_merges)
            assert (nbytes > 0) == (case == "workspace-instance")
            got = labels.bits()
            M.same_bits(got[written], M.bits(ref[0])[written], what + ": d_labels of the live rows")
            M.keeps_prefill(labels, got[~written], what + ": d_labels past d_n_seg")
            M.same_bits(count.bits(), M.bits(ref[1]), what + ": d_n_clusters")
            if want_merges:
                M.same_bits(pair.bits(), M.bits(ref[2]), what + ": d_merge_pair")
                M.same_bits(sim.bits(), M.bits(ref[3]), what + ": d_merge_sim")
            M.counter_is(bad, sum(rejected), what + ": d_bad_count")


# ---- svk_spectral_embed ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("grouped", (False, True), ids=("windows-as-nodes", "groups-given"))
@pytest.mark.parametrize("dim", (13, 128))
@pytest.mark.parametrize("case", tuple(CASES))
def test_spectral_embed(eng, case, dim, grouped, placed):
    n_seg = CASES[case]
    n_rec, K = len(n_seg), 8
    ns = torch.tensor(n_seg, dtype=torch.int32)
    aff = eng.segment_affinity(_embeddings(n_rec, STRIDE, dim), ns).cpu()
    rejected = [n > STRIDE for n in n_seg]
    group = None
    if grouped:                      # svk_ahc's labels for about ten clusters a recording
        group = eng.ahc(aff, ns.clamp(0, STRIDE), target=torch.tensor([10, 9][:n_rec], dtype=torch.int32))[0].cpu()
    nodes = eng.spectral_limits()[0] if grouped else STRIDE
    lo, step, count = 2, 2, 16
    ref = eng.spectral_embed(aff, ns, group=group, neighbours=(lo, lo + step * (count - 1), step), max_speakers=K,
                             want_spectrum=True, want_graph=True)
    embed_r, nodes_r, spk_r, nb_r, eigval_r, eigvec_r, graph_r, ratio_r = (M.bits(t) for t in ref)
    m = [max(int(v), 0) for v in ref[1].cpu()]
    k = [max(int(v), 0) for v in ref[2].cpu()]
    assert all((mm == 0) == r for mm, r in zip(m, rejected)), "the reference run rejects exactly the out-of-range counts"
    a = np.arange(nodes)
    # the elements the header defines: embedding rows below m (all node_stride rows of a rejected recording: zeros), the m
    # eigenvalues, the first m entries of the first k eigenvectors, the m x m block of the graph
    embed_w = np.stack([np.broadcast_to((a < (nodes if r else mm))[:, None], (nodes, K)) for mm, r in zip(m, rejected)])
    eigval_w = np.stack([a < mm for mm in m])
    eigvec_w = np.stack([(np.arange(K) < kk)[:, None] & (a < mm)[None, :] for mm, kk in zip(m, k)])
    graph_w = np.stack([(a < mm)[:, None] & (a < mm)[None, :] for mm in m])
    nbytes = eng.lib.svk_spectral_workspace_bytes(n_rec, STRIDE, nodes)
    assert nbytes > 0
    for env in M.ENV_NAMES:
        what = "svk_spectral_embed %s dim %d groups %s, %s, environment %s" % (n_seg, dim, grouped, placed, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        da = c.input_where("d_aff", aff, _read_by_clustering(n_seg, STRIDE))
        dn = c.input("d_n_seg", ns)
        dg = c.input_where("d_group", group, _live(n_seg, STRIDE) & ~torch.tensor(rejected)[:, None]) if grouped else None
        work = c.workspace(nbytes)
        embed = c.output("d_embed", torch.float32, (n_rec, nodes, K))
        n_nodes, n_spk, chosen = (c.output(name, torch.int32, (n_rec,)) for name in ("d_n_nodes", "d_n_speakers", "d_neighbours"))
        eigval, eigvec = c.output("d_eigval", torch.float64, (n_rec, nodes)), c.output("d_eigvec", torch.float64, (n_rec, K, nodes))
        graph, ratio = c.output("d_graph", torch.uint8, (n_rec, nodes, nodes)), c.output("d_ratio", torch.float64, (n_rec, count))
        cnt = c.counter("d_bad_count")
        c.call(eng.lib.svk_spectral_embed, da, n_rec, STRIDE, dn, dg, nodes, lo, step, count, 1, K, None, work, nbytes, embed,
               n_nodes, n_spk, chosen, eigval, eigvec, graph, ratio, cnt)
        for got, want, name in ((n_nodes, nodes_r, "d_n_nodes"), (n_spk, spk_r, "d_n_speakers"), (chosen, nb_r, "d_neighbours"),
                                (ratio, ratio_r, "d_ratio")):
            M.same_bits(got.bits(), want, what + ": " + name)
        for got, want, mask, name in ((embed, embed_r, embed_w, "d_embed"), (eigval, eigval_r, eigval_w, "d_eigval"),
                                      (eigvec, eigvec_r, eigvec_w, "d_eigvec"), (graph, graph_r, graph_w, "d_graph")):
            b = got.bits()
            M.same_bits(b[mask], want[mask], what + ": %s, the elements the header defines" % name)
            M.keeps_prefill(got, b[~mask], what + ": %s outside them" % name)
        M.counter_is(cnt, sum(rejected), what + ": d_bad_count")
