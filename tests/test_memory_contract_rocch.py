"""The memory contract of include/svk.h (Conventions) for the entries of its sections "the ROC convex hull" and "the PAV map", svk_rocch and svk_pav_apply
(csrc/roc.hip, csrc/rocch.h): called directly on guarded arenas (tests/memory_contract.py) in the environments A, B and C,
placed for the vector paths and for the scalar ones.  The guards stay intact, the inputs byte-identical, and the results are the
same bits in all three environments and equal the Engine wrapper's on ordinary tensors -- so nothing in the workspace (the two
hull buffers and their counts included) or in the output planes is read before it is written; plane elements from the vertex
count on keep the prefill.  svk_rocch's cases: one point more than a tile (the first global merge, a one-point right hull) and
a hull that keeps every point (tests/rocch_ref.py)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M              # noqa: E402  (tests/ is on sys.path)
import rocch_ref as R                    # noqa: E402

pytestmark = pytest.mark.gpu

OPS = R.OPS


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _f64bits(values):
    return np.asarray(list(values), dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("name", ("points_2049", "farey_8"))
def test_rocch(eng, name, placed):
    lab, sc = R.gpu_cases()[name]
    s, lb = torch.from_numpy(sc.copy()), torch.from_numpy(lab.copy())
    n = s.numel()
    ref = eng.rocch(s, lb, OPS)
    count = len(ref["vertices"])
    assert count == len(R.reference(name)[2])
    want = [ref["eer"], ref["auc"], ref["positives"], ref["points"], ref["eer_threshold"]]
    for o in range(len(OPS)):
        want += [ref[k][o] for k in ("min_dcf", "threshold", "p_miss", "p_fa")]
    want.append(count)
    ops = (C.c_double * (3 * len(OPS)))(*[v for op in OPS for v in op])
    nbytes, n_out = eng.lib.svk_rocch_workspace_bytes(n), 6 + 4 * len(OPS)
    for capacity in (count, int(eng.lib.svk_rocch_max_vertices(n))):
        for env in M.ENV_NAMES:
            what = "svk_rocch %s capacity %d, %s, environment %s" % (name, capacity, placed, env)
            c = M.Contract(eng, env, scalar=placed == "scalar")
            ds, dl, work = c.input("d_scores", s), c.input("d_labels", lb), c.workspace(nbytes)
            vf, vt = c.output("d_vf", torch.int32, (capacity,)), c.output("d_vt", torch.int32, (capacity,))
            vs = c.output("d_vscore", torch.float32, (capacity,))
            out = (C.c_double * (n_out + 4))(*([-5.0] * (n_out + 4)))
            c.call(eng.lib.svk_rocch, ds, dl, n, ops, len(OPS), work, nbytes, vf, vt, vs, capacity, out)
            assert list(out[n_out:]) == [-5.0] * 4, what + ": h_out was written past its %d entries" % n_out
            M.same_bits(_f64bits(out[:n_out]), _f64bits(want), what + ": h_out")
            M.same_bits(vf.bits()[:count], ref["vertices"][:, 0].astype(np.uint32), what + ": d_vf")
            M.same_bits(vt.bits()[:count], ref["vertices"][:, 1].astype(np.uint32), what + ": d_vt")
            M.same_bits(vs.bits()[:count], ref["vertex_scores"].view(np.uint32), what + ": d_vscore")
            for plane, label in ((vf, "d_vf"), (vt, "d_vt"), (vs, "d_vscore")):
                M.keeps_prefill(plane, plane.bits()[count:], what + ": %s from the vertex count on" % label)


# scores / output placement in the scalar placing: both one float past the boundary (a scalar head, 16-byte body), or the
# output two floats past it (no common 16-byte phase: the scalar kernel)
PAV_OUT_OFF = {"same-phase": None, "other-phase": 8}


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("phase", list(PAV_OUT_OFF))
@pytest.mark.parametrize("n_bins", (33, 4097), ids=("table-in-lds", "table-in-global"))
@pytest.mark.parametrize("n", (1, 5, 4099))
def test_pav_apply(eng, n, n_bins, phase, placed):
    rng = np.random.default_rng(n + n_bins)
    edges = np.sort(np.unique(rng.standard_normal(2 * n_bins).astype(np.float32)))[::-1][:n_bins].copy()
    llr = rng.standard_normal(n_bins).astype(np.float32)
    sc = np.r_[edges[:1], rng.choice(np.r_[edges, rng.standard_normal(64).astype(np.float32) * 2, np.float32(np.nan)], n)][:n]
    sc = np.ascontiguousarray(sc, dtype=np.float32)
    ref = M.bits(eng.pav_apply(sc, edges, llr))
    M.same_bits(ref, R.pav_apply(sc, edges, llr), "the wrapper against the reference")
    for env in M.ENV_NAMES:
        what = "svk_pav_apply n %d n_bins %d, %s %s, environment %s" % (n, n_bins, placed, phase, env)
        c = M.Contract(eng, env, scalar=placed == "scalar")
        ds, de, dl = c.input("d_scores", sc), c.input("d_edges", edges), c.input("d_llr", llr)
        out = c.output("d_out", torch.float32, (n,), off=PAV_OUT_OFF[phase])
        c.call(eng.lib.svk_pav_apply, ds, n, de, dl, n_bins, out)
        M.same_bits(out.bits(), ref, what)
        if phase == "same-phase":            # in place
            c = M.Contract(eng, env, scalar=placed == "scalar")
            de, dl = c.input("d_edges", edges), c.input("d_llr", llr)
            both = c.output("d_scores == d_out", torch.float32, (n,), prefill=torch.from_numpy(sc))
            c.call(eng.lib.svk_pav_apply, both, n, de, dl, n_bins, both)
            M.same_bits(both.bits(), ref, what + ", in place")
