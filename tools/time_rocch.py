"""HIP-event medians of the ROC convex hull and the PAV map (include/svk.h: "the ROC convex hull", "the PAV map"), 20 calls each, alternated call by call:

  svk_rocch against svk_roc_dcf on the same buffers at 148 642 x 1 211 = 1.8e8 trials (cosine scores of seeded unit-norm
  embeddings, as tools/time_roc.py) and at the 581 480 trials of VoxCeleb1-E (seeded N(0, 1) + 2 label scores): the difference
  is the hull's cost.  With it: the merge levels and the points that survive the tile pass and every level (the counts the
  entry leaves in its workspace, at svk_rocch_level_counts_offset).
  svk_pav_apply at 1.8e8 scores with 112 and 3 177 bins (out of place) against torch.bucketize + index on the same operands;
  design bytes (a score read, an LLR written: 8 B per score) and TB/s.  svk_calibration_apply on the same scores is the
  yardstick for how far the search is from the bytes.

SVK_ROCCH_SMALL=1 leaves out the 1.8e8-trial shapes.  One JSON line on stdout."""
import ctypes as C
import json
import os

import _timing as T          # (puts the repository on sys.path)

NT, NS, D = 148642, 1211, 128
VOX1_E = 581480
REPS = 20
OPS = ((0.01, 1, 1), (0.05, 1, 1))


def level_counts(torch, lib, work, n, points):
    """[points surviving the tile pass, then every merge level] from the counts the entry leaves in its workspace."""
    counts = work[int(lib.svk_rocch_level_counts_offset(n)):].view(torch.int32).cpu().numpy()
    out, at, hulls = [], 0, (points + 2047) // 2048
    while True:
        out.append(int(counts[at:at + hulls].sum()))
        if hulls == 1:
            return out
        at, hulls = at + hulls, (hulls + 1) // 2


def roc_pair(torch, eng, lib, name, sc, lb, res):
    n = sc.numel()
    ops = (C.c_double * (3 * len(OPS)))(*[v for op in OPS for v in op])
    work = torch.empty(int(lib.svk_rocch_workspace_bytes(n)), dtype=torch.uint8, device=eng.device)
    cap = int(lib.svk_rocch_max_vertices(n))
    planes = torch.empty((3, cap), dtype=torch.int32, device=eng.device)
    out = (C.c_double * (6 + 4 * len(OPS)))()
    eng._stream()

    def dcf():
        assert lib.svk_roc_dcf(eng.ctx, eng._ptr(sc), eng._ptr(lb), n, ops, len(OPS), eng._ptr(work), work.numel(), out) == 0

    def rocch():
        assert lib.svk_rocch(eng.ctx, eng._ptr(sc), eng._ptr(lb), n, ops, len(OPS), eng._ptr(work), work.numel(),
                             eng._ptr(planes[0]), eng._ptr(planes[1]), eng._ptr(planes[2]), cap, out) == 0

    times = T.alternated(torch, {"roc_dcf": dcf, "rocch": rocch}, REPS, 2)
    a = T.put("roc_dcf_" + name, times["roc_dcf"])
    b = T.put("rocch_" + name, times["rocch"])
    rocch()
    torch.cuda.synchronize()
    points = int(out[3]) + 1
    survivors = level_counts(torch, lib, work, n, points)
    # what can be checked at this size without a second sort: the ends, and a strict right turn at every interior vertex
    count = int(out[5 + 4 * len(OPS)])
    v = planes[:2, :count].cpu().numpy().view("uint32").T.astype(object)
    assert tuple(v[0]) == (0, 0) and tuple(v[-1]) == (n - int(out[2]), int(out[2])) and survivors[-1] == count
    assert all((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0 for a, b, c in zip(v[:-2], v[1:-1], v[2:]))
    res["hull"][name] = {"trials": n, "points": points, "vertices": count, "capacity": cap,
                         "merge_levels": len(survivors) - 1, "survivors": survivors, "hull_ms": round(b - a, 4),
                         "workspace_bytes": {"roc_dcf": int(lib.svk_roc_dcf_workspace_bytes(n)), "rocch": work.numel()}}


def pav_pair(torch, eng, sc, n_bins, res):
    import numpy as np
    lo, hi = float(sc.min()), float(sc.max())
    edges = torch.from_numpy(np.linspace(hi, lo, n_bins + 2)[1:-1].astype(np.float32)).to(eng.device)
    llr = torch.linspace(8.0, -8.0, n_bins, device=eng.device)
    out = torch.empty_like(sc)
    asc = edges.flip(0).contiguous()             # bucketize wants ascending boundaries

    def ours():
        eng.pav_apply(sc, edges, llr, out=out)

    def torch_route():
        # boundaries e_asc; right=True counts the edges <= s: bin k = n_bins - that count, the last bin below every edge
        k = (n_bins - torch.bucketize(sc, asc, right=True)).clamp_(max=n_bins - 1)
        return llr[k]

    ours()
    assert torch.equal(out, torch_route())
    times = T.alternated(torch, {"pav": ours, "torch": torch_route}, REPS, 2)
    T.put("pav_apply_%d_bins" % n_bins, times["pav"], 8 * sc.numel())
    T.put("torch_bucketize_index_%d_bins" % n_bins, times["torch"], 8 * sc.numel())


def main():
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, sha=True, reps=REPS, ms={}, spread_ms={}, bytes={}, tb_s={}, hull={})
    rng = np.random.default_rng(7)
    lab = (rng.random(VOX1_E) < 0.5).astype(np.uint8)
    sc = (rng.standard_normal(VOX1_E) + 2.0 * lab).astype(np.float32)
    roc_pair(torch, eng, lib, "vox1_e", eng.to_device(sc), eng.to_device(lab), res)
    if not os.environ.get("SVK_ROCCH_SMALL"):
        g = torch.Generator(device=eng.device).manual_seed(1)
        test = torch.nn.functional.normalize(torch.randn(NT, D, device=eng.device, generator=g), dim=1)
        enroll = torch.nn.functional.normalize(torch.randn(NS, D, device=eng.device, generator=g), dim=1)
        scores = eng.cosine_scores(test, enroll)
        true = torch.randint(0, NS, (NT,), device=eng.device, generator=g)
        labels = torch.zeros((NT, NS), dtype=torch.uint8, device=eng.device)
        labels[torch.arange(NT, device=eng.device), true] = 1
        big, big_lab = scores.reshape(-1), labels.reshape(-1)
        roc_pair(torch, eng, lib, "dev_set", big, big_lab, res)
        for n_bins in (112, 3177):
            pav_pair(torch, eng, big, n_bins, res)
        w = np.array([7.0, -1.0])
        out = torch.empty_like(big)
        T.put("calibration_apply", T.alternated(torch, {"fn": lambda: eng.calibration_apply(big, w, out=out)}, REPS, 2)["fn"],
              8 * big.numel())
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
