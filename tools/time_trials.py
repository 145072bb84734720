"""HIP-event medians of the trial-list entries:
  * svk_pair_scores at the sizes of the public VoxCeleb1 lists (--lists "trials:rows,...": by default 581 480 trials over
    145 160 utterances, VoxCeleb1-E, and 37 720 over 4 874, VoxCeleb1-O; both metrics), with its design bytes
    n_pairs (2 dim 4 + 20) and the resulting TB/s, next to torch's F.cosine_similarity(a[ia], b[ib]) on the same indices;
  * svk_roc_dcf with 0 and 2 operating points against svk_roc_eer on the same --pairs (1.8e8) scores, ALTERNATED call by
    call in one process (its extra cost is one pass over the distinct-score points and a one-workgroup reduction);
  * svk_decision_counts with 1 and 16 thresholds on those scores against its design bytes (5 B per pair).
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build; entries that build lacks are reported as missing.
One JSON line on stdout."""
import argparse
import json

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lists", default="581480:145160,37720:4874", help="trials:rows of each trial list")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=148642 * 1211, help="scores of the ROC / decision-count timings")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={}, missing=[])

    g = torch.Generator(device=eng.device).manual_seed(1)
    if hasattr(lib, "svk_pair_scores"):
        for spec in args.lists.split(","):
            n_pairs, rows = (int(v) for v in spec.split(":"))
            emb = torch.randn(rows, args.dim, device=eng.device, generator=g)
            ia = torch.randint(0, rows, (n_pairs,), device=eng.device, generator=g)
            ib = torch.randint(0, rows, (n_pairs,), device=eng.device, generator=g)
            design = n_pairs * (2 * args.dim * 4 + 20)
            fns = {"pair_cosine": lambda: eng.pair_scores(emb, emb, ia, ib),
                   "pair_l2": lambda: eng.pair_scores(emb, emb, ia, ib, metric="l2"),
                   "torch_cosine": lambda: torch.nn.functional.cosine_similarity(emb[ia], emb[ib])}
            times = T.alternated(torch, fns, args.reps, args.warmup)
            tag = "%dx%d" % (n_pairs, rows)
            ours = T.put("pair_cosine_" + tag, times["pair_cosine"], design)
            T.put("pair_l2_" + tag, times["pair_l2"], design)
            ref = T.put("torch_cosine_" + tag, times["torch_cosine"])
            res["ratio"]["torch_cosine/pair_cosine_" + tag] = round(ref / ours, 3)
            del emb, ia, ib
    else:
        res["missing"].append("svk_pair_scores")

    # dev-set scale scores: unit-variance noise plus a shift for the targets (about one ROC point per pair, like cosine scores)
    n = args.pairs
    lb = torch.rand(n, device=eng.device, generator=g) < 1.0 / 1211
    sc = torch.randn(n, device=eng.device, generator=g) * 0.1 + lb * 0.3
    lb = lb.to(torch.uint8)
    res["n_pairs"] = n
    fns = {"roc_eer": lambda: eng.roc_eer(sc, lb)}
    if hasattr(lib, "svk_roc_dcf"):
        fns["roc_dcf_0"] = lambda: eng.roc_dcf(sc, lb, ())
        fns["roc_dcf_2"] = lambda: eng.roc_dcf(sc, lb, ((0.01, 1, 1), (0.05, 1, 1)))
    else:
        res["missing"].append("svk_roc_dcf")
    times = T.alternated(torch, fns, max(3, args.reps // 2), min(args.warmup, 2))
    base = T.put("roc_eer", times["roc_eer"])
    for name in ("roc_dcf_0", "roc_dcf_2"):
        if name in times:
            res["ratio"][name + "/roc_eer"] = round(T.put(name, times[name]) / base, 4)
    if hasattr(lib, "svk_roc_dcf"):
        res["roc_points"] = eng.roc_dcf(sc, lb, ())["points"]
    if hasattr(lib, "svk_decision_counts"):
        thr16 = [float(v) for v in torch.linspace(-0.2, 0.5, 16)]
        times = T.alternated(torch, {"decision_counts_1": lambda: eng.decision_counts(sc, lb, thr16[8:9]),
                                     "decision_counts_16": lambda: eng.decision_counts(sc, lb, thr16)}, args.reps, args.warmup)
        for name, t in times.items():
            T.put(name, t, n * 5)
    else:
        res["missing"].append("svk_decision_counts")
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
