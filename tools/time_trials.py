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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (6.3 TB/s is the measured copy rate)


def one(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(torch, fns, reps, warmup):
    """{name: sorted times in ms}: the functions take turns, call by call, so that clocks and cache state drift for all alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(one(torch, fn))
    return {name: sorted(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lists", default="581480:145160,37720:4874", help="trials:rows of each trial list")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=148642 * 1211, help="scores of the ROC / decision-count timings")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if os.environ.get("SVK_TOOL_LIB"):      # A/B: time another build of the library in the same process layout
        from speaker_verification_amd import _lib
        _lib.LIB_PATH = os.environ["SVK_TOOL_LIB"]
        lib = _lib.C.CDLL(_lib.LIB_PATH)
        _lib.VERSION = lib.svk_version()
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(lib, k)}
    from speaker_verification_amd import _lib
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    lib = _lib.load()
    res = {"lib": _lib.LIB_PATH, "version": int(lib.svk_version()), "csrc_sha": _lib.provenance()["csrc_sha"],
           "reps": args.reps, "ms": {}, "spread_ms": {}, "bytes": {}, "tb_s": {}, "ratio": {}, "missing": []}

    def put(name, times, nbytes=None):
        med = times[len(times) // 2]
        res["ms"][name] = round(med, 4)
        res["spread_ms"][name] = [round(times[0], 4), round(times[-1], 4)]
        if nbytes:
            res["bytes"][name] = int(nbytes)
            res["tb_s"][name] = round(nbytes / (med * 1e-3) / 1e12, 3)
        return med

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
            times = alternated(torch, fns, args.reps, args.warmup)
            tag = "%dx%d" % (n_pairs, rows)
            ours = put("pair_cosine_" + tag, times["pair_cosine"], design)
            put("pair_l2_" + tag, times["pair_l2"], design)
            ref = put("torch_cosine_" + tag, times["torch_cosine"])
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
    times = alternated(torch, fns, max(3, args.reps // 2), min(args.warmup, 2))
    base = put("roc_eer", times["roc_eer"])
    for name in ("roc_dcf_0", "roc_dcf_2"):
        if name in times:
            res["ratio"][name + "/roc_eer"] = round(put(name, times[name]) / base, 4)
    if hasattr(lib, "svk_roc_dcf"):
        res["roc_points"] = eng.roc_dcf(sc, lb, ())["points"]
    if hasattr(lib, "svk_decision_counts"):
        thr16 = [float(v) for v in torch.linspace(-0.2, 0.5, 16)]
        times = alternated(torch, {"decision_counts_1": lambda: eng.decision_counts(sc, lb, thr16[8:9]),
                                   "decision_counts_16": lambda: eng.decision_counts(sc, lb, thr16)}, args.reps, args.warmup)
        for name, t in times.items():
            put(name, t, n * 5)
    else:
        res["missing"].append("svk_decision_counts")
    res["hbm_peak_tb_s"] = HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
