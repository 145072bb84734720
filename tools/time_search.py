"""HIP-event medians of svk_cosine_topk (the k best gallery rows of every query, no score matrix) at three shapes:
  * 148 642 x 1 211 (the reference's evaluation set against its enrolled speakers) with k = 1 / 5 / 32,
  * 148 642 x 148 642 with k = 10 and exclude_self (the corpus searched against itself),
  * 1 x 1 000 000 with k = 10 (one query against a long gallery),
each next to today's route through the score matrix, ALTERNATED call by call in the same process: svk_cosine_scores followed
by torch.topk (svk_top1 for k = 1).  Where the matrix does not fit the card (--matrix-limit-gb) the route is reported as null.
Design bytes of the search: both matrices once, plus the lists written (n_query k 12 B); the rate is reported in TF/s of the
product's 2 n_query n_gallery dim flops as well.  Medians of --reps calls after --warmup; the spread (min .. max) beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="148642:1211:1,148642:1211:5,148642:1211:32,148642:148642:10:self,1:1000000:10",
                    help="n_query:n_gallery:k[:self] of each timing")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matrix-limit-gb", type=float, default=64.0, help="largest score matrix the existing route is timed with")
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, dim=args.dim, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, tf_s={}, ratio={},
                   missing=[])
    if not hasattr(lib, "svk_cosine_topk"):
        res["missing"].append("svk_cosine_topk")

    g = torch.Generator(device=eng.device).manual_seed(1)
    made = {}

    def rows(n):
        if n not in made:
            made[n] = torch.randn(n, args.dim, device=eng.device, generator=g)
        return made[n]

    for spec in args.shapes.split(","):
        parts = spec.split(":")
        nq, ng, k = int(parts[0]), int(parts[1]), int(parts[2])
        own = len(parts) > 3 and parts[3] == "self"
        query = rows(nq)
        gallery = query if own else rows(ng + 1)[:ng]             # (another matrix than a query of the same row count)
        exclude = torch.arange(nq, dtype=torch.int64, device=eng.device) if own else None
        tag = "%dx%d_k%d%s" % (nq, ng, k, "_self" if own else "")
        flops = 2.0 * nq * ng * args.dim
        fns = {}
        if "svk_cosine_topk" not in res["missing"]:
            fns["topk"] = lambda: eng.cosine_topk(query, gallery, k, exclude=exclude)
        fits = 4.0 * nq * ng <= args.matrix_limit_gb * 1e9
        if fits:
            true = torch.zeros(nq, dtype=torch.int32, device=eng.device)

            def matrix_route():
                scores = eng.cosine_scores(query, gallery)
                if own:
                    scores.fill_diagonal_(float("-inf"))
                return eng.top1(scores, true) if k == 1 else torch.topk(scores, k, dim=1)
            fns["matrix"] = matrix_route
        times = T.alternated(torch, fns, args.reps, args.warmup)
        ours = None
        if "topk" in times:
            ours = T.put("topk_" + tag, times["topk"], 4 * args.dim * (nq + (0 if own else ng)) + 12 * nq * k, flops)
        if "matrix" in times:
            ref = T.put("matrix_" + tag, times["matrix"], None, flops)
            if ours:
                res["ratio"]["matrix/topk_" + tag] = round(ref / ours, 3)
        else:
            res["ms"]["matrix_" + tag] = None                      # the matrix does not fit
        if not own:
            del gallery
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
