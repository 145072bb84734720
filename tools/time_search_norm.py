"""HIP-event medians of svk_cosine_topk_norm (the k best gallery rows of every query by NORMALISED score, no score matrix):
  * 148 642 x 1 211 (the reference's evaluation set against its enrolled speakers) with k = 1 / 5 / 32, S-norm (both tables)
    and Z-norm (the gallery table alone),
  * 148 642 x 148 642 with k = 10 and exclude_self, S-norm,
each ALTERNATED call by call in the same process with
  * plain svk_cosine_topk on the same operands -- the difference is the cost of the float64 epilogue --, and
  * the route through the matrix: svk_cosine_scores, svk_score_norm in place, torch.topk; null where the matrix does not fit the
    card (--matrix-limit-gb).
The moment tables are random (means N(0, 0.1), deviations in 0.05 .. 0.15): the time of the selection depends on how often a
score passes a row's threshold, which random tables exercise like real ones do.  Medians of --reps calls after --warmup, the
spread (min .. max) beside them; ratios above 1 mean the search on normalised scores is the faster of the two.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="148642:1211:1:s,148642:1211:5:s,148642:1211:32:s,148642:1211:1:z,148642:1211:5:z,"
                    "148642:1211:32:z,148642:148642:10:s:self", help="n_query:n_gallery:k:mode[:self] of each timing")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--matrix-limit-gb", type=float, default=64.0, help="largest score matrix the matrix route is timed with")
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, dim=args.dim, reps=args.reps, ms={}, spread_ms={}, tf_s={}, ratio={}, missing=[])
    if not hasattr(lib, "svk_cosine_topk_norm"):
        res["missing"].append("svk_cosine_topk_norm")

    g = torch.Generator(device=eng.device).manual_seed(1)
    made, tables = {}, {}

    def rows(n):
        if n not in made:
            made[n] = torch.randn(n, args.dim, device=eng.device, generator=g)
        return made[n]

    def moments(n):
        if n not in tables:
            mu = 0.1 * torch.randn(n, device=eng.device, generator=g, dtype=torch.float64)
            sd = 0.05 + 0.1 * torch.rand(n, device=eng.device, generator=g, dtype=torch.float64)
            tables[n] = torch.stack([mu, sd], dim=1).contiguous()
        return tables[n]

    for spec in args.shapes.split(","):
        parts = spec.split(":")
        nq, ng, k, mode = int(parts[0]), int(parts[1]), int(parts[2]), parts[3]
        own = len(parts) > 4 and parts[4] == "self"
        query = rows(nq)
        gallery = query if own else rows(ng + 1)[:ng]             # (another matrix than a query of the same row count)
        exclude = torch.arange(nq, dtype=torch.int64, device=eng.device) if own else None
        qm = moments(nq) if mode in "ts" else None
        gm = moments(ng + 1)[:ng] if mode in "zs" else None
        tag = "%dx%d_k%d_%s%s" % (nq, ng, k, mode, "_self" if own else "")
        flops = 2.0 * nq * ng * args.dim
        fns = {"plain": lambda: eng.cosine_topk(query, gallery, k, exclude=exclude)}
        if not res["missing"]:
            fns["norm"] = lambda: eng.cosine_topk_norm(query, gallery, k, query_moments=qm, gallery_moments=gm, exclude=exclude)
        if 4.0 * nq * ng <= args.matrix_limit_gb * 1e9:
            def matrix_route():
                scores = eng.cosine_scores(query, gallery)
                eng.score_norm(scores, qm, gm, out=scores)
                if own:
                    scores.fill_diagonal_(float("-inf"))
                return torch.topk(scores, k, dim=1)
            fns["matrix"] = matrix_route
        times = T.alternated(torch, fns, args.reps, args.warmup)
        plain = T.put("plain_" + tag, times["plain"], None, flops)
        ours = T.put("norm_" + tag, times["norm"], None, flops) if "norm" in times else None
        if ours:
            res["ratio"]["norm/plain_" + tag] = round(ours / plain, 3)          # the epilogue's cost: above 1
        if "matrix" in times:
            ref = T.put("matrix_" + tag, times["matrix"], None, flops)
            if ours:
                res["ratio"]["matrix/norm_" + tag] = round(ref / ours, 3)     # below 1: the search is SLOWER than the matrix route
        else:
            res["ms"]["matrix_" + tag] = None                      # the matrix does not fit
        if not own:
            del gallery
    print(json.dumps(res))


if __name__ == "__main__":
    main()
