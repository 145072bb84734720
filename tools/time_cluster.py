"""HIP-event medians of svk_knn_cluster (include/svk.h "shared-neighbour (Jarvis-Patrick) clustering of k-NN lists": k-NN lists -> shared-neighbour components -> labels) on a
synthetic corpus of the development set's size: --rows 148 642 embeddings of --speakers 1 211 (a random unit centre per
speaker + --noise N(0, I), rows in shuffled order), k = 10 and k = 32, mutual arcs at --threshold with --min-shared common
neighbours.  Per k, ALTERNATED call by call in the same process:
  * cluster   svk_knn_cluster on the lists of the self-search (all seven launches),
  * search    the svk_cosine_topk self-search that feeds it, for scale.
Beside them the HOST yardstick, WALL time (time.perf_counter, one call after one warm-up, labelled host_wall_ms): copy the two
lists to the host and run scipy.sparse.csgraph.connected_components on the mutual graph.  scipy has no shared-neighbour
test, so the yardstick is timed against the device entry with min_shared = 0 (cluster0) -- the same rule, checked to give the
same partition.  ratio host/cluster0 above 1 means the device route is the faster one.

bytes: the design traffic -- 12 n k for the lists, 8 k per gathered neighbour row (a forward arc in mutual mode), 32 per row
for the mask, the parents, the sizes and the three outputs -- and the TB/s that amounts to.  pair_f: pairwise precision /
recall / F of the labels against the speakers (clustering.pair_precision_recall_f), with gave_up and n_bad (both 0).

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout, and in --out when given."""
import argparse
import json
import time

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=148642)
    ap.add_argument("--speakers", type=int, default=1211)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--min-shared", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd import clustering
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    n = args.rows
    res = T.header(_lib, lib, rows=n, speakers=args.speakers, dim=args.dim, noise=args.noise, threshold=args.threshold,
                   min_shared=args.min_shared, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, host_wall_ms={}, ratio={},
                   clusters={}, counts={}, pair_f={}, missing=[])
    if not hasattr(lib, "svk_knn_cluster"):
        res["missing"].append("svk_knn_cluster")
        print(json.dumps(res))
        return

    g = torch.Generator(device=eng.device).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(args.speakers, args.dim, device=eng.device, generator=g), dim=1)
    speaker = (torch.randperm(n, device=eng.device, generator=g) % args.speakers)
    emb = (centres[speaker] + args.noise * torch.randn(n, args.dim, device=eng.device, generator=g)).contiguous()
    truth = speaker.cpu().numpy()
    own = torch.arange(n, dtype=torch.int64, device=eng.device)

    for k in (int(v) for v in args.ks.split(",")):
        scores, indices = eng.cosine_topk(emb, emb, k, exclude=own)
        rule = dict(threshold=args.threshold, mutual=True)
        fns = {"cluster": lambda: eng.knn_cluster(scores, indices, min_shared=args.min_shared, **rule),
               "cluster0": lambda: eng.knn_cluster(scores, indices, min_shared=0, **rule),
               "search": lambda: eng.cosine_topk(emb, emb, k, exclude=own)}
        times = T.alternated(torch, fns, args.reps, args.warmup)
        gathered = int(((indices >= 0) & (scores >= args.threshold)).sum())
        nbytes = 12 * n * k + 8 * k * gathered + 32 * n
        tag = "%d_k%d" % (n, k)
        ours = T.put("cluster_" + tag, times["cluster"], nbytes)
        plain = T.put("cluster0_" + tag, times["cluster0"], nbytes)
        search = T.put("search_" + tag, times["search"])
        res["ratio"]["search/cluster_" + tag] = round(search / ours, 2)

        got = clustering.Clustering(*fns["cluster"]())
        res["clusters"][tag] = int(got.counts[0])
        res["counts"][tag] = got.counts.tolist()
        res["pair_f"][tag] = [round(v, 4) for v in clustering.pair_precision_recall_f(got.labels, truth)]

        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import connected_components

        def host_route():
            sc, ix = scores.cpu().numpy(), indices.cpu().numpy()
            keep = (ix >= 0) & (sc >= np.float32(args.threshold))
            rows = np.broadcast_to(np.arange(n)[:, None], ix.shape)[keep]
            arcs = csr_matrix((np.ones(rows.size, dtype=np.int8), (rows, ix[keep])), shape=(n, n))
            return connected_components(arcs.multiply(arcs.T), directed=False)
        host_route()
        t0 = time.perf_counter()
        count, comp = host_route()
        wall = (time.perf_counter() - t0) * 1e3
        res["host_wall_ms"]["lists_to_host_scipy_" + tag] = round(wall, 2)
        res["ratio"]["host_wall/cluster0_" + tag] = round(wall / plain, 2)      # below 1: the device route is SLOWER
        # the same partition: scipy's component of a row <-> the device's root
        root0 = fns["cluster0"]()[1].cpu().numpy()
        first = np.full(count, n, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(n))
        res["counts"]["host_agrees_" + tag] = bool(np.array_equal(first[comp], root0))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
