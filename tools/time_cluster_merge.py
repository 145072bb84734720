"""WALL time of the second stage of corpus clustering (`clustering.merge_clusters`) on the corpus of
tools/time_cluster.py: --rows 148 642 embeddings of --speakers 1 211 (a random unit centre per speaker + --noise N(0, I), rows
in shuffled order), dim 128.  Per first-stage k (--ks 10,32; mutual arcs at --threshold with --min-shared common neighbours,
min_size 1) the fragments `svk_knn_cluster` leaves are merged on their centroids: k-NN rounds with --merge-k neighbours
(mutual, --merge-min-shared) while there are more than --ahc-max clusters (default: all svk_ahc takes), then average linkage.

Everything here is WALL time (time.perf_counter between stream synchronisations), because the second stage's integer
bookkeeping runs on the host between its launches and a HIP-event pair would leave it out:
  * second_stage   one `merge_clusters` call, labels in, labels out; median and spread of --reps calls,
  * search         the `svk_cosine_topk` self-search over the ROWS that feeds the first stage, for scale; ALTERNATED with
                   second_stage call by call in the same process,
  * rounds         per round of ONE further call: kind, clusters in and out, and the wall time from the round's first launch
                   (its centroids) to the next round's, the host work between them included; `before_ms` is the time ahead of
                   the first round (the labels to the host, the density check), and the last round's time takes in the
                   assembly of the result.
pair_f: pairwise precision / recall / F against the speakers before and after (clustering.pair_precision_recall_f).

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout, and in --out when given."""
import argparse
import json
import time

import _timing as T          # (puts the repository on sys.path)


class Stamped:
    """The engine with a wall-clock stamp, after a synchronise, ahead of every centroid launch: a round begins with one."""

    def __init__(self, eng, torch):
        self._eng, self._torch, self.stamps = eng, torch, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def embedding_pool(self, *args, **kw):
        self._torch.cuda.synchronize()
        self.stamps.append(time.perf_counter())
        return self._eng.embedding_pool(*args, **kw)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=148642)
    ap.add_argument("--speakers", type=int, default=1211)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--noise", type=float, default=0.05)
    ap.add_argument("--ks", default="10,32")
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--min-shared", type=int, default=3)
    ap.add_argument("--merge-k", type=int, default=10)
    ap.add_argument("--merge-min-shared", type=int, default=0)
    ap.add_argument("--ahc-max", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd import clustering
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    n = args.rows
    res = T.header(_lib, lib, rows=n, speakers=args.speakers, dim=args.dim, noise=args.noise, threshold=args.threshold,
                   min_shared=args.min_shared, merge_k=args.merge_k, merge_min_shared=args.merge_min_shared,
                   ahc_max=eng.ahc_limits()[1] if args.ahc_max is None else args.ahc_max, reps=args.reps, timer="wall",
                   wall_ms={}, spread_ms={}, ratio={}, rounds={}, before_ms={}, clusters={}, counts={}, pair_f={})

    g = torch.Generator(device=eng.device).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(args.speakers, args.dim, device=eng.device, generator=g), dim=1)
    speaker = (torch.randperm(n, device=eng.device, generator=g) % args.speakers)
    emb = (centres[speaker] + args.noise * torch.randn(n, args.dim, device=eng.device, generator=g)).contiguous()
    truth = speaker.cpu().numpy()
    own = torch.arange(n, dtype=torch.int64, device=eng.device)
    rule = dict(threshold=args.threshold, k=args.merge_k, mutual=True, min_shared=args.merge_min_shared, ahc_max=args.ahc_max)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for k in (int(v) for v in args.ks.split(",")):
        tag = "%d_k%d" % (n, k)
        scores, indices = eng.cosine_topk(emb, emb, k, exclude=own)
        first = clustering.Clustering(*eng.knn_cluster(scores, indices, threshold=args.threshold, min_shared=args.min_shared,
                                                       mutual=True, min_size=1))
        fns = {"search": lambda: eng.cosine_topk(emb, emb, k, exclude=own),
               "second_stage": lambda: clustering.merge_clusters(eng, emb, first, **rule)}
        times, last = {name: [] for name in fns}, {}
        for rep in range(args.warmup + args.reps):
            for name, fn in fns.items():
                ms, last[name] = wall(fn)
                if rep >= args.warmup:
                    times[name].append(ms)
        for name, v in times.items():
            v.sort()
            res["wall_ms"][name + "_" + tag] = round(v[len(v) // 2], 3)
            res["spread_ms"][name + "_" + tag] = [round(v[0], 3), round(v[-1], 3)]
        res["ratio"]["second_stage/search_" + tag] = round(res["wall_ms"]["second_stage_" + tag] / res["wall_ms"]["search_" + tag], 3)

        stamped = Stamped(eng, torch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = clustering.merge_clusters(stamped, emb, first, **rule)
        torch.cuda.synchronize()
        ends = stamped.stamps[1:] + [time.perf_counter()]
        res["before_ms"][tag] = round((stamped.stamps[0] - t0) * 1e3, 3) if stamped.stamps else None
        res["rounds"][tag] = [dict(kind=r["kind"], clusters_in=r["clusters_in"], clusters_out=r["clusters_out"],
                                   wall_ms=round((b - a) * 1e3, 3)) for r, a, b in zip(got.rounds, stamped.stamps, ends)]
        res["clusters"][tag] = [int(first.counts[0]), int(got.counts[0])]
        res["counts"][tag] = got.counts.tolist()
        res["pair_f"]["first_stage_" + tag] = [round(v, 4) for v in clustering.pair_precision_recall_f(first.labels, truth)]
        res["pair_f"]["second_stage_" + tag] = [round(v, 4) for v in clustering.pair_precision_recall_f(got.labels, truth)]
        assert torch.equal(got.labels, last["second_stage"].labels)        # the timed calls gave these labels
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
