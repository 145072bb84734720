"""HIP-event medians of the diarization kernels (csrc/cluster.hip), ALTERNATED call by call with the route a framework offers:
  * svk_segment_affinity at 4 096 recordings x 80 windows x 128 and at 64 x 1 024 x 128, against torch.bmm on rows normalised by
    torch (f32; the library's product is float64).  Design bytes: the embeddings once and the affinities once;
  * svk_ahc at the same shapes (rows from 4 speaker centres + noise, merged down to 4 clusters: n - 4 steps per recording),
    against scipy's linkage(method="average") on the HOST for a sample of the recordings -- WALL time of that sample,
    extrapolated linearly to the batch and labelled so (scipy_extrapolated_ms); the D2H of the matrices is not counted;
  * one whole `diarize` of a batch of 60 s recordings (20 synthetic turns of 3 s each, the committed checkpoint): WALL time of the
    call, the D2H and the host timeline included.
Medians of --reps calls after --warmup; the spread (min .. max) beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json
import os
import time

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="4096:80,64:1024", help="n_rec:n_windows of each kernel timing")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-sample", type=int, default=8, help="recordings of each shape clustered by scipy on the host")
    ap.add_argument("--recordings", type=int, default=16, help="60 s recordings in the whole-diarize timing (0: skip it)")
    ap.add_argument("--diarize-reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, dim=args.dim, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={},
                   scipy_sample_ms={}, scipy_extrapolated_ms={}, missing=[])
    for name in ("svk_segment_affinity", "svk_ahc", "svk_window_crops"):
        if not hasattr(lib, name):
            res["missing"].append(name)
    if res["missing"]:
        print(json.dumps(res))
        return

    g = torch.Generator(device=eng.device).manual_seed(1)
    for spec in args.shapes.split(","):
        n_rec, n_win = (int(v) for v in spec.split(":"))
        tag = "%dx%d" % (n_rec, n_win)
        centres = torch.randn(n_rec, 4, args.dim, device=eng.device, generator=g)
        who = torch.randint(0, 4, (n_rec, n_win), device=eng.device, generator=g)
        emb = torch.gather(centres, 1, who[:, :, None].expand(-1, -1, args.dim)) + \
            0.7 * torch.randn(n_rec, n_win, args.dim, device=eng.device, generator=g)
        n_seg = torch.full((n_rec,), n_win, dtype=torch.int32, device=eng.device)
        aff = torch.zeros((n_rec, n_win, n_win), dtype=torch.float32, device=eng.device)

        def bmm_route():
            unit = emb / emb.norm(dim=2, keepdim=True).clamp_min(1e-30)
            return torch.bmm(unit, unit.transpose(1, 2))
        times = T.alternated(torch, {"svk": lambda: eng.segment_affinity(emb, n_seg, out=aff), "bmm": bmm_route}, args.reps, args.warmup)
        ours = T.put("affinity_" + tag, times["svk"], 4 * n_rec * n_win * (args.dim + n_win))
        ref = T.put("bmm_" + tag, times["bmm"], 4 * n_rec * n_win * (args.dim + n_win))
        res["ratio"]["bmm/affinity_" + tag] = round(ref / ours, 3)

        target = torch.full((n_rec,), 4, dtype=torch.int32, device=eng.device)
        times = T.alternated(torch, {"ahc": lambda: eng.ahc(aff, n_seg, target=target)}, args.reps, args.warmup)
        ours = T.put("ahc_" + tag, times["ahc"])
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
        sample = min(args.scipy_sample, n_rec)
        dist = 1.0 - aff[:sample].double().cpu().numpy()
        t0 = time.perf_counter()
        for r in range(sample):
            d = (dist[r] + dist[r].T) / 2
            np.fill_diagonal(d, 0.0)
            linkage(squareform(d, checks=False), method="average")
        wall = (time.perf_counter() - t0) * 1e3
        res["scipy_sample_ms"][tag] = {"recordings": sample, "wall_ms": round(wall, 3)}
        res["scipy_extrapolated_ms"][tag] = round(wall * n_rec / sample, 1)
        res["ratio"]["scipy_extrapolated/ahc_" + tag] = round(wall * n_rec / sample / ours, 2)
        del emb, aff, centres

    if args.recordings > 0:
        from speaker_verification_amd import synth
        from speaker_verification_amd.model import C3D2
        from speaker_verification_amd.pipeline import VerificationPipeline
        here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        ck = torch.load(os.path.join(here, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu",
                        weights_only=True)
        model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
        model.load_state_dict(ck["state_dict"])
        pipe = VerificationPipeline(model, use_vad=True)
        turns = 20
        clips, _ = synth.corpus_device(args.recordings * turns, eng.device, utts_per_speaker=5)
        pcm = clips.view(args.recordings, turns * clips.shape[1])
        walls = []
        for rep in range(args.diarize_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.diarize(pcm, num_speakers=4)
            walls.append((time.perf_counter() - t0) * 1e3)
        walls = sorted(walls[1:])            # the first call warms up
        res["diarize"] = {"recordings": args.recordings, "seconds_each": turns * clips.shape[1] / synth.SAMPLE_RATE,
                          "wall_ms": round(walls[len(walls) // 2], 2), "spread_ms": [round(walls[0], 2), round(walls[-1], 2)],
                          "turns_found": [len(t) for t in out][:4]}
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
