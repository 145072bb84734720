"""HIP-event medians of svk_spectral_embed (csrc/spectral.hip), ALTERNATED call by call with the route a framework offers:
  * 4 096 recordings x 80 windows (rows from 4 speaker centres + noise) with ONE neighbour candidate and with the sweep
    (2, 32, 2) of 16 candidates;
  * 64 recordings x 1 024 windows grouped to 128 nodes by svk_ahc, whose pass is timed on its own (group_*), then the sweep on
    the nodes.
The yardstick is torch.linalg.eigvalsh on the SAME float64 Laplacians, all candidates of the sweep in one batched call.  It
times the decompositions ALONE -- no node means, no graphs, no eigenvectors, no decisions -- which favours torch; the result
line says so (yardstick_note).  The sweep timings take --sweep-reps calls (the yardstick is slow), the others --reps.
  * one whole diarize(method="spectral") of a batch of 60 s recordings beside method="ahc" with the count given: WALL time of
    the call, the D2H and the host timeline included.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json
import os
import time

import _timing as T          # (puts the repository on sys.path)

SWEEP = (2, 32, 2)


def laplacians(torch, eng, aff, n_seg, group, candidates):
    """float64 [n_rec * len(candidates), m, m]: L of every candidate's graph, from the entry's own d_graph."""
    out = []
    for p in candidates:
        g2 = eng.spectral_embed(aff, n_seg, group=group, neighbours=int(p), want_graph=True)[4].double() / 2
        out.append(torch.diag_embed(g2.sum(2)) - g2)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--recordings", type=int, default=16, help="60 s recordings in the whole-diarize timing (0: skip it)")
    ap.add_argument("--diarize-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    res = T.header(_lib, lib, dim=args.dim, reps=args.reps, sweep_reps=args.sweep_reps, ms={}, spread_ms={}, ratio={}, found={},
                   missing=[], yardstick_note="eigvalsh_* times the eigenvalue decompositions alone on Laplacians built beforehand: "
                   "no node means, graphs, eigenvectors or decisions -- the comparison favours torch")
    if not hasattr(lib, "svk_spectral_embed"):
        res["missing"].append("svk_spectral_embed")
        print(json.dumps(res))
        return
    g = torch.Generator(device=eng.device).manual_seed(1)
    candidates = list(range(SWEEP[0], SWEEP[1] + 1, SWEEP[2]))

    def rows(n_rec, n_win):
        centres = torch.randn(n_rec, 4, args.dim, device=eng.device, generator=g)
        who = torch.randint(0, 4, (n_rec, n_win), device=eng.device, generator=g)
        emb = torch.gather(centres, 1, who[:, :, None].expand(-1, -1, args.dim)) + \
            0.7 * torch.randn(n_rec, n_win, args.dim, device=eng.device, generator=g)
        n_seg = torch.full((n_rec,), n_win, dtype=torch.int32, device=eng.device)
        return eng.segment_affinity(emb, n_seg), n_seg

    def compare(tag, ours, L, reps):
        times = T.alternated(torch, {"svk": ours, "eigvalsh": lambda: torch.linalg.eigvalsh(L)}, reps, args.warmup)
        a, b = T.put("spectral_" + tag, times["svk"]), T.put("eigvalsh_" + tag, times["eigvalsh"])
        res["ratio"]["eigvalsh/spectral_" + tag] = round(b / a, 3)

    # 4 096 x 80: every window a node
    aff, n_seg = rows(4096, 80)
    out = eng.spectral_embed(aff, n_seg, neighbours=SWEEP)
    res["found"]["4096x80"] = {"speakers": torch.bincount(out[2].clamp(min=0)).tolist(), "neighbours": torch.bincount(out[3].clamp(min=0)).tolist()}
    compare("4096x80_p10", lambda: eng.spectral_embed(aff, n_seg, neighbours=10), laplacians(torch, eng, aff, n_seg, None, [10]), args.reps)
    compare("4096x80_sweep16", lambda: eng.spectral_embed(aff, n_seg, neighbours=SWEEP),
            laplacians(torch, eng, aff, n_seg, None, candidates), args.sweep_reps)
    del aff

    # 64 x 1 024 -> 128 nodes
    aff, n_seg = rows(64, 1024)
    limit = eng.spectral_limits()[0]
    T.put("group_64x1024", T.alternated(torch, {"ahc": lambda: eng.ahc(aff, n_seg, max_clusters=limit)}, args.reps, args.warmup)["ahc"])
    group = eng.ahc(aff, n_seg, max_clusters=limit)[0]
    out = eng.spectral_embed(aff, n_seg, group=group, neighbours=SWEEP)
    res["found"]["64x1024"] = {"speakers": torch.bincount(out[2].clamp(min=0)).tolist(), "neighbours": torch.bincount(out[3].clamp(min=0)).tolist()}
    compare("64x1024_grouped_sweep16", lambda: eng.spectral_embed(aff, n_seg, group=group, neighbours=SWEEP),
            laplacians(torch, eng, aff, n_seg, group, candidates), args.sweep_reps)
    del aff

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
        routes = {"spectral": dict(method="spectral"), "ahc": dict(num_speakers=4)}
        walls = {name: [] for name in routes}
        for rep in range(args.diarize_reps + 1):
            for name, kw in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pipe.diarize(pcm, **kw)
                walls[name].append((time.perf_counter() - t0) * 1e3)
                if name == "spectral":
                    speakers = [len({t.speaker for t in ts}) for ts in out]
        res["diarize"] = {"recordings": args.recordings, "seconds_each": turns * clips.shape[1] / synth.SAMPLE_RATE,
                          "speakers_found_spectral": speakers[:8]}
        for name, w in walls.items():
            w = sorted(w[1:])            # the first call warms up
            res["diarize"]["wall_ms_" + name] = round(w[len(w) // 2], 2)
            res["diarize"]["spread_ms_" + name] = [round(w[0], 2), round(w[-1], 2)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
