"""HIP-event medians of the score normalisation entries, each ALTERNATED call by call with the framework route it replaces on
the same device operands:
  * svk_cohort_moments ("moments_RxC_kK") against torch.topk(scores, K).values.double() -> mean and population std
    ("torch_moments_..."; K = 0: scores.double() as a whole) at 148 642 x 1 211 with top_k 0 and 300, at 148 642 x 4 096 with
    top_k 300 and at 64 x 100 000 (rows beyond the LDS: the re-read path).  Rows are a multiple of four floats apart (the
    16-byte loads); "moments_148642x1211_k300_dense" is the same matrix as svk_cosine_scores leaves it, rows 1 211 floats apart
    (the 4-byte loads: what `ScoreNorm.moments` meets).  Design bytes: the matrix once, 4 R C;
  * svk_score_norm, S-norm ("norm_148642x1211") against the float64 torch expression.  Design bytes: every score read and
    written, 8 R C;
  * svk_score_norm_pairs ("norm_pairs") at the 581 480 trials of VoxCeleb1-E over two tables of 148 642 rows, against the
    torch gathers and the same expression;
  * a whole `ScoreNorm` S-norm ("snorm_whole", host clock, ends in a synchronise): 148 642 test rows against 1 211 enrolled rows
    of dim 128 and a cohort of --cohort rows: the cohort scores of both sides in chunks, their moments, and the matrix
    normalised in place (the 148 642 x 1 211 raw scores are formed before the clock starts);
  * the EER and minDCF (p_target 0.01 and 0.05) of the synthetic-speaker corpus behind the shipped checkpoint (2 048 clips, 8 per
    speaker; the first three quarters of the speakers make the trials -- half of a speaker's clips enrol a mean model, the
    other half test -- the last quarter's clips are the cohort), raw and S-normed with --eer-top-k.  --skip-eer leaves it out.
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json
import os
import time

import _timing as T          # (puts the repository on sys.path)

SHAPES = [(148642, 1211, 0), (148642, 1211, 300), (148642, 4096, 300), (64, 100000, 300)]


def synthetic_eer(eng, top_k):
    import numpy as np
    import torch
    from speaker_verification_amd import synth
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline, enroll_mean
    from speaker_verification_amd.score_norm import ScoreNorm
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = torch.load(os.path.join(here, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu", weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    n, per = 2048, 8
    pcm, spk = synth.corpus_device(n, eng.device, utts_per_speaker=per)[:2]
    spk = np.asarray(spk.cpu() if hasattr(spk, "cpu") else spk)
    pipe = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98, crop_rng="device")
    emb = pipe.embed(pcm)
    uniq = np.unique(spk)
    trial_spk = uniq[:len(uniq) * 3 // 4]
    rank = np.zeros(n, dtype=np.int64)
    for s in uniq:
        rows = np.nonzero(spk == s)[0]
        rank[rows] = np.arange(len(rows))
    in_trials = np.isin(spk, trial_spk)
    pick = lambda mask: emb[torch.from_numpy(np.nonzero(mask)[0]).to(eng.device)]      # noqa: E731
    enrol, test, cohort = in_trials & (rank < per // 2), in_trials & (rank >= per // 2), ~in_trials
    ids, models = enroll_mean(pick(enrol), spk[enrol])
    labels = (spk[test][:, None] == ids[None, :]).astype(np.uint8).reshape(-1)
    ops = [(0.01, 1, 1), (0.05, 1, 1)]
    out = {"clips": n, "speakers": int(len(uniq)), "trial_speakers": int(len(trial_spk)), "cohort_rows": int(cohort.sum()),
           "trials": int(labels.size), "targets": int(labels.sum()), "top_k": top_k}
    sn = ScoreNorm(top_k=top_k, mode="s").fit(pick(cohort), engine=eng)
    for name, norm in (("raw", None), ("snorm", sn)):
        pipe.score_norm = norm
        res = eng.roc_dcf(pipe.score(pick(test), models).reshape(-1), labels, ops)
        out[name] = {"eer": res["eer"], "min_dcf_0.01": res["min_dcf"][0], "min_dcf_0.05": res["min_dcf"][1]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=581480)
    ap.add_argument("--cohort", type=int, default=1211)
    ap.add_argument("--whole-reps", type=int, default=5)
    ap.add_argument("--eer-top-k", type=int, default=100)
    ap.add_argument("--skip-eer", action="store_true")
    args = ap.parse_args()
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.score_norm import ScoreNorm
    eng = get_engine(0)
    dev = eng.device
    res = T.header(_lib, lib, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={})
    g = torch.Generator(device=dev).manual_seed(1)

    def matrix(rows, cols, stride):
        """Cosine-like scores, rows `stride` floats apart."""
        buf = torch.empty((rows, stride), dtype=torch.float32, device=dev)
        buf.normal_(0.0, 0.1, generator=g)
        return buf[:, :cols]

    def torch_moments(sc, k):
        v = (torch.topk(sc, k, dim=1).values if k else sc).double()
        return torch.stack([v.mean(1), v.std(1, unbiased=False)], dim=1)

    def race(tag, ours, theirs, nbytes):
        times = T.alternated(torch, {"ours": ours, "torch": theirs}, args.reps, args.warmup)
        a, b = T.put(tag, times["ours"], nbytes), T.put("torch_" + tag, times["torch"])
        res["ratio"]["torch_%s/%s" % (tag, tag)] = round(b / a, 3)

    sc = None
    for rows, cols, k in SHAPES:
        if sc is None or tuple(sc.shape) != (rows, cols):
            sc = None                                   # one large matrix at a time
            sc = matrix(rows, cols, (cols + 3) // 4 * 4)
        tag = "moments_%dx%d_k%d" % (rows, cols, k)
        race(tag, lambda: eng.cohort_moments(sc, k), lambda: torch_moments(sc, k), 4 * rows * cols)
        res["max_diff_from_torch_" + tag] = float((eng.cohort_moments(sc, k) - torch_moments(sc, k)).abs().max().item())
        if (rows, cols, k) == (148642, 1211, 300):
            dense = sc.contiguous()
            times = T.alternated(torch, {"ours": lambda: eng.cohort_moments(dense, k)}, args.reps, args.warmup)
            T.put(tag + "_dense", times["ours"], 4 * rows * cols)
            del dense

    rows, cols = 148642, 1211
    sc = None
    sc = matrix(rows, cols, (cols + 3) // 4 * 4)
    rm, cm = eng.cohort_moments(sc, 300), eng.cohort_moments(sc[:cols].t().contiguous(), 300)
    work = torch.empty((rows, sc.stride(0)), dtype=torch.float32, device=dev)[:, :cols]

    def torch_norm():
        s = sc.double()
        return (0.5 * ((s - rm[:, None, 0]) / rm[:, None, 1] + (s - cm[None, :, 0]) / cm[None, :, 1])).float()

    race("norm_%dx%d" % (rows, cols), lambda: eng.score_norm(sc, rm, cm, out=work), torch_norm, 8 * rows * cols)
    res["max_diff_from_torch_norm"] = float((eng.score_norm(sc, rm, cm, out=work) - torch_norm()).abs().max().item())

    n = args.pairs
    ia = torch.randint(0, rows, (n,), device=dev, generator=g)
    ib = torch.randint(0, rows, (n,), device=dev, generator=g)
    trial = torch.empty((n,), dtype=torch.float32, device=dev).normal_(0.0, 0.1, generator=g)
    mb = eng.cohort_moments(sc, 0)
    out = torch.empty_like(trial)
    race("norm_pairs", lambda: eng.score_norm_pairs(trial, rm, ia, mb, ib, out=out),
         lambda: (0.5 * ((trial.double() - rm[ia, 0]) / rm[ia, 1] + (trial.double() - mb[ib, 0]) / mb[ib, 1])).float(),
         n * (4 + 4 + 16 + 32))
    del work, ia, ib, trial, out

    # the whole S-norm of a rows x cols score matrix
    sc = None
    emb = lambda m: torch.empty((m, 128), dtype=torch.float32, device=dev).normal_(generator=g)     # noqa: E731
    test, enroll = emb(rows), emb(cols)
    sn = ScoreNorm(top_k=300, mode="s").fit(emb(args.cohort), engine=eng)
    whole = []
    for _ in range(args.whole_reps + 1):               # the first is the warm-up
        raw = eng.cosine_scores(test, enroll)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sn.normalize(raw, *sn.side_moments(test, enroll), out=raw)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    T.put("snorm_whole", sorted(whole[1:]))
    res["snorm_whole"] = {"test_rows": rows, "enrolled_rows": cols, "cohort_rows": args.cohort, "top_k": 300}
    del test, enroll, raw

    if not args.skip_eer:
        res["synthetic_corpus"] = synthetic_eer(eng, args.eer_top_k)
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
