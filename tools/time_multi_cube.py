#!/usr/bin/env python3
"""K cubes per clip and pooled embeddings in numbers (HIP-event medians of --reps runs after a warm-up):
  * first-block: svk_c3d2_stage1 on N cubes; svk_c3d2_stage1_multi at K = 1 (N clips) and K = 4 (N / 4 clips), the K = 4 run
    beside the old entry fed with each clip's rows repeated four times (the new entry reads a quarter of the distinct bytes);
  * pool: svk_embedding_pool at 148 642 x 4 rows (uniform) and at 1 211 speakers over 148 642 rows (CSR + row index): time,
    design bytes (rows read once + means written once) and TB/s;
  * embed: VerificationPipeline.embed in clips/s at K = 1, 2, 4;
  * eer: the bench's synthetic-speaker corpus with the shipped checkpoint, EER at K = 1, 2, 4 with last-utterance and mean
    enrolment (half of every speaker's clips enrol, the other half test).
--old-entries: only the two old first-block entries, ten cold-started series each -- the form that also runs on a library
without the new symbols (SVK_TOOL_LIB=<the parent commit's libsvk.so>), for the parent-against-this-build comparison.
      python tools/time_multi_cube.py [n_cubes] [--reps R] [--old-entries] [--skip-eer]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speaker_verification_amd import _lib                                    # noqa: E402
if os.environ.get("SVK_TOOL_LIB"):
    _lib.LIB_PATH = os.environ["SVK_TOOL_LIB"]
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib.SIGNATURES if not hasattr(have, k)]:       # an older library: bind what it has
        del _lib.SIGNATURES[name]
from speaker_verification_amd.engine import get_engine                       # noqa: E402
from speaker_verification_amd.model import C3D2, perturb_inference_state, seeded_model   # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def first_block(eng, models, n, reps, old_only):
    g = torch.Generator(device=eng.device).manual_seed(0)
    T, r = 297, {"n_cubes": n}
    for ch in (1, 3):
        tables = models[ch].fused_inference().stage1_tables()
        feat = torch.randn((n, T, 40) if ch == 1 else (n, 3, T, 40), device=eng.device, generator=g) * 2 - 6
        crops = torch.randint(0, T - 80, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
        tag = "stage1_%dch" % ch
        r[tag + "_old_ms"] = timed(lambda: eng.c3d2_stage1(feat, crops, tables), reps)
        if old_only:
            r[tag + "_old_ms_again"] = timed(lambda: eng.c3d2_stage1(feat, crops, tables), reps)
            continue
        r[tag + "_multi_k1_ms"] = timed(lambda: eng.c3d2_stage1(feat, crops[:, None, :].contiguous(), tables), reps)
        m = n // 4
        table4 = crops[:4 * m].view(m, 4, 20)
        rep4 = feat[:m].repeat_interleave(4, 0)
        r[tag + "_multi_k4_ms"] = timed(lambda: eng.c3d2_stage1(feat[:m], table4, tables), reps)
        r[tag + "_old_repeated_rows_k4_ms"] = timed(lambda: eng.c3d2_stage1(rep4, table4.reshape(4 * m, 20), tables), reps)
        r[tag + "_k4_feature_bytes"] = [int(feat[:m].numel() * 4), int(rep4.numel() * 4)]
    return r


def pool(eng, reps):
    g = torch.Generator(device=eng.device).manual_seed(1)
    n, r = 148642, {}
    emb4 = torch.randn((4 * n, 128), device=eng.device, generator=g) + 3
    ms = timed(lambda: eng.embedding_pool(emb4, rows_per_seg=4), reps)
    by = (4 * n + n) * 128 * 4
    r["uniform_148642x4"] = {"ms": ms, "design_bytes": by, "TBps": by / ms / 1e9}
    ms = timed(lambda: eng.embedding_pool(emb4, rows_per_seg=4, l2_rows=True), reps)
    r["uniform_148642x4_l2_rows"] = {"ms": ms, "design_bytes": by, "TBps": by / ms / 1e9}
    from speaker_verification_amd.pipeline import speaker_segments
    ids = np.random.default_rng(2).integers(0, 1211, size=n)
    uniq, start, index = speaker_segments(ids)
    emb, start_d, index_d = emb4[:n], eng.to_device(start), eng.to_device(index)
    ms = timed(lambda: eng.embedding_pool(emb, seg_start=start_d, row_index=index_d, l2_rows=True), reps)
    by = n * (128 * 4 + 8) + len(uniq) * (128 * 4 + 8)
    r["speakers_1211_over_148642"] = {"ms": ms, "design_bytes": by, "TBps": by / ms / 1e9, "speakers": int(len(uniq))}
    return r


def shipped_model(eng):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = torch.load(os.path.join(here, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu", weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    return model.to(eng.device).eval()


def embed_and_eer(eng, n, reps, skip_eer):
    from speaker_verification_amd import synth
    from speaker_verification_amd.evaluation import get_eer_auc_device
    from speaker_verification_amd.pipeline import VerificationPipeline, enroll_last_utterance, enroll_mean
    model = shipped_model(eng)
    per = 8
    n = n // per * per
    pcm, spk = synth.corpus_device(n, eng.device, utts_per_speaker=per)[:2]
    spk = np.asarray(spk.cpu() if hasattr(spk, "cpu") else spk)
    r = {"clips": n, "utts_per_speaker": per}
    for K in (1, 2, 4):
        # the front end the shipped checkpoint was trained behind (tools/train_synth_checkpoint.py, bench.py)
        pipe = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98, crop_rng="device", cubes_per_clip=K)
        ms = timed(lambda: pipe.embed(pcm), reps, warm=1)
        r["embed_k%d_clips_per_s" % K] = n / ms * 1e3
        if skip_eer:
            continue
        emb = pipe.embed(pcm)
        # every speaker's first half of clips enrols, the second half tests
        rank = np.zeros(n, dtype=np.int64)
        for s in np.unique(spk):
            rows = np.nonzero(spk == s)[0]
            rank[rows] = np.arange(len(rows))
        enrol, test = np.nonzero(rank < per // 2)[0], np.nonzero(rank >= per // 2)[0]
        e_emb, t_emb = emb[torch.from_numpy(enrol).to(eng.device)], emb[torch.from_numpy(test).to(eng.device)]
        uniq, last = enroll_last_utterance(e_emb, spk[enrol])
        models = {"last": e_emb[torch.from_numpy(last).to(eng.device)], "mean": enroll_mean(e_emb, spk[enrol])[1]}
        labels = torch.from_numpy((spk[test][:, None] == uniq[None, :]).astype(np.uint8)).to(eng.device)
        for how, m in models.items():
            eer, auc = get_eer_auc_device(labels, eng.cosine_scores(t_emb, m))
            r["eer_k%d_%s" % (K, how)] = eer
            r["auc_k%d_%s" % (K, how)] = auc
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=4018)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--old-entries", action="store_true")
    ap.add_argument("--skip-eer", action="store_true")
    a = ap.parse_args()
    eng = get_engine(0)
    models = {}
    for ch in (1, 3):
        m = seeded_model(1, 8, ch)
        m.load_state_dict(perturb_inference_state(m.state_dict(), 2))
        models[ch] = m.to(eng.device).eval()
    out = {"lib": os.path.basename(_lib.LIB_PATH), "first_block": first_block(eng, models, a.n, a.reps, a.old_entries)}
    if not a.old_entries:
        out["pool"] = pool(eng, a.reps)
        out.update(embed_and_eer(eng, min(a.n, 2048), max(2, a.reps // 3), a.skip_eer))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
