"""HIP-event medians of svk_vad_adaptive (include/svk.h, "level-adaptive energy VAD") ALTERNATED call by call with svk_vad_energy on the same device
buffers, called through the C-ABI on outputs allocated once:
  * "short_index" / "short_copy": --clips (16 384) clips of 3 s, the benchmark's shape (99 frames of 480 samples: the one-kernel
    route of both entries), in the index form (nothing copied) and in the copying form;
  * "long_index" / "long_copy": 14 ragged clips of 31 .. 145 s through offsets / lengths, the case csrc/vad.hip's comment
    measures (up to 4 833 frames: the chunked kernels of both entries).
The clips are the synthetic speakers' (synth.corpus_device), so both rules keep most frames.  Design bytes: every sample of a
whole frame read once (2 B), plus 2 B read and 2 B written per kept sample in the copying form; the outputs per frame are left out
(under 1 % of the PCM).  The adaptive entry's extra 8 B per frame of energies on the long route are reported beside it.
--quality N adds, on the first N clips of the corpus bench.py draws its EER from (the shipped checkpoint, the bench's pipeline
settings, the last utterance of a speaker enrols, svk_roc_eer): the share of frames kept and the EER under each rule at full level,
and under the adaptive rule on the same clips 24 dB down (x >> 4; the absolute rule keeps nothing there).
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json
import math
import os

import _timing as T          # (puts the repository on sys.path)

LONG_SECONDS = (31, 38, 44, 52, 60, 67, 75, 83, 91, 99, 108, 120, 133, 145)
FS, FSAMP, RING = 16000, 480, 10


def quality(eng, n):
    import numpy as np
    import torch
    from speaker_verification_amd import evaluation, synth
    from speaker_verification_amd.model import C3D2
    from speaker_verification_amd.pipeline import VerificationPipeline, enroll_last_utterance
    from speaker_verification_amd.vad import AdaptiveEnergyVad
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ck = torch.load(os.path.join(here, "speaker_verification_amd", "checkpoints", "c3d2_synth.pt"), map_location="cpu", weights_only=True)
    model = C3D2(int(ck["state_dict"]["FC6.weight"].shape[0]), 1)
    model.load_state_dict(ck["state_dict"])
    per = 123                                                        # bench.py's UTTS_PER_SPK
    pcm, spk = synth.corpus_device(n, eng.device, utts_per_speaker=per)[:2]
    spk = np.asarray(spk.cpu() if hasattr(spk, "cpu") else spk)
    ids, last = enroll_last_utterance(None, spk)
    labels = (spk[:, None] == ids[None, :]).astype(np.float64)
    out = {"clips": n, "speakers": int(len(ids)), "utts_per_speaker": per}
    for name, vad, x in (("absolute", None, pcm), ("adaptive", AdaptiveEnergyVad(), pcm), ("adaptive_24dB_down", AdaptiveEnergyVad(), pcm >> 4),
                         ("absolute_24dB_down", None, pcm >> 4)):
        pipe = VerificationPipeline(model, use_vad=True, normalize=True, preemph_cof=0.98, crop_rng="device", micro_batch=1024, vad=vad)
        kept = frames = 0
        for lo, hi in pipe.chunks(n):
            vlen, _ = pipe.vad(x[lo:hi])
            kept += int(vlen.sum().item())
            frames += (hi - lo) * ((2 * x.shape[1] - 1) // (2 * FSAMP))
        if name == "absolute_24dB_down":                             # no frame kept, every clip a bad clip: nothing to score
            out[name] = {"frames_kept": round(kept / FSAMP / frames, 4)}
            continue
        emb = pipe.embed(x)
        scores = pipe.score(emb, emb[torch.from_numpy(last).to(eng.device)])
        eer, auc = evaluation.get_eer_auc_device(labels, scores)
        out[name] = {"frames_kept": round(kept / FSAMP / frames, 4), "eer": eer, "auc": auc, "bad_clips": int(pipe.bad_clips.item())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=16384, help="short clips (at least 1 800: the long clips are cut from them)")
    ap.add_argument("--quality", type=int, default=0, metavar="N")
    args = ap.parse_args()
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd import constants as c, synth
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.vad import AdaptiveEnergyVad
    eng = get_engine(0)
    dev = eng.device
    res = T.header(_lib, lib, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={}, energy_bytes={})
    vad = AdaptiveEnergyVad()
    ptr = eng._ptr
    ring_thresh = int(math.floor(0.9 * RING))

    def race(tag, x, offs, lens, stride, longest, n, copy):
        """Both entries on the same input and the same output buffers; each one's design bytes from what it keeps itself."""
        max_vf = max(1, (2 * longest - 1) // (2 * FSAMP))
        keep = torch.empty((n, max_vf), dtype=torch.uint8, device=dev)
        nvf, vlen = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
        voiced = torch.empty_like(x) if copy else None
        src = None if copy else torch.empty((n, max_vf), dtype=torch.int32, device=dev)
        levels = torch.empty((n, 3), dtype=torch.int64, device=dev)
        head = (ptr(x), ptr(offs), ptr(lens), stride, longest, n, FSAMP, RING, ring_thresh)
        tail = (ptr(keep), None, ptr(nvf), ptr(voiced), ptr(vlen), ptr(src))
        eng._stream()

        def energy():
            _lib.check(lib.svk_vad_energy(eng.ctx, *head, c.VAD_ENERGY_THRESHOLD, max_vf, *tail), eng.ctx)

        def adaptive():
            _lib.check(lib.svk_vad_adaptive(eng.ctx, *head, vad.floor_q16, vad.peak_q16, vad.above_floor_q16, vad.below_peak_q16,
                                            vad.min_threshold, max_vf, *tail, ptr(levels), None), eng.ctx)

        fns = {"adaptive": adaptive, "energy": energy} if has_adaptive else {"energy": energy}
        nbytes = {}
        for name, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            nbytes[name] = 2 * FSAMP * int(nvf.sum().item()) + (4 * int(vlen.sum().item()) if copy else 0)
            res.setdefault("frames_kept", {})["%s_%s" % (name, tag)] = round(int(vlen.sum().item()) / FSAMP / max(1, int(nvf.sum().item())), 4)
        times = T.alternated(torch, fns, args.reps, args.warmup)
        b = T.put("energy_" + tag, times["energy"], nbytes["energy"])
        if not has_adaptive:                                     # (a build from before the entry: the absolute rule alone)
            return
        a = T.put("adaptive_" + tag, times["adaptive"], nbytes["adaptive"])
        res["ratio"]["adaptive_%s/energy_%s" % (tag, tag)] = round(a / b, 3)
        if max_vf > 512:
            res["energy_bytes"]["adaptive_" + tag] = 16 * int(nvf.sum().item())          # written once, read once

    has_adaptive = hasattr(lib, "svk_vad_adaptive")
    pcm = synth.corpus_device(args.clips, dev)[0]
    for copy in (False, True):
        race("short_copy" if copy else "short_index", pcm, None, None, pcm.shape[1], pcm.shape[1], args.clips, copy)
    # 14 long clips: 3 s synthetic clips of one speaker each, repeated to length, on 16-byte boundaries
    lens = np.array([s * FS for s in LONG_SECONDS], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 7) // 8 * 8)[:-1]]).astype(np.int64)
    flat = torch.empty((int(offs[-1]) + int(lens[-1]),), dtype=torch.int16, device=dev)
    for u, (o, n) in enumerate(zip(offs, lens)):
        flat[o:o + n] = pcm[u * 123:u * 123 + 60].reshape(-1)[:n]
    d_offs, d_lens = torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)
    del pcm
    for copy in (False, True):
        race("long_copy" if copy else "long_index", flat, d_offs, d_lens, 0, int(lens.max()), len(lens), copy)
    del flat
    if args.quality:
        res["quality"] = quality(eng, args.quality)
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
