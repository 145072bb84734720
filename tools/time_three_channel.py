#!/usr/bin/env python3
"""HIP-event times per N cubes (default 4 018) of the three-channel model (constants.DERIVATIVE = True):
  * the first block: svk_c3d2_stage1_c3 next to the one-channel svk_c3d2_stage1, same feature rows and crop starts;
  * the whole embedding: FusedEmbedder.embed_features on [n, 3, T, 40] rows against the torch layers (MIOpen) of the same
    model on the materialised (n, 3, 20, 80, 40) cubes (in chunks of 512: the torch path's activations do not fit at once).
  * the input (--input): the sequence evaluation.dataset_embeddings ran before the fused kernels (derivative x 2, cmvn_ x 3,
    torch.stack) against delta_cmvn_stats + delta_planes, alternated in one process after warm-up, at the benchmark's
    micro-batch shape (n clips of bench.py's default length) and at a ragged-scale shape (a few clips above 1 024 frames:
    the chunked statistics path); design bytes (19 F against 5 F, F = one [n, T, 40] plane) and TB/s for each, the spread
    between repeated runs of the same code, cube_gather_delta, and VerificationPipeline.embed in utterances/s for the
    three-channel model beside the one-channel model.
Medians of --reps timed runs after one warm-up.      python tools/time_three_channel.py [n_cubes] [--reps R] [--input]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speaker_verification_amd.engine import get_engine                       # noqa: E402
from speaker_verification_amd.model import perturb_inference_state, seeded_model   # noqa: E402


def timed(fn, reps):
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
    return sorted(out)[len(out) // 2]


def alternate(fns, reps):
    """{name: sorted HIP-event times in ms}: the candidates take turns inside every repetition, after one warm-up round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: sorted(v) for k, v in out.items()}


def input_times(eng, models, n, reps):
    """The three-channel input: parent sequence against the fused pair, gather, and the pipeline's embed rate."""
    from speaker_verification_amd import synth
    from speaker_verification_amd.pipeline import VerificationPipeline
    g = torch.Generator(device=eng.device).manual_seed(1)
    r = {}
    for tag, (m, T) in {"bench": (n, 297), "ragged": (24, 9000)}.items():
        feat = torch.randn((m, T, 40), device=eng.device, generator=g) * 3 + 1
        nf = torch.randint(T // 2, T + 1, (m,), device=eng.device, dtype=torch.int32, generator=g)
        feat *= (torch.arange(T, device=eng.device)[None, :] < nf[:, None])[:, :, None]      # pad rows are zeros

        def parent():
            chans = [feat, eng.derivative(feat, 2)]
            chans.append(eng.derivative(chans[1], 2))
            chans[0] = feat.clone()                    # (the parent normalised the front end's own buffer in place: no copy
            for ch in chans:                           #  there; the clone keeps `feat` raw for the next repetition and is
                eng.cmvn_(ch, nf, variance=True)       #  timed separately below, then subtracted)
            return torch.stack(chans, 1)

        def fused():
            return eng.delta_planes(feat, nf, stats=eng.delta_cmvn_stats(feat, nf, variance=True))

        assert torch.equal(parent(), fused())
        crops = eng.draw_crops(nf, 20, 80, 1, 0)
        stats = eng.delta_cmvn_stats(feat, nf, variance=True)
        t = alternate({"parent": parent, "fused": fused, "parent_again": parent, "fused_again": fused,
                       "clone": lambda: feat.clone(), "gather": lambda: eng.cube_gather_delta(feat, crops, 80, stats=stats)}, reps)
        med = {k: v[len(v) // 2] for k, v in t.items()}
        F = feat.numel() * 4
        parent_ms, fused_ms = med["parent"] - med["clone"], med["fused"]
        r[tag] = {"clips": m, "frames": T, "F_bytes": F,
                  "parent_ms": parent_ms, "fused_ms": fused_ms, "speedup": parent_ms / fused_ms,
                  "parent_TBps_at_19F": 19 * F / parent_ms / 1e9, "fused_TBps_at_5F": 5 * F / fused_ms / 1e9,
                  # the spread between repeated runs of the same code: the two series of each candidate, and min .. max
                  "spread_parent_ms": abs(med["parent"] - med["parent_again"]), "spread_fused_ms": abs(med["fused"] - med["fused_again"]),
                  "range_parent_ms": [t["parent"][0] - med["clone"], t["parent"][-1] - med["clone"]], "range_fused_ms": [t["fused"][0], t["fused"][-1]],
                  "gather_ms": med["gather"], "gather_TBps": (20 * 80 * 40 * 4 * 4 * m) / med["gather"] / 1e9}
    pcm = synth.corpus_device(n, eng.device)[0]
    for ch in (1, 3):
        pipe = VerificationPipeline(models[ch], use_vad=True, normalize=True, crop_rng="device", micro_batch=n)
        ms = timed(lambda: pipe.embed(pcm), reps)
        r["embed_%dch_utt_per_s" % ch] = n / ms * 1e3
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=4018)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--input", action="store_true", help="time the three-channel input kernels and the pipeline instead")
    a = ap.parse_args()
    eng = get_engine(0)
    models = {}
    for ch in (1, 3):
        m = seeded_model(1, 8, ch)
        m.load_state_dict(perturb_inference_state(m.state_dict(), 2))
        models[ch] = m.to(eng.device).eval()
    if a.input:
        print(json.dumps(input_times(eng, models, a.n, a.reps)))
        return
    g = torch.Generator(device=eng.device).manual_seed(0)
    n, T = a.n, 297
    feat3 = torch.randn((n, 3, T, 40), device=eng.device, generator=g) * 2 - 6
    feat1 = feat3[:, 0].contiguous()
    crops = torch.randint(0, T - 80, (n, 20), device=eng.device, dtype=torch.int32, generator=g)
    e1, e3 = models[1].fused_inference(), models[3].fused_inference()
    r = {"n_cubes": n}
    r["stage1_1ch_ms"] = timed(lambda: eng.c3d2_stage1(feat1, crops, e1.stage1_tables()), a.reps)
    r["stage1_3ch_ms"] = timed(lambda: eng.c3d2_stage1(feat3, crops, e3.stage1_tables()), a.reps)
    r["stage1_ratio"] = r["stage1_3ch_ms"] / r["stage1_1ch_ms"]
    r["embed_3ch_kernels_ms"] = timed(lambda: e3.embed_features(feat3, crops), a.reps)
    r["embed_1ch_kernels_ms"] = timed(lambda: e1.embed_features(feat1, crops), a.reps)
    starts = crops.long()[:, :, None] + torch.arange(80, device=eng.device)                    # [n, 20, 80]
    cubes = feat3[torch.arange(n, device=eng.device)[:, None, None, None], torch.arange(3, device=eng.device)[None, :, None, None],
                  starts[:, None]]                                                               # (n, 3, 20, 80, 40)

    def torch_path():
        with torch.no_grad():
            for lo in range(0, n, 512):
                models[3].torch_layers(cubes[lo:lo + 512])
    r["embed_3ch_torch_layers_ms"] = timed(torch_path, max(1, a.reps // 2))
    r["torch_over_kernels"] = r["embed_3ch_torch_layers_ms"] / r["embed_3ch_kernels_ms"]
    with torch.no_grad():
        diff = (e3.embed_features(feat3[:64], crops[:64]) - models[3].torch_layers(cubes[:64])).abs().max().item()
    r["max_abs_diff_kernels_vs_torch_64"] = diff
    print(json.dumps(r))


if __name__ == "__main__":
    main()
