#!/usr/bin/env python3
"""HIP-event times per N cubes (default 4 018) of the three-channel model (constants.DERIVATIVE = True):
  * the first block: svk_c3d2_stage1_c3 next to the one-channel svk_c3d2_stage1, same feature rows and crop starts;
  * the whole embedding: FusedEmbedder.embed_features on [n, 3, T, 40] rows against the torch layers (MIOpen) of the same
    model on the materialised (n, 3, 20, 80, 40) cubes (in chunks of 512: the torch path's activations do not fit at once).
Medians of --reps timed runs after one warm-up.      python tools/time_three_channel.py [n_cubes] [--reps R]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=4018)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    eng = get_engine(0)
    models = {}
    for ch in (1, 3):
        m = seeded_model(1, 8, ch)
        m.load_state_dict(perturb_inference_state(m.state_dict(), 2))
        models[ch] = m.to(eng.device).eval()
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
