"""HIP-event medians of the embedding back end's two entries at the development-set size (--rows 148 642 x --dim 128, --speakers
1 211), each ALTERNATED call by call with the framework route it replaces:
  * svk_class_scatter (row norms, class means, S_w; flag bit 0 set, a shuffled row index) against torch: gather, .double(),
    F.normalize, per-class centre (index_add means), d^T d.  Design bytes: three reads of the rows (norm, mean and scatter
    passes) plus the row index twice and the norms written once and read twice;
  * svk_embedding_project with out_dim 128 and 64 (flags 3, mean and W given) against torch:
    F.normalize((F.normalize(x) - mu) @ W).  Design bytes: the rows in, the projected rows out, W once.
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=148642)
    ap.add_argument("--speakers", type=int, default=1211)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--out-dims", default="128,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd.engine import get_engine
    from speaker_verification_amd.pipeline import speaker_segments
    eng = get_engine(0)
    F = torch.nn.functional
    n, dim, n_spk = args.rows, args.dim, args.speakers
    res = T.header(_lib, lib, rows=n, dim=dim, speakers=n_spk, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={})

    g = torch.Generator(device=eng.device).manual_seed(1)
    x = torch.randn(n, dim, device=eng.device, generator=g) + 3.0
    ids = np.random.default_rng(2).integers(0, n_spk, size=n)
    _, seg_start, row_index = speaker_segments(ids)
    start = eng.to_device(seg_start)
    index = eng.to_device(row_index)
    cls = torch.repeat_interleave(torch.arange(start.numel() - 1, device=eng.device), start[1:] - start[:-1])
    counts = (start[1:] - start[:-1]).double().clamp(min=1).unsqueeze(1)

    def torch_scatter():
        xd = F.normalize(x[index].double(), dim=1)
        mean = torch.zeros((counts.shape[0], dim), dtype=torch.float64, device=eng.device).index_add_(0, cls, xd) / counts
        d = xd - mean[cls]
        return mean, d.T @ d

    times = T.alternated(torch, {"class_scatter": lambda: eng.class_scatter(x, start, row_index=index, l2_rows=True),
                                 "torch_scatter": torch_scatter}, args.reps, args.warmup)
    ours = T.put("class_scatter", times["class_scatter"], n * (3 * dim * 4 + 2 * 8 + 3 * 8))
    ref = T.put("torch_scatter", times["torch_scatter"])
    res["ratio"]["torch_scatter/class_scatter"] = round(ref / ours, 3)
    sw, sw_t = eng.class_scatter(x, start, row_index=index, l2_rows=True)[1], torch_scatter()[1]
    res["scatter_max_rel_diff"] = float(((sw - sw_t).abs().max() / sw_t.abs().max()).item())

    mu = x.mean(0)
    for out_dim in (int(v) for v in args.out_dims.split(",")):
        w = torch.randn(dim, out_dim, device=eng.device, generator=g) / dim ** 0.5
        fns = {"project": lambda: eng.embedding_project(x, mean=mu, w=w, l2_in=True, l2_out=True),
               "torch_project": lambda: F.normalize((F.normalize(x, dim=1) - mu) @ w, dim=1)}
        times = T.alternated(torch, fns, args.reps, args.warmup)
        tag = "_%d" % out_dim
        ours = T.put("project" + tag, times["project"], n * (dim + out_dim) * 4 + dim * out_dim * 4)
        ref = T.put("torch_project" + tag, times["torch_project"])
        res["ratio"]["torch_project/project" + tag] = round(ref / ours, 3)
        res["project_max_diff" + tag] = float((fns["project"]() - fns["torch_project"]()).abs().max().item())
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
