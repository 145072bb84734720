"""HIP-event medians of the two PLDA scoring entries, each ALTERNATED call by call with the cosine entry of the same shape and
with the framework route it replaces:
  * svk_plda_scores at the development-set size (--rows 148 642 x --speakers 1 211 x --dim 128), counts off ("plda") and on
    ("plda_counts"), against svk_cosine_scores of the same build ("cosine": the same MFMA count as the counts-off form and the
    same bytes written) and against torch on PREPARED operands, (v * alpha) @ u^T + s[:, None] + t[None, :] ("torch": one GEMM
    and two broadcast adds; the operands' preparation is not timed).  Design bytes: both operands in, the output out, plus the
    pre-pass (the enrolled operand written and read; with counts also both second halves).  FLOP: 2 K per score, K = dim or
    2 dim;
  * svk_plda_pair_scores at the sizes of the public VoxCeleb1 lists (--lists "trials:rows,...": 581 480 over 145 160,
    VoxCeleb1-E, and 37 720 over 4 874, VoxCeleb1-O, the lists of tools/time_trials.py) against svk_pair_scores (cosine).
    Design bytes: two rows, two indices and one score per trial.
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json

import _timing as T          # (puts the repository on sys.path)

F32_MATRIX_PEAK = 157.3e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=148642)
    ap.add_argument("--speakers", type=int, default=1211)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--lists", default="581480:145160,37720:4874", help="trials:rows of each trial list")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    _lib, lib = T.load_lib()
    from speaker_verification_amd import plda as plda_mod
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    n, ns, dim = args.rows, args.speakers, args.dim
    res = T.header(_lib, lib, rows=n, speakers=ns, dim=dim, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, flop={},
                   tf_s={}, ratio={})

    g = torch.Generator(device=eng.device).manual_seed(1)
    psi_host = np.sort(np.random.default_rng(2).random(dim) ** 3 * 100.0)[::-1].copy()
    psi = eng.to_device(psi_host)
    scale = torch.sqrt(1.0 + psi).float()
    v = torch.randn(n, dim, device=eng.device, generator=g) * scale
    u = torch.randn(ns, dim, device=eng.device, generator=g) * scale
    counts = eng.to_device(np.random.default_rng(3).integers(1, 8, ns).astype(np.int32))
    # the torch route's prepared operands (counts off): float32 b = alpha u, s and t as float32 vectors
    alpha, beta, gamma, c = plda_mod.coefficients(psi_host, 1)
    b_t = (u.double() * eng.to_device(alpha)).float()
    s_t = (-0.5 * (v.double() ** 2) @ eng.to_device(beta)).float()
    t_t = (-0.5 * (u.double() ** 2) @ eng.to_device(gamma) + c).float()
    fns = {"plda": lambda: eng.plda_scores(v, u, psi),
           "cosine": lambda: eng.cosine_scores(v, u),
           "plda_counts": lambda: eng.plda_scores(v, u, psi, counts),
           "torch": lambda: (v @ b_t.T).add_(s_t[:, None]).add_(t_t[None, :])}
    times = T.alternated(torch, fns, args.reps, args.warmup)
    out_bytes, in_bytes = 4 * n * ns, 4 * (n + ns) * dim
    ours = T.put("plda", times["plda"], out_bytes + in_bytes + 4 * n * dim + 3 * 4 * ns * dim, 2 * n * ns * dim)
    cos = T.put("cosine", times["cosine"], out_bytes + in_bytes, 2 * n * ns * dim)
    with_counts = T.put("plda_counts", times["plda_counts"], out_bytes + in_bytes + 3 * 4 * n * dim + 5 * 4 * ns * dim, 4 * n * ns * dim)
    ref = T.put("torch", times["torch"], 5 * out_bytes + in_bytes, 2 * n * ns * dim)
    res["ratio"]["plda/cosine"] = round(ours / cos, 3)
    res["ratio"]["plda_counts/plda"] = round(with_counts / ours, 3)
    res["ratio"]["torch/plda"] = round(ref / ours, 3)
    res["plda_max_diff_from_torch"] = float((fns["plda"]() - fns["torch"]()).abs().max().item())

    for spec in args.lists.split(","):
        n_trials, rows = (int(x) for x in spec.split(":"))
        x = torch.randn(rows, dim, device=eng.device, generator=g) * scale
        r = np.random.default_rng(n_trials)
        ia, ib = eng.to_device(r.integers(0, rows, n_trials)), eng.to_device(r.integers(0, rows, n_trials))
        cnt = eng.to_device(r.integers(1, 8, rows).astype(np.int32))
        fns = {"plda_pairs": lambda: eng.plda_pair_scores(x, x, ia, ib, psi),
               "cosine_pairs": lambda: eng.pair_scores(x, x, ia, ib),
               "plda_pairs_counts": lambda: eng.plda_pair_scores(x, x, ia, ib, psi, counts_b=cnt)}
        times = T.alternated(torch, fns, args.reps, args.warmup)
        tag = "_%d" % n_trials
        nbytes = n_trials * (2 * dim * 4 + 2 * 8 + 4)
        a = T.put("plda_pairs" + tag, times["plda_pairs"], nbytes)
        b = T.put("cosine_pairs" + tag, times["cosine_pairs"], nbytes)
        T.put("plda_pairs_counts" + tag, times["plda_pairs_counts"], nbytes + 4 * n_trials)
        res["ratio"]["plda_pairs/cosine_pairs" + tag] = round(a / b, 3)
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    res["f32_matrix_peak_tf_s"] = F32_MATRIX_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
