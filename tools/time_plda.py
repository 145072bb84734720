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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (6.3 TB/s is the measured copy rate)
F32_MATRIX_PEAK = 157.3e12


def one(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(torch, fns, reps, warmup):
    """{name: sorted times in ms}: the functions take turns, call by call, so that clocks and cache state drift for all alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(one(torch, fn))
    return {name: sorted(v) for name, v in times.items()}


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
    if os.environ.get("SVK_TOOL_LIB"):      # A/B: time another build of the library in the same process layout
        from speaker_verification_amd import _lib
        _lib.LIB_PATH = os.environ["SVK_TOOL_LIB"]
        lib = _lib.C.CDLL(_lib.LIB_PATH)
        _lib.VERSION = lib.svk_version()
        _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(lib, k)}
    from speaker_verification_amd import _lib
    from speaker_verification_amd import plda as plda_mod
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    lib = _lib.load()
    n, ns, dim = args.rows, args.speakers, args.dim
    res = {"lib": _lib.LIB_PATH, "version": int(lib.svk_version()), "csrc_sha": _lib.provenance()["csrc_sha"], "rows": n,
           "speakers": ns, "dim": dim, "reps": args.reps, "ms": {}, "spread_ms": {}, "bytes": {}, "tb_s": {}, "flop": {},
           "tf_s": {}, "ratio": {}}

    def put(name, times, nbytes=None, flop=None):
        med = times[len(times) // 2]
        res["ms"][name] = round(med, 4)
        res["spread_ms"][name] = [round(times[0], 4), round(times[-1], 4)]
        if nbytes:
            res["bytes"][name] = int(nbytes)
            res["tb_s"][name] = round(nbytes / (med * 1e-3) / 1e12, 3)
        if flop:
            res["flop"][name] = int(flop)
            res["tf_s"][name] = round(flop / (med * 1e-3) / 1e12, 2)
        return med

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
    times = alternated(torch, fns, args.reps, args.warmup)
    out_bytes, in_bytes = 4 * n * ns, 4 * (n + ns) * dim
    ours = put("plda", times["plda"], out_bytes + in_bytes + 4 * n * dim + 3 * 4 * ns * dim, 2 * n * ns * dim)
    cos = put("cosine", times["cosine"], out_bytes + in_bytes, 2 * n * ns * dim)
    with_counts = put("plda_counts", times["plda_counts"], out_bytes + in_bytes + 3 * 4 * n * dim + 5 * 4 * ns * dim, 4 * n * ns * dim)
    ref = put("torch", times["torch"], 5 * out_bytes + in_bytes, 2 * n * ns * dim)
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
        times = alternated(torch, fns, args.reps, args.warmup)
        tag = "_%d" % n_trials
        nbytes = n_trials * (2 * dim * 4 + 2 * 8 + 4)
        a = put("plda_pairs" + tag, times["plda_pairs"], nbytes)
        b = put("cosine_pairs" + tag, times["cosine_pairs"], nbytes)
        put("plda_pairs_counts" + tag, times["plda_pairs_counts"], nbytes + 4 * n_trials)
        res["ratio"]["plda_pairs/cosine_pairs" + tag] = round(a / b, 3)
    res["hbm_peak_tb_s"] = HBM_PEAK / 1e12
    res["f32_matrix_peak_tf_s"] = F32_MATRIX_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
