"""HIP-event medians of the two calibration entries at the development-set size (--n 180 005 462 = 148 642 x 1 211 trials), each
ALTERNATED call by call with the framework route it replaces on the same device operands:
  * svk_calibration_stats for --systems 1,2, full ("stats_D") and value only ("value_D"), against torch in float64 ("torch_stats_D"
    / "torch_value_D": z = w . s + b + tau, softplus(-z) / softplus(z) masked sums, sigmoid, the class-weighted residual, the sums of r x_i
    and h x_i x_j as element-wise products and reductions, the results brought to the host as the entry brings them).  Design bytes: every score and label once,
    n (4 D + 1);
  * svk_calibration_apply ("apply_D") against (w * s.double()).sum(0).add(b).float() ("torch_apply_D").  Design bytes: every
    score once and the output, n (4 D + 4);
  * a whole Calibration.fit on one system ("fit"), host clock around it (it ends in a stream synchronise): the statistics
    passes plus the NumPy Newton steps.  Its iteration count and passes are reported beside it.
Medians of --reps calls after --warmup; the spread (min .. max) is reported beside them.  The scores are drawn on the device:
targets (10 %) ~ N(2, 1), non-targets ~ N(-1, 1.5), further systems noisy affine copies.

SVK_TOOL_LIB=path/to/libsvk.so times another build.  One JSON line on stdout."""
import argparse
import json
import time

import _timing as T          # (puts the repository on sys.path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=148642 * 1211)
    ap.add_argument("--systems", default="1,2")
    ap.add_argument("--p-target", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    _lib, lib = T.load_lib()
    from speaker_verification_amd.calibration import Calibration, logit
    from speaker_verification_amd.engine import get_engine
    eng = get_engine(0)
    n, p = args.n, args.p_target
    systems = [int(v) for v in args.systems.split(",")]
    res = T.header(_lib, lib, n=n, reps=args.reps, ms={}, spread_ms={}, bytes={}, tb_s={}, ratio={})

    g = torch.Generator(device=eng.device).manual_seed(1)
    target = torch.rand(n, device=eng.device, generator=g) < 0.1
    labels = target.to(torch.uint8)
    # planes a multiple of four floats apart: the 16-byte loads (Engine.calibration_stats pads a sequence of systems the same way)
    planes = torch.empty((max(systems), (n + 3) // 4 * 4), dtype=torch.float32, device=eng.device)[:, :n]
    planes[0] = torch.randn(n, device=eng.device, generator=g)
    planes[0] = torch.where(target, planes[0] + 2.0, 1.5 * planes[0] - 1.0)
    for d in range(1, max(systems)):
        planes[d] = (0.7 + 0.2 * d) * planes[0] + 0.3 * d + 0.5 * torch.randn(n, device=eng.device, generator=g)
    n_tar = int(target.sum().item())
    tau, cw = logit(p), (p / n_tar, (1.0 - p) / (n - n_tar))
    c_vec = torch.full((n,), cw[1], dtype=torch.float64, device=eng.device)
    c_vec[target] = cw[0]

    def torch_stats(sc, w, value_only):
        s = sc.double()
        z = (w[:-1, None] * s).sum(0) + w[-1] + tau
        l_tar, l_non = (F.softplus(-z) * target).sum(), (F.softplus(z) * ~target).sum()
        if value_only:
            return torch.stack([l_tar, l_non]).cpu()
        sig = torch.sigmoid(z)
        r, h = torch.where(target, sig - 1.0, sig) * c_vec, sig * (1.0 - sig) * c_vec
        x = list(s) + [None]                                       # None: the constant 1 of the offset
        # element-wise products and sums, the packed upper triangle (a [D + 1, n] float64 GEMM with n = 1.8e8 as the inner
        # dimension took 5 s per call on this stack: not a route anyone would keep)
        grad = [(r if xi is None else r * xi).sum() for xi in x]
        hess = []
        for i, xi in enumerate(x):
            hx = h if xi is None else h * xi
            hess += [(hx if xj is None else hx * xj).sum() for xj in x[i:]]
        return torch.stack([l_tar, l_non] + grad + hess).cpu()

    for d in systems:
        sc = planes[:d]
        w_host = np.r_[np.full(d, 0.8 / d), 0.3]
        w_dev = eng.to_device(w_host)
        out = torch.empty((n,), dtype=torch.float32, device=eng.device)
        fns = {"stats": lambda: eng.calibration_stats(sc, labels, w_host, tau, cw),
               "torch_stats": lambda: torch_stats(sc, w_dev, False),
               "value": lambda: eng.calibration_stats(sc, labels, w_host, tau, cw, value_only=True),
               "torch_value": lambda: torch_stats(sc, w_dev, True),
               "apply": lambda: eng.calibration_apply(sc, w_host, out=out),
               "torch_apply": lambda: (w_dev[:-1, None] * sc.double()).sum(0).add_(w_dev[-1]).float()}
        times = T.alternated(torch, fns, args.reps, args.warmup)
        tag = "_%d" % d
        for name in ("stats", "value", "apply"):
            nbytes = n * (4 * d + (4 if name == "apply" else 1))
            ours = T.put(name + tag, times[name], nbytes)
            ref = T.put("torch_" + name + tag, times["torch_" + name])
            res["ratio"]["torch_%s/%s%s" % (name, name, tag)] = round(ref / ours, 3)
        # the two routes on the same operands
        mine = eng.calibration_stats(sc, labels, w_host, tau, cw)
        theirs = torch_stats(sc, w_dev, False).numpy()
        flat = np.r_[mine[0], mine[1], mine[2], mine[3][np.triu_indices(d + 1)]]
        res["stats_max_rel_diff_from_torch" + tag] = float(np.max(np.abs(flat - theirs) / np.maximum(np.abs(theirs), 1e-300)))
        res["apply_max_diff_from_torch" + tag] = float((fns["apply"]() - fns["torch_apply"]()).abs().max().item())

    fit_times, cal = [], None
    for _ in range(args.fit_reps + 1):                 # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cal = Calibration(p_target=p).fit(planes[0], labels, engine=eng)
        torch.cuda.synchronize()
        fit_times.append((time.perf_counter() - t0) * 1e3)
    T.put("fit", sorted(fit_times[1:]))
    res["fit"] = {"n_iter": cal.n_iter_, "converged": bool(cal.converged_), "weights": [float(v) for v in cal.weights_],
                  "objective": cal.objective_}
    res["hbm_peak_tb_s"] = T.HBM_PEAK / 1e12
    print(json.dumps(res))


if __name__ == "__main__":
    main()
