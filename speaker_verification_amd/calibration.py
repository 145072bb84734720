"""Score calibration and fusion: from scores to log-likelihood ratios a Bayes threshold can be applied to.

A verifier's raw scores order the trials (EER, minDCF) but say nothing about where to cut: a cosine lives in [-1, 1], and a PLDA
score is an LLR only under its model.  `Calibration` fits the affine map

    llr = sum_d w_d s_d + b            D = 1: calibration of one system;  D > 1: fusion of D systems

on a development trial list by prior-weighted logistic regression (Bruemmer's objective, the one Bosaris and the NIST SRE /
VoxSRC recipes minimise): with tau = logit(p_target),

    f(w) = p / N_tar  sum_targets softplus(-(llr + tau))  +  (1 - p) / N_non  sum_non-targets softplus(llr + tau)

After it the threshold for ANY operating point is `bayes_threshold(p_target, c_miss, c_fa)`; `cllr` and `act_dcf` judge the
result (minDCF against actDCF is the calibration loss).

    fit      damped Newton in NumPy float64 on the host; each iteration is ONE pass over the trials on the device
             (`svk_calibration_stats`: objective, gradient and Hessian, float64, deterministic)
    apply    scores -> calibrated float32 LLRs, device to device (`svk_calibration_apply`)

`fit(..., stats=fn)` takes any callable with `Engine.calibration_stats`' signature, so the iteration itself needs no GPU.
DESIGN 3.13, INTEGRATION "Calibration and fusion".
"""
import math

import numpy as np

LN2 = math.log(2.0)


def logit(p):
    return math.log(p) - math.log1p(-p)


def bayes_threshold(p_target, c_miss=1.0, c_fa=1.0):
    """log(c_fa (1 - p_target) / (c_miss p_target)): accept when a calibrated LLR is at or above it."""
    p_target, c_miss, c_fa = float(p_target), float(c_miss), float(c_fa)
    if not (0.0 < p_target < 1.0 and c_miss > 0 and c_fa > 0):
        raise ValueError("need 0 < p_target < 1 and c_miss, c_fa > 0")
    return math.log(c_fa) + math.log1p(-p_target) - math.log(c_miss) - math.log(p_target)


def _stats_of(engine, stats):
    if stats is not None:
        return stats
    from .engine import get_engine
    return (engine or get_engine()).calibration_stats


def cllr(scores, labels, engine=None, stats=None):
    """Cllr of scores read as LLRs, in bits: (mean_targets softplus(-s) + mean_non-targets softplus(s)) / (2 ln 2), one
    value-only `svk_calibration_stats` call.  0 is perfect, 1 is what llr = 0 for every trial gives.  scores: one system, [n].
    ValueError for a single class or a non-finite score."""
    l_tar, l_non, _, _, (n_tar, n_non, skipped) = _stats_of(engine, stats)(scores, labels, (1.0, 0.0), 0.0, (1.0, 1.0),
                                                                          value_only=True)
    if skipped or n_tar == 0 or n_non == 0:
        raise ValueError("Cllr needs finite scores of both classes: %d targets, %d non-targets, %d non-finite" % (n_tar, n_non, skipped))
    return (l_tar / n_tar + l_non / n_non) / (2.0 * LN2)


def act_dcf(scores, labels, operating_points, engine=None):
    """The detection cost of deciding calibrated LLRs at the Bayes thresholds: ONE `svk_decision_counts` call over the trials.
    operating_points: up to 16 (p_target, c_miss, c_fa).  Returns (act_dcf, p_miss, p_fa), a list each, normalised as min_dcf
    is: (c_miss p p_miss + c_fa (1 - p) p_fa) / min(c_miss p, c_fa (1 - p)).  The thresholds are rounded to float32, the
    precision of the scores."""
    from .engine import get_engine
    ops = [tuple(float(v) for v in op) for op in operating_points]
    if not ops:
        return [], [], []
    thresholds = [bayes_threshold(*op) for op in ops]
    accepted, (n_tar, n_non) = (engine or get_engine()).decision_counts(scores, labels, thresholds)
    if n_tar == 0 or n_non == 0:
        raise ValueError("actDCF needs both classes: %d targets, %d non-targets" % (n_tar, n_non))
    dcf, p_miss, p_fa = [], [], []
    for (p, c_miss, c_fa), (acc_tar, acc_non) in zip(ops, accepted):
        a, b = c_miss * p, c_fa * (1.0 - p)
        miss, fa = 1.0 - float(acc_tar) / n_tar, float(acc_non) / n_non
        dcf.append((a * miss + b * fa) / min(a, b))
        p_miss.append(miss)
        p_fa.append(fa)
    return dcf, p_miss, p_fa


class Calibration:
    """Affine calibration (one system) or fusion (several) of verification scores.  `fit` on a development trial list, `apply`
    to any score list; `VerificationPipeline(..., calibration=c)` and `evaluation.evaluate_trials(..., calibration=c)` apply it
    themselves.  p_target is the prior the regression is weighted for (the operating region it is most exact in), not a
    limit on the operating points the result is used at."""

    ARMIJO = 1e-4
    MAX_HALVINGS = 40

    def __init__(self, p_target=0.01, max_iter=100, tol=1e-12):
        if not 0.0 < float(p_target) < 1.0:
            raise ValueError("need 0 < p_target < 1")
        self.p_target, self.max_iter, self.tol = float(p_target), int(max_iter), float(tol)
        self.weights_ = None
        self.n_iter_, self.converged_, self.objective_ = 0, False, None

    @property
    def n_sys(self):
        return None if self.weights_ is None else int(self.weights_.size) - 1

    def _fitted(self):
        if self.weights_ is None:
            raise RuntimeError("the calibration is not fitted")

    def fit(self, scores, labels, engine=None, stats=None):
        """Minimises the prior-weighted objective over (w, b) from all weights and the offset at ZERO (there every trial has
        sigma = p_target or 1 - p_target and the Hessian is as well conditioned as the scores allow).  Per iteration: the
        Newton direction d = -H^-1 G by Cholesky -- a Levenberg term lambda I, grown tenfold from 1e-10 tr(H) / dim, only when
        the factorisation fails or d is no descent direction --, then backtracking (halving) until the Armijo condition
        f(w + t d) <= f(w) + 1e-4 t G.d holds; every trial point costs one statistics pass.  Converged when the Newton
        decrement -G.d <= tol AND the step just taken moved no weight by more than sqrt(tol) max(1, |w|_inf): at a minimum
        both shrink quadratically, while on separable data, which has no minimum, the objective and with it the decrement go
        to zero as the weights grow by a constant step, so the decrement alone would call that converged.  Separable data ends
        after max_iter iterations with finite weights and converged_ = False.
        scores: [n] or [n_sys, n] (tensor, array) or a sequence of [n]; labels: non-zero = target.  stats: a callable with
        `Engine.calibration_stats`' signature instead of the device.  Sets weights_ (float64 [n_sys + 1], the offset last),
        n_iter_, converged_, objective_; returns self.  ValueError: a single class, or a non-finite score."""
        stat = _stats_of(engine, stats)
        p, tau = self.p_target, logit(self.p_target)
        if isinstance(scores, (list, tuple)) and stats is None:
            from .engine import get_engine
            scores, _ = (engine or get_engine())._score_planes(scores)      # stacked once, not once per iteration
        n_sys = len(scores) if isinstance(scores, (list, tuple)) else (1 if len(scores.shape) == 1 else int(scores.shape[0]))
        dim = n_sys + 1
        w = np.zeros(dim, dtype=np.float64)
        _, _, _, _, (n_tar, n_non, skipped) = stat(scores, labels, w, tau, (1.0, 1.0), value_only=True)
        if skipped:
            raise ValueError("calibration: %d trials have a non-finite score" % skipped)
        if n_tar == 0 or n_non == 0:
            raise ValueError("calibration needs both classes: %d targets, %d non-targets" % (n_tar, n_non))
        cw = (p / n_tar, (1.0 - p) / n_non)

        def evaluate(at):
            l_tar, l_non, grad, hess, _ = stat(scores, labels, at, tau, cw)
            return cw[0] * l_tar + cw[1] * l_non, grad, hess

        f, grad, hess = evaluate(w)
        self.converged_, self.n_iter_ = False, 0
        for _ in range(self.max_iter):
            step = self._direction(grad, hess)
            if step is None:
                break
            slope = float(grad @ step)
            t, taken = 1.0, None
            for _ in range(self.MAX_HALVINGS):
                trial = w + t * step
                f_new, g_new, h_new = evaluate(trial)
                if np.isfinite(f_new) and f_new <= f + self.ARMIJO * t * slope:
                    taken = trial
                    break
                t *= 0.5
            if taken is None:
                break
            moved = float(np.max(np.abs(taken - w)))
            w, f, grad, hess = taken, f_new, g_new, h_new
            self.n_iter_ += 1
            if -slope <= self.tol and moved <= math.sqrt(self.tol) * max(1.0, float(np.max(np.abs(w)))):
                self.converged_ = True
                break
        self.weights_, self.objective_ = w, float(f)
        return self

    @staticmethod
    def _direction(grad, hess):
        """-H^-1 G, or the same with H + lambda I when H is not positive definite to working precision or the solve gives no
        descent direction; None when nothing finite comes out."""
        dim = grad.size
        if not (np.isfinite(grad).all() and np.isfinite(hess).all()):
            return None
        lam, base = 0.0, 1e-10 * max(float(np.trace(hess)) / dim, np.finfo(np.float64).tiny)
        for _ in range(60):
            try:
                chol = np.linalg.cholesky(hess + lam * np.eye(dim))
                step = -np.linalg.solve(chol.T, np.linalg.solve(chol, grad))
                if np.isfinite(step).all() and float(grad @ step) < 0.0:
                    return step
                if not grad.any():
                    return np.zeros(dim)
            except np.linalg.LinAlgError:
                pass
            lam = base if lam == 0.0 else lam * 10.0
        return None

    def apply(self, scores, engine=None, out=None):
        """Calibrated LLRs, float32 [n] on the device: sum_d w_d scores[d] + b in float64, rounded once."""
        from .engine import get_engine
        self._fitted()
        return (engine or get_engine()).calibration_apply(scores, self.weights_, out=out)

    def save(self, path):
        """An .npz of the float64 weights plus the settings and the fit's outcome."""
        self._fitted()
        with open(path, "wb") as fh:
            np.savez(fh, weights=self.weights_, p_target=np.array(self.p_target), max_iter=np.array(self.max_iter),
                     tol=np.array(self.tol), n_iter=np.array(self.n_iter_), converged=np.array(self.converged_),
                     objective=np.array(np.nan if self.objective_ is None else self.objective_))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cal = cls(p_target=float(z["p_target"]), max_iter=int(z["max_iter"]), tol=float(z["tol"]))
            weights = np.ascontiguousarray(z["weights"], dtype=np.float64).reshape(-1)
            if weights.size < 2 or not np.isfinite(weights).all():
                raise ValueError("a calibration holds at least one finite weight and the offset")
            cal.weights_ = weights
            cal.n_iter_, cal.converged_ = int(z["n_iter"]), bool(z["converged"])
            objective = float(z["objective"])
            cal.objective_ = None if math.isnan(objective) else objective
        return cal


# ---- the ROC convex hull: minCllr, ROCCH-EER, PAV --------------------------------------------------------------------------
# How good a calibration COULD have been: minCllr is the Cllr of the best monotone map of the scores, which is PAV (isotonic
# regression of the labels on the scores); cllr - min_cllr is the calibration loss.  PAV's bins are the edges of the upper
# convex hull of the ROC and its posteriors their slopes; `Engine.rocch` (svk_rocch; include/svk.h, "the ROC convex hull", has the definitions)
# returns the hull's integer vertices from the device sort.  Everything below is host arithmetic on those K + 1 vertices.
def hull_chain(points):
    """Andrew's monotone chain over lexicographically sorted integer points (f, t), popping while cross >= 0: the indices of
    the upper hull's vertices.  Python integers: exact."""
    keep = []
    for i, (f, t) in enumerate(points):
        f, t = int(f), int(t)
        while len(keep) >= 2:
            (af, at), (bf, bt) = points[keep[-2]], points[keep[-1]]
            af, at, bf, bt = int(af), int(at), int(bf), int(bt)
            if (bf - af) * (t - at) - (bt - at) * (f - af) >= 0:
                keep.pop()
            else:
                break
        keep.append(i)
    return keep


def _vertex_list(vertices):
    v = [(int(f), int(t)) for f, t in np.asarray(vertices).reshape(-1, 2)]
    if len(v) < 2 or v[0] != (0, 0) or v[-1][0] < 1 or v[-1][1] < 1:
        raise ValueError("hull vertices run from the origin to (N, P) with both classes present")
    return v


def min_cllr_of(vertices):
    """minCllr in bits from the hull's vertices [K + 1, 2] (fps, tps): [(1/P) sum_k dt_k log1p(df_k P / (dt_k N)) + (1/N) sum_k
    df_k log1p(dt_k N / (df_k P))] / (2 ln 2) over the edges, an edge with dt_k = 0 or df_k = 0 contributing 0.  The arguments
    are quotients of Python integers (rounded once); every term is non-negative."""
    v = _vertex_list(vertices)
    n_non, n_tar = v[-1]
    s_tar = s_non = 0.0
    for (f0, t0), (f1, t1) in zip(v[:-1], v[1:]):
        df, dt = f1 - f0, t1 - t0
        if df and dt:
            s_tar += dt * math.log1p((df * n_tar) / (dt * n_non))
            s_non += df * math.log1p((dt * n_non) / (df * n_tar))
    return (s_tar / n_tar + s_non / n_non) / (2.0 * LN2)


def rocch_eer_of(vertices):
    """The EER of the hull: `svk_roc_eer`'s rule on the vertices.  On the one edge with g_0 = 1 - f_0/N - t_0/P > 0 >= g_1,
    x_0 + (x_1 - x_0) g_0 / (g_0 - g_1) -- formed as one quotient of Python integers, rounded once."""
    v = _vertex_list(vertices)
    n_non, n_tar = v[-1]
    gap = lambda f, t: n_non * n_tar - f * n_tar - t * n_non            # noqa: E731  (g times N P)
    for (f0, t0), (f1, t1) in zip(v[:-1], v[1:]):
        g0, g1 = gap(f0, t0), gap(f1, t1)
        if g0 > 0 >= g1:
            return (f0 * (g0 - g1) + (f1 - f0) * g0) / (n_non * (g0 - g1))
    raise ValueError("no edge of the hull crosses the diagonal")


def min_cllr(scores, labels, engine=None):
    """minCllr of a trial set in bits: one `Engine.rocch` call.  0 <= min_cllr <= 1; cllr - min_cllr is the calibration loss."""
    from .engine import get_engine
    return (engine or get_engine()).rocch(scores, labels)["min_cllr"]


def rocch_eer(scores, labels, engine=None):
    """The EER on the ROC convex hull (the one Bosaris-style recipes quote): one `Engine.rocch` call.  rocch_eer <= eer."""
    from .engine import get_engine
    return (engine or get_engine()).rocch(scores, labels)["rocch_eer"]


def pav_table(vertices, vertex_scores, laplace=False):
    """The PAV calibration of a trial set from its hull -> (edges float32 [B] descending, llr float32 [B]): bin k holds the
    scores s >= edges[k] not taken by a bin above it, edges[k] being the lowest score of the bin, and maps them to
    llr[k] = log(dt_k / df_k) - log(P / N) (+inf for df_k = 0, -inf for dt_k = 0).
    laplace=True is Bosaris' rule: in descending score order a non-target and then a target are added above the best score and a
    non-target and then a target below the worst.  The hull of that sequence is the hull of the four dummy points and the
    shifted vertices (the hull of a union is the hull of the hulls), taken here exactly; only bins that hold a real trial are
    kept, and all their LLRs are finite.  The prior log odds stay log(P / N) of the real trials."""
    v = _vertex_list(vertices)
    sc = np.asarray(vertex_scores, dtype=np.float32).reshape(-1)
    if sc.size != len(v):
        raise ValueError("one score per vertex")
    n_non, n_tar = v[-1]
    prior = math.log(n_tar) - math.log(n_non)
    if laplace:
        pts = [(0, 0), (1, 0), (1, 1)] + [(f + 1, t + 1) for f, t in v[1:]] + [(n_non + 2, n_tar + 1), (n_non + 2, n_tar + 2)]
        low = [None, None, None] + [float(s) for s in sc[1:]] + [float(sc[-1]), float(sc[-1])]
        real = lambda f, t: min(max(f - 1, 0), n_non) + min(max(t - 1, 0), n_tar)      # noqa: E731  (real trials at or above)
        keep = hull_chain(pts)
    else:
        pts, low, real, keep = v, [float(s) for s in sc], (lambda f, t: f + t), list(range(len(v)))
    edges, llr = [], []
    for a, b in zip(keep[:-1], keep[1:]):
        (f0, t0), (f1, t1) = pts[a], pts[b]
        if real(f1, t1) - real(f0, t0) <= 0:
            continue
        df, dt = f1 - f0, t1 - t0
        edges.append(low[b])
        llr.append(math.inf if df == 0 else -math.inf if dt == 0 else math.log(dt) - math.log(df) - prior)
    return np.asarray(edges, dtype=np.float32), np.asarray(llr, dtype=np.float32)


class PavCalibration:
    """Non-parametric calibration by PAV: the monotone step map of scores to LLRs that minimises Cllr on the trial list it is
    fitted on (there, cllr of the mapped scores equals min_cllr).  `fit` on a development trial list, `apply` to any scores; a
    fitted one can be passed wherever `calibration=` is taken.  Without laplace the best and worst bins of separable ends map
    to +-inf, which the metrics refuse; laplace=True keeps every LLR finite."""

    n_sys = 1

    def __init__(self, laplace=False):
        self.laplace = bool(laplace)
        self.edges_ = self.llr_ = None

    def _fitted(self):
        if self.edges_ is None:
            raise RuntimeError("the calibration is not fitted")

    def fit(self, scores=None, labels=None, engine=None, hull=None):
        """One `Engine.rocch` call, then the table on the host (`pav_table`).  hull: (vertices, vertex_scores) instead of
        scores and labels, so that the table's logic needs no GPU.  Sets edges_ and llr_ (float32 [bins]); returns self."""
        if hull is None:
            from .engine import get_engine
            res = (engine or get_engine()).rocch(scores, labels)
            hull = (res["vertices"], res["vertex_scores"])
        self.edges_, self.llr_ = pav_table(hull[0], hull[1], self.laplace)
        return self

    def apply(self, scores, engine=None, out=None):
        """The mapped scores, float32 [n] on the device (`svk_pav_apply`); out may be the scores themselves."""
        from .engine import get_engine
        self._fitted()
        return (engine or get_engine()).pav_apply(scores, self.edges_, self.llr_, out=out)

    def save(self, path):
        self._fitted()
        with open(path, "wb") as fh:
            np.savez(fh, edges=self.edges_, llr=self.llr_, laplace=np.array(self.laplace))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            cal = cls(laplace=bool(z["laplace"]))
            edges = np.ascontiguousarray(z["edges"], dtype=np.float32).reshape(-1)
            llr = np.ascontiguousarray(z["llr"], dtype=np.float32).reshape(-1)
            if edges.size < 1 or edges.size != llr.size or np.isnan(edges).any() or (np.diff(edges) > 0).any():
                raise ValueError("a PAV table holds at least one bin, one LLR per edge, the edges descending")
            cal.edges_, cal.llr_ = edges, llr
        return cal
