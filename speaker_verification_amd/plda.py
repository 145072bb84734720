"""PLDA back end: the last step of the embedding -> back end -> scorer -> metrics chain.  Two-covariance model, stated in the
basis that diagonalises both covariances: a projected utterance is u = V^T (x' - mu), x' = x or x / ||x||, and

    u = y + e,    y ~ N(0, diag psi) for the speaker,    e ~ N(0, I) for the session.

An enrolled model is the mean of n >= 1 projected utterances, a test utterance is v; the score is the log-likelihood ratio of
"same speaker" against "different speakers" (`coefficients` has the closed form).

    fit      labelled development embeddings -> class means and within-class scatter on the device (`svk_class_scatter`,
             float64, deterministic) -> `solve_plda` on the host: a closed-form moment estimate, no EM
    project  u = V^T (l2(x) - mu), device to device (`svk_embedding_project`)
    score    the LLR of every test row against every enrolled model (`svk_plda_scores`: float64 pre-pass, f32 MFMA product),
             or of the trials of a list (`svk_plda_pair_scores`, float64)

`solve_plda` and `coefficients` need no GPU.  DESIGN 3.12, INTEGRATION "Fitting and scoring with PLDA".
"""
import numpy as np

from .backend import _inverse_root, class_statistics, scatter_matrices


def solve_plda(class_mean, counts, sw, out_dim=None, shrinkage=0.0):
    """The model from the class statistics of svk_class_scatter -> (mean float64 [dim], V float64 [dim, out_dim], psi float64
    [out_dim], descending and >= 0).  One-way random-effects ANOVA over the C non-empty classes of n_c rows, N rows in all:
      W   = S_w / (N - C), then W <- W + shrinkage tr(W) / dim I          the within-speaker covariance
      M_b = sum_c n_c (m_c - m)(m_c - m)^T / (C - 1), m the weighted mean    E[M_b] = W + n0 B
      n0  = (N - sum_c n_c^2 / N) / (C - 1)
    Whiten W with P, eigendecompose P^T M_b P = U diag(lambda) U^T (descending):  V = P U[:, :out_dim], so V^T W V = I and
    V^T M_b V = diag(lambda), and psi_k = max((lambda_k - 1) / n0, 0).  out_dim <= min(dim, C - 1), the default; a dropped
    direction has psi = 0 in expectation and a direction with psi = 0 changes no score.
    ValueError: fewer than 2 non-empty classes, N <= C (no within-class degree of freedom), non-finite statistics, a singular
    W (use shrinkage), out_dim out of range."""
    if not (np.isfinite(shrinkage) and shrinkage >= 0):
        raise ValueError("shrinkage must be a finite number >= 0")
    mean, s_w, s_b = scatter_matrices(class_mean, counts, sw)          # both divided by N
    cnt = np.asarray(counts, dtype=np.float64).reshape(-1)
    cnt = cnt[cnt > 0]
    n_rows, n_class, dim = float(cnt.sum()), int(cnt.size), int(mean.size)
    if n_class < 2:
        raise ValueError("PLDA needs at least 2 non-empty classes, got %d" % n_class)
    if not n_rows > n_class:
        raise ValueError("PLDA needs a class of more than one row (%d rows in %d classes leave no within-class scatter)"
                         % (int(n_rows), n_class))
    limit = min(dim, n_class - 1)
    if out_dim is None:
        out_dim = limit
    out_dim = int(out_dim)
    if out_dim < 1 or out_dim > limit:
        raise ValueError("out_dim = %d is out of range (dim %d, %d classes: at most %d)" % (out_dim, dim, n_class, limit))
    w = s_w * (n_rows / (n_rows - n_class))
    w = w + shrinkage * np.trace(w) / dim * np.eye(dim)
    m_b = s_b * (n_rows / (n_class - 1))
    n0 = (n_rows - (cnt * cnt).sum() / n_rows) / (n_class - 1)
    p, _ = _inverse_root(w, "W")
    g = p.T @ m_b @ p
    lam, u = np.linalg.eigh((g + g.T) / 2.0)
    lam, u = lam[::-1][:out_dim], u[:, ::-1][:, :out_dim]
    psi = np.maximum((lam - 1.0) / n0, 0.0)
    return mean, np.ascontiguousarray(p @ u), np.ascontiguousarray(psi)


def coefficients(psi, n):
    """(alpha [dim], beta [dim], gamma [dim], c) of the LLR of a model of n utterances (mean u) against a test utterance v:
        llr = sum_k [ alpha_k u_k v_k - 1/2 beta_k v_k^2 - 1/2 gamma_k u_k^2 ] + c
        alpha = n psi / d1,  beta = n psi^2 / (d1 d3),  gamma = n^2 psi^2 / (d1 d2),  c = -1/2 sum_k log(d1 / (d2 d3))
        d1 = (n + 1) psi + 1,  d2 = n psi + 1,  d3 = psi + 1
    (log(d1 / (d2 d3)) = log((d1 / n)) - log(psi + 1 / n) - log(psi + 1), the by-the-book form; here as log1p, which keeps
    its accuracy for small psi.)  NumPy float64; psi = 0 gives exact zeros."""
    psi = _checked_psi(psi)
    n = float(n)
    if not n >= 1:
        raise ValueError("a model holds at least one utterance, got n = %r" % (n,))
    d1, d2, d3 = (n + 1.0) * psi + 1.0, n * psi + 1.0, psi + 1.0
    alpha = n * psi / d1
    return alpha, alpha * psi / d3, alpha * n * psi / d2, float(-0.5 * np.log1p(-(n * psi * psi) / (d2 * d3)).sum())


def _checked_psi(psi):
    psi = np.ascontiguousarray(psi, dtype=np.float64).reshape(-1)
    if not (np.isfinite(psi).all() and (psi >= 0).all()):
        raise ValueError("psi must be finite and >= 0")
    return psi


def _checked_counts(counts, n_rows):
    """counts as int32 [n_rows] after the host check (>= 1), or None.  A device tensor is read back once for it."""
    if counts is None:
        return None
    host = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts).reshape(-1)
    if host.size != n_rows:
        raise ValueError("counts holds one entry per enrolled row (%d), got %d" % (n_rows, host.size))
    if host.size and not (host >= 1).all():
        raise ValueError("every enrolled model holds at least one utterance (counts >= 1)")
    return counts if hasattr(counts, "cpu") else host.astype(np.int32)


class Plda:
    """A fitted PLDA model.  `fit` on labelled development embeddings (after the back end, if there is one), `project` both
    sides of a trial, `enroll` speaker models, `score` / `score_trials` the projected rows;
    `VerificationPipeline(..., plda=p)` and `evaluation.evaluate_trials(..., plda=p)` do the projecting themselves."""

    def __init__(self, mean=None, v=None, psi=None, l2_in=True, shrinkage=0.0):
        self.mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.v = None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        self.psi = None if psi is None else _checked_psi(psi)
        if (self.mean is None) != (self.v is None) or (self.mean is None) != (self.psi is None):
            raise ValueError("mean, v and psi come together")
        if self.mean is not None and (self.v.ndim != 2 or self.v.shape != (self.mean.size, self.psi.size)):
            raise ValueError("v wants (dim, out_dim) with one row per entry of mean and one column per entry of psi")
        self.l2_in, self.shrinkage = bool(l2_in), float(shrinkage)
        self._device = {}

    @property
    def dim(self):
        return None if self.mean is None else int(self.mean.size)

    @property
    def out_dim(self):
        return None if self.psi is None else int(self.psi.size)

    def _fitted(self):
        if self.mean is None:
            raise RuntimeError("the PLDA model is not fitted")

    def _held(self, eng):
        """(mean f32, V f32, psi f64) on eng's device, uploaded once per device."""
        held = self._device.get(eng.device_index)
        if held is None:
            held = self._device[eng.device_index] = (eng.to_device(self.mean.astype(np.float32)),
                                                     eng.to_device(self.v.astype(np.float32)), eng.to_device(self.psi))
        return held

    def fit(self, embeddings, speaker_ids, out_dim=None, l2_in=True, shrinkage=1e-3, engine=None):
        """Class statistics of embeddings [n, dim] (device tensor or array) under speaker_ids [n] on the device, then
        `solve_plda`.  l2_in: rows are L2-normalised before the statistics -- and in `project`.  Returns self."""
        mean, v, psi = solve_plda(*class_statistics(embeddings, speaker_ids, l2_in, engine), out_dim=out_dim, shrinkage=shrinkage)
        self.mean, self.v, self.psi, self.l2_in, self.shrinkage = mean, v, _checked_psi(psi), bool(l2_in), float(shrinkage)
        self._device = {}
        return self

    def project(self, emb, engine=None):
        """[n, dim] -> u = V^T (l2(x) - mean) as float32 [n, out_dim] on the device through svk_embedding_project (flag bit 0 =
        l2_in, no length norm afterwards: the model's scale lives in u); mean and V are cast to f32 once per device."""
        from .engine import get_engine
        self._fitted()
        eng = engine or get_engine()
        held = self._held(eng)
        return eng.embedding_project(emb, mean=held[0], w=held[1], l2_in=self.l2_in, l2_out=False)

    def enroll(self, emb, speaker_ids, projected=False, engine=None):
        """Speaker models: the mean of each speaker's projected utterances (svk_embedding_pool over `speaker_segments`, no
        length norm) -> (sorted unique ids, models float32 [S, out_dim] on the device, counts int32 [S] on the device).  emb:
        raw rows [n, dim], projected here, or with projected=True rows that `project` returned."""
        import torch
        from .engine import get_engine
        from .pipeline import speaker_segments
        self._fitted()
        eng = engine or get_engine()
        uniq, seg_start, row_index = speaker_segments(speaker_ids)
        if int(row_index.size) != int(emb.shape[0]):
            raise ValueError("enroll wants one speaker id per row")
        rows = eng.to_device(emb, torch.float32) if projected else self.project(emb, engine=eng)
        if rows.dim() != 2 or int(rows.shape[1]) != self.out_dim:
            raise ValueError("enroll wants projected rows of %d columns, got %s" % (self.out_dim, tuple(rows.shape)))
        models = eng.embedding_pool(rows, seg_start=seg_start, row_index=row_index)
        return uniq, models, eng.to_device(np.diff(seg_start).astype(np.int32))

    def score(self, test_u, enroll_u, counts=None, engine=None):
        """LLR of every projected test row against every enrolled model -> float32 [n_test, n_enroll] on the device.  counts:
        the utterances behind each model (`enroll`), None = one each."""
        from .engine import get_engine
        self._fitted()
        eng = engine or get_engine()
        return eng.plda_scores(test_u, enroll_u, self._held(eng)[2], counts=_checked_counts(counts, int(enroll_u.shape[0])))

    def score_trials(self, u_a, idx_a, idx_b, u_b=None, counts_b=None, bad_count=None, engine=None):
        """One LLR per trial: the test row u_a[idx_a[p]] against the model u_b[idx_b[p]] (u_b = u_a when not given) of
        counts_b[idx_b[p]] utterances -> float32 [n_trials] on the device (svk_plda_pair_scores)."""
        from .engine import get_engine
        self._fitted()
        eng = engine or get_engine()
        u_b = u_a if u_b is None else u_b
        return eng.plda_pair_scores(u_a, u_b, idx_a, idx_b, self._held(eng)[2],
                                    counts_b=_checked_counts(counts_b, int(u_b.shape[0])), bad_count=bad_count)

    def save(self, path):
        """An .npz of the float64 mean, V and psi plus the settings."""
        self._fitted()
        with open(path, "wb") as fh:
            np.savez(fh, mean=self.mean, v=self.v, psi=self.psi, l2_in=np.array(self.l2_in), shrinkage=np.array(self.shrinkage))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(mean=z["mean"], v=z["v"], psi=z["psi"], l2_in=bool(z["l2_in"]), shrinkage=float(z["shrinkage"]))
