"""The embedding back end: what every d-vector / x-vector recipe puts between the network and the cosine scorer.

    fit        labelled development embeddings -> class means and the within-class scatter on the device
               (`svk_class_scatter`, float64, deterministic) -> `solve` on the host (n_class x dim numbers, NumPy float64)
    transform  y = l2((l2(x) - mean) @ W), device to device, one kernel (`svk_embedding_project`)

`solve` needs no GPU; `EmbeddingBackend.transform` has no framework operator in it.  DESIGN 3.11, INTEGRATION "Fitting a
back end".
"""
import numpy as np

METHODS = ("center", "whiten", "wccn", "lda")


def scatter_matrices(class_mean, counts, sw):
    """(global mean [dim], S_w / n, S_b / n) from the class means [n_class, dim], the class sizes and the within-class scatter
    SUM that svk_class_scatter returns; n = the number of rows.  Empty classes (count 0) carry no weight."""
    class_mean = np.asarray(class_mean, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    sw = np.asarray(sw, dtype=np.float64)
    if class_mean.ndim != 2 or counts.size != class_mean.shape[0] or sw.shape != (class_mean.shape[1],) * 2:
        raise ValueError("solve wants class_mean (n_class, dim), counts (n_class,) and sw (dim, dim)")
    n = counts.sum()
    if not (n > 0) or (counts < 0).any():
        raise ValueError("the classes hold no rows")
    used = counts > 0
    if not (np.isfinite(class_mean[used]).all() and np.isfinite(sw).all()):
        raise ValueError("the statistics are not finite (a NaN embedding, or a row index outside the embeddings)")
    mean = (counts[used, None] * class_mean[used]).sum(0) / n
    centred = class_mean[used] - mean
    sb = (counts[used, None] * centred).T @ centred / n
    return mean, sw / n, sb


def _inverse_root(mat, what):
    """V diag(lambda^-1/2), eigenvalues descending; ValueError when `mat` is singular to working precision."""
    lam, vec = np.linalg.eigh((mat + mat.T) / 2.0)
    lam, vec = lam[::-1], vec[:, ::-1]
    if not lam[0] > 0 or lam[-1] <= lam[0] * mat.shape[0] * np.finfo(np.float64).eps:
        raise ValueError("%s is singular (eigenvalues %.3e .. %.3e): fewer independent rows than dimensions -- use shrinkage"
                         % (what, lam[-1], lam[0]))
    return vec / np.sqrt(lam), lam


def solve(class_mean, counts, sw, method, out_dim=None, shrinkage=0.0):
    """The back end's parameters from the class statistics -> (mean float64 [dim], W float64 [dim, out_dim] or None).
    The scatters are divided by the row count and S_w <- S_w + shrinkage tr(S_w) / dim I.
      "center"  W = None
      "whiten"  the eigenvectors of S_t = S_w + S_b scaled by lambda^-1/2, the out_dim largest:  W^T S_t W = I
      "wccn"    W W^T = S_w^-1 (out_dim = dim)
      "lda"     whiten S_w with P, eigendecompose P^T S_b P, keep the out_dim <= min(dim, n_class - 1) leading directions:
                W^T S_w W = I, W^T S_b W = diag(the leading generalised eigenvalues)
    ValueError: non-finite statistics, a singular matrix (S_w without shrinkage on too few rows), out_dim out of range."""
    if method not in METHODS:
        raise ValueError("method must be one of %r, got %r" % (METHODS, method))
    if not (np.isfinite(shrinkage) and shrinkage >= 0):
        raise ValueError("shrinkage must be a finite number >= 0")
    mean, s_w, s_b = scatter_matrices(class_mean, counts, sw)
    dim = int(mean.size)
    n_class = int((np.asarray(counts).reshape(-1) > 0).sum())
    s_w = s_w + shrinkage * np.trace(s_w) / dim * np.eye(dim)
    limit = {"center": dim, "whiten": dim, "wccn": dim, "lda": min(dim, n_class - 1)}[method]
    if out_dim is None:
        out_dim = limit
    out_dim = int(out_dim)
    if out_dim < 1 or out_dim > limit or (method in ("center", "wccn") and out_dim != dim):
        raise ValueError("out_dim = %d is out of range for %r (dim %d, %d classes: at most %d)" % (out_dim, method, dim, n_class, limit))
    if method == "center":
        return mean, None
    if method == "whiten":
        w, _ = _inverse_root(s_w + s_b, "S_t")
        return mean, np.ascontiguousarray(w[:, :out_dim])
    p, _ = _inverse_root(s_w, "S_w")
    if method == "wccn":
        return mean, np.ascontiguousarray(p)
    lam, u = np.linalg.eigh(p.T @ s_b @ p)
    return mean, np.ascontiguousarray(p @ u[:, ::-1][:, :out_dim])


def class_statistics(embeddings, speaker_ids, l2_in, engine):
    """(class_mean [n_class, dim], counts [n_class], sw [dim, dim]) of embeddings [n, dim] (device tensor or array) under
    speaker_ids [n]: svk_class_scatter on the device (engine None: the current device's), as NumPy float64 (counts int64)."""
    from .engine import get_engine
    from .pipeline import speaker_segments
    uniq, seg_start, row_index = speaker_segments(speaker_ids)
    if int(row_index.size) != int(embeddings.shape[0]):
        raise ValueError("fit wants one speaker id per embedding row")
    class_mean, sw = (engine or get_engine()).class_scatter(embeddings, seg_start, row_index=row_index, l2_rows=l2_in)
    return class_mean.cpu().numpy(), np.diff(seg_start), sw.cpu().numpy()


class EmbeddingBackend:
    """A fitted back end.  `fit` on labelled development embeddings, `transform` anything scored afterwards (both sides of a
    trial); `VerificationPipeline(..., backend=b)` and `evaluation.evaluate_trials(..., backend=b)` do the latter themselves."""

    def __init__(self, mean=None, w=None, l2_in=True, l2_out=True, method=None, shrinkage=0.0):
        self.mean = None if mean is None else np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        self.w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        if self.w is not None and (self.w.ndim != 2 or self.mean is None or self.w.shape[0] != self.mean.size):
            raise ValueError("w wants (dim, out_dim) with one row per entry of mean")
        self.l2_in, self.l2_out, self.method, self.shrinkage = bool(l2_in), bool(l2_out), method, float(shrinkage)
        self._device = {}

    @property
    def dim(self):
        return None if self.mean is None else int(self.mean.size)

    @property
    def out_dim(self):
        return self.dim if self.w is None else int(self.w.shape[1])

    def fit(self, embeddings, speaker_ids, method="lda", out_dim=None, l2_in=True, shrinkage=1e-3, engine=None):
        """Class statistics of embeddings [n, dim] (device tensor or array) under speaker_ids [n] on the device, then `solve`.
        l2_in: rows are L2-normalised before the statistics -- and in `transform`.  engine: the `Engine` (device) to run on,
        default the current device's.  Returns self."""
        mean, w = solve(*class_statistics(embeddings, speaker_ids, l2_in, engine), method, out_dim=out_dim, shrinkage=shrinkage)
        self.mean, self.w, self.l2_in, self.method, self.shrinkage = mean, w, bool(l2_in), method, float(shrinkage)
        self._device = {}
        return self

    def transform(self, emb, l2_out=None, engine=None):
        """[n, dim] -> float32 [n, out_dim] on the device through svk_embedding_project; mean and W are cast to f32 once per
        device.  l2_out: None = the instance's setting (True unless constructed otherwise).  engine: the `Engine` to run on
        (a pipeline passes its own), default the current device's."""
        from .engine import get_engine
        if self.mean is None:
            raise RuntimeError("the back end is not fitted")
        eng = engine or get_engine()
        held = self._device.get(eng.device_index)
        if held is None:
            held = self._device[eng.device_index] = (
                eng.to_device(self.mean.astype(np.float32)),
                None if self.w is None else eng.to_device(self.w.astype(np.float32)))
        return eng.embedding_project(emb, mean=held[0], w=held[1], l2_in=self.l2_in,
                                     l2_out=self.l2_out if l2_out is None else l2_out)

    def save(self, path):
        """An .npz of the float64 mean and W plus the settings (an empty W stands for None)."""
        if self.mean is None:
            raise RuntimeError("the back end is not fitted")
        with open(path, "wb") as fh:
            np.savez(fh, mean=self.mean, w=np.zeros((self.dim, 0)) if self.w is None else self.w,
                     has_w=np.array(self.w is not None), l2_in=np.array(self.l2_in), l2_out=np.array(self.l2_out),
                     method=np.array("" if self.method is None else self.method), shrinkage=np.array(self.shrinkage))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(mean=z["mean"], w=z["w"] if bool(z["has_w"]) else None, l2_in=bool(z["l2_in"]), l2_out=bool(z["l2_out"]),
                       method=str(z["method"]) or None, shrinkage=float(z["shrinkage"]))
