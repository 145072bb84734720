"""NumPy restatement of svk_calibration_stats / svk_calibration_apply (include/svk.h), the reference of the calibration tests.

`z_float64` is the header's z_p to the bit: float64 products and sums, each rounded on its own, in the order d = 0, 1, ..,
then the offset, then tau.  The header fixes that arithmetic, so the device and the reference start from the SAME z_p; what the
bounds then measure is everything after it.  (A reference that formed z_p more exactly would be asking for more than any
summation bound covers: sigma(-z) has relative condition |z| in z, so the half-ulp of z's last rounding alone moves a
term by |z| 2^-53 of itself.)

`stats_longdouble`: every term (exp, log1p, the division, the products with the class weight and x) and every sum in
np.longdouble -- the exact values the device's error is measured against -- plus sum_p |term_p| per output for the bound.
`stats_float64`: the same in plain float64 with Engine.calibration_stats' signature and return: the `stats=` provider that
lets Calibration.fit run without a GPU.
"""
import math

import numpy as np

LD = np.longdouble
# the shapes of the GPU tests; the last: 1 465 workgroups, two quads per thread, a ragged tail
SIZES = [1, 3, 4, 5, 255, 256, 257, 3_000_007]
SYSTEMS = [1, 2, 3, 8]


def as_planes(scores):
    if isinstance(scores, (list, tuple)):
        scores = np.stack([np.asarray(s, dtype=np.float32).reshape(-1) for s in scores])
    scores = np.asarray(scores, dtype=np.float32)
    return scores.reshape(1, -1) if scores.ndim == 1 else scores


def z_float64(scores, weights, tau=None):
    """((w_0 s_0 + w_1 s_1) + .. + b) [+ tau], float64, every operation rounded on its own."""
    s = as_planes(scores).astype(np.float64)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    assert w.size == s.shape[0] + 1
    z = w[0] * s[0]
    for d in range(1, s.shape[0]):
        z = z + w[d] * s[d]
    z = z + w[-1]
    return z if tau is None else z + np.float64(tau)


def packed_pairs(dim):
    return [(i, j) for i in range(dim) for j in range(i, dim)]


def _terms(scores, labels, weights, tau, class_weight, ftype):
    """Per-trial terms of every output, columns ordered as h_out: L_tar, L_non, G.., H.. -> (terms [n_out, n_kept], counts)."""
    s = as_planes(scores)
    lab = np.asarray(labels).reshape(-1) != 0
    finite = np.isfinite(s).all(axis=0)
    skipped = int((~finite).sum())
    s, lab = s[:, finite], lab[finite]
    n_sys, n = s.shape
    dim = n_sys + 1
    z = z_float64(s, weights, tau).astype(ftype) if n else np.zeros(0, dtype=ftype)
    x = np.concatenate([s.astype(ftype), np.ones((1, n), dtype=ftype)])
    one = ftype(1)
    e = np.exp(-np.abs(z))
    lp = np.log1p(e)
    q = one / (one + e)
    sig_pos = np.where(z >= 0, q, e * q)            # sigma(z)
    sig_neg = np.where(z >= 0, e * q, q)            # sigma(-z)
    c = np.where(lab, ftype(class_weight[0]), ftype(class_weight[1]))
    cr = c * np.where(lab, -sig_neg, sig_pos)
    ch = c * (sig_pos * sig_neg)
    sp = np.where(lab, np.maximum(-z, 0), np.maximum(z, 0)) + lp
    terms = np.empty((2 + dim + dim * (dim + 1) // 2, n), dtype=ftype)
    terms[0], terms[1] = np.where(lab, sp, 0), np.where(lab, 0, sp)
    np.multiply(cr, x, out=terms[2:2 + dim])
    k = 2 + dim
    for i in range(dim):
        np.multiply(ch * x[i], x[i:], out=terms[k:k + dim - i])
        k += dim - i
    return terms, (int(lab.sum()), int((~lab).sum()), skipped)


def stats_longdouble(scores, labels, weights, tau, class_weight, chunk=1 << 16):
    """-> (values longdouble [n_out], abs_sums longdouble [n_out], counts); the trials go through in chunks (memory)."""
    s, lab = as_planes(scores), np.asarray(labels).reshape(-1)
    dim = s.shape[0] + 1
    values = np.zeros(2 + dim + dim * (dim + 1) // 2, dtype=LD)
    abs_sums, counts = values.copy(), np.zeros(3, dtype=np.int64)
    for lo in range(0, s.shape[1], chunk):
        terms, cnt = _terms(s[:, lo:lo + chunk], lab[lo:lo + chunk], weights, tau, class_weight, LD)
        values += terms.sum(axis=1, dtype=LD)
        abs_sums += np.abs(terms.astype(np.float64)).sum(axis=1)          # the bound's scale: float64 is plenty
        counts += cnt
    return values, abs_sums, tuple(int(v) for v in counts)


def stats_float64(scores, labels, weights, tau, class_weight, value_only=False):
    """Engine.calibration_stats in NumPy float64: (l_tar, l_non, grad, hess, counts)."""
    terms, counts = _terms(scores, labels, weights, tau, class_weight, np.float64)
    flat = terms.sum(axis=1)
    if value_only:
        return float(flat[0]), float(flat[1]), None, None, counts
    dim = as_planes(scores).shape[0] + 1
    hess = np.zeros((dim, dim))
    hess[np.triu_indices(dim)] = flat[2 + dim:]
    hess = hess + np.triu(hess, 1).T
    return float(flat[0]), float(flat[1]), flat[2:2 + dim].copy(), hess, counts


def additions(n):
    """A of the header: the additions on the longest path of svk_calibration_stats' summation order for n trials."""
    def ceil_div(a, b):
        return -(-a // b)
    quads = ceil_div(max(n, 1), 4)
    steps = ceil_div(ceil_div(quads, 256), 2048)            # S: quads per thread
    groups = ceil_div(quads, 256 * steps)                   # W: workgroups = rows of partial sums
    return 4 * steps + 6 + 4 + ceil_div(groups, 16) + 16


def apply_longdouble(scores, weights):
    """-> (ref longdouble [n], abs_sums longdouble [n]): sum_d w_d s_d + b and sum of the |terms|, |b| included."""
    s = as_planes(scores).astype(LD)
    w = np.asarray(weights, dtype=np.float64).astype(LD)
    prod = w[:-1, None] * s
    return prod.sum(axis=0) + w[-1], np.abs(prod).sum(axis=0) + abs(w[-1])


def problem(n, n_sys, seed):
    """Seeded scores [n_sys, n] f32 (targets sit higher), labels in {0, 1, 7}, weights, tau and class weights of a fit at
    p = 0.01: z spreads over about [-15, 8]."""
    rng = np.random.default_rng(seed)
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    labels[(rng.random(n) < 0.3) & (labels != 0)] = 7
    base = np.where(labels != 0, rng.normal(2.0, 1.0, n), rng.normal(-1.0, 1.5, n))
    planes = [base] + [rng.uniform(0.5, 2.0) * base + rng.uniform(-1, 1) + rng.normal(0, 0.5, n) for _ in range(1, n_sys)]
    scores = np.stack(planes).astype(np.float32)
    weights = np.r_[rng.uniform(0.3, 1.5, n_sys) / n_sys, rng.uniform(-1, 1)]
    n_tar = max(1, int((labels != 0).sum()))
    return scores, labels, weights, math.log(0.01 / 0.99), (0.01 / n_tar, 0.99 / max(1, n - n_tar))


def place(eng, planes, stride, offset):
    """The planes on the device, `stride` floats apart, the first `offset` floats into a fresh (256-byte aligned) buffer."""
    import torch
    n_sys, n = planes.shape
    buf = torch.zeros((offset + n_sys * stride + 4,), dtype=torch.float32, device=eng.device)
    view = torch.as_strided(buf, (n_sys, n), (stride, 1), storage_offset=offset)
    view.copy_(torch.from_numpy(planes))
    return view
