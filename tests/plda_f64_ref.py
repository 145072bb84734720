"""Float64 restatement of PLDA scoring (csrc/plda.hip, speaker_verification_amd/plda.py) for the tests.  NumPy float64 and
nothing from the library under test.

The model: a projected utterance is u = y + e, y ~ N(0, diag psi) (speaker), e ~ N(0, I) (session).  An enrolled model is the
mean of n projected utterances, a test utterance is v.

  llr        the by-the-book closed form, written as the issue states it (three logarithms per direction)
  llr_joint  the same quantity from the two joint Gaussian log-densities of (model, test) with slogdet and solve: the
             same-speaker covariance is [[psi + I / n, psi], [psi, psi + I]], the different-speaker one its block diagonal
  operands   the float64 operands a, b and the terms s, t of svk_plda_scores' contract, BEFORE any rounding to f32
"""
import numpy as np

U32 = 2.0 ** -24                   # float32 unit roundoff


def coef(psi, n):
    """(alpha, beta, gamma [.., dim], log terms [.., dim, 3]) for psi [dim] and n scalar or [m] (-> leading axis m).
    c(n) = -1/2 sum_k (logs[k, 0] - logs[k, 1] - logs[k, 2])."""
    psi = np.asarray(psi, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[..., None]
    d1 = (n + 1.0) * psi + 1.0
    alpha = n * psi / d1
    beta = n * psi ** 2 / (d1 * (psi + 1.0))
    gamma = n ** 2 * psi ** 2 / (d1 * (n * psi + 1.0))
    logs = np.stack([np.log(d1 / n), np.log(psi + 1.0 / n), np.log(psi + 1.0) + 0.0 * n], axis=-1)
    return alpha, beta, gamma, logs


def llr(test, enroll, psi, counts=None):
    """-> (scores float64 [nt, ne], sum of |terms| [nt, ne]): every test row v against every enrolled row u of counts[j]
    utterances (None: 1).  The terms are the 6 dim summands alpha u v, beta v^2 / 2, gamma u^2 / 2 and the three half
    logarithms per direction."""
    v = np.asarray(test).astype(np.float64)
    u = np.asarray(enroll).astype(np.float64)
    n = np.ones(u.shape[0]) if counts is None else np.asarray(counts, dtype=np.float64)
    alpha, beta, gamma, logs = coef(psi, n)                          # [ne, dim]
    c = -0.5 * (logs[..., 0] - logs[..., 1] - logs[..., 2]).sum(-1)    # [ne]
    cross = v @ (alpha * u).T
    quad_v = 0.5 * (v * v) @ beta.T
    quad_u = 0.5 * (gamma * u * u).sum(1)
    score = cross - quad_v - quad_u[None, :] + c[None, :]
    mag = np.abs(v) @ np.abs(alpha * u).T + quad_v + quad_u[None, :] + 0.5 * np.abs(logs).sum((-1, -2))[None, :]
    return score, mag


def llr_pairs(a, b, idx_a, idx_b, psi, counts_b=None):
    """The trials of a list: a[idx_a[p]] is the test side, b[idx_b[p]] the enrolled side -> (scores [n], sum of |terms| [n])."""
    v = np.asarray(a).astype(np.float64)[idx_a]
    u = np.asarray(b).astype(np.float64)[idx_b]
    n = np.ones(len(idx_b)) if counts_b is None else np.asarray(counts_b, dtype=np.float64)[idx_b]
    alpha, beta, gamma, logs = coef(psi, n)
    terms = np.concatenate([alpha * u * v, -0.5 * beta * v * v, -0.5 * gamma * u * u,
                            -0.5 * logs[..., 0], 0.5 * logs[..., 1], 0.5 * logs[..., 2]], axis=1)
    return terms.sum(1), np.abs(terms).sum(1)


def llr_joint(u, n, v, psi):
    """One model (mean u of n utterances) against one test utterance v, from the joint Gaussian log-densities."""
    psi = np.asarray(psi, dtype=np.float64)
    d = psi.size
    p, eye = np.diag(psi), np.eye(d)
    same = np.block([[p + eye / n, p], [p, p + eye]])
    diff = np.block([[p + eye / n, np.zeros((d, d))], [np.zeros((d, d)), p + eye]])
    z = np.concatenate([np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)])

    def logpdf(cov):
        return -0.5 * (np.linalg.slogdet(cov)[1] + z @ np.linalg.solve(cov, z))       # the 2 pi terms cancel
    return logpdf(same) - logpdf(diff)


def operands(test, enroll, psi, counts=None):
    """svk_plda_scores' contract in float64: (a [nt, K], b [ne, K], s [nt], t [ne]) with K = dim (counts None) or 2 dim, so that
    score = a @ b.T + s[:, None] + t[None, :]."""
    v = np.asarray(test).astype(np.float64)
    u = np.asarray(enroll).astype(np.float64)
    n = np.ones(u.shape[0]) if counts is None else np.asarray(counts, dtype=np.float64)
    alpha, beta, gamma, logs = coef(psi, n)
    t = -0.5 * (gamma * u * u).sum(1) - 0.5 * (logs[..., 0] - logs[..., 1] - logs[..., 2]).sum(-1)
    if counts is None:
        return v, alpha * u, -0.5 * (v * v) @ beta[0], t
    return np.concatenate([v, v * v], axis=1), np.concatenate([alpha * u, -0.5 * beta], axis=1), np.zeros(v.shape[0]), t


def matrix_bound(test, enroll, psi, counts, ref, headroom=4):
    """(K + headroom) 2^-24 sum_k |a_k b_k| + 2^-24 |ref| (tests/test_plda_scores.py derives it)."""
    a, b, _, _ = operands(test, enroll, psi, counts)
    return (a.shape[1] + headroom) * U32 * (np.abs(a) @ np.abs(b).T) + U32 * np.abs(ref)


def make_psi(dim, seed):
    """Between-speaker variances spanning 0 .. 300, descending, every fifth one (and the last) exactly 0."""
    rng = np.random.default_rng(seed)
    psi = np.sort(300.0 * rng.random(dim) ** 3)[::-1].copy()
    psi[4::5] = 0.0
    if dim > 1:
        psi[-1] = 0.0
    psi[0] = 300.0
    return psi


def make_rows(n, psi, seed):
    """float32 rows ~ N(0, 1 + psi)."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, psi.size)) * np.sqrt(1.0 + psi)).astype(np.float32)
