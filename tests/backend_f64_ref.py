"""High-precision restatements, derived bounds and shared cases for the back-end kernels svk_class_scatter,
svk_embedding_project (csrc/backend.hip) and svk_embedding_pool (csrc/pool.hip).  The GPU tests (test_class_scatter*.py,
test_embedding_project*.py, test_embedding_pool*.py) and the host test of the checks (test_backend_checks_host.py) share what
is here, so that a check which passes on the device is the check that was shown, without a device, to be able to fail.

THE BOUNDS (derived in the docstrings of test_class_scatter.py, test_embedding_project.py, test_embedding_pool.py):
  * class means:  (n_c + 2) u mean|x|, u = 2^-53, x the row as it enters;
  * S_w:          (2 n_max + 8) u sum (|x_a| + |m_a|)(|x_b| + |m_b|);
  * projection:   (dim + 8) 2^-24 sum_k (|x'_k| + |mu_k|) |W_kj|;
  * l2_out, pool: float32(ref64) or the float next to it."""
import numpy as np

U = 2.0 ** -53


def rows(n, dim, seed):
    return (np.random.default_rng(seed).standard_normal((n, dim)) + 3.0).astype(np.float32)


def chunk_rows(dim):
    """Rows of the effective sequence per partial matrix of svk_class_scatter: a function of dim alone."""
    return 4 * max(16 * ((dim + 15) // 16), 128)


# ---- svk_class_scatter ---------------------------------------------------------------------------------------------------------
def scatter_ref(x, groups, flags):
    """np.longdouble restatement -> (means, sw, bound of the means, bound of sw)."""
    v = x.astype(np.longdouble)
    if flags & 1:
        nrm = np.sqrt((v * v).sum(1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(nrm == 0, np.longdouble(0), v / nrm)
    dim = x.shape[1]
    means = np.zeros((len(groups), dim), dtype=np.longdouble)
    mean_bound = np.zeros((len(groups), dim))
    sw = np.zeros((dim, dim), dtype=np.longdouble)
    mag = np.zeros((dim, dim), dtype=np.longdouble)
    n_max = max(len(g) for g in groups)
    for c, g in enumerate(groups):
        if len(g) == 0:
            continue
        means[c] = v[g].sum(0) / len(g)
        mean_bound[c] = (len(g) + 2) * U * np.abs(v[g]).mean(0).astype(np.float64)
        d = v[g] - means[c]
        sw += d.T @ d
        a = np.abs(v[g]) + np.abs(means[c])
        mag += a.T @ a
    return means, sw, mean_bound, (2 * n_max + 8) * U * mag.astype(np.float64)


def check_scatter(got_mean, got_sw, ref, what):
    """Means and S_w within their bounds of `ref` = scatter_ref(...) -> (worst mean error / bound, worst S_w error / bound),
    printed before anything is asserted.  Where a bound is zero (an empty class; all of S_w when no class has two rows) the
    value must be the reference's exactly."""
    means, sw, mean_bound, sw_bound = ref
    assert got_mean.shape == means.shape and got_sw.shape == sw.shape, "%s: shapes %s, %s" % (what, got_mean.shape, got_sw.shape)
    assert got_mean.dtype == np.float64 and got_sw.dtype == np.float64
    with np.errstate(invalid="ignore"):
        em = np.abs(got_mean.astype(np.longdouble) - means).astype(np.float64)
        es = np.abs(got_sw.astype(np.longdouble) - sw).astype(np.float64)
    rm = float(np.nan_to_num(em / np.maximum(mean_bound, 1e-300), nan=np.inf).max())
    rs = float(np.nan_to_num(es / np.maximum(sw_bound, 1e-300), nan=np.inf).max())
    print("%s: worst mean error / bound = %.3f, worst S_w error / bound = %.4f" % (what, rm, rs))
    bad_m, bad_s = ~(em <= mean_bound), ~(es <= sw_bound)
    assert not bad_m.any(), "%s: %d class means outside the bound" % (what, int(bad_m.sum()))
    assert not bad_s.any(), "%s: %d entries of S_w outside the bound" % (what, int(bad_s.sum()))
    return rm, rs


def check_symmetric(sw, what):
    assert np.array_equal(sw.view(np.uint64), sw.T.view(np.uint64)), "%s: S_w is not symmetric bit for bit" % what


def same_bytes(a, b, what):
    """Bit-for-bit equality of two float arrays (a NaN equals itself, -0.0 differs from +0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s %s against %s %s" % (what, a.shape, a.dtype, b.shape, b.dtype)
    ua, ub = a.view("u%d" % a.itemsize), b.view("u%d" % b.itemsize)
    diff = np.flatnonzero(ua.reshape(-1) != ub.reshape(-1))
    assert diff.size == 0, "%s: %d of %d elements differ in their bits, the first at flat index %d" % (what, diff.size, ua.size, diff[0])


def all_plus_zero(a, what):
    """Every byte of `a` is zero: +0.0 everywhere (no -0.0, nothing left unwritten)."""
    a = np.ascontiguousarray(a)
    assert not a.view(np.uint8).any(), "%s: %d elements are not +0.0" % (what, int((a.view("u%d" % a.itemsize) != 0).sum()))


def check_additive(sw_joint, sw_first, sw_added, what):
    """S_w(first + added) == S_w(first) + S_w(added) as one float64 addition per entry, bit for bit: `added` is one chunk that
    follows the chunks of `first`, and the partials are added in chunk order from +0.0."""
    same_bytes(sw_joint, sw_first + sw_added, what)


def csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def groups_of(start, index):
    """The row numbers of every class: index[start[c] : start[c + 1]]."""
    return [index[start[c]:start[c + 1]] for c in range(len(start) - 1)]


class ScatterCase:
    """Rows N(0, 1) + 3, CSR classes of `lengths`, `outside` further rows in no class, a seeded shuffled row index."""

    def __init__(self, name, dim, lengths, seed, outside=0):
        self.name, self.dim, self.lengths = name, int(dim), [int(n) for n in lengths]
        self.start = csr(self.lengths)
        self.n_rows = int(self.start[-1]) + outside
        self.x = rows(self.n_rows, self.dim, seed)
        self.index = np.random.default_rng(seed + 1000).permutation(self.n_rows).astype(np.int64)
        self.groups = groups_of(self.start, self.index)
        self.outside_rows = self.index[int(self.start[-1]):]
        self._ref = {}

    def ref(self, flags):
        """scatter_ref, computed once per flag value and shared (never modified)."""
        if flags not in self._ref:
            self._ref[flags] = scatter_ref(self.x, self.groups, flags)
        return self._ref[flags]


CARRY_FORCED = (1023, 1024, 1025, 2047, 2048, 2099)       # the classes around the scan's blocks of 1 024, and the last


def carry_case():
    """2 100 classes (two full scan blocks and a ragged third) of 0, 1, 2, 3 or 5 rows at dim 40, three rows outside."""
    lengths = np.random.default_rng(77).choice([0, 1, 2, 3, 5], size=2100)
    lengths[list(CARRY_FORCED)] = 3
    return ScatterCase("carry", 40, lengths, 11, outside=3)


LONG_LENGTHS = [3, 1100, 0, 1, 433, 512, 2]               # dim 40, chunk 512: 2 050 effective rows in five chunks
WIDE_LENGTHS = [7, 600, 1, 569, 130]                      # dim 130, chunk 576: 1 306 effective rows, chunks 576 + 576 + 154
EDGE_LENGTHS = [5, 0, 1, 9, 2]
EDGE_DIMS = (1, 15, 16, 17, 129, 512)


def long_case():
    return ScatterCase("long class", 40, LONG_LENGTHS, 21)


def wide_case():
    return ScatterCase("wide staging", 130, WIDE_LENGTHS, 31)


def edge_case(dim):
    return ScatterCase("dim %d" % dim, dim, EDGE_LENGTHS, 41 + dim)


# ---- svk_embedding_pool --------------------------------------------------------------------------------------------------------
def pool_ref(x, groups, flags):
    """float64 restatement: groups = a list of row-index arrays."""
    x = x.astype(np.float64)
    out = np.zeros((len(groups), x.shape[1]))
    for s, rows in enumerate(groups):
        if len(rows) == 0:
            continue
        v = x[rows]
        if flags & 1:
            nrm = np.sqrt((v * v).sum(1, keepdims=True))
            with np.errstate(invalid="ignore", divide="ignore"):
                v = np.where(nrm == 0, 0.0, v / nrm)
        m = v.sum(0) / len(rows)
        if flags & 2:
            nrm = np.sqrt((m * m).sum())
            m = m if nrm == 0 else m / nrm
        out[s] = m
    return out


def assert_f32_or_neighbour(got, ref64, what):
    want = ref64.astype(np.float32)
    ok = (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    ok |= np.isnan(got) & np.isnan(want)
    exact = float((got == want).mean())
    print("%s: %d values, %.4f equal float32(ref64), worst |got - ref64| / ulp = %.3f"
          % (what, got.size, exact, float(np.nanmax(np.abs(got.astype(np.float64) - ref64) / np.maximum(np.spacing(np.abs(want)), 1e-45)))))
    assert ok.all(), "%s: %d values are neither float32(ref64) nor its neighbour" % (what, int((~ok).sum()))


POOL_LENGTHS = [1, 2, 5, 0, 64, 65, 130]                  # 267 rows: an empty segment, the 64-row block full, crossed, crossed twice
POOL_DIMS = (256, 257, 260, 1024, 1028, 4096)             # one chunk per thread | four | four | four | sixteen | sixteen


# ---- svk_embedding_project -----------------------------------------------------------------------------------------------------
def l2_f32(x):
    """x' = float32(x / ||x||), norm and division in float64; a zero row stays zero."""
    x64 = x.astype(np.float64)
    nrm = np.sqrt((x64 * x64).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(nrm == 0, 0.0, x64 / nrm).astype(np.float32)


def project_ref(x, mu, w, flags):
    """float64 restatement of the un-normalised output -> (y, bound)."""
    dim = x.shape[1]
    xp = (l2_f32(x) if flags & 1 else x).astype(np.float64)
    mu64 = np.zeros(dim) if mu is None else mu.astype(np.float64)
    w64 = w.astype(np.float64)
    return (xp - mu64) @ w64, (dim + 8) * 2.0 ** -24 * ((np.abs(xp) + np.abs(mu64)) @ np.abs(w64))


def unit_rows(y):
    y64 = y.astype(np.float64)
    nrm = np.sqrt((y64 * y64).sum(1, keepdims=True))
    return y64 / np.where(nrm == 0, 1.0, nrm)
