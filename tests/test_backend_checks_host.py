"""The checks of the back-end path tests, run without a GPU: a NumPy float64 emulation of the order DESIGN 3.11 and pool.hip
document -- the effective row sequence (classes of two rows or more), chunks of chunk_rows(dim) rows, the chunks' partial
matrices added in chunk order from +0.0, means and pooled sums in blocks of 64 rows -- goes through the checker functions of
tests/backend_f64_ref.py on the cases of test_class_scatter_paths.py and test_embedding_pool_paths.py, and passes.  Three
deliberately wrong emulations must be REJECTED by the same checkers: classes behind index 1 024 lose their offset in the
effective sequence (a scan without its carry), the last chunk's partial is not added, the second tile group stays zero.  So the
checks can fail, and the longdouble bounds are not vacuous at a 1 100-row class."""
import numpy as np
import pytest

import backend_f64_ref as R       # (tests/ is on sys.path)


def entered_rows(x, flags):
    v = x.astype(np.float64)
    if flags & 1:
        nrm = np.sqrt((v * v).sum(1, keepdims=True))
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(nrm == 0, 0.0, v / nrm)
    return v


def block_sum(v):
    """Rows added in order inside blocks of 64, the blocks' sums added in order."""
    acc = np.zeros(v.shape[1])
    for b in range(0, len(v), 64):
        part = np.zeros(v.shape[1])
        for r in v[b:b + 64]:
            part = part + r
        acc = acc + part
    return acc


def emulate_scatter(x, start, index, flags, no_carry=False, drop_last_chunk=False, skip_second_group=False):
    """-> (means, S_w) in float64, in the documented order; the three keywords are the three wrong kernels."""
    n_class, dim = len(start) - 1, x.shape[1]
    v = entered_rows(x, flags)
    means = np.zeros((n_class, dim))
    for c in range(n_class):
        g = index[start[c]:start[c + 1]]
        if len(g):
            means[c] = block_sum(v[g]) / len(g)
    count = np.diff(start)
    count = np.where(count >= 2, count, 0)
    eff = np.concatenate([[0], np.cumsum(count)])
    if no_carry:                                         # every block of 1 024 classes scans from zero
        for base in range(1024, n_class, 1024):
            eff[base + 1:base + 1025] = np.cumsum(count[base:base + 1024])
    total, chunk = int(eff[n_class]), R.chunk_rows(dim)
    nb = (dim + 15) // 16
    computed = np.zeros((16 * nb, 16 * nb), dtype=bool)   # the upper-triangle tiles, ids row-major, 36 to a group
    tile = 0
    for a in range(nb):
        for b in range(a, nb):
            if not (skip_second_group and 36 <= tile < 72):
                computed[16 * a:16 * a + 16, 16 * b:16 * b + 16] = True
            tile += 1
    computed = computed[:dim, :dim]
    n_chunks = -(-total // chunk) - (1 if drop_last_chunk else 0)
    sw = np.zeros((dim, dim))
    for k in range(n_chunks):
        d = np.zeros((min(chunk, total - k * chunk), dim))
        for j, pos in enumerate(range(k * chunk, min((k + 1) * chunk, total))):
            lo, hi = 0, n_class                          # the first class whose effective range ends behind pos
            while lo < hi:
                mid = (lo + hi) // 2
                if eff[mid + 1] <= pos:
                    lo = mid + 1
                else:
                    hi = mid
            i = int(start[lo] + pos - eff[lo])
            d[j] = v[index[i]] - means[lo] if 0 <= i < len(index) else np.nan
        sw = sw + np.where(computed, d.T @ d, 0.0)
    upper = np.triu(sw)
    return means, upper + np.triu(sw, 1).T


def emulate_case(case, flags, **wrong):
    return emulate_scatter(case.x, case.start, case.index, flags, **wrong)


CASES = {"carry": R.carry_case, "long": R.long_case, "wide": R.wide_case}


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, make in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_documented_order_passes(cases, name):
    case = cases[name]
    for flags in (0, 1):
        mean, sw = emulate_case(case, flags)
        _, rs = R.check_scatter(mean, sw, case.ref(flags), "%s, flags %d (emulated)" % (case.name, flags))
        R.check_symmetric(sw, case.name)
        assert rs < 0.02, "the emulation uses %.3f of the S_w bound: the bound leaves the kernel's order no room" % rs


@pytest.mark.parametrize("dim", R.EDGE_DIMS)
def test_the_edge_dims_pass(dim):
    case = R.edge_case(dim)
    mean, sw = emulate_case(case, 1)
    R.check_scatter(mean, sw, case.ref(1), "%s (emulated)" % case.name)
    R.all_plus_zero(mean[1], "the empty class")


def test_additivity_holds_in_the_documented_order(cases):
    case = cases["long"]
    g = case.groups
    rest = lambda used: np.setdiff1d(np.arange(case.n_rows), used)      # noqa: E731
    _, sw = emulate_case(case, 0)
    _, sw_a = emulate_scatter(case.x, case.start[:6], case.index, 0)
    _, sw_ab1 = emulate_scatter(case.x, case.start[:7], case.index, 0)
    _, sw_b1 = emulate_scatter(case.x, np.array([0, 512]), np.concatenate([g[5], rest(g[5])]), 0)
    _, sw_b2 = emulate_scatter(case.x, np.array([0, 2]), np.concatenate([g[6], rest(g[6])]), 0)
    R.check_additive(sw_ab1, sw_a, sw_b1, "A u B1 (emulated)")
    R.check_additive(sw, sw_ab1, sw_b2, "A u B1 u B2 (emulated)")
    # ... and the checker rejects a result whose last chunk was not added
    _, short = emulate_case(case, 0, drop_last_chunk=True)
    with pytest.raises(AssertionError):
        R.check_additive(short, sw_ab1, sw_b2, "the last chunk missing")


def test_degenerate_totals_pass():
    case = R.ScatterCase("0 or 1 rows", 128, np.random.default_rng(5).choice([0, 1], size=1500, p=[1 / 3, 2 / 3]), 51)
    mean, sw = emulate_case(case, 0)
    R.check_scatter(mean, sw, case.ref(0), "0 or 1 rows (emulated)")
    R.all_plus_zero(sw, "S_w without a class of two rows")
    with pytest.raises(AssertionError):
        R.all_plus_zero(-sw, "-0.0 is not +0.0")
    with pytest.raises(AssertionError):
        R.same_bytes(sw, -sw, "-0.0 against +0.0")


@pytest.mark.parametrize("name,wrong", (("carry", "no_carry"), ("long", "drop_last_chunk"), ("wide", "skip_second_group")))
def test_a_wrong_kernel_is_rejected(cases, name, wrong):
    case = cases[name]
    for flags in (0, 1):
        mean, sw = emulate_case(case, flags, **{wrong: True})
        with pytest.raises(AssertionError, match="S_w outside the bound"):
            R.check_scatter(mean, sw, case.ref(flags), "%s, %s, flags %d" % (case.name, wrong, flags))


def emulate_pool(x, groups, flags):
    v = entered_rows(x, flags)
    out = np.zeros((len(groups), x.shape[1]))
    for s, g in enumerate(groups):
        if len(g) == 0:
            continue
        m = block_sum(v[g]) / len(g)
        if flags & 2:
            nrm = np.sqrt((m * m).sum())
            m = m if nrm == 0 else m / nrm
        out[s] = m
    return out.astype(np.float32)


@pytest.mark.parametrize("dim", (257, 1028))
def test_pooling_in_blocks_of_64_passes(dim):
    start = R.csr(R.POOL_LENGTHS)
    x = R.rows(int(start[-1]), dim, dim)
    groups = R.groups_of(start, np.random.default_rng(dim + 1).permutation(int(start[-1])))
    for flags in range(4):
        got = emulate_pool(x, groups, flags)
        R.assert_f32_or_neighbour(got, R.pool_ref(x, groups, flags), "dim %d flags %d (emulated)" % (dim, flags))
        two_off = np.nextafter(np.nextafter(got, np.float32(np.inf)), np.float32(np.inf))
        with pytest.raises(AssertionError):
            R.assert_f32_or_neighbour(two_off, R.pool_ref(x, groups, flags), "two floats off")
