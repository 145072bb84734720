"""svk_class_scatter (csrc/backend.hip) on the launch paths test_class_scatter.py never reaches: eff_scan_kernel's carry across
blocks of 1 024 classes, a class that spans three chunks, chunk boundaries on class boundaries, an effective row count that is a
multiple of the chunk, scatter_kernel<32> over several chunks with a ragged last stage, chunk slots without an effective row,
an effective total of zero, no rows at all, and the dims at the edges of a tile, of the wide instance and of the ABI.

Every case: means and S_w within the bounds of tests/backend_f64_ref.py against its np.longdouble restatement (the bounds are
the ones test_class_scatter.py derives; they are a function of the class lengths, so a 1 100-row class has its own, wider S_w
bound: a float64 emulation of the documented chunk order stays below 0.02 of it), S_w symmetric bit for bit, two runs the same
bytes, the worst error / bound printed.  The properties asserted on BITS are the ones include/svk.h and DESIGN 3.11 state: a mean
depends on its own class alone; empty and one-row classes move no chunk boundary; partials are added in chunk order from +0.0;
zero padding changes no bit; NaN stays in its row and column.

Several chunks at dim 512 would need 2 049 or more rows and a longdouble reference that takes tens of seconds: left out on
purpose.  Dim 512 runs in one chunk (17 rows), which is what reaches its 15th tile group and its 32 896 bytes of dynamic LDS
(measured: the launch gets them without an opt-in).

Measured on the MI355X, worst error / bound: S_w 0.016 (carry), 0.0001 (long class), 0.0004 (dim 130), 0.0067 (dim 512), 0.025
(host chain); means 0.13 with flag bit 0 clear; with it set 0.70 (carry) and 0.98 for the one-row classes of the surplus-slot
case, whose bound is 3 u |x| and whose error is that of the row's float64 norm (16 lanes, eight squares each, four butterfly
steps, a square root and a division)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import backend_f64_ref as R       # noqa: E402  (tests/ is on sys.path)


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def run(eng, x, start, index=None, flags=0):
    mean, sw = eng.class_scatter(x, np.asarray(start, dtype=np.int64), row_index=index, l2_rows=bool(flags & 1))
    return mean.cpu().numpy(), sw.cpu().numpy()


def run_case(eng, case, flags, dev=None):
    """The case through the kernel, held to what every case asserts -> (means, S_w)."""
    what = "%s, flags %d" % (case.name, flags)
    dev = eng.to_device(case.x) if dev is None else dev
    mean, sw = run(eng, dev, case.start, case.index, flags)
    R.check_scatter(mean, sw, case.ref(flags), what)
    R.check_symmetric(sw, what)
    mean2, sw2 = run(eng, dev, case.start, case.index, flags)
    R.same_bytes(mean2, mean, what + ": the means of a second run")
    R.same_bytes(sw2, sw, what + ": S_w of a second run")
    return mean, sw


def test_carry_across_scan_blocks(eng):
    """2 100 classes: eff_scan_kernel runs three blocks of 1 024 and carries the running total twice."""
    case = R.carry_case()
    assert len(case.lengths) == 2100 and len(case.outside_rows) == 3 and all(case.lengths[c] == 3 for c in R.CARRY_FORCED)
    dev = eng.to_device(case.x)
    for flags in (0, 1):
        mean, sw = run_case(eng, case, flags, dev)
        # 1. the classes around the blocks' edges alone, their own rows in the same order: the mean bits they have in the batch
        for c in R.CARRY_FORCED:
            alone, _ = run(eng, case.x[case.groups[c]], [0, 3], None, flags)
            R.same_bytes(alone[0], mean[c], "class %d alone, flags %d" % (c, flags))
        # 2. 1 024 empty classes in front, the three outside rows as one-row classes at the start, in the middle and at the end:
        #    every contributing class now lies behind the first carry, and no chunk boundary moved
        extra = {0: case.outside_rows[0:1], 1050: case.outside_rows[1:2], 2100: case.outside_rows[2:3]}
        groups, kept = [np.zeros(0, dtype=np.int64)] * 1024, []
        for c in range(2101):
            if c in extra:
                groups.append(extra[c])
            if c < 2100:
                kept.append(len(groups))
                groups.append(case.groups[c])
        assert len(groups) == 1024 + 2100 + 3
        index2 = np.concatenate(groups).astype(np.int64)
        assert index2.size == case.n_rows
        mean_b, sw_b = run(eng, dev, R.csr([len(g) for g in groups]), index2, flags)
        R.same_bytes(sw_b, sw, "S_w behind 1 024 empty classes, flags %d" % flags)
        R.same_bytes(mean_b[kept], mean, "the kept classes' means behind 1 024 empty classes, flags %d" % flags)
        R.all_plus_zero(mean_b[:1024], "the means of the empty classes")
        # 3. the same rows gathered contiguously, no row index
        mean_c, sw_c = run(eng, case.x[case.index], case.start, None, flags)
        R.same_bytes(sw_c, sw, "S_w of the gathered rows, flags %d" % flags)
        R.same_bytes(mean_c, mean, "means of the gathered rows, flags %d" % flags)


def test_class_longer_than_a_chunk_and_coinciding_boundaries(eng):
    """dim 40 (chunk 512), lengths [3, 1100, 0, 1, 433, 512, 2]: the 1 100-row class spans chunks 0 - 2, chunk 2 ends with the
    433-row class, the 512-row class is chunk 3 exactly, the last chunk holds 2 rows."""
    case = R.long_case()
    assert R.chunk_rows(case.dim) == 512 and sum(n for n in case.lengths if n >= 2) == 2050
    dev = eng.to_device(case.x)
    g = case.groups
    rest = lambda used: np.setdiff1d(np.arange(case.n_rows), used)      # noqa: E731
    for flags in (0, 1):
        mean, sw = run_case(eng, case, flags, dev)
        mean_a, sw_a = run(eng, dev, case.start[:6], case.index, flags)                       # A: up to the 433-row class
        mean_ab1, sw_ab1 = run(eng, dev, case.start[:7], case.index, flags)                   # A and B1: 2 048 rows, four full chunks
        _, sw_b1 = run(eng, dev, [0, 512], np.concatenate([g[5], rest(g[5])]).astype(np.int64), flags)
        _, sw_b2 = run(eng, dev, [0, 2], np.concatenate([g[6], rest(g[6])]).astype(np.int64), flags)
        R.same_bytes(mean_a, mean[:5], "means of A, flags %d" % flags)
        R.same_bytes(mean_ab1, mean[:6], "means of A and B1, flags %d" % flags)
        R.check_additive(sw_ab1, sw_a, sw_b1, "S_w(A u B1) == S_w(A) + S_w(B1), flags %d" % flags)
        R.check_additive(sw, sw_ab1, sw_b2, "S_w(A u B1 u B2) == S_w(A u B1) + S_w(B2), flags %d" % flags)


def test_wide_staging_over_several_chunks(eng):
    """dim 130: nb = 9, chunk 576, 45 tiles in two groups, 8 rows per stage; 1 306 effective rows are chunks of 576, 576 and 154
    (19 stages and a quarter)."""
    case = R.wide_case()
    assert R.chunk_rows(130) == R.chunk_rows(132) == 576 and sum(n for n in case.lengths if n >= 2) == 1306
    padded = np.zeros((case.n_rows, 132), dtype=np.float32)
    padded[:, :130] = case.x
    clean = {}
    for flags in (0, 1):
        mean, sw = clean[flags] = run_case(eng, case, flags)
        # two zero columns: the same tiles and chunks, x + 0 = x
        mean_p, sw_p = run(eng, padded, case.start, case.index, flags)
        R.same_bytes(sw_p[:130, :130], sw, "S_w of the zero-padded rows, flags %d" % flags)
        R.same_bytes(mean_p[:, :130], mean, "means of the zero-padded rows, flags %d" % flags)
        R.all_plus_zero(sw_p[130:], "the padded rows of S_w")
        R.all_plus_zero(sw_p[:, 130:], "the padded columns of S_w")
        R.all_plus_zero(mean_p[:, 130:], "the padded columns of the means")
    # one NaN at column 129 of the 10th row of the last class: effective position 7 + 600 + 569 + 9 = 1 185, in the third chunk
    mean, sw = clean[0]
    x = case.x.copy()
    x[case.groups[4][9], 129] = np.nan
    mean_n, sw_n = run(eng, x, case.start, case.index, 0)
    hit = np.zeros((130, 130), dtype=bool)
    hit[129, :] = hit[:, 129] = True
    assert np.array_equal(np.isnan(sw_n), hit), "NaN outside row and column 129 of S_w, or missing inside"
    R.same_bytes(sw_n[:129, :129], sw[:129, :129], "S_w outside row and column 129")
    hit_m = np.zeros(mean.shape, dtype=bool)
    hit_m[4, 129] = True
    assert np.array_equal(np.isnan(mean_n), hit_m)
    R.same_bytes(mean_n[~hit_m], mean[~hit_m], "the means beside the NaN")


@pytest.mark.parametrize("dim", R.EDGE_DIMS)
def test_dims_at_the_edges(eng, dim):
    """One tile with waves that have no live tile (1, 15, 16, 17); the first dim of the wide instance and of a second tile
    group (129); 528 tiles in 15 groups, the last with 24, and more than 32 KiB of dynamic LDS (512)."""
    case = R.edge_case(dim)
    for flags in (0, 1):
        mean, _ = run_case(eng, case, flags)
        R.all_plus_zero(mean[1], "the empty class's mean")


def test_no_effective_row(eng):
    """(a) 1 500 classes of 0 or 1 rows: the effective total is 0, every launched chunk slot is surplus."""
    lengths = np.random.default_rng(5).choice([0, 1], size=1500, p=[1 / 3, 2 / 3])
    case = R.ScatterCase("0 or 1 rows", 128, lengths, 51)
    assert 900 < case.n_rows < 1100
    one = np.flatnonzero(lengths == 1)
    rows_of = np.array([case.groups[c][0] for c in one])
    for flags in (0, 1):
        mean, sw = run_case(eng, case, flags)
        R.all_plus_zero(sw, "S_w without a class of two rows, flags %d" % flags)
        R.all_plus_zero(mean[lengths == 0], "the means of the empty classes, flags %d" % flags)
        if flags == 0:      # the entered row is the row: its float64 exactly (under bit 0 the norm's bits are the kernel's own)
            R.same_bytes(mean[one], case.x[rows_of].astype(np.float64), "the means of the one-row classes")


def test_no_rows(eng):
    """(b) n_rows == 0 with three classes: no chunk slot is launched at all; means and S_w are zeros."""
    x = np.zeros((0, 128), dtype=np.float32)
    for flags in (0, 1):
        for index in (None, np.zeros(0, dtype=np.int64)):
            mean, sw = run(eng, x, [0, 0, 0, 0], index, flags)
            assert mean.shape == (3, 128) and sw.shape == (128, 128)
            R.all_plus_zero(mean, "means without rows")
            R.all_plus_zero(sw, "S_w without rows")


def test_surplus_chunk_slot(eng):
    """(c) 600 one-row classes, then two classes of 3 rows: 606 rows size two chunk slots, the 6 effective rows use one."""
    case = R.ScatterCase("surplus slot", 128, [1] * 600 + [3, 3], 61)
    assert -(-case.n_rows // R.chunk_rows(128)) == 2
    two = np.concatenate(case.groups[600:])
    for flags in (0, 1):
        mean, sw = run_case(eng, case, flags)
        mean_t, sw_t = run(eng, case.x[two], [0, 3, 6], None, flags)
        R.same_bytes(sw, sw_t, "S_w against the two 3-row classes alone, flags %d" % flags)
        R.same_bytes(mean[600:], mean_t, "the 3-row classes' means, flags %d" % flags)


def test_host_chain(eng):
    """backend.class_statistics (speaker_segments -> Engine.class_scatter) on 1 300 string ids of 2 - 4 rows in shuffled order."""
    from speaker_verification_amd.backend import class_statistics
    rng = np.random.default_rng(71)
    counts = rng.integers(2, 5, size=1300)
    ids = rng.permutation(np.repeat(np.array(["spk%05d" % (7 * s % 1300) for s in range(1300)]), counts))
    x = R.rows(len(ids), 24, 72)
    uniq = np.unique(ids)
    groups = [np.flatnonzero(ids == sid) for sid in uniq]
    for l2 in (False, True):
        mean, got_counts, sw = class_statistics(x, ids, l2, eng)
        assert got_counts.dtype == np.int64 and np.array_equal(got_counts, [len(g) for g in groups])
        R.check_scatter(mean, sw, R.scatter_ref(x, groups, int(l2)), "class_statistics, l2_in %d" % l2)
        R.check_symmetric(sw, "class_statistics")
