"""The feature post-processing kernels of csrc/stages.hip against float64 on every launch path (tests/postproc_f64_ref.py:
references, the derived bars, CPU emulations of the kernels and their mutants).

CPU (default pass):
  * the strided-view cmvnw reference is oracle.speechpy_ref.cmvnw (bit for bit on the centred rows; its second pass is float32);
  * NumPy emulations of cmvn_kernel, cmvnw_kernel and cmvnw_tile_kernel (same order of operations, f32 stores) pass the bars on
    the GPU tests' own inputs, and every mutant of them fails: the bars have teeth;
  * the crop generator restated in Python integers: its mutants differ, its draws are uniform (chi-square);
  * the cmvn_stats inputs keep the one-pass E[x^2] - mean^2 inside the rtol = 1e-12 / 1e-9 bars by themselves.
GPU (-m gpu): each kernel on each path against those references; lines starting with "ULPS" carry the measured worst case.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import postproc_f64_ref as R          # noqa: E402  (tests/ is on sys.path, as for test_c3d2_float64)
from oracle import speechpy_ref as ref   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clip(seed, *shape):
    """Features with mean 2 and std 0.5 .. 1.5 by column: |mean| / std <= 4, so E[x^2] - mean^2 loses nothing that matters."""
    rng = np.random.default_rng(seed)
    C = shape[-1]
    return (rng.standard_normal(shape) * (0.5 * (1 + np.arange(C) % 3)) + 2.0).astype(np.float32)


_REFS = {}


def cmvnw_reference(seed, T, C, win):
    """The clip and its float64 reference, computed once and shared (read-only) by the CPU and the GPU tests."""
    key = (seed, T, C, win)
    if key not in _REFS:
        x = clip(seed, T, C)
        r = R.cmvnw_ref(x, win)
        for a in (x, r["centred"], r["out"], r["inv"]):
            a.setflags(write=False)
        _REFS[key] = (x, r)
    return _REFS[key]


def cmvnw_check(got, x, r, variance, path, win, what):
    """The bar of one cmvnw result; prints the measured worst case.  -> (worst ulps, k)."""
    T = x.shape[0]
    floor = R.cmvnw_floor(x, r, variance, R.cmvnw_n(path, T, win))
    want = r["out"] if variance else r["centred"]
    k = 2 if variance else 1
    w = R.worst_ulps(got, want, floor)
    print("ULPS cmvnw %-8s %-34s variance=%d: %.3f ulp beyond the floor (bar %d)" % (path, what, variance, w, k))
    return w, k


SLIDING_SHAPES = [(3901, 5, 301), (3901, 5, 1), (4100, 3, 8301), (14500, 5, 301)]
TILE_SMALL = [(T, 5, win) for T in (1, 2, 63, 64, 65, 128, 129) for win in (1, 3, 301)]
MUTANT_SHAPES = [(700, 5, 31), (700, 5, 3), (300, 5, 301)]
CMVN_PAIRS = [(1, 1), (2, 5), (5, 40), (255, 5), (256, 256), (257, 257), (1025, 5), (5, 600), (1025, 40), (256, 255), (2, 600),
              (257, 1), (255, 256)]          # (T, C)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle():
    """The strided-view reference against oracle.speechpy_ref.cmvnw on float64 input: windows shorter than the clip, longer,
    and longer than twice the clip (several reflection periods).  The centred rows agree bit for bit.  The oracle's second
    pass runs on its float32 centred array, so NumPy takes the window std, the sum with 2^-30 and the quotient in float32:
    it is within a few float32 roundings (8 ulp allowed: pairwise sums of 301 terms, a square root, a quotient) of the
    float64 second pass used here, which is what the bars are measured against."""
    for T, C, win in ((90, 5, 31), (90, 5, 301), (7, 3, 41), (1, 2, 3), (129, 5, 1)):
        x = clip(5, T, C)
        r = R.cmvnw_ref(x, win)
        np.testing.assert_array_equal(r["centred"], ref.cmvnw(x.astype(np.float64), win, False))
        assert R.worst_ulps(ref.cmvnw(x.astype(np.float64), win, True), r["out"], R.cmvnw_floor(x, r, True, win)) <= 8.0
    x = clip(6, 9, 13)
    assert R.derivative_bar(x, 2).shape == x.shape
    f = np.arange(24, dtype=np.float32).reshape(1, 6, 4)
    cube = R.cube_ref(f, np.array([[0, 4, 5, 6, 7, -1]], dtype=np.int32), 2)
    np.testing.assert_array_equal(cube[0, 0, 1], f[0, 4:6])
    np.testing.assert_array_equal(cube[0, 0, 2, 0], f[0, 5])
    assert not cube[0, 0, 2, 1].any() and not cube[0, 0, 3:].any()


@pytest.mark.parametrize("T,C,win", SLIDING_SHAPES + [(3900, 5, 301), (300, 45, 301)] + TILE_SMALL + MUTANT_SHAPES)
def test_cmvnw_emulations_pass_the_bars(T, C, win):
    """The emulations of both cmvnw kernels on the GPU tests' inputs: inside the ulp bars, and no more elements off the
    reference than rounding boundaries can explain (R.mismatches)."""
    x, r = cmvnw_reference(1, T, C, win)
    for path, emul in (("sliding", R.emul_cmvnw_sliding), ("tile", R.emul_cmvnw_tile)):
        if path == "tile" and T > R.CW_CAP:
            continue
        for variance in (False, True):
            got = emul(x, win, variance)
            w, k = cmvnw_check(got, x, r, variance, path, win, "emulation (%d, %d, %d)" % (T, C, win))
            assert w <= k, (path, T, C, win, variance, w)
            n_off, budget = _mismatch_count(got, x, r, variance, path, win)
            assert n_off <= budget, (path, T, C, win, variance, n_off, budget)


def _mismatch_count(got, x, r, variance, path, win):
    """R.mismatches for a cmvnw result; with variance the budget also covers centred rows stored one ulp off (each moves its
    quotient too)."""
    n = R.cmvnw_n(path, x.shape[0], win)
    n_off, budget = R.mismatches(got, r["out"] if variance else r["centred"], R.cmvnw_floor(x, r, variance, n))
    if variance:
        budget += R.mismatches(r["centred"], r["centred"], R.cmvnw_floor(x, r, False, n))[1]
    return n_off, budget


def _mutant_fails(path, emul, mut):
    """-> (fails the ulp bar somewhere, fails the mismatch budget somewhere, worst ulps) over MUTANT_SHAPES, variance on and off."""
    ulp_fail, count_fail, worst = False, False, 0.0
    for T, C, win in MUTANT_SHAPES:
        x, r = cmvnw_reference(1, T, C, win)
        for variance in (False, True):
            got = emul(x, win, variance, mut)
            floor = R.cmvnw_floor(x, r, variance, R.cmvnw_n(path, T, win))
            want = r["out"] if variance else r["centred"]
            w = R.worst_ulps(got, want, floor)
            n_off, budget = _mismatch_count(got, x, r, variance, path, win)
            worst = max(worst, w)
            ulp_fail |= w > (2 if variance else 1)
            count_fail |= n_off > budget
    return ulp_fail, count_fail, worst


@pytest.mark.parametrize("path,mut", [("sliding", m) for m in R.SLIDING_MUTANTS] + [("tile", m) for m in R.TILE_MUTANTS])
def test_cmvnw_mutants_fail_the_bars(path, mut):
    """Window shifted by one row, 'reflect' padding, sample std, epsilon 2^-20, centred rows kept in float64 between the
    passes, variance over the raw rows, a dropped scan carry, a leaking running sum: each fails the ulp bars, and each leaves
    more elements off the reference than rounding boundaries explain.  The float64 centred rows are the narrowest case: at
    windows of 31 and 301 rows half an ulp of the centred row is less than one ulp of the quotient and stays inside the two-ulp
    allowance; the three-row window, whose std is ill-conditioned, takes it to 3 ulp, and the count (a third of the elements
    differ where a handful may) catches it at every window."""
    emul = R.emul_cmvnw_sliding if path == "sliding" else R.emul_cmvnw_tile
    ulp_fail, count_fail, worst = _mutant_fails(path, emul, mut)
    print("cmvnw %s mutant %-8s worst %.3g ulp beyond the floor; ulp bar %s, mismatch budget %s"
          % (path, mut, worst, "FAILS" if ulp_fail else "passes", "FAILS" if count_fail else "passes"))
    assert ulp_fail and count_fail, (path, mut, worst)


def _live(x, variance):
    """Columns whose std is more than the rounding of their own mean: where the ulp bar applies."""
    x = x.astype(np.float64)
    return (x.std(0) > 2.0 ** -20 * np.abs(x).max(0)) | (not variance)


@pytest.mark.parametrize("T,C", CMVN_PAIRS)
def test_cmvn_emulation_passes_and_its_mutants_fail(T, C):
    x = clip(2, T, C)
    for variance in (False, True):
        want, _, _, floor = R.cmvn_ref(x, variance)
        live = _live(x, variance)                                         # std = 0 (T = 1): the floor alone decides
        got = R.emul_cmvn(x, variance)
        w = R.worst_ulps(got[:, live], want[:, live], floor[live])
        print("ULPS cmvn emulation (%d, %d) variance=%d: %.3f ulp beyond the floor (bar 1)" % (T, C, variance, w))
        assert w <= 1.0 and np.all(np.abs(got.astype(np.float64) - want)[:, ~live] <= floor[~live])
    if T >= 255:
        want, _, _, floor = R.cmvn_ref(x, True)
        for mut in R.CMVN_MUTANTS:
            w = R.worst_ulps(R.emul_cmvn(x, True, mut), want, floor)
            print("cmvn mutant %-6s (%d, %d): %.3g ulp beyond the floor" % (mut, T, C, w))
            assert w > 1.0, (mut, T, C, w)


def _stats_cases():
    """(features [7, T, C] with mean 3 and std 0.5 .. 1.5, ragged frame counts) for svk_cmvn_stats."""
    for T, C in ((300, 40), (1500, 13), (260, 5), (257, 600)):
        yield clip(3, 7, T, C) + np.float32(1.0), np.array([T, T - 1, T // 3, 100, T, T, 257], dtype=np.int32)


def test_cmvn_stats_inputs_stay_inside_the_one_pass_bars():
    """|mean| / std <= 10 on the svk_cmvn_stats inputs, and the one-pass formula in float64 on exactly summed moments is
    within rtol = 1e-12 (mean) and 1e-9 (inverse std) of the two-pass float64 reference: the bars of the GPU test are not
    asked to absorb the formula's own cancellation."""
    for feat, nf in _stats_cases():
        for x in list(feat) + [feat[u, :n] for u, n in enumerate(nf)]:
            x64 = x.astype(np.float64)
            assert float(np.max(np.abs(x64.mean(0)) / x64.std(0))) <= 10.0
            mean, inv = R.cmvn_stats_one_pass(x)
            np.testing.assert_allclose(mean, x64.mean(0), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(inv, 1.0 / (x64.std(0) + R.EPS), rtol=1e-9)


DRAW_FRAMES = [80, 81, 82, 300, 2 ** 31 - 1, 79, 0]


def test_draw_crops_restatement():
    """The restatement's own sanity: starts in range, -1 for clips not longer than the crop, 'seed + g' and the low half of the
    product both differ from it, and 200 x 20 draws over a range of 16 are uniform (chi-square below the 99.9 % point of
    15 degrees of freedom, 37.697; checked against scipy when it is there)."""
    nf = np.array(DRAW_FRAMES)
    got, bad = R.draw_ref(nf, np.arange(7) + 2 ** 40, 20, 80, 2 ** 63)
    assert bad == 3 and (got[[0, 5, 6]] == -1).all() and (got[1] == 0).all()
    for u in (2, 3, 4):
        assert got[u].min() >= 0 and got[u].max() < nf[u] - 80 and len(set(got[u])) > 1
    for mut in ("plus", "low"):
        other, _ = R.draw_ref(nf, np.arange(7) + 2 ** 40, 20, 80, 2 ** 63 + 0xFFFF, mut)       # low bits set: seed + g carries where seed ^ g does not
        mine, _ = R.draw_ref(nf, np.arange(7) + 2 ** 40, 20, 80, 2 ** 63 + 0xFFFF)
        assert (other[[3, 4]] != mine[[3, 4]]).mean() > 0.9, mut
    draws, _ = R.draw_ref([96] * 200, range(200), 20, 80, 12345)
    counts = np.bincount(draws.ravel(), minlength=16)
    expect = draws.size / 16.0
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    crit = 37.697
    try:
        from scipy.stats import chi2 as dist
        assert abs(dist.ppf(0.999, 15) - crit) < 1e-3
    except ImportError:
        pass
    print("draw_crops: chi-square %.2f over 16 cells (99.9 %% point %.3f)" % (chi2, crit))
    assert counts.size == 16 and chi2 < crit


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _grid_cap(eng):
    """capped_grid's workgroup cap, read from the source it lives in."""
    for name in ("svk_internal.h", "stages.hip"):
        with open(os.path.join(REPO, "speaker_verification_amd", "csrc", name)) as f:
            m = re.search(r"cap = \(int64_t\)ctx->num_cu \* (\d+);", f.read())
        if m:
            return eng.num_cu * int(m.group(1))
    raise AssertionError("capped_grid's cap not found")


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,win", SLIDING_SHAPES)
def test_cmvnw_sliding_path(eng, T, C, win):
    """cmvnw_kernel (max_frames > 3900): the first shape past the cap, a window of one row, a window longer than 2 T, a
    VoxCeleb-length clip; mean only and with variance."""
    x, r = cmvnw_reference(1, T, C, win)
    assert T > R.CW_CAP
    for variance in (False, True):
        got = eng.cmvnw(x, win, variance).cpu().numpy()
        w, k = cmvnw_check(got, x, r, variance, "sliding", win, "(%d, %d, %d)" % (T, C, win))
        assert w <= k, (T, C, win, variance, w)


def _ragged(eng, max_frames, nfr, C, win, path):
    batch = clip(4, len(nfr), max_frames, C)
    nfr = np.array(nfr, dtype=np.int32)
    for variance in (False, True):
        got = eng.cmvnw(batch, win, variance, n_frames=nfr).cpu().numpy()
        for u, n in enumerate(nfr):
            np.testing.assert_array_equal(got[u, n:], batch[u, n:])          # rows past n_frames untouched
            if n:
                r = R.cmvnw_ref(batch[u, :n], win)
                w, k = cmvnw_check(got[u, :n], batch[u, :n], r, variance, path, win, "ragged, %d of %d rows" % (n, max_frames))
                assert w <= k, (u, n, variance, w)


@pytest.mark.gpu
def test_cmvnw_sliding_path_ragged(eng):
    _ragged(eng, 4000, [4000, 3901, 129, 128, 1, 0], 5, 301, "sliding")


@pytest.mark.gpu
def test_cmvnw_sliding_grid_stride_wraps(eng):
    """More (segment, column) threads than the capped grid holds (num_cu * 4 workgroups of 256).  The columns repeat with a
    period that does not divide the grid's stride, so a thread's second trip works on another column than its first: every
    repeat must be bit-identical to the first period, and that period meets the bar."""
    T, win = 14500, 301
    stride = eng.num_cu * 4 * 256
    period = next(p for p in (7, 11, 13) if stride % p)
    nseg = -(-T // R.SEG)
    C = stride // nseg + period + 1
    assert nseg * C > stride
    x7, r = cmvnw_reference(1, T, period, win)
    x = np.ascontiguousarray(np.tile(x7, (1, C // period + 1))[:, :C])
    got = eng.cmvnw(x, win, True).cpu().numpy()
    k = C // period
    assert np.array_equal(got[:, :k * period].reshape(T, k, period), np.broadcast_to(got[:, None, :period], (T, k, period)))
    assert np.array_equal(got[:, k * period:], got[:, :C - k * period])
    w, bar = cmvnw_check(got[:, :period], x7, r, True, "sliding", win, "grid-stride wrap, C = %d" % C)
    assert w <= bar


@pytest.mark.gpu
def test_cmvnw_tile_path(eng):
    """cmvnw_tile_kernel: the cap itself, the scan-step boundaries (T around 64 and 128) with windows of 1, 3 and 301 rows, a
    ragged batch (prefix stride T + 1, not max_frames + 1) and 45 columns at 300 frames (cg = 13: four column groups, the last
    ragged)."""
    fails = []
    for T, C, win in [(3900, 5, 301), (300, 45, 301)] + TILE_SMALL:
        x, r = cmvnw_reference(1, T, C, win)
        for variance in (False, True):
            got = eng.cmvnw(x, win, variance).cpu().numpy()
            w, k = cmvnw_check(got, x, r, variance, "tile", win, "(%d, %d, %d)" % (T, C, win))
            if not w <= k:
                fails.append((T, C, win, variance, w))
    assert not fails, fails
    _ragged(eng, 300, [300, 129, 64, 1, 0], 5, 301, "tile")


@pytest.mark.gpu
def test_cmvnw_paths_agree(eng):
    """The same 3900-frame clip through the tile kernel (max_frames = 3900) and through the sliding kernel (padded to
    max_frames = 3901, n_frames = 3900): within the variance bar of each other."""
    x, r = cmvnw_reference(1, 3900, 5, 301)
    padded = np.concatenate([x, np.zeros((1, 5), dtype=np.float32)])[None]
    for variance in (False, True):
        a = eng.cmvnw(x, 301, variance).cpu().numpy()
        b = eng.cmvnw(padded, 301, variance, n_frames=np.array([3900], dtype=np.int32)).cpu().numpy()[0]
        assert not b[3900].any()
        floor = R.cmvnw_floor(x, r, variance, R.cmvnw_n("tile", 3900, 301))
        w = R.worst_ulps(b[:3900], a, floor)
        print("ULPS cmvnw tile vs sliding (3900, 5, 301) variance=%d: %.3f ulp beyond the floor (bar 2)" % (variance, w))
        assert w <= 2.0
        assert cmvnw_check(b[:3900], x, r, variance, "sliding", 301, "3900 of 3901 rows")[0] <= (2 if variance else 1)


def _cmvn_clip_check(got, x, variance, what):
    want, _, _, floor = R.cmvn_ref(x, variance)
    live = _live(x, variance)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    # a column of std 0: 2^30 multiplies whatever rounding the mean carries, the ulp bar is meaningless, the floor decides
    assert np.all(np.abs(got.astype(np.float64) - want)[:, ~live] <= floor[~live]), what
    return R.worst_ulps(got[:, live], want[:, live], floor[live])


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, "0", "1"])
def test_cmvn_every_path(eng, monkeypatch, split):
    """cmvn_kernel<true> and the partial / stats / apply kernels: one and many column blocks (cb = 256, R = 1; cb not a divisor
    of 256), T < R, more rows than a chunk, n_frames above max_frames (clamped), a clip without frames, a constant column."""
    if split is None:
        monkeypatch.delenv("SVK_CMVN_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SVK_CMVN_SPLIT", split)
    worst = 0.0
    for T, C in CMVN_PAIRS:
        feat = clip(2, 4, T, C)
        feat[3, :, 0] = np.float32(0.3)                                    # a constant column (0.3f is not exact: sums round)
        nf = np.array([T, max(1, T // 2), 0, T + 9], dtype=np.int32)
        for variance in (False, True):
            got = eng.cmvn_(eng.to_device(feat).clone(), nf, variance).cpu().numpy()
            for u, n in enumerate(np.minimum(nf, T)):
                np.testing.assert_array_equal(got[u, n:], feat[u, n:])
                if n:
                    worst = max(worst, _cmvn_clip_check(got[u, :n], feat[u, :n], variance, (T, C, u, variance)))
    print("ULPS cmvn SVK_CMVN_SPLIT=%s: %.3f ulp beyond the floor (bar 1)" % (split, worst))
    assert worst <= 1.0


@pytest.mark.gpu
def test_cmvn_more_clips_than_grid_rows(eng, monkeypatch):
    """65 536 clips with the split forced: gridDim.y cannot hold them, svk_cmvn falls back to the one-kernel path."""
    monkeypatch.setenv("SVK_CMVN_SPLIT", "1")
    feat = clip(8, 65536, 2, 1)
    got = eng.cmvn_(eng.to_device(feat).clone(), None, True).cpu().numpy()
    x = feat.astype(np.float64)
    inv = 1.0 / (x.std(1, keepdims=True) + R.EPS)
    want = ((x - x.mean(1, keepdims=True)) * inv).astype(np.float32)
    w = R.worst_ulps(got, want, 2 * 2.0 ** -50 * np.abs(x).max(1, keepdims=True) * inv)
    print("ULPS cmvn 65536 clips, one-kernel fall-back: %.3f ulp beyond the floor (bar 1)" % w)
    assert w <= 1.0


def GATHER_STARTS(T, cf):
    """Inside, last full crop, one row past it (zero tail), last row, at and above max_frames, too short."""
    return [0, T - cf, T - cf + 1, T - 1, T, T + 7, -1]


def _offset_by_one_float(eng, a):
    """a on the device at a base that is 4-byte- but not 16-byte-aligned."""
    buf = torch.empty((a.size + 1,), dtype=torch.float32, device=eng.device)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and eng.to_device(view, torch.float32).data_ptr() == view.data_ptr()
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("C", [40, 13, 5])
@pytest.mark.parametrize("cf", [80, 3])
def test_cube_gather_every_copy_path(eng, C, cf):
    """Vector and scalar copies, with and without statistics: columns that are no multiple of 4, crops that run past
    max_frames (zero tail), start at or above it, or are -1; a feature tensor off 16-byte alignment.  Without statistics
    bit-exact; with them bit-identical to cmvn_ in place + a plain gather, and within the cmvn bar of float64."""
    T, n = 100, 3
    feat = clip(9, n, T, C)
    crops = np.tile(np.array(GATHER_STARTS(T, cf), dtype=np.int32), (n, 1))
    ref64 = [R.cmvn_ref(feat[u], True) for u in range(n)]
    want_n = R.cube_ref(np.stack([r[0] for r in ref64]), crops, cf)
    for dev in (eng.to_device(feat), _offset_by_one_float(eng, feat)):
        np.testing.assert_array_equal(eng.cube_gather(dev, crops, cf).cpu().numpy(), R.cube_ref(feat, crops, cf))
        stats = eng.cmvn_stats(dev, None, variance=True)
        got = eng.cube_gather(dev, crops, cf, stats=stats)
        assert torch.equal(got, eng.cube_gather(eng.cmvn_(dev.clone(), None, True), crops, cf))
        got = got.cpu().numpy()
        assert not got[:, :, 4:].any()
        w = max(R.worst_ulps(got[u], want_n[u], ref64[u][3]) for u in range(n))
        print("ULPS cmvn_stats + gather C=%d crop=%d base %% 16 = %d: %.3f ulp beyond the floor (bar 1)" % (C, cf, dev.data_ptr() % 16, w))
        assert w <= 1.0


@pytest.mark.gpu
def test_cube_gather_more_jobs_than_workgroups(eng):
    n, k, T, C, cf = eng.num_cu * 16 // 7 + 20, 7, 10, 5, 3
    assert n * k > eng.num_cu * 16
    feat = clip(10, n, T, C)
    crops = np.tile(np.array(GATHER_STARTS(T, cf), dtype=np.int32), (n, 1))
    crops[1::2] = crops[1::2, ::-1]
    dev = eng.to_device(feat)
    np.testing.assert_array_equal(eng.cube_gather(dev, crops, cf).cpu().numpy(), R.cube_ref(feat, crops, cf))
    stats = eng.cmvn_stats(dev, None, variance=True)
    assert torch.equal(eng.cube_gather(dev, crops, cf, stats=stats), eng.cube_gather(eng.cmvn_(dev.clone(), None, True), crops, cf))


@pytest.mark.gpu
@pytest.mark.parametrize("split", [None, "0", "1"])
def test_cmvn_stats_against_float64(eng, monkeypatch, split):
    """svk_cmvn_stats (cmvn_kernel<false>, or the partial + stats kernels) at rtol = 1e-12 (mean) and 1e-9 (inverse std),
    ragged frame counts included."""
    if split is None:
        monkeypatch.delenv("SVK_CMVN_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SVK_CMVN_SPLIT", split)
    for feat, nf in _stats_cases():
        T = feat.shape[1]
        for n_frames in (None, nf):
            stats = eng.cmvn_stats(eng.to_device(feat), n_frames, variance=True).cpu().numpy()
            for u in range(feat.shape[0]):
                x = feat[u, :T if n_frames is None else nf[u]].astype(np.float64)
                np.testing.assert_allclose(stats[u, 0], x.mean(0), rtol=1e-12, atol=1e-12)
                np.testing.assert_allclose(stats[u, 1], 1.0 / (x.std(0) + R.EPS), rtol=1e-9)


@pytest.mark.gpu
def test_derivative_against_float64(eng):
    """delta 1, 2, 9 on 1, 2, 13, 40 columns (delta >= C: every tap clamps to the last column), a leading batch dimension, and
    more elements than the capped grid's threads."""
    worst = 0.0
    cases = [((37, C), d) for d in (1, 2, 9) for C in (1, 2, 13, 40)] + [((3, 11, 13), 2)]
    cases.append(((_grid_cap(eng) * 256 // 13 + 300, 13), 2))
    for shape, delta in cases:
        x = clip(11, *shape)
        got = eng.derivative(x, delta).cpu().numpy().astype(np.float64)
        want = ref.derivative_extraction(x.reshape(-1, shape[-1]).astype(np.float64), delta).reshape(shape)
        bar = R.derivative_bar(x, delta)
        ratio = float(np.max(np.abs(got - want) / bar))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (shape, delta, ratio)
    print("ULPS derivative: %.3f of the bar (delta + 2) 2^-24 sum k |x_k| / scale" % worst)


@pytest.mark.gpu
def test_log_power_exact_relations(eng):
    """No tolerance is invented for log10f: normalised == un-normalised - max bit for bit with max exactly 0; everything
    <= 1e-20f gives exactly -200 and +inf stays +inf; n = 1; more elements than the capped grid's threads."""
    rng = np.random.default_rng(12)
    for n in (1, 7 * 257, _grid_cap(eng) * 256 + 1000):
        p = (rng.standard_normal(n).astype(np.float32) ** 2)
        p[::5] = 0.0
        u = eng.log_power_(eng.to_device(p).clone(), normalize=False).cpu().numpy()
        v = eng.log_power_(eng.to_device(p).clone(), normalize=True).cpu().numpy()
        assert u.dtype == np.float32 and np.array_equal(v, u - u.max()) and v.max() == 0.0
        want = 10 * np.log10(np.maximum(p.astype(np.float64), 1e-20))
        np.testing.assert_allclose(u, want, rtol=0, atol=2e-4)
    tiny = np.float32(1e-20)
    above = np.nextafter(tiny, np.float32(1))
    p = np.array([0.0, -0.0, -1.0, -np.inf, tiny, above, 1e-40, 1.4e-45, np.inf, 1.0], dtype=np.float32)
    u = eng.log_power_(eng.to_device(p).clone(), normalize=False).cpu().numpy()
    assert np.array_equal(u[[0, 1, 2, 3, 4, 6, 7]], np.full(7, -200.0, dtype=np.float32)), u
    assert abs(float(u[5]) + 200.0) <= 2e-4 and u[8] == np.inf and u[9] == 0.0, u     # just above the floor: log10f's own error


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 2 ** 63, 2 ** 64 - 1])
def test_draw_crops_bit_exact(eng, seed):
    """svk_cube_draw_crops against the Python-integer restatement: first_utt 0 and 2^40, 1 / 20 / 257 crops, frame counts
    around the crop length and 2^31 - 1, the bad-clip counter given and NULL, and the utt_index form equal to the first_utt
    form row for row once its permutation is undone."""
    nf = np.array(DRAW_FRAMES, dtype=np.int32)
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    for first in (0, 2 ** 40):
        for n_crops in (1, 20, 257):
            want, bad_want = R.draw_ref(nf, first + np.arange(7), n_crops, 80, seed)
            bad = torch.zeros((1,), dtype=torch.int32, device=eng.device)
            got = eng.draw_crops(nf, n_crops, 80, seed, first_utt=first, bad_count=bad).cpu().numpy()
            np.testing.assert_array_equal(got, want)
            assert int(bad) == bad_want == 3
            np.testing.assert_array_equal(eng.draw_crops(nf, n_crops, 80, seed, first_utt=first).cpu().numpy(), want)
            by_index = eng.draw_crops(nf[perm], n_crops, 80, seed, first_utt=12345, utt_index=first + perm).cpu().numpy()
            np.testing.assert_array_equal(by_index, want[perm])
    many = np.full(600, 96, dtype=np.int32)                              # 12 000 draws: more than one workgroup
    np.testing.assert_array_equal(eng.draw_crops(many, 20, 80, seed).cpu().numpy(), R.draw_ref(many, range(600), 20, 80, seed)[0])
