"""A clip's CMVN statistics are a function of its rows and its n_frames -- not of max_frames, n_utt or its place in the batch
(include/svk.h at svk_cmvn; DESIGN §4 "One clip, one embedding").

svk_cmvn, svk_cmvn_stats and svk_delta_cmvn_stats pick a launch by the call's max_frames: up to 1 024 one workgroup per clip,
above it the partial / stats / apply trio.  The two launches used to add a column's rows in different orders, so a 9 s clip got
other last bits next to an 11 s clip than alone.  Now the ORDER follows the clip's own frame count on either launch.

CPU (default pass): NumPy float64 emulations of both orders (tests/postproc_f64_ref.py) give DIFFERENT bits on the GPU test's
own inputs wherever a clip has more than one chunk: a kernel that let the launch choose the order fails the GPU test on them.
GPU (-m gpu): each clip in every layout -- alone, padded, next to a longer neighbour, first and last of five -- gives
bit-identical statistics, rows and cubes; each stays inside the float64 bars of tests/postproc_f64_ref.py; and the two forced
launches (SVK_CMVN_SPLIT, a test switch) still agree on long clips within that bar.  Lines starting with "ROUTE" carry what
differed, for the record in DESIGN.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import delta_f64_ref as D             # noqa: E402  (tests/ is on sys.path)
import postproc_f64_ref as R          # noqa: E402

COLS = [40, 13, 300]
SHORT = [1, 81, 255, 256, 257, 300, 1000, 1024]          # one workgroup per clip when alone
LONG = [1025, 1148, 2000]                                # the chunked trio when alone
NEIGHBOURS = [1025, 1400, 14500]                         # max_frames a longer neighbour brings
CROP = 80

_CLIPS = {}


def clip(T, C):
    """Seeded N(-7, 3) float32 rows [T, C] (log-mel magnitudes), drawn once and shared read-only."""
    if (T, C) not in _CLIPS:
        x = (np.random.default_rng([T, C, 20]).standard_normal((T, C)) * 3.0 - 7.0).astype(np.float32)
        x.setflags(write=False)
        _CLIPS[T, C] = x
    return _CLIPS[T, C]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", COLS)
def test_the_two_orders_differ_on_these_inputs(C):
    """The teeth of the GPU test: on its own inputs cmvn_kernel's order and the chunked order give different float64 sums of
    squares, and with them a different 1 / (std + 2^-30), in some column of every clip with more than one chunk, for the static
    rows and for both delta planes.  The plain sums do NOT differ: a few thousand float32 values within 2^-14 .. 2^5 add
    exactly in float64 in any order (24 + 19 + 11 bits), so the means are order-free and the whole dependence sits in the
    48-bit squares.  A clip of one chunk (T <= 256) is summed alike by both orders -- there the launch never mattered -- and
    the two stay within the n 2^-52 max|x|^2 that the bars of postproc_f64_ref allow between any two orders."""
    for T in SHORT + LONG:
        for plane in D.planes32(clip(T, C)):
            sw, qw = R.emul_cmvn_sums(plane, "whole")
            sc, qc = R.emul_cmvn_sums(plane, "chunked")
            if T <= R.CMVN_CHUNK:
                assert np.array_equal(sw, sc) and np.array_equal(qw, qc), (T, C)
                continue
            assert (qw != qc).any(), (T, C)
            mean = sw / T
            inv_w = 1.0 / (np.sqrt(np.maximum(qw / T - mean * mean, 0.0)) + R.EPS)
            inv_c = 1.0 / (np.sqrt(np.maximum(qc / T - sc / T * (sc / T), 0.0)) + R.EPS)
            assert (inv_w != inv_c).any(), (T, C)
            assert np.all(np.abs(qw - qc) / T <= T * 2.0 ** -52 * (plane.astype(np.float64) ** 2).max(0)), (T, C)
            assert np.all(np.abs(sw - sc) / T <= T * 2.0 ** -52 * np.abs(plane.astype(np.float64)).max(0)), (T, C)
    assert R.cmvn_order(1024) == "whole" and R.cmvn_order(1025) == "chunked"


def test_the_inputs_stay_inside_the_one_pass_bars():
    """var = E[x^2] - mean^2 on exactly summed moments is within rtol 1e-12 (mean) and 1e-9 (inverse std) of the two-pass float64
    reference on these inputs (|mean| / std ~ 2.3): the bars of the GPU test are not asked to absorb the formula's cancellation."""
    for C in COLS:
        for T in SHORT[1:] + LONG:
            x = clip(T, C)
            x64 = x.astype(np.float64)
            mean, inv = R.cmvn_stats_one_pass(x)
            np.testing.assert_allclose(mean, x64.mean(0), rtol=1e-12)
            np.testing.assert_allclose(inv, 1.0 / (x64.std(0) + R.EPS), rtol=1e-9)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _starts(T):
    """Crop starts that lie inside the clip (rows past n_frames belong to the layout, not to the clip)."""
    cf = min(CROP, T)
    return cf, np.array([0, T - cf, (T - cf) // 2], dtype=np.int32)


def layouts(T):
    """(name, max_frames, n_utt, position of the clip) of every layout the clip is run in."""
    out = [("alone", T, 1, 0)]
    if T < 1024:
        out.append(("padded to 1024", 1024, 1, 0))
    out += [("next to %d frames" % M, M, 2, 0) for M in NEIGHBOURS if M > T]
    out += [("first of five", T + 3, 5, 0), ("last of five", T + 3, 5, 4)]
    return out


def _batch(eng, x, max_frames, n_utt, pos, filler):
    """The clip at `pos` of a [n_utt, max_frames, C] batch whose every other value (pad rows included) comes from `filler`;
    the other clips are full length, except in the batch of five, where their lengths vary.  -> (feat, n_frames)"""
    T, C = x.shape
    feat = filler[:n_utt * max_frames * C].view(n_utt, max_frames, C).clone()
    feat[pos, :T] = torch.from_numpy(np.array(x)).to(eng.device)
    nf = np.full(n_utt, max_frames, dtype=np.int32)
    if n_utt == 5:
        nf[:] = [max_frames, max(1, T // 2), 0, max(1, T - 1), max_frames]
    nf[pos] = T
    return feat.contiguous(), nf


def results(eng, x, layout, filler):
    """Every CMVN result of the clip in one layout, cut down to the clip: name -> device tensor."""
    _, max_frames, n_utt, pos = layout
    T, C = x.shape
    feat, nf = _batch(eng, x, max_frames, n_utt, pos, filler)
    cf, starts = _starts(T)
    crops = np.tile(starts, (n_utt, 1))
    out = {}
    for variance in (False, True):
        out["cmvn_stats v=%d" % variance] = eng.cmvn_stats(feat, nf, variance=variance)[pos]
        out["delta_cmvn_stats v=%d" % variance] = eng.delta_cmvn_stats(feat, nf, variance=variance)[pos]
        out["cmvn_ rows v=%d" % variance] = eng.cmvn_(feat.clone(), nf, variance)[pos, :T]
    stats = eng.cmvn_stats(feat, nf, variance=True)
    out["cube_gather"] = eng.cube_gather(feat, crops, cf, stats=stats)[pos]
    stats3 = eng.delta_cmvn_stats(feat, nf, variance=True)
    out["cube_gather_delta"] = eng.cube_gather_delta(feat, crops, cf, stats=stats3)[pos]
    return {k: v.clone() for k, v in out.items()}


def _differences(name, got, want):
    """-> None where the two are the same bits, else a line for the record: how many values moved and by how much."""
    if torch.equal(got, want):
        return None
    g, w = got.cpu().numpy(), want.cpu().numpy()
    moved = g != w
    if g.dtype == np.float64:
        return "%s: %d of %d statistics differ, by up to %d ulp of float64" % (name, moved.sum(), g.size, R.ulp64_distance(g, w).max())
    rows = moved.reshape(-1, g.shape[-1]).any(1).sum()
    return "%s: %d of %d float32 values in %d rows differ" % (name, moved.sum(), g.size, rows)


_REFS = {}


def _refs(x):
    """The clip's float64 references, computed once: cmvn_ref without and with variance, delta_f64_ref."""
    key = x.shape
    if key not in _REFS:
        _REFS[key] = (R.cmvn_ref(x, False), R.cmvn_ref(x, True), D.delta_f64_ref(x, 2, True) if x.shape[0] > 1 else None)
    return _REFS[key]


def _check_against_float64(x, res, what):
    """The bars of tests/postproc_f64_ref.py, not restated: statistics at rtol 1e-12 / 1e-9, normalised rows and cubes within
    one float32 ulp beyond the cmvn floor.  A one-row clip has std = 0: 2^30 multiplies the rounding of the mean, the floor
    alone decides (and the mean is the row itself)."""
    T, C = x.shape
    x64 = np.asarray(x, dtype=np.float64)
    for variance in (False, True):
        stats = res["cmvn_stats v=%d" % variance].cpu().numpy()
        np.testing.assert_allclose(stats[0], x64.mean(0), rtol=1e-12, err_msg=what)
        if T > 1:
            want_inv = 1.0 / (x64.std(0) + R.EPS) if variance else np.ones(C)
            np.testing.assert_allclose(stats[1], want_inv, rtol=1e-9, err_msg=what)
        want, _, _, floor = _refs(x)[int(variance)]
        got = res["cmvn_ rows v=%d" % variance].cpu().numpy()
        if T > 1:
            assert R.worst_ulps(got, want, floor) <= 1.0, (what, variance)
        else:
            assert np.all(np.abs(got.astype(np.float64) - want) <= floor), (what, variance)
    if T > 1:
        cf, starts = _starts(T)
        want, _, _, floor = _refs(x)[1]
        want_cube = R.cube_ref(want[None], starts[None], cf)[0]
        assert R.worst_ulps(res["cube_gather"].cpu().numpy(), want_cube, floor) <= 1.0, what
        r = _refs(x)[2]
        rms = np.sqrt((r["planes"].astype(np.float64) ** 2).mean(1))
        stats3 = res["delta_cmvn_stats v=1"].cpu().numpy()
        assert np.all(np.abs(stats3[:, 0] - r["mean"]) <= 1e-12 * rms), what          # tests/test_delta_planes.py's derived bars
        assert np.all(np.abs(stats3[:, 1] - r["inv"]) <= 1e-11 * r["inv"]), what
        want3 = np.stack([R.cube_ref(r["want"][ch][None], starts[None], cf)[0, 0] for ch in range(3)])
        assert R.worst_ulps(res["cube_gather_delta"].cpu().numpy(), want3, r["floor"][:, None, None]) <= 1.0, what


@pytest.mark.gpu
@pytest.mark.parametrize("C", COLS)
def test_a_clips_cmvn_does_not_depend_on_the_launch(eng, monkeypatch, C):
    """Every clip length in every layout: the float64 output of cmvn_stats and delta_cmvn_stats, the float32 rows of cmvn_ and
    the cubes of cube_gather(stats=) and cube_gather_delta(stats=) are the bits the clip gives alone, and every one of them is
    inside its float64 bar."""
    monkeypatch.delenv("SVK_CMVN_SPLIT", raising=False)
    gen = torch.Generator(device="cpu").manual_seed(C)
    filler = (torch.randn(2 * 14500 * C, generator=gen) * 3.0 - 7.0).to(eng.device)    # >= 5 (2000 + 3) C values as well
    found = []
    for T in SHORT + LONG:
        x = clip(T, C)
        alone = None
        for layout in layouts(T):
            res = results(eng, x, layout, filler)
            what = "T=%d C=%d %s" % (T, C, layout[0])
            _check_against_float64(x, res, what)
            if alone is None:
                alone = res
                continue
            for name in res:
                line = _differences(name, res[name], alone[name])
                if line:
                    found.append("ROUTE %s: %s" % (what, line))
    print("\n".join(found) if found else "ROUTE C=%d: every layout gives the clip's own bits" % C)
    assert not found, "%d results depend on the launch (first: %s)" % (len(found), found[0])


@pytest.mark.gpu
@pytest.mark.parametrize("C", COLS)
def test_the_forced_launches_agree_on_long_clips(eng, monkeypatch, C):
    """SVK_CMVN_SPLIT=0 puts a long clip on one workgroup, which adds its rows in the other order: the two forced launches stay
    within the cmvn bar of each other (float64 values at most the floor apart round to float32 values at most one ulp apart) and
    of float64, and the unforced launch is the chunked one bit for bit."""
    for T in LONG:
        x = clip(T, C)
        feat = eng.to_device(np.array(x)[None])
        nf = np.array([T], dtype=np.int32)
        got = {}
        for split in ("0", "1", None):
            if split is None:
                monkeypatch.delenv("SVK_CMVN_SPLIT", raising=False)
            else:
                monkeypatch.setenv("SVK_CMVN_SPLIT", split)
            got[split] = (eng.cmvn_stats(feat, nf, variance=True).cpu().numpy()[0],
                          eng.cmvn_(feat.clone(), nf, True).cpu().numpy()[0],
                          eng.delta_cmvn_stats(feat, nf, variance=True).cpu().numpy()[0])
        want, mean, inv, floor = R.cmvn_ref(x, True)
        for split in ("0", "1"):
            np.testing.assert_allclose(got[split][0][0], mean, rtol=1e-12)
            np.testing.assert_allclose(got[split][0][1], inv, rtol=1e-9)
            assert R.worst_ulps(got[split][1], want, floor) <= 1.0, (T, C, split)
        w = R.worst_ulps(got["0"][1], got["1"][1], floor)
        print("ULPS cmvn forced launches T=%d C=%d: %.3f ulp beyond the floor of each other (bar 1); %d statistics differ"
              % (T, C, w, (got["0"][0] != got["1"][0]).sum()))
        assert w <= 1.0
        r = D.delta_f64_ref(x, 2, True)                                         # tests/test_delta_planes.py's derived bars, each side
        rms = np.sqrt((r["planes"].astype(np.float64) ** 2).mean(1))
        for split in ("0", "1"):
            assert np.all(np.abs(got[split][2][:, 0] - r["mean"]) <= 1e-12 * rms), (T, C, split)
            assert np.all(np.abs(got[split][2][:, 1] - r["inv"]) <= 1e-11 * r["inv"]), (T, C, split)
        for k in range(3):
            np.testing.assert_array_equal(got[None][k], got["1"][k])
