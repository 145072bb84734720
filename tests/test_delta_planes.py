"""The three-channel input kernels: svk_delta_cmvn_stats, svk_delta_planes and svk_cube_gather_delta against the sequence they
replace (svk_derivative twice, svk_cmvn[_stats] per channel, svk_cube_gather: bit for bit) and against float64
(tests/delta_f64_ref.py), on every launch path.

CPU (default pass): the reference arithmetic is pinned to the golden three-channel CMVN output and to the oracle.
GPU (-m gpu): lines starting with "ULPS" / "STATS" carry the measured worst cases.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import delta_f64_ref as D             # noqa: E402  (tests/ is on sys.path)
import postproc_f64_ref as R          # noqa: E402
from oracle import speechpy_ref as ref   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c3d2_3c.npz")

# (max_frames, n_frames): the one-workgroup CMVN path, and the chunked one (max_frames > 1024) with chunk boundaries at 256
SHAPES = {"short": (300, [300, 83, 1, 0]), "chunked": (1030, [1030, 257, 256, 0])}
CASES = [("short", 40), ("short", 13), ("short", 1), ("chunked", 40)]    # 13: a ragged 16-byte tail; 1: every tap clamps
SPLITS = [None, "0", "1"]                                                # SVK_CMVN_SPLIT: by size, one workgroup, chunked
CROP_FRAMES = 80

_INPUTS = {}


def inputs(shape, C):
    """Seeded N(1, 3) float32 features [4, max_frames, C] with zero pad rows + the frame counts; computed once, read-only."""
    key = (shape, C)
    if key not in _INPUTS:
        T, nf = SHAPES[shape]
        x = (np.random.default_rng([T, C]).standard_normal((len(nf), T, C)) * 3.0 + 1.0).astype(np.float32)
        for u, n in enumerate(nf):
            x[u, n:] = 0.0
        x.setflags(write=False)
        refs = [D.delta_f64_ref(x[u, :n], 2, True) if n else None for u, n in enumerate(nf)]
        _INPUTS[key] = (x, np.array(nf, dtype=np.int32), refs)
    return _INPUTS[key]


def crops_for(shape):
    """[4, 6] crop starts: inside, the last full crop, -1, past the end and half inside the clip (clip 0 fills max_frames);
    clips shorter than max_frames keep their crops inside their own rows, clips too short to crop get -1."""
    T, nf = SHAPES[shape]
    out = np.full((len(nf), 6), -1, dtype=np.int32)
    out[0] = [0, T - CROP_FRAMES, T // 2 - 13, -1, T + 5, T - CROP_FRAMES // 2]
    for u in (1, 2):
        if nf[u] > CROP_FRAMES:
            last = nf[u] - CROP_FRAMES
            out[u] = [0, last, last // 2, -1, min(2, last), last]
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_reference_matches_the_golden_three_channel_cmvn():
    """delta_f64_ref (float32 planes, float64 statistics) against the reference's own output for its seeded features, at the
    tolerance tests/test_three_channel.py uses for that array (the reference works in float64 from float64 features)."""
    g = np.load(GOLDEN, allow_pickle=False)
    feat = np.random.default_rng(int(g["cmvn_feat_seed"][0])).standard_normal((120, 40)) * 3.0 + 1.0
    got = D.delta_f64_ref(feat.astype(np.float32), 2, True)["want"].transpose(1, 2, 0)
    assert got.shape == g["cmvn_out"].shape == (120, 40, 3)
    np.testing.assert_allclose(got, g["cmvn_out"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("T,C", [(120, 40), (83, 13), (5, 1), (1, 4)])
def test_reference_matches_the_oracle(T, C):
    """The same reference against oracle.speechpy_ref.extract_derivative_feature + cmvn per channel (float64 throughout)."""
    x = (np.random.default_rng([T, C, 1]).standard_normal((T, C)) * 3.0 + 1.0).astype(np.float32)
    r = D.delta_f64_ref(x, 2, True)
    stacked = ref.extract_derivative_feature(x.astype(np.float64))
    np.testing.assert_allclose(r["planes"].transpose(1, 2, 0), stacked, rtol=1e-6, atol=4e-6)   # float32 roundings at |x| <= 32
    if T > 1:                                                          # one row: std = 0 and 2^30 multiplies rounding noise
        want = np.stack([ref.cmvn(stacked[:, :, ch], variance_normalization=True) for ch in range(3)])
        np.testing.assert_allclose(r["want"], want, rtol=1e-3, atol=1e-4)
    assert np.array_equal(D.derivative32(x, 1), (x[:, np.minimum(np.arange(C) + 1, C - 1)] * np.float32(0.5)))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("SVK_CMVN_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SVK_CMVN_SPLIT", split)


def _parent_planes(eng, feat, nf, normalize):
    """What evaluation.dataset_embeddings ran before these kernels: two derivative launches, a CMVN per channel, a stack."""
    chans = [feat.clone(), eng.derivative(feat, 2)]
    chans.append(eng.derivative(chans[1], 2))
    if normalize:
        for ch in chans:
            eng.cmvn_(ch, nf, variance=True)
    return torch.stack(chans, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,C", CASES)
def test_delta_planes_without_statistics(eng, shape, C):
    """Plane 0 is the input, plane 1 svk_derivative of it, plane 2 svk_derivative of plane 1, bit for bit, for windows 1, 2 and
    3 (40 columns: the 16-byte paths with the taps in registers and re-read; 13 and 1: the scalar path); window 2 is also the
    NumPy float32 planes bit for bit.  Rows at or past n_frames are zeros, a clip without frames is all zeros -- also where the
    input's pad rows are NOT zero."""
    x, nf, _ = inputs(shape, C)
    feat = eng.to_device(x)
    for delta in (1, 2, 3):
        got = eng.delta_planes(feat, nf, delta=delta)
        assert tuple(got.shape) == (x.shape[0], 3, x.shape[1], C)
        assert torch.equal(got[:, 0], feat)
        p1 = eng.derivative(feat, delta)
        assert torch.equal(got[:, 1], p1), delta
        assert torch.equal(got[:, 2], eng.derivative(p1, delta)), delta
        if delta == 2:
            np.testing.assert_array_equal(got.cpu().numpy(), D.planes32(x, 2).transpose(1, 0, 2, 3))
        for u, n in enumerate(nf):
            assert not bool(got[u, :, n:].any())
    dirty = x.copy()
    dirty[1, nf[1]:] = 5.0
    got = eng.delta_planes(dirty, nf)
    assert not bool(got[1, :, nf[1]:].any()) and torch.equal(got[1, :, :nf[1]], eng.delta_planes(feat, nf)[1, :, :nf[1]])
    assert torch.equal(eng.delta_planes(feat), eng.delta_planes(feat, np.full(len(nf), x.shape[1], np.int32)))   # NULL = max_frames


def _raw_stats(eng, feat, nf, variance, sentinel=7.0):
    n, T, C = feat.shape
    stats = torch.full((n, 3, 2, C), sentinel, dtype=torch.float64, device=eng.device)
    nfd = eng.to_device(nf, torch.int32)
    eng._stream()
    rc = eng.lib.svk_delta_cmvn_stats(eng.ctx, eng._ptr(feat), n, T, C, eng._ptr(nfd), 2, int(variance), eng._ptr(stats))
    assert rc == 0
    return stats


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape,C", CASES)
def test_delta_cmvn_stats_equal_cmvn_stats_of_each_plane(eng, monkeypatch, shape, C, split):
    """delta_cmvn_stats[:, ch] == cmvn_stats(plane ch) bit for bit, with and without variance, on both CMVN paths (chosen by
    size and forced either way); the zero-frame clip's slot keeps what was there."""
    _set_split(monkeypatch, split)
    x, nf, _ = inputs(shape, C)
    feat = eng.to_device(x)
    planes = eng.delta_planes(feat, nf)
    live = torch.from_numpy(nf > 0).to(eng.device)
    for variance in (False, True):
        got = _raw_stats(eng, feat, nf, variance)
        assert bool((got[~live] == 7.0).all())
        for ch in range(3):
            want = eng.cmvn_stats(planes[:, ch].contiguous(), nf, variance=variance)
            assert torch.equal(got[live][:, ch], want[live]), (ch, variance)
        assert torch.equal(eng.delta_cmvn_stats(feat, nf, variance=variance)[live], got[live])


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape,C", CASES)
def test_delta_cmvn_stats_against_float64(eng, monkeypatch, shape, C, split):
    """Against two-pass float64 statistics of the float32 planes.  The bound is derived: a float64 sum of n <= 1 030 values is
    off by at most n 2^-53 sum|x| <= 1.2e-13 n rms, so |mean - ref| <= 1e-12 rms; var = E[x^2] - mean^2 with E[x^2] / var ~ 1.1
    (static N(1, 3)) .. 1.2 (the delta planes: mean 0.3, variance 0.45) multiplies the same relative error of the two moments by
    ~2.4, and 1 / (std + 2^-30) takes half of that: |inv - ref| <= 1e-11 ref.  A one-row clip has var = v v - v v = 0 exactly in
    float64 on both sides (inv = 2^30)."""
    _set_split(monkeypatch, split)
    x, nf, refs = inputs(shape, C)
    got = eng.delta_cmvn_stats(x, nf, variance=True).cpu().numpy()
    worst_m = worst_i = 0.0
    for u, r in enumerate(refs):
        if r is None:
            continue
        rms = np.sqrt((r["planes"].astype(np.float64) ** 2).mean(1))
        dm = np.abs(got[u, :, 0] - r["mean"]) / rms
        di = np.abs(got[u, :, 1] - r["inv"]) / r["inv"]
        worst_m, worst_i = max(worst_m, float(dm.max())), max(worst_i, float(di.max()))
    print("STATS %s C=%d SVK_CMVN_SPLIT=%s: |mean - ref| / rms %.2e (bar 1e-12), |inv - ref| / ref %.2e (bar 1e-11)"
          % (shape, C, split, worst_m, worst_i))
    assert worst_m <= 1e-12 and worst_i <= 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape,C", CASES)
def test_normalised_planes_and_cubes(eng, monkeypatch, shape, C, split):
    """delta_planes(stats=...) and cube_gather_delta(stats=...) equal the sequence they replace bit for bit (derivative twice,
    cmvn_ per channel; cube_gather of those planes), with crops that are -1, start past the end and lie half inside the clip;
    and they are within one float32 ulp of the float64 reference: one rounding of (v - mean) inv.  The statistics are
    accurate to 1e-11, which moves the float64 value by up to tests/postproc_f64_ref.py's cmvn floor (T 2^-50 max|v| inv,
    ~1e-12) before it is rounded -- that floor is subtracted first, as for svk_cmvn."""
    _set_split(monkeypatch, split)
    x, nf, refs = inputs(shape, C)
    n, T, _ = x.shape
    feat = eng.to_device(x)
    stats = eng.delta_cmvn_stats(feat, nf, variance=True)
    parent = _parent_planes(eng, feat, nf, True)
    got = eng.delta_planes(feat, nf, stats=stats)
    assert torch.equal(got, parent)
    crops = crops_for(shape)
    parent_cube = eng.cube_gather(parent.view(3 * n, T, C), np.repeat(crops, 3, axis=0), CROP_FRAMES).view(n, 3, 6, CROP_FRAMES, C)
    cube = eng.cube_gather_delta(feat, crops, CROP_FRAMES, stats=stats)
    assert tuple(cube.shape) == (n, 3, 6, CROP_FRAMES, C) and torch.equal(cube, parent_cube)
    raw_cube = eng.cube_gather_delta(feat, crops, CROP_FRAMES)                 # no statistics: the raw planes' rows
    raw = eng.delta_planes(feat, nf)
    assert torch.equal(raw_cube, eng.cube_gather(raw.view(3 * n, T, C), np.repeat(crops, 3, axis=0), CROP_FRAMES).view(n, 3, 6, CROP_FRAMES, C))
    assert bool(cube[0, :, 1].any()) and not bool(cube[:, :, 3].any()) and not bool(cube[0, :, 4].any())
    assert bool(cube[0, :, 5, :CROP_FRAMES // 2].any()) and not bool(cube[0, :, 5, CROP_FRAMES // 2:].any())
    got, cube = got.cpu().numpy(), cube.cpu().numpy()
    worst = 0.0
    for u, r in enumerate(refs):
        if r is None:
            assert not got[u].any() and not cube[u].any()
            continue
        want = np.zeros((3, T, C), dtype=np.float32)
        want[:, :nf[u]] = r["want"]
        floor = r["floor"][:, None, :]
        worst = max(worst, R.worst_ulps(got[u], want, floor))
        want_cube = np.stack([R.cube_ref(want[ch][None], crops[u:u + 1], CROP_FRAMES)[0, 0] for ch in range(3)])
        worst = max(worst, R.worst_ulps(cube[u], want_cube, floor[:, None]))
    print("ULPS delta planes + cubes %s C=%d SVK_CMVN_SPLIT=%s: %.3f ulp beyond the floor (bar 1)" % (shape, C, split, worst))
    assert worst <= 1.0


@pytest.mark.gpu
def test_cube_gather_delta_more_jobs_than_workgroups_and_windows(eng):
    """More crops than the capped grid has workgroups, and windows 1 and 3 (40 columns: 16-byte path with re-read taps; 5:
    scalar), against cube_gather of the planes."""
    n, k, T, cf = eng.num_cu * 16 // 7 + 20, 7, 12, 3
    assert n * k > eng.num_cu * 16
    for C, delta in ((40, 2), (40, 3), (5, 1), (5, 2)):
        x = (np.random.default_rng([n, C]).standard_normal((n, T, C)) * 3.0 + 1.0).astype(np.float32)
        crops = np.tile(np.array([0, T - cf, T - cf + 1, T - 1, T, T + 7, -1], dtype=np.int32), (n, 1))
        crops[1::2] = crops[1::2, ::-1]
        feat = eng.to_device(x)
        stats = eng.delta_cmvn_stats(feat, None, delta=delta, variance=True)
        planes = eng.delta_planes(feat, None, delta=delta, stats=stats)
        want = eng.cube_gather(planes.view(3 * n, T, C), np.repeat(crops, 3, axis=0), cf).view(n, 3, k, cf, C)
        assert torch.equal(eng.cube_gather_delta(feat, crops, cf, delta=delta, stats=stats), want), (C, delta)


@pytest.mark.gpu
def test_bad_arguments_are_error_codes(eng):
    """NULL buffers, negative sizes, delta = 0 and aliased planes are SVK_ERR_BAD_ARG before any launch; empty shapes are
    SVK_OK; the device is healthy afterwards."""
    lib, ctx = eng.lib, eng.ctx
    feat = torch.zeros((2, 100, 40), device=eng.device)
    out = torch.zeros((2, 3, 100, 40), device=eng.device)
    cube = torch.zeros((2, 3, 4, 80, 40), device=eng.device)
    stats = torch.zeros((2, 3, 2, 40), dtype=torch.float64, device=eng.device)
    crops = torch.zeros((2, 4), dtype=torch.int32, device=eng.device)
    p = eng._ptr
    eng._stream()
    BAD, OK = -1, 0
    # svk_delta_cmvn_stats(ctx, feat, n_utt, max_frames, n_cols, n_frames, delta, variance, stats)
    assert lib.svk_delta_cmvn_stats(None, p(feat), 2, 100, 40, None, 2, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, None, 2, 100, 40, None, 2, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, p(feat), 2, 100, 40, None, 2, 1, None) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, p(feat), -1, 100, 40, None, 2, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, p(feat), 2, -100, 40, None, 2, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, p(feat), 2, 100, -40, None, 2, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, p(feat), 2, 100, 40, None, 0, 1, p(stats)) == BAD
    assert lib.svk_delta_cmvn_stats(ctx, None, 0, 100, 40, None, 2, 1, None) == OK
    # svk_delta_planes(ctx, feat, n_utt, max_frames, n_cols, n_frames, delta, stats, out)
    assert lib.svk_delta_planes(None, p(feat), 2, 100, 40, None, 2, None, p(out)) == BAD
    assert lib.svk_delta_planes(ctx, None, 2, 100, 40, None, 2, None, p(out)) == BAD
    assert lib.svk_delta_planes(ctx, p(feat), 2, 100, 40, None, 2, None, None) == BAD
    assert lib.svk_delta_planes(ctx, p(feat), -2, 100, 40, None, 2, None, p(out)) == BAD
    assert lib.svk_delta_planes(ctx, p(feat), 2, 100, 40, None, 0, None, p(out)) == BAD
    assert lib.svk_delta_planes(ctx, p(out), 2, 100, 40, None, 2, None, p(out)) == BAD                  # d_out == d_feat
    assert lib.svk_delta_planes(ctx, None, 0, 100, 40, None, 2, None, None) == OK
    assert lib.svk_delta_planes(ctx, None, 2, 0, 40, None, 2, None, None) == OK
    # svk_cube_gather_delta(ctx, feat, n_utt, max_frames, n_cols, crop_idx, n_crops, crop_frames, delta, stats, out)
    assert lib.svk_cube_gather_delta(None, p(feat), 2, 100, 40, p(crops), 4, 80, 2, None, p(cube)) == BAD
    assert lib.svk_cube_gather_delta(ctx, None, 2, 100, 40, p(crops), 4, 80, 2, None, p(cube)) == BAD
    assert lib.svk_cube_gather_delta(ctx, p(feat), 2, 100, 40, None, 4, 80, 2, None, p(cube)) == BAD
    assert lib.svk_cube_gather_delta(ctx, p(feat), 2, 100, 40, p(crops), 4, 80, 2, None, None) == BAD
    assert lib.svk_cube_gather_delta(ctx, p(feat), 2, 100, 40, p(crops), -4, 80, 2, None, p(cube)) == BAD
    assert lib.svk_cube_gather_delta(ctx, p(feat), 2, 100, 40, p(crops), 4, 80, 0, None, p(cube)) == BAD
    assert lib.svk_cube_gather_delta(ctx, p(feat), 2, 100, 40, p(crops), 4, 101, 2, None, p(cube)) == BAD  # crop longer than the clip
    assert lib.svk_cube_gather_delta(ctx, p(cube), 2, 100, 40, p(crops), 4, 80, 2, None, p(cube)) == BAD   # d_out == d_feat
    assert lib.svk_cube_gather_delta(ctx, None, 0, 100, 40, None, 4, 80, 2, None, None) == OK
    assert lib.svk_cube_gather_delta(ctx, None, 2, 100, 0, None, 4, 80, 2, None, None) == OK
    with pytest.raises(ValueError):
        eng.delta_planes(feat, stats=stats[:, :2])                                # not the [n, 3, 2, cols] statistics
    with pytest.raises(ValueError):
        eng.cube_gather_delta(feat, crops, 80, stats=torch.zeros((2, 2, 40), dtype=torch.float64, device=eng.device))
    with pytest.raises(ValueError):
        eng.delta_cmvn_stats(feat[0])
    torch.cuda.synchronize()
    assert not bool(out.any()) and not bool(cube.any())
