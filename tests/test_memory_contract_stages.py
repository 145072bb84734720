"""The memory contract of include/svk.h (Conventions) for the fifteen stage and cube entries of stages.hip, called directly on
guarded arenas (tests/memory_contract.py) in the environments A, B and C, placed for the vector paths (256-byte boundaries) and
for the scalar ones (one element past a boundary).  Every comparison is on bytes, against the Engine wrapper's result for the
same call on ordinary tensors; regions the header calls untouched must still hold the prefill, rows it calls zeroed are zeros,
and elements of an input it calls "not read" hold the payload pattern (0, NaN, a finite other number)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memory_contract as M       # noqa: E402  (tests/ is on sys.path)

pytestmark = pytest.mark.gpu

F32, F64, I32 = torch.float32, torch.float64, torch.int32


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def _each_env(eng, placed, run, ref, what):
    """run(contract) -> {name: bits}; every name of `ref` has the reference's bytes in every environment."""
    for env in M.ENV_NAMES:
        got = run(M.Contract(eng, env, scalar=placed == "scalar"))
        for name, want in ref.items():
            M.same_bits(got[name], want, "%s, %s, environment %s: %s" % (what, placed, env, name))


def _pcm(seed, n, kind):
    g = torch.Generator().manual_seed(seed)
    if kind == "i16":
        return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)
    return torch.randn((n,), generator=g, dtype=F32)


def _i32(values):
    return torch.tensor(values, dtype=I32)


def _rows_below(nf, T):
    """[n][T] bool: row t of clip u lies below n_frames[u]."""
    return torch.arange(T)[None, :] < torch.tensor(nf)[:, None]


# ---- svk_preemphasis ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("kind", ("i16", "f32"))
@pytest.mark.parametrize("n,shift", ((1, 1), (1, 3), (7, 1), (7, 2), (7, 7), (7, 9), (1025, 1), (1025, 2), (1025, 2051)))
def test_preemphasis(eng, n, shift, kind, placed):
    x = _pcm(n + shift, n, kind)
    ref = {"d_out": M.bits(eng.preemphasis(x, shift, 0.98))}

    def run(c):
        dx, out = c.input("d_in", x), c.output("d_out", F32, (n,))
        c.call(eng.lib.svk_preemphasis, dx, 0 if kind == "i16" else 1, n, shift, 0.98, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "svk_preemphasis %s n %d shift %d" % (kind, n, shift))


# ---- svk_stack_frames --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("window", (False, True))
@pytest.mark.parametrize("n,flen,stride,T", ((1001, 400, 160, 6), (37, 25, 10, 4), (5, 9, 1, 3)),
                         ids=("1001-400-160-6", "37-25-10-4", "5-9-1-3"))
def test_stack_frames(eng, n, flen, stride, T, window, placed):
    """(T - 1) * stride + flen exceeds n: the frames' tail is zeros, and nothing is read past the signal's last sample (in B a
    sample from there would be NaN times the window)."""
    assert (T - 1) * stride + flen > n
    sig = M.randn(n, n)
    win = M.randn(flen, flen) if window else None
    ref = {"d_out": M.bits(eng.stack_frames(sig, flen, stride, T, win))}

    def run(c):
        ds, dw, out = c.input("d_sig", sig), c.input("d_window", win), c.output("d_out", F32, (T, flen))
        c.call(eng.lib.svk_stack_frames, ds, n, flen, stride, T, dw, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "svk_stack_frames n %d frame_len %d stride %d frames %d" % (n, flen, stride, T))


# ---- svk_spectrum ------------------------------------------------------------------------------------------------------------
# (nfft, frame_len, frames): the two wave-FFT instances (512: two frames share a transform, so an odd count leaves a half-empty
# one), the LDS radix-2 kernel, the direct DFT; frame_len below, equal to and above nfft on each
SPECTRUM = ((512, 400, 9), (512, 512, 3), (512, 700, 1), (1024, 401, 5), (1024, 1024, 2), (1024, 1100, 3),
            (64, 50, 17), (64, 64, 5), (8, 13, 129), (100, 80, 6), (100, 100, 5), (100, 130, 3))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("power", (0, 1))
@pytest.mark.parametrize("nfft,flen,T", SPECTRUM, ids=["%d-%d-%d" % s for s in SPECTRUM])
def test_spectrum(eng, nfft, flen, T, power, placed):
    frames = M.randn(nfft + flen + T, T, flen)
    ref = {"d_out": M.bits(eng.spectrum(frames, nfft, power))}

    def run(c):
        df, out = c.input("d_frames", frames), c.output("d_out", F32, (T, nfft // 2 + 1))
        c.call(eng.lib.svk_spectrum, df, T, flen, nfft, power, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "svk_spectrum nfft %d frame_len %d frames %d power %d" % (nfft, flen, T, power))


# ---- svk_mel_features --------------------------------------------------------------------------------------------------------
# (frames, bins, filters): the MFMA kernel (64 frames per workgroup) and the kernel for more than 256 filters (16 frames)
MEL = ((70, 257, 40), (65, 129, 256), (17, 65, 257), (33, 65, 300))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("energy", (False, True))
@pytest.mark.parametrize("out_kind", (0, 1, 2))
@pytest.mark.parametrize("T,nbins,nf", MEL, ids=["%d-%d-%d" % m for m in MEL])
def test_mel_features(eng, T, nbins, nf, out_kind, energy, placed):
    power = M.randn(T + nbins, T, nbins).abs() + 0.01
    bank = M.randn(nf + nbins, nf, nbins).abs()
    ceps = 13
    cols = ceps if out_kind == 2 else nf
    f, e = eng.mel_features(power, bank, out_kind, ceps, True, energy)
    ref = {"d_feat": M.bits(f)}
    if energy:
        ref["d_energy"] = M.bits(e)

    def run(c):
        dp, db = c.input("d_power", power), c.input("d_bank", bank)
        feat, en = c.output("d_feat", F32, (T, cols)), c.output("d_energy", F32, (T,)) if energy else None
        c.call(eng.lib.svk_mel_features, dp, T, nbins, db, nf, out_kind, ceps, 1, feat, en)
        return {"d_feat": feat.bits(), "d_energy": en.bits() if energy else None}
    _each_env(eng, placed, run, ref, "svk_mel_features %d frames %d bins %d filters out_kind %d" % (T, nbins, nf, out_kind))


# ---- svk_cmvn ----------------------------------------------------------------------------------------------------------------
CMVN_T, CMVN_C = 300, 13              # two chunks of 256 frames on the split path
CMVN_NF = (0, 1, CMVN_T, 37)


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("variance", (0, 1))
@pytest.mark.parametrize("split", ("0", "1"))
@pytest.mark.parametrize("counts", ("given", "NULL"))
def test_cmvn_in_place(eng, monkeypatch, counts, split, variance, placed):
    """In place: only rows < n_frames hold data, the rows beyond hold the prefill and keep it -- B's NaN rows reach no
    statistic."""
    monkeypatch.setenv("SVK_CMVN_SPLIT", split)
    n = len(CMVN_NF)
    nf = CMVN_NF if counts == "given" else (CMVN_T,) * n
    x = M.randn(variance, n, CMVN_T, CMVN_C) * 3 + 1
    want = M.bits(eng.cmvn_(x.to(eng.device), _i32(nf) if counts == "given" else None, bool(variance)))
    live = _rows_below(nf, CMVN_T).numpy()
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        feat = c.output("d_feat", F32, (n, CMVN_T, CMVN_C))
        for u, k in enumerate(nf):
            feat.tensor[u, :k] = x[u, :k].to(eng.device)
        dn = c.input("d_n_frames", _i32(nf)) if counts == "given" else None
        c.call(eng.lib.svk_cmvn, feat, n, CMVN_T, CMVN_C, dn, variance)
        what = "svk_cmvn split %s variance %d n_frames %s, %s, environment %s" % (split, variance, counts, placed, env)
        got = feat.bits()
        M.same_bits(got[live], want[live], what + ": rows below n_frames")
        M.keeps_prefill(feat, got[~live], what + ": rows at or past n_frames")


# ---- svk_cmvn_stats, svk_delta_cmvn_stats ------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("variance", (0, 1))
@pytest.mark.parametrize("split", ("0", "1"))
@pytest.mark.parametrize("entry", ("svk_cmvn_stats", "svk_delta_cmvn_stats"))
def test_cmvn_statistics(eng, monkeypatch, entry, split, variance, placed):
    """Rows at or past n_frames are not read (they hold the pattern); the statistics of a clip with no rows keep the prefill."""
    monkeypatch.setenv("SVK_CMVN_SPLIT", split)
    n, three = len(CMVN_NF), entry == "svk_delta_cmvn_stats"
    x = M.randn(7 + variance, n, CMVN_T, CMVN_C) * 3 + 1
    nf = _i32(CMVN_NF)
    xd = x.to(eng.device)
    want = M.bits(eng.delta_cmvn_stats(xd, nf, 2, bool(variance)) if three else eng.cmvn_stats(xd, nf, bool(variance)))
    live = _rows_below(CMVN_NF, CMVN_T)[:, :, None].expand(n, CMVN_T, CMVN_C)
    full = np.array([k > 0 for k in CMVN_NF])
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        feat, dn = c.input_where("d_feat", x, live), c.input("d_n_frames", nf)
        stats = c.output("d_stats", F64, (n, 3, 2, CMVN_C) if three else (n, 2, CMVN_C))
        if three:
            c.call(eng.lib.svk_delta_cmvn_stats, feat, n, CMVN_T, CMVN_C, dn, 2, variance, stats)
        else:
            c.call(eng.lib.svk_cmvn_stats, feat, n, CMVN_T, CMVN_C, dn, variance, stats)
        what = "%s split %s variance %d, %s, environment %s" % (entry, split, variance, placed, env)
        got = stats.bits()
        M.same_bits(got[full], want[full], what + ": clips with rows")
        M.keeps_prefill(stats, got[~full], what + ": the clip with no rows")


# ---- svk_cmvnw ---------------------------------------------------------------------------------------------------------------
# (clips' n_frames, max_frames, cols, win): the tile kernel (a clip's columns fit LDS: max_frames <= 3900) with a window longer
# and shorter than the clips, and the sliding kernel
CMVNW = (((50, 0, 17), 50, 13, 301), ((50, 0, 17), 50, 13, 5), ((3905, 1000), 3905, 3, 301))


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("variance,tmp", ((0, "given"), (0, "NULL"), (1, "given")))     # (the variance pass needs d_tmp)
@pytest.mark.parametrize("nf,T,cols,win", CMVNW, ids=("tile-301", "tile-5", "sliding-301"))
def test_cmvnw(eng, nf, T, cols, win, variance, tmp, placed):
    """d_out rows at or past n_frames keep the prefill; d_tmp is a workspace: without the variance pass it keeps its prefill
    entirely and may be NULL, with it its contents on entry change nothing."""
    n = len(nf)
    x = M.randn(T + win, n, T, cols) * 2 + 0.5
    want = M.bits(eng.cmvnw(x, win, bool(variance), _i32(nf)))
    rows = _rows_below(nf, T)
    live, below = rows[:, :, None].expand(n, T, cols), rows.numpy()
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        din, dn = c.input_where("d_in", x, live), c.input("d_n_frames", _i32(nf))
        dtmp = c.output("d_tmp", F32, (n, T, cols)) if tmp == "given" else None
        out = c.output("d_out", F32, (n, T, cols))
        c.call(eng.lib.svk_cmvnw, din, n, T, cols, dn, win, variance, dtmp, out)
        what = "svk_cmvnw %s win %d variance %d d_tmp %s, %s, environment %s" % (nf, win, variance, tmp, placed, env)
        got = out.bits()
        M.same_bits(got[below], want[below], what + ": rows below n_frames")
        M.keeps_prefill(out, got[~below], what + ": d_out rows at or past n_frames")
        if dtmp is not None and not variance:
            M.keeps_prefill(dtmp, dtmp.bits(), what + ": d_tmp")
        elif dtmp is not None:
            M.keeps_prefill(dtmp, dtmp.bits()[~below], what + ": d_tmp rows at or past n_frames")


# ---- svk_derivative ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("delta", (1, 2, 3))
@pytest.mark.parametrize("rows,cols", ((7, 1), (7, 5), (7, 40), (301, 5)))
def test_derivative(eng, rows, cols, delta, placed):
    x = M.randn(rows + cols + delta, rows, cols)
    ref = {"d_out": M.bits(eng.derivative(x, delta))}

    def run(c):
        din, out = c.input("d_in", x), c.output("d_out", F32, (rows, cols))
        c.call(eng.lib.svk_derivative, din, rows, cols, delta, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "svk_derivative %d x %d delta %d" % (rows, cols, delta))


# ---- svk_log_power -----------------------------------------------------------------------------------------------------------
def _power(seed, n):
    p = M.randn(seed, n).abs() * 10.0 ** float(seed % 5)
    p[::7] = 0.0                        # floored at 1e-20
    if n > 3:
        p[3] = 1e-30
    return p


def _log_power_direct(eng, env, placed, p, normalize):
    c = M.Contract(eng, env, scalar=placed == "scalar")
    arena = c.output("d_power", F32, (p.numel(),), prefill=p)
    c.call(eng.lib.svk_log_power, arena, p.numel(), normalize)
    return arena.bits()


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("normalize", (0, 1))
@pytest.mark.parametrize("n", (1, 1000, 70001))
def test_log_power_in_place(eng, n, normalize, placed):
    p = _power(n, n)
    want = M.bits(eng.log_power_(p.to(eng.device), bool(normalize)))
    for env in M.ENV_NAMES:
        M.same_bits(_log_power_direct(eng, env, placed, p, normalize), want,
                    "svk_log_power n %d normalize %d, %s, environment %s" % (n, normalize, placed, env))


def test_log_power_maximum_starts_afresh_at_every_call(eng):
    """The running maximum lives in the handle's fixed scratch.  On a fresh handle: a loud spectrum, then a quiet one (a maximum
    left over from the first call would be subtracted from it), then svk_top1 (a neighbouring scratch slot) and the quiet one
    again -- each time the long-lived handle's bytes."""
    from speaker_verification_amd.engine import Engine
    loud, quiet = _power(4, 1000), _power(1, 1000) * 1e-6
    want_loud, want_quiet = (_log_power_direct(eng, "A", "vector", p, 1) for p in (loud, quiet))
    assert not np.array_equal(want_loud, want_quiet)
    for want in (want_loud, want_quiet):                              # its own maximum was subtracted, not an earlier call's
        assert float(want.view(np.float32).max()) == 0.0
    fresh = Engine(eng.device_index)
    M.same_bits(_log_power_direct(fresh, "B", "vector", loud, 1), want_loud, "the first call of a fresh handle")
    M.same_bits(_log_power_direct(fresh, "C", "vector", quiet, 1), want_quiet, "a quiet spectrum after a loud one")
    fresh.top1(M.randn(3, 300, 65), torch.arange(300, dtype=I32) % 65)
    M.same_bits(_log_power_direct(fresh, "A", "scalar", quiet, 1), want_quiet, "after svk_top1 used the handle")
    M.same_bits(_log_power_direct(fresh, "B", "vector", loud, 1), want_loud, "the loud spectrum again")


# ---- svk_delta_planes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("with_stats", (False, True))
@pytest.mark.parametrize("delta", (2, 3))
@pytest.mark.parametrize("cols", (40, 5))
def test_delta_planes(eng, cols, delta, with_stats, placed):
    """Rows at or past n_frames are not read and are written as zeros in all three planes (130 rows of 40 columns: two jobs
    per clip on the 16-byte path)."""
    T, nf = 130, (130, 0, 77)
    n = len(nf)
    x = M.randn(cols + delta, n, T, cols)
    xd = x.to(eng.device)
    st = eng.delta_cmvn_stats(xd, _i32(nf), delta, True) if with_stats else None
    want = M.bits(eng.delta_planes(xd, _i32(nf), delta, st))
    rows = _rows_below(nf, T)
    assert not want[~rows.numpy()[:, None, :].repeat(3, 1)].any()
    ref = {"d_out": want}

    def run(c):
        feat = c.input_where("d_feat", x, rows[:, :, None].expand(n, T, cols))
        dn, ds = c.input("d_n_frames", _i32(nf)), c.input("d_stats", st.cpu() if with_stats else None)
        out = c.output("d_out", F32, (n, 3, T, cols))
        c.call(eng.lib.svk_delta_planes, feat, n, T, cols, dn, delta, ds, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "svk_delta_planes cols %d delta %d stats %s" % (cols, delta, with_stats))


# ---- svk_cube_gather, svk_cube_gather_cmvn, svk_cube_gather_delta --------------------------------------------------------------
CUBE_T = 100


def _crop_table(cf):
    """Per clip: a start inside, the last full crop, -1 (too short a clip), a start past the end, a start half inside -- the
    last clip's half-inside crop runs toward the trailing guard.  -> (starts [2][5] int32, the rows some crop reads [2][T])."""
    half = CUBE_T - (cf + 1) // 2
    starts = _i32([[10, CUBE_T - cf, -1, CUBE_T + 50, half], [2, CUBE_T - cf, -1, CUBE_T + 1, half]])
    read = torch.zeros((2, CUBE_T), dtype=torch.bool)
    for u in range(2):
        for s in starts[u].tolist():
            if 0 <= s < CUBE_T:
                read[u, s:min(s + cf, CUBE_T)] = True
    assert not read.all() and read[:, -1].all()
    return starts, read


@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("entry", ("svk_cube_gather", "svk_cube_gather_cmvn", "svk_cube_gather_delta-2", "svk_cube_gather_delta-3",
                                   "svk_cube_gather_delta-2-stats"))
@pytest.mark.parametrize("cf", (80, 3))
@pytest.mark.parametrize("cols", (40, 5))
def test_cube_gather(eng, cols, cf, entry, placed):
    """Rows of d_feat that no crop covers hold the pattern: they are not read."""
    starts, read = _crop_table(cf)
    n, k = starts.shape
    x = M.randn(cols + cf, n, CUBE_T, cols)
    xd = x.to(eng.device)
    name, _, rest = entry.partition("-")
    delta = int(rest[0]) if rest else 0
    if name == "svk_cube_gather":
        st, want, shape = None, eng.cube_gather(xd, starts, cf), (n, 1, k, cf, cols)
    elif name == "svk_cube_gather_cmvn":
        st = eng.cmvn_stats(xd, None, True)
        want, shape = eng.cube_gather(xd, starts, cf, stats=st), (n, 1, k, cf, cols)
    else:
        st = eng.delta_cmvn_stats(xd, None, delta, True) if rest.endswith("stats") else None
        want, shape = eng.cube_gather_delta(xd, starts, cf, delta, st), (n, 3, k, cf, cols)
    ref = {"d_out": M.bits(want)}

    def run(c):
        feat = c.input_where("d_feat", x, read[:, :, None].expand(n, CUBE_T, cols))
        idx, ds = c.input("d_crop_idx", starts), c.input("d_stats", st.cpu() if st is not None else None)
        out = c.output("d_out", F32, shape)
        if name == "svk_cube_gather":
            c.call(eng.lib.svk_cube_gather, feat, n, CUBE_T, cols, idx, k, cf, out)
        elif name == "svk_cube_gather_cmvn":
            c.call(eng.lib.svk_cube_gather_cmvn, feat, n, CUBE_T, cols, idx, k, cf, ds, out)
        else:
            c.call(eng.lib.svk_cube_gather_delta, feat, n, CUBE_T, cols, idx, k, cf, delta, ds, out)
        return {"d_out": out.bits()}
    _each_env(eng, placed, run, ref, "%s cols %d crop_frames %d" % (entry, cols, cf))


# ---- svk_cube_draw_crops -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placed", M.PLACED)
@pytest.mark.parametrize("counter", ("given", "NULL"))
@pytest.mark.parametrize("index", ("given", "NULL"))
def test_cube_draw_crops(eng, index, counter, placed):
    """Clips of n_frames <= crop_frames (80 and 5 here) get -1 and add one each to the counter the caller zeroes."""
    nf, n_crops, cf, seed, first = _i32([81, 80, 500, 5, 200]), 20, 80, 0x9E3779B97F4A7C15, 1000
    gi = torch.tensor([5, 2 ** 40, 0, 7, 3], dtype=torch.int64) if index == "given" else None
    want = eng.draw_crops(nf, n_crops, cf, seed, first, None, gi)
    assert (want.cpu()[[1, 3]] == -1).all() and (want.cpu()[[0, 2, 4]] >= 0).all()
    for env in M.ENV_NAMES:
        c = M.Contract(eng, env, scalar=placed == "scalar")
        dn, di = c.input("d_n_frames", nf), c.input("d_utt_index", gi)
        out = c.output("d_crop_idx", I32, (5, n_crops))
        bad = c.counter("d_bad_count") if counter == "given" else None
        c.call(eng.lib.svk_cube_draw_crops, dn, 5, first, di, n_crops, cf, seed, out, bad)
        what = "svk_cube_draw_crops utt_index %s bad_count %s, %s, environment %s" % (index, counter, placed, env)
        M.same_bits(out.bits(), M.bits(want), what)
        if bad is not None:
            M.counter_is(bad, 2, what + ": d_bad_count")
