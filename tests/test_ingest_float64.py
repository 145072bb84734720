"""svk_ingest_resample against float64 on both kernels and every branch of them (tests/ingest_f64_ref.py: the reference, the
derived bars, NumPy emulations of resample_kernel and decimate_kernel, their mutants, the case list).

CPU (default pass):
  * the reference is oracle.ingest_ref.resample_poly up to the float32 rounding of the taps;
  * on every random-input case at most 10 % of the int16 intervals hold two values (from the reference alone; 1/1 is held
    to the exactly rounded channel mean instead: half of a two-channel clip's samples ARE ties);
  * the emulations of both kernels pass the float bar and the int16 interval on the GPU cases, and their int16 output is
    sat(rintf(32768 y)) of their float output;
  * every mutant of them fails a bar on some case: the bars have teeth.
GPU (-m gpu): the same cases through Engine.resample with both output types, the strides of the C-ABI through ctypes, and a
batch of zero frames.  Lines starting with "ULPS" carry the measured worst error-to-bar ratio of each case.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ingest_f64_ref as R             # noqa: E402  (tests/ is on sys.path, as for test_c3d2_float64)
from oracle import ingest_ref          # noqa: E402

CASES = R.cases()
IDS = [c["name"] for c in CASES]
SENTINEL_F32, SENTINEL_I16 = 123.0, -21846


def check_row(case, u, got_f32, got_i16, n_out_got=None):
    """One clip's float32 and int16 outputs (whole rows) against the bars.  -> worst error / bar of the float output."""
    pcm, refs = R.case_reference(case)
    y64, bar, _ = refs[u]
    n_out = len(y64)
    assert n_out == R.n_out_of(case["lengths"][u], case["up"], case["down"])
    if n_out_got is not None:
        assert n_out_got == n_out, (case["name"], u, n_out_got, n_out)
    what = "%s, clip %d (%d frames)" % (case["name"], u, case["lengths"][u])
    ratio = R.float_ratio(got_f32[:n_out], y64, bar)
    assert ratio <= 1.0, "float32 output of %s: error / bar = %.3f" % (what, ratio)
    lo, hi = R.int16_interval(y64, bar)
    g = got_i16[:n_out].astype(np.int64)
    bad = np.nonzero((g < lo) | (g > hi))[0]
    assert bad.size == 0, "int16 output of %s: %d samples outside their interval, first m = %d: got %d, interval [%d, %d]" % (
        what, bad.size, bad[0], g[bad[0]], lo[bad[0]], hi[bad[0]])
    assert not got_f32[n_out:].any() and not got_i16[n_out:].any(), "output past out_len of " + what
    np.testing.assert_array_equal(got_i16[:n_out], R.int16_from_float(got_f32[:n_out]), err_msg="int16 against float32 output of " + what)
    return ratio


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_reference_is_the_oracle_up_to_the_taps_rounding():
    """y64 (float32 taps, as uploaded) against oracle.ingest_ref.resample_poly (float64 taps): <= 1e-7, the float32 rounding of
    the taps (relative 6e-8 each, sum |x| |h| <= 1.6 at full scale).  The default taps are the oracle's own design."""
    for case in CASES:
        pcm, refs = R.case_reference(case)
        taps = R.custom_taps() if case["custom"] else None
        if taps is None:
            np.testing.assert_allclose(R.resample_taps(case["up"], case["down"]), ingest_ref.firwin_kaiser(case["up"], case["down"]),
                                       rtol=0, atol=1e-15)
        for u in (0, 1, len(case["lengths"]) - 1):
            n = case["lengths"][u]
            want = ingest_ref.resample_poly(ingest_ref.to_mono(pcm[u, :n]), case["up"], case["down"], taps)
            assert len(want) == len(refs[u][0])
            np.testing.assert_allclose(refs[u][0], want, rtol=0, atol=1e-7, err_msg=case["name"])


def test_two_valued_intervals_are_rare_and_full_scale_hits_the_rails():
    """The int16 bar's condition, from the reference alone: on every random-input case at most 10 % of the samples have an
    interval of two values.  The full-scale cases reach both rails (and overshoot them: the clamp is needed)."""
    shares = []
    for case in CASES:
        _, refs = R.case_reference(case)
        if (case["up"], case["down"]) == (1, 1):
            continue        # the mean of two channels lies ON a tie for every odd sum: held to the exact rint(acc / n_ch) on the GPU instead
        if case["kind"] == "random":
            two = n = 0
            for y64, bar, _ in refs:
                lo, hi = R.int16_interval(y64, bar)
                assert ((hi - lo) <= 1).all()
                two += int((hi != lo).sum())
                n += len(lo)
            shares.append(two / n)
            print("SHARE two-valued int16 intervals, %-45s %.2f %%" % (case["name"] + ":", 100.0 * two / n))
            assert two / n <= 0.10, (case["name"], two / n)
        else:
            v = [32768.0 * r[0] for r in refs]
            print("OVERSHOOT %-45s +32767: %.0f, -32768: %.0f, step: %.0f / %.0f" % (case["name"] + ":", v[0].max(), v[1].min(), v[2].min(), v[2].max()))
            assert v[0].max() > 32767.5 and v[1].min() < -32768.5 and v[2].max() > 32767.5 and v[2].min() < -32768.5
            for (y64, bar, _), rails in zip(refs, ((32767,), (-32768,), (32767, -32768))):
                lo, hi = R.int16_interval(y64, bar)
                for rail in rails:
                    assert ((lo == rail) & (hi == rail)).sum() >= 3
    print("SHARE range: %.2f .. %.2f %%" % (100 * min(shares), 100 * max(shares)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulations_pass_both_bars(case):
    """The emulation of the kernel the library picks for the case, and (where that is decimate_kernel) of the generic kernel
    on the same input: inside the float bar and the int16 interval on every clip."""
    pcm, refs = R.case_reference(case)
    worst = 0.0
    for u, n in enumerate(case["lengths"]):
        worst = max(worst, check_row(case, u, R.emulate(case, pcm[u], n, "f32", u=u), R.emulate(case, pcm[u], n, "i16", u=u)))
        if case["up"] == 1:
            worst = max(worst, check_row(case, u, R.emul_resample(pcm[u], n, 1, case["down"], case["h32"], "f32"),
                                         R.emul_resample(pcm[u], n, 1, case["down"], case["h32"], "i16")))
    print("ULPS emulation %-45s worst error / bar = %.3f" % (case["name"] + ":", worst))


def test_one_to_one_emulation_returns_the_input():
    """1/1: the taps are an exact unit impulse (sinc is 0 at the other integers; resample_taps does not keep np.sinc's ~4e-17
    there), so the chain returns every sample bit for bit, the zero samples of the input included."""
    n_cases = 0
    for case in CASES:
        if (case["up"], case["down"]) != (1, 1):
            continue
        n_cases += 1
        pcm, _ = R.case_reference(case)
        assert case["h32"][10] == np.float32(1.0) and np.count_nonzero(case["h32"]) == 1
        x32 = pcm[0].astype(np.int64).sum(axis=1).astype(np.float32) * (np.float32(1.0) / (np.float32(32768.0) * np.float32(case["n_ch"])))
        assert (x32 == 0).sum() >= 10
        np.testing.assert_array_equal(R.emul_resample(pcm[0], case["frames"], 1, 1, case["h32"], "f32"), x32)
    assert n_cases == 2


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_emulation_fails_a_bar(mutant):
    caught = []
    for case in CASES:
        pcm, refs = R.case_reference(case)
        for u, n in enumerate(case["lengths"]):
            if n == case["frames"] and mutant == "samples past in_len read":
                continue
            try:
                f = R.emulate(case, pcm[u], n, "f32", mutant, u=u)
                i = R.emulate(case, pcm[u], n, "i16", mutant, u=u)
                n_out = len(refs[u][0])
                if len(f) != n_out:                   # the output count itself: the library writes zeros past out_len
                    f = np.concatenate([f, np.zeros(n_out - len(f), dtype=np.float32)])
                    i = np.concatenate([i, np.zeros(n_out - len(i), dtype=np.int16)])
                y64, bar, _ = refs[u]
                lo, hi = R.int16_interval(y64, bar)
                ok = R.float_ratio(f, y64, bar) <= 1.0 and bool(((i >= lo) & (i <= hi)).all())
            except AssertionError:
                ok = False
            if not ok:
                caught.append("%s, clip %d" % (case["name"], u))
                break
        if len(caught) == 3:
            break
    print("MUTANT %s: caught by %s" % (mutant, caught))
    assert caught, mutant


# ---- GPU ----------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def library_input(case, pcm):
    return pcm[:, :, 0] if case["n_ch"] == 1 else pcm


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resample_equals_float64(eng, case):
    """Both output types of one batch: every clip inside the float bar and the int16 interval, zeros past out_len, the garbage
    behind in_len without effect (the reference never saw it), int16 == sat(rintf(32768 float32)) bit for bit."""
    pcm, refs = R.case_reference(case)
    lens = np.array(case["lengths"], dtype=np.int32)
    taps = R.custom_taps() if case["custom"] else R.resample_taps(case["up"], case["down"])
    f32, len_f = eng.resample(library_input(case, pcm), case["up"], case["down"], taps, lengths=lens, out_dtype="f32")
    i16, len_i = eng.resample(library_input(case, pcm), case["up"], case["down"], taps, lengths=lens, out_dtype="i16")
    f32, i16, len_f, len_i = f32.cpu().numpy(), i16.cpu().numpy(), len_f.cpu().numpy(), len_i.cpu().numpy()
    assert f32.dtype == np.float32 and i16.dtype == np.int16
    assert f32.shape == i16.shape == (len(lens), R.n_out_of(case["frames"], case["up"], case["down"]))
    np.testing.assert_array_equal(len_f, len_i)
    worst = 0.0
    for u in range(len(lens)):
        worst = max(worst, check_row(case, u, f32[u], i16[u], len_f[u]))
    print("ULPS resample %-45s worst error / bar = %.3f" % (case["name"] + ":", worst))
    if (case["up"], case["down"]) == (1, 1):
        x32 = pcm.astype(np.int64).sum(axis=2).astype(np.float32) * (np.float32(1.0) / (np.float32(32768.0) * np.float32(case["n_ch"])))
        for u, n in enumerate(lens):
            np.testing.assert_array_equal(f32[u, :n], x32[u, :n])          # the input / 32768 (the channel mean), bit for bit
            # the int16 output is the input, or the channel mean rounded half to even (every odd sum of two channels is a tie)
            np.testing.assert_array_equal(i16[u, :n], np.rint(pcm[u, :n].astype(np.int64).sum(axis=1) / case["n_ch"]).astype(np.int16))


def _raw(eng, case, pcm_t, in_stride, lens_t, clip_in, out_t, out_kind, out_stride, clip_out, len_t):
    from speaker_verification_amd import _lib
    h = eng.to_device(case["h32"])
    eng._stream()
    _lib.check(eng.lib.svk_ingest_resample(eng.ctx, eng._ptr(pcm_t), case["n_ch"], in_stride, eng._ptr(lens_t), clip_in, pcm_t.shape[0],
                                           eng._ptr(h), int(h.numel()), case["up"], case["down"], eng._ptr(out_t),
                                           {"f32": _lib.PCM_F32, "i16": _lib.PCM_I16}[out_kind], out_stride, clip_out, eng._ptr(len_t)),
               eng.ctx)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("name", ["1/3 mono, rows of 8 k + 1 frames", "1/2, 2 channels", "160/441, 1 channel", "1/6 mono (generic, up == 1)"])
@pytest.mark.parametrize("cut", [0, 5, 700])
def test_strides_and_clip_out_through_the_c_abi(eng, name, cut):
    """in_stride > clip_in (full-scale garbage in the padding), out_stride > clip_out (the columns beyond clip_out keep their
    sentinel), clip_out `cut` samples short of the natural count (the output is truncated, out_len clamped)."""
    case = CASES[IDS.index(name)]
    pcm, refs = R.case_reference(case)
    n_utt, frames, n_ch = pcm.shape
    in_stride = frames + 13
    padded = np.empty((n_utt, in_stride, n_ch), dtype=np.int16)
    padded[:, :frames] = pcm
    padded[:, frames:] = 32767
    natural = R.n_out_of(frames, case["up"], case["down"])
    clip_out = natural - cut
    out_stride = clip_out + 7
    lens = np.array(case["lengths"], dtype=np.int32)
    outs = {}
    for kind, dt, sentinel in (("f32", torch.float32, SENTINEL_F32), ("i16", torch.int16, SENTINEL_I16)):
        out = torch.full((n_utt, out_stride), sentinel, dtype=dt, device=eng.device)
        out_len = torch.full((n_utt,), -7, dtype=torch.int32, device=eng.device)
        _raw(eng, case, eng.to_device(padded), in_stride, eng.to_device(lens), frames, out, kind, out_stride, clip_out, out_len)
        got, got_len = out.cpu().numpy(), out_len.cpu().numpy()
        assert (got[:, clip_out:] == sentinel).all(), "columns beyond clip_out were written"
        np.testing.assert_array_equal(got_len, np.minimum([len(r[0]) for r in refs], clip_out))
        outs[kind] = got[:, :clip_out]
    for u, (y64, bar, _) in enumerate(refs):
        n = min(len(y64), clip_out)
        assert R.float_ratio(outs["f32"][u, :n], y64[:n], bar[:n]) <= 1.0
        lo, hi = R.int16_interval(y64[:n], bar[:n])
        assert ((outs["i16"][u, :n] >= lo) & (outs["i16"][u, :n] <= hi)).all()
        assert not outs["f32"][u, n:].any() and not outs["i16"][u, n:].any()
        np.testing.assert_array_equal(outs["i16"][u, :n], R.int16_from_float(outs["f32"][u, :n]))


@gpu
@pytest.mark.parametrize("out_dtype", ["f32", "i16"])
@pytest.mark.parametrize("shape", [(3, 0), (2, 0, 2)])
def test_zero_frames_give_empty_output_and_zero_lengths(eng, shape, out_dtype):
    """A batch without frames: an empty output and out_len == 0 for every clip (the library returns before any launch; the
    lengths must be written all the same)."""
    for up, down in ((1, 3), (160, 441)):
        out, out_len = eng.resample(np.zeros(shape, dtype=np.int16), up, down, R.resample_taps(up, down), out_dtype=out_dtype)
        assert tuple(out.shape) == (shape[0], 0)
        np.testing.assert_array_equal(out_len.cpu().numpy(), np.zeros(shape[0], dtype=np.int32))
    # the C-ABI itself: clip_out == 0 with a lengths array
    from speaker_verification_amd import _lib
    out_len = torch.full((5,), -7, dtype=torch.int32, device=eng.device)
    dummy = torch.zeros((16,), dtype=torch.int16, device=eng.device)
    h = eng.to_device(R.taps32(1, 3))
    eng._stream()
    _lib.check(eng.lib.svk_ingest_resample(eng.ctx, eng._ptr(dummy), 1, 0, None, 0, 5, eng._ptr(h), int(h.numel()), 1, 3, eng._ptr(dummy),
                                           _lib.PCM_I16, 0, 0, eng._ptr(out_len)), eng.ctx)
    torch.cuda.synchronize()
    assert not out_len.cpu().numpy().any()
