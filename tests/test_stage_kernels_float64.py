"""The stage kernels of the speechpy drop-in (csrc/stages.hip: svk_preemphasis, svk_stack_frames, svk_spectrum,
svk_mel_features) against float64 on every kernel and launch path (tests/stages_f64_ref.py: the float64 restatements, the
float32 yardstick of the FFT paths, the bars -- derived for pre-emphasis, framing, the direct DFT and the mel stage,
measured against the yardstick with K = 4 for the three FFT kernels).

CPU (default pass):
  * the restatements equal oracle.speechpy_ref on the golden speechpy vectors to 1e-12;
  * every planted fault (stages_f64_ref.MUTANTS, 15 of them) fails the bars on the GPU tests' own inputs;
  * no mel element of any case is left out as a possible float32 underflow.
GPU (-m gpu): every launch goes through Engine.preemphasis / stack_frames / spectrum / mel_features (ctypes for the one
argument check).  Which kernel a spectrum launch runs follows from nfft alone (svk_spectrum): 512 and 1024 the wave FFT
(two frames per transform at 512), every other power of two from 4 to 8192 the Stockham kernel, anything else the direct
DFT.  The shapes sit on the kernels' edges: pairs, frames per workgroup, chunk and tile sizes, and one launch per kernel
past the capped grid (8 workgroups per CU, read from the engine), so that the grid-stride loop wraps.  Lines starting
with "ULPS" carry the worst error / bar of each spectrum case.

Two kernel changes came out of these tests (DESIGN section 4 has the figures).  spectrum_fft_kernel<false> (nfft 512)
packs two frames into one complex transform and separates them only to rounding, so a frame of zeros beside a non-zero
frame came back with about 3e-15 of its partner's power where SpeechPy has an exact 0 (log_power_spectrum: about -81 dB
where the reference has its floor, -200); the kernel now flags silent frames as frontend.hip does, and
test_silent_frames_* and the speech-like nfft-512 cases hold it.  The mel kernels' float32 library logarithm was up to
2.2 ulp32 off, past the 2 ulp32 of the log bar at one bin (test_mel_features[T64-bins1-nf128]: 1.03 x the bar); they now
round a float64 logarithm once.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import stages_f64_ref as R                                     # noqa: E402  (tests/ is on sys.path)
from oracle import speechpy_ref as ref                         # noqa: E402
from speaker_verification_amd import synth                     # noqa: E402

MFE, LMFE, MFCC = R.MFE, R.LMFE, R.MFCC
NOMINAL_CU = 256          # only for sizing the CPU tests' view of the grid cases; the GPU tests read the engine's count


# ---- inputs -----------------------------------------------------------------------------------------------------------
def noise(seed, shape, scale):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def speech_like(seed, T, flen):
    """A loud frame, a frame 2^-12 of a loud one, a frame of zeros, cycled: over six frames each kind lands on both halves
    of an nfft-512 pair."""
    x = noise(seed, (T, flen), 2.0 ** 15)
    x[1::3] *= np.float32(2.0 ** -12)
    x[2::3] = 0
    return x


def family(name, seed, T, flen):
    if name == "speech":
        return speech_like(seed, T, flen)
    return noise(seed, (T, flen), {"hi": 2.0 ** 15, "lo": 2.0 ** -20}[name])


# ---- spectrum cases ---------------------------------------------------------------------------------------------------
def pow2_fpb(nfft):
    """Frames per workgroup of spectrum_pow2_kernel: 256 / min(256, nfft / 4) threads per frame."""
    return 256 // max(1, min(256, nfft // 4))


def kernel_of(nfft):
    if nfft == 512:
        return "fft512"
    if nfft == 1024:
        return "fft1024"
    if nfft & (nfft - 1) == 0 and 4 <= nfft <= 8192:
        return "pow2"
    return "dft"


def grid_frames(nfft, num_cu):
    """One frame count past what the capped grid covers in one sweep."""
    per_block = {"fft512": 8, "fft1024": 4, "pow2": pow2_fpb(nfft), "dft": 4}[kernel_of(nfft)]
    return 8 * num_cu * per_block + 1


def spectrum_cases():
    """(nfft, frame_len, frame count or "grid", family).  A covering selection: every frame count and every frame
    length of each kernel with both noise families, the speech-like batch per kernel, one grid case per kernel."""
    cases = []
    counts = [1, 2, 3, 7, 8, 9]
    for i, flen in enumerate([1, 64, 400, 511, 512, 513, 700]):
        cases += [(512, flen, counts[i % 6], "hi"), (512, flen, counts[(i + 3) % 6], "lo")]
    cases += [(512, 400, 9, "speech"), (512, 512, 8, "speech"), (512, 64, 7, "speech"), (512, 64, "grid", "hi")]
    counts = [1, 3, 4, 5]
    for i, flen in enumerate([1, 2, 401, 1023, 1024, 1025, 1100]):
        cases += [(1024, flen, counts[i % 4], "hi"), (1024, flen, counts[(i + 2) % 4], "lo")]
    cases += [(1024, 401, 5, "speech"), (1024, 401, "grid", "lo")]
    for nfft in (4, 8, 16, 32, 64, 256, 2048, 8192):
        fpb = pow2_fpb(nfft)
        flens = [nfft - 1, nfft, nfft + 3, max(1, nfft // 2 - 1)]
        for i, T in enumerate(sorted({1, fpb - 1, fpb, fpb + 1} - {0})):
            cases.append((nfft, flens[i % 4], T, ("hi", "lo")[i % 2]))
        cases += [(nfft, flens[(nfft // 4) % 3], 3, ("lo", "hi")[(nfft // 4) % 2]), (nfft, nfft - 1, fpb + 1, "speech")]
    cases.append((8, 8, "grid", "hi"))
    counts = [1, 3, 4, 5]
    for i, nfft in enumerate((2, 3, 5, 6, 12, 255, 400, 1000, 1023)):
        for j, flen in enumerate((max(1, nfft - 1), nfft, nfft + 3)):
            cases.append((nfft, flen, counts[(i + j) % 4], ("hi", "lo")[(i + j) % 2]))
        cases.append((nfft, max(1, nfft - 1), 5, "speech"))
    cases += [(16384, 160, 8, "hi"), (16384, 160, 8, "speech"), (12, 12, "grid", "lo")]
    return cases


SPECTRUM_CASES = spectrum_cases()


def _sid(c):
    return "%s-nfft%d-flen%d-T%s-%s" % (kernel_of(c[0]), c[0], c[1], c[2], c[3])


@functools.lru_cache(maxsize=None)
def spectrum_input(case, num_cu=NOMINAL_CU):
    nfft, flen, T, fam = case
    T = grid_frames(nfft, num_cu) if T == "grid" else T
    fr = family(fam, 1000 + nfft + 7 * flen, T, flen)
    fr.setflags(write=False)
    amp, pw = R.spectrum(fr, nfft)
    return fr, (amp, pw)


def judge_spectrum(got_amp, got_pow, case, fr, want):
    """Both outputs of one case against the bar of the kernel that runs it -> (amplitude verdict, power verdict, margin)."""
    nfft = case[0]
    if kernel_of(nfft) == "dft":
        return R.dft_judge(got_amp, fr, nfft, False, ref=want), R.dft_judge(got_pow, fr, nfft, True, ref=want), 1
    pair = nfft == 512
    margin = R.margin512(fr)[0] if pair else R.K
    return (R.fft_judge(got_amp, fr, nfft, False, pair, margin, ref=want),
            R.fft_judge(got_pow, fr, nfft, True, pair, margin, ref=want), margin)


# ---- pre-emphasis and framing cases -----------------------------------------------------------------------------------
COFS = (0.98, 0.5, 1.0, 0.0)


def preemph_shifts(n):
    return (0, 1, 2, n - 1, n, n + 1, -1, -(n + 3), 2 ** 31 - 1)


def preemph_signal(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "i16":
        x = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
        x[0] = -32768                                    # the rails, next to each other
        if n > 1:
            x[1] = 32767
        return x
    return noise(seed, n, (2.0 ** 15, 2.0 ** -20)[seed % 2])


def preemph_cases(sizes=(1, 2, 255, 256, 257)):
    """(n, kind, shift, cof): every shift on every small size with both PCM types, the coefficients cycling."""
    out = []
    for n in sizes:
        for kind in ("i16", "f32"):
            for i, s in enumerate(preemph_shifts(n)):
                out.append((n, kind, s, COFS[(i + n + (kind == "f32")) % 4]))
    return out


def hamming32(n):
    return np.hamming(n).astype(np.float32) if n > 1 else np.array([0.75], dtype=np.float32)


def frame_cases():
    """(frame_len, stride, T, n, windowed): per geometry a signal that ends exactly at the last frame's end, one that is one
    sample short of it, and one so short that the last two frames are all padding; with and without a window."""
    out = []
    for flen, stride in ((1, 1), (7, 3), (400, 160), (400, 400), (320, 500), (512, 1)):
        T = 5
        end = (T - 1) * stride + flen
        for n in (end, end - 1, max(1, (T - 2) * stride)):
            for win in (False, True):
                out.append((flen, stride, T, n, win))
    return out


def frame_input(case):
    flen, stride, T, n, win = case
    sig = noise(flen * 31 + stride + n, n, (2.0 ** 15, 2.0 ** -20)[n % 2])
    return sig, (hamming32(flen) if win else None)


# ---- mel cases ----------------------------------------------------------------------------------------------------------
def mel_triples():
    """(T, nbins, nf): about twenty triples of the MFMA kernel that hold every value of every axis, and the wide-bank
    kernel's (not the product)."""
    Ts, bins = [1, 15, 16, 17, 63, 64, 65, 130], [1, 63, 64, 65, 129, 257]
    nfs = [1, 15, 16, 17, 63, 64, 65, 128, 129, 256]
    out = []
    for i in range(20):
        out.append((Ts[(3 * i) % 8], bins[(5 * i + i // 6) % 6], nfs[i % 10]))
    wide_T, wide_bins = [1, 15, 16, 17, 33], [65, 129]
    for i, nf in enumerate((257, 300, 1024, 257, 300, 1024)):
        out.append((wide_T[(2 * i + i // 5) % 5], wide_bins[i % 2 if i < 3 else (i + 1) % 2], nf))
    return out


MEL_TRIPLES = mel_triples()


def _covers():
    t = MEL_TRIPLES[:20]
    assert {c[0] for c in t} == {1, 15, 16, 17, 63, 64, 65, 130}
    assert {c[1] for c in t} == {1, 63, 64, 65, 129, 257}
    assert {c[2] for c in t} == {1, 15, 16, 17, 63, 64, 65, 128, 129, 256}
    w = MEL_TRIPLES[20:]
    assert {c[0] for c in w} == {1, 15, 16, 17, 33} and {c[1] for c in w} == {65, 129} and {c[2] for c in w} == {257, 300, 1024}


_covers()


def mel_bank(kind, nf, nbins):
    """dense: every entry distinct, in (0, 1], one all-zero filter row (nf > 1); banded: non-negative triangles;
    signed: the dense bank with alternating signs."""
    f, k = np.arange(nf)[:, None], np.arange(nbins)[None, :]
    dense = (1.0 + f * nbins + k) / (nf * nbins + 1.0)
    if kind == "banded":
        centre = (f + 0.5) * nbins / nf
        width = max(2.0, 2.5 * nbins / nf)
        b = np.maximum(0.0, 1.0 - np.abs(k - centre) / width) * (0.5 + dense)
    elif kind == "signed":
        b = dense * np.where((f + k) % 2 == 0, 1.0, -1.0)
    else:
        b = dense.copy()
        if nf > 1:
            b[nf // 2] = 0.0
    return b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def mel_power(T, nbins, fam):
    """Power rows: squares of the noise families; speech-like rows cycle loud / 2^-24 of loud / zero.  hi and lo carry one
    zero frame (T > 1)."""
    g = np.random.default_rng(77 + T * 1000 + nbins).standard_normal((T, nbins))
    p = (g * g + 1e-3) * {"hi": 2.0 ** 30, "lo": 2.0 ** -40, "speech": 2.0 ** 30}[fam]
    if fam == "speech":
        p[1::3] *= 2.0 ** -24
        p[2::3] = 0
    elif T > 1:
        p[T // 2] = 0
    p = p.astype(np.float32)
    p.setflags(write=False)
    return p


def mel_launches(T, nbins, nf):
    """(family, bank kind, out_kind, num_ceps, dc_elimination, want_energy) of one triple."""
    ceps = sorted({1, min(13, nf), nf})
    out = [("hi", "dense", MFE, 1, True, True), ("lo", "dense", LMFE, 1, True, False),
           ("speech", "dense", LMFE, 1, True, True), ("lo", "signed", MFE, 1, True, True),
           ("hi", "banded", LMFE, 1, True, False)]
    for i, nc in enumerate(ceps):
        fam = ("hi", "lo", "speech")[i % 3]
        out += [(fam, "dense", MFCC, nc, True, i % 2 == 0), (fam, "dense", MFCC, nc, False, i % 2 == 1)]
    out.append(("speech", "banded", MFCC, min(13, nf), True, False))
    return out


@functools.lru_cache(maxsize=None)
def mel_reference(T, nbins, nf, fam, kind, num_ceps):
    p, b = mel_power(T, nbins, fam), mel_bank(kind, nf, nbins)
    want = R.mel(p, b, num_ceps)
    return p, b, want, R.mel_bars(p, b, want)


def mel_output(res, out_kind, num_ceps, dc):
    if out_kind == MFE:
        return res["mel"]
    if out_kind == LMFE:
        return res["logmel"]
    return (res["ceps_dc"] if dc else res["ceps_nodc"])[:, :num_ceps]


# =======================================================================================================================
# CPU
# =======================================================================================================================
def test_restatements_are_the_oracle(golden):
    g = golden["speechpy"]
    tight = dict(rtol=1e-12, atol=1e-12)
    short = synth.noise_clip(*g["short_seed"])
    np.testing.assert_allclose(R.preemphasis(short, 1, 0.98, cof32=False)[0], g["pre_short_i16"], **tight)
    np.testing.assert_allclose(R.preemphasis(short, 3, 0.5)[0], g["pre_short_shift3"], **tight)
    for shift in (0, 1, 5, -1, 4001, -4003, 2 ** 31 - 1):
        np.testing.assert_array_equal(R.preemphasis(short, shift, 0.5)[0], ref.preemphasis(short, shift, 0.5))
    x = short.astype(float)
    np.testing.assert_array_equal(R.frames(x, 320, 160, 23), g["frames_nopad"])
    np.testing.assert_array_equal(R.frames(x, 320, 320, 12), g["frames_pad"])
    np.testing.assert_allclose(R.frames(x, 400, 160, 23, np.hamming(400)), g["frames_hamming"], **tight)
    fr = g["frames_nopad"]
    np.testing.assert_allclose(R.spectrum(fr, 512)[0], g["fftmag_512"], **tight)
    np.testing.assert_allclose(R.spectrum(fr, 512)[1], g["pow_512"], rtol=1e-12, atol=1e-6)
    np.testing.assert_allclose(R.spectrum(g["frames_hamming"], 1024)[1], g["pow_1024"], rtol=1e-12, atol=1e-6)
    np.testing.assert_allclose(R.spectrum(fr, 256)[1], g["pow_256_crop"], rtol=1e-12, atol=1e-6)
    for nfft in (12, 255, 700):
        np.testing.assert_allclose(R.spectrum(fr, nfft)[0], ref.fft_spectrum(fr[:, :nfft], nfft), rtol=1e-12, atol=1e-7)
    one = synth.noise_clip(*g["one_seed"])
    power = ref.power_spectrum(ref.stack_frames(one.astype(float), 16000, 0.020, 0.010, zero_padding=False), 512)
    m = R.mel(power, g["fb_A"], 13)
    np.testing.assert_allclose(m["mel"], g["mfe_A_feat"], rtol=1e-12)
    np.testing.assert_allclose(m["energy"], g["mfe_A_energy"], rtol=1e-12)
    np.testing.assert_allclose(m["logmel"], g["lmfe_A"], **tight)
    np.testing.assert_allclose(m["ceps_dc"], g["mfcc_A"], rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(m["ceps_nodc"], g["mfcc_A_nodc"], rtol=1e-12, atol=1e-11)
    np.testing.assert_allclose(R.mel(power, g["fb_A"], 40)["ceps_dc"], g["mfcc_A_40"], rtol=1e-12, atol=1e-11)
    zero = R.mel(np.zeros((3, 257)), g["fb_A"], 13)
    np.testing.assert_allclose(zero["ceps_dc"], np.repeat(g["mfcc_A_zero"][:1], 3, axis=0), rtol=1e-12, atol=1e-11)


def test_references_pass_their_own_bars_and_nothing_is_left_out():
    """The float32-rounded reference passes every bar (so a correct kernel can), the yardstick passes the FFT bar, and no
    mel element of any launch is left out."""
    for case in SPECTRUM_CASES:
        if case[2] == "grid":
            continue
        fr, want = spectrum_input(case)
        a, p, _ = judge_spectrum(want[0].astype(np.float32), want[1].astype(np.float32), case, fr, want)
        assert a["ok"] and p["ok"], (_sid(case), a["why"], p["why"])
        if kernel_of(case[0]) != "dft":
            y = R.yardstick32(fr, case[0])
            assert R.fft_judge(y, fr, case[0], False, case[0] == 512, ref=want)["ratio"] <= 1.0 + 1e-9
    left = 0
    for T, nbins, nf in MEL_TRIPLES:
        for fam, kind, out_kind, nc, dc, en in mel_launches(T, nbins, nf):
            p, b, want, bars = mel_reference(T, nbins, nf, fam, kind, nc)
            got = mel_output(want, out_kind, nc, dc).astype(np.float32)
            v = R.mel_judge(got, want["energy"].astype(np.float32) if en else None, p, b, out_kind, nc, dc, want, bars)
            assert v["ok"], ((T, nbins, nf), fam, kind, out_kind, nc, dc, v["why"])
            left += v["left_out"]
            if kind != "signed":
                assert (want["mel_raw"] >= 0).all()
    assert left == 0


def _spectrum_applies(mutant, case, fr):
    nfft, flen = case[0], case[1]
    x = R.seen(fr, nfft)
    return {"wrap": flen < nfft, "fold": flen > nfft, "div_flen": flen != nfft, "no_nyquist": nfft % 2 == 0,
            "bin_mirror": min(flen, nfft) > 1, "pair_swap": len(fr) >= 2,
            "silent_leak": any(x[i].any() != x[i + 1].any() for i in range(0, len(fr) - 1, 2))}[mutant]


@pytest.mark.parametrize("mutant", R.MUTANTS["spectrum"])
def test_spectrum_mutants_fail_the_bar(mutant):
    hit = set()
    for case in SPECTRUM_CASES:
        if case[2] == "grid":
            continue
        fr, want = spectrum_input(case)
        if not _spectrum_applies(mutant, case, fr):
            continue
        amp, pw = R.spectrum(fr, case[0], mutant)
        a, p, _ = judge_spectrum(amp.astype(np.float32), pw.astype(np.float32), case, fr, want)
        assert not (a["ok"] and p["ok"]), (mutant, _sid(case))
        hit.add(kernel_of(case[0]))
    assert hit == {"fft512", "fft1024", "pow2", "dft"}, (mutant, hit)


def test_preemphasis_mutant_fails_the_bar():
    n_hit = 0
    for n, kind, shift, cof in preemph_cases():
        if (2 * shift) % n == 0 or cof == 0.0:
            continue
        x = preemph_signal(n, kind, n + abs(shift) % 97)
        y, cx = R.preemphasis(x, shift, cof)
        bad, _ = R.preemphasis(x, shift, cof, mutant="shift_sign")
        assert not (np.abs(bad - y) <= R.preemph_bar(y, cx)).all(), (n, kind, shift, cof)
        n_hit += 1
    assert n_hit > 20


@pytest.mark.parametrize("mutant", R.MUTANTS["frames"])
def test_framing_mutants_fail_the_bar(mutant):
    n_hit = 0
    for case in frame_cases():
        flen, stride, T, n, win = case
        sig, window = frame_input(case)
        padded = (T - 1) * stride + flen > n
        if (mutant == "pad_last" and not padded) or (mutant == "window_shift" and (not win or flen == 1)):
            continue
        want = R.frames32(sig, flen, stride, T, window)
        assert not np.array_equal(R.frames(sig, flen, stride, T, window, mutant, np.float32), want), case
        n_hit += 1
    assert n_hit >= 10


@pytest.mark.parametrize("mutant", R.MUTANTS["mel"])
def test_mel_mutants_fail_the_bar(mutant):
    hit = set()
    for T, nbins, nf in MEL_TRIPLES:
        for fam, kind, out_kind, nc, dc, en in mel_launches(T, nbins, nf):
            p, b, want, bars = mel_reference(T, nbins, nf, fam, kind, nc)
            applies = {"energy_64_bins": nbins > 64 and (en or (out_kind == MFCC and dc)),
                       "no_eps": kind != "signed" and (
                           ((want["mel_raw"] == 0).any() and (out_kind != MFCC or nc > 1 or not dc))
                           or ((want["energy_raw"] == 0).any() and (en or (out_kind == MFCC and dc)))),
                       "dct_row0": out_kind == MFCC and not dc and nf > 1,
                       "c0_replaced": out_kind == MFCC and not dc,
                       # (judged on the mel outputs: one bin's share of one filter is inside a long cepstrum chain's bar)
                       "filter_last_bin": kind == "dense" and out_kind != MFCC and nf // 2 != nf - 1}[mutant]
            if not applies:
                continue
            bad = R.mel(p, b, nc, mutant)
            with np.errstate(over="ignore"):
                got = mel_output(bad, out_kind, nc, dc).astype(np.float32)
                e = bad["energy"].astype(np.float32) if en else None
            v = R.mel_judge(got, e, p, b, out_kind, nc, dc, want, bars)
            assert not v["ok"], (mutant, (T, nbins, nf), fam, kind, out_kind, nc, dc)
            hit.add("mfma" if nf <= 256 else "wide")
    assert hit == {"mfma", "wide"}, (mutant, hit)


def test_mutant_count():
    """15 planted faults, every one of them fails (the parametrised tests above run each)."""
    names = [m for group in R.MUTANTS.values() for m in group]
    assert len(names) == len(set(names)) == 15


def test_emulation_of_the_packed_path_stays_within_the_margin():
    """The packed path's float32 emulation on the nfft-512 cases: the margin it gives is K unless it exceeds K itself."""
    for case in SPECTRUM_CASES:
        if case[0] != 512 or case[2] == "grid":
            continue
        fr, want = spectrum_input(case)
        margin, r = R.margin512(fr)
        assert margin == (R.K if r <= R.K else min(16.0, 2 * r)), (_sid(case), r)
        assert R.fft_judge(R.emulation_packed512(fr), fr, 512, False, True, margin, ref=want)["ok"]


# =======================================================================================================================
# GPU
# =======================================================================================================================
@pytest.fixture(scope="module")
def eng():
    from speaker_verification_amd.engine import get_engine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return get_engine(0)


def run_spectrum(eng, fr, nfft):
    dev = eng.to_device(np.asarray(fr))
    amp, pw = eng.spectrum(dev, nfft, False), eng.spectrum(dev, nfft, True)
    torch.cuda.synchronize()
    return amp.cpu().numpy(), pw.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPECTRUM_CASES, ids=[_sid(c) for c in SPECTRUM_CASES])
def test_spectrum(eng, case):
    fr, want = spectrum_input(case, eng.num_cu)
    got_amp, got_pow = run_spectrum(eng, fr, case[0])
    assert got_amp.shape == got_pow.shape == (fr.shape[0], case[0] // 2 + 1)
    a, p, margin = judge_spectrum(got_amp, got_pow, case, fr, want)
    print("ULPS %s frames=%d amplitude %.3f (margin %g) power %.3f (of 1)%s"
          % (_sid(case), fr.shape[0], a["ratio"], margin, p["ratio"], " yardstick %.3g" % a["y"] if "y" in a else ""))
    assert a["ok"], a["why"]
    assert p["ok"], p["why"]


def _loud_and_silent():
    """[loud, 0, 0, loud, 0]: a silent frame second of a pair and first of a pair beside a loud partner, and last alone."""
    fr = noise(5, (5, 400), 1000.0)
    fr[[1, 2, 4]] = 0
    return fr


@pytest.mark.gpu
def test_silent_frames_are_exact_zeros_at_512(eng):
    fr = _loud_and_silent()
    amp, pw = run_spectrum(eng, fr, 512)
    for out in (amp, pw):
        assert (out[[0, 3]] > 0).any()
        leak = np.abs(out[[1, 2, 4]]).max() / out[[0, 3]].max()
        print("ULPS silent frames at nfft 512: worst bin / the partner's peak = %.3g, non-zero bins %d"
              % (leak, int((out[[1, 2, 4]] != 0).sum())))
        assert same(out[[1, 2, 4]], np.zeros((3, 257), dtype=np.float32))
    # a quiet but non-zero frame is not silent: it keeps its bins (and the packing's 2^-24 x amplitude-ratio error)
    fr2 = noise(6, (2, 400), 1000.0)
    fr2[1] = 0
    fr2[1, 17] = 1e-3
    amp2, _ = run_spectrum(eng, fr2, 512)
    assert (amp2[1] != 0).any()
    v = R.fft_judge(amp2, fr2, 512, False, True, R.margin512(fr2)[0])
    assert v["ok"], v["why"]


@pytest.mark.gpu
def test_silent_frames_through_the_drop_in(eng):
    from speaker_verification_amd.speechpy import processing
    fr = _loud_and_silent()
    p = processing.power_spectrum(fr, 512)
    assert p.dtype == np.float64 and (p[[1, 2, 4]] == 0).all() and (p[[0, 3]] > 0).all()
    lp = processing.log_power_spectrum(fr, 512, normalize=False)
    assert (lp[[1, 2, 4]] == -200.0).all(), lp[[1, 2, 4]].max()
    want = ref.log_power_spectrum(fr.astype(np.float64), 512, normalize=False)
    np.testing.assert_allclose(lp[[0, 3]], want[[0, 3]], rtol=0, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("nfft,flen,T", [(512, 400, 9), (512, 700, 7), (1024, 401, 5), (4, 4, 258), (8, 5, 129), (64, 64, 17),
                                         (2048, 700, 3), (8192, 8192, 2), (12, 12, 9), (400, 403, 5), (1000, 160, 6)])
def test_a_frame_alone_equals_itself_in_the_batch(eng, nfft, flen, T):
    """A result does not depend on where in the batch (which wave, workgroup slot or loop trip) a frame is computed.  At
    nfft 512 the unit is the pair (2i, 2i + 1) -- a frame's rounding depends on its partner -- and an odd batch's last
    frame, which must equal that frame run alone."""
    fr = speech_like(3, T, flen) if nfft != 8192 else noise(3, (T, flen), 2.0 ** 15)
    amp, pw = run_spectrum(eng, fr, nfft)
    step = 2 if nfft == 512 else 1
    picks = sorted({0, (T // 2) // step * step, (T - 1) // step * step})
    for i in picks:
        a1, p1 = run_spectrum(eng, fr[i:i + step], nfft)
        assert same(a1, amp[i:i + step]) and same(p1, pw[i:i + step]), (nfft, i)


@pytest.mark.gpu
def test_dft_length_beyond_lds_is_refused_before_any_launch(eng):
    from speaker_verification_amd import _lib
    nfft = eng.lds_per_cu // 8 + 3                      # the twiddle table alone (8 bytes a point) exceeds the device's LDS
    assert kernel_of(nfft) == "dft"
    fr = eng.to_device(noise(1, (2, 16), 1.0))
    out = torch.full((2, nfft // 2 + 1), -7.0, dtype=torch.float32, device=eng.device)
    eng._stream()
    rc = eng.lib.svk_spectrum(eng.ctx, C.c_void_p(fr.data_ptr()), 2, 16, nfft, 1, C.c_void_p(out.data_ptr()))
    msg = eng.lib.svk_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    assert rc == _lib.SVK_ERR_UNSUPPORTED and "fft_points" in msg, (rc, msg)
    assert bool((out == -7.0).all())                   # nothing ran
    with pytest.raises(_lib.SvkError, match="fft_points"):
        eng.spectrum(fr, nfft, True)
    # the largest power of two on this path still runs (spectrum_cases has it); the handle is usable afterwards
    amp, _ = run_spectrum(eng, noise(2, (1, 5), 1.0), 5)
    assert np.isfinite(amp).all()


# ---- pre-emphasis -----------------------------------------------------------------------------------------------------
def check_preemphasis(eng, x, shift, cof):
    got = eng.preemphasis(x, shift=shift, cof=cof).cpu().numpy()
    y, cx = R.preemphasis(x, shift, cof)
    assert got.shape == y.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= R.preemph_bar(y, cx)).all(), (x.size, x.dtype, shift, cof, float((err / np.maximum(R.preemph_bar(y, cx), 1e-300)).max()))
    if cof in (0.5, 1.0, 0.0):                           # c x_j is exact in float32: one rounding, of the exact difference
        assert same(got, y.astype(np.float32)), (x.size, x.dtype, shift, cof)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_preemphasis_small(eng, n):
    for nn, kind, shift, cof in preemph_cases((n,)):
        check_preemphasis(eng, preemph_signal(nn, kind, nn + abs(shift) % 97), shift, cof)
    x = preemph_signal(n, "i16", 9)
    for cof in COFS:                                     # every coefficient with the rails adjacent
        check_preemphasis(eng, x, 1, cof)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_preemphasis_past_the_capped_grid(eng, kind):
    n = 8 * eng.num_cu * 256 + 3                         # 524 288 + 3 on 256 CUs: the grid-stride loop wraps
    x = preemph_signal(n, kind, 4)
    for i, shift in enumerate(preemph_shifts(n)):
        check_preemphasis(eng, x, shift, COFS[i % 4])


# ---- framing ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stack_frames_is_bit_exact(eng):
    for case in frame_cases():
        flen, stride, T, n, win = case
        sig, window = frame_input(case)
        got = eng.stack_frames(sig, flen, stride, T, window).cpu().numpy()
        assert same(got, R.frames32(sig, flen, stride, T, window)), case
        # float32 framing is the float64 framing rounded: zeros past the end, one multiply
        np.testing.assert_allclose(got, R.frames(sig, flen, stride, T, window), rtol=2.0 ** -24, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("win", [False, True])
def test_stack_frames_past_the_capped_grid(eng, win):
    flen, stride = 512, 1
    T = 8 * eng.num_cu * 256 // flen + 77               # T * flen elements: past one sweep of the capped grid
    n = T + flen - 1 - 40                                # the last 40 frames reach into the padding
    sig = noise(8, n, 2.0 ** 15)
    window = hamming32(flen) if win else None
    got = eng.stack_frames(sig, flen, stride, T, window).cpu().numpy()
    assert same(got, R.frames32(sig, flen, stride, T, window))


# ---- mel / log / DCT ------------------------------------------------------------------------------------------------------
def run_mel(eng, p, b, out_kind, nc, dc, en):
    feat, energy = eng.mel_features(p, b, out_kind, nc, dc, want_energy=en)
    torch.cuda.synchronize()
    return feat.cpu().numpy(), (energy.cpu().numpy() if en else None)


@pytest.mark.gpu
@pytest.mark.parametrize("T,nbins,nf", MEL_TRIPLES, ids=["T%d-bins%d-nf%d" % t for t in MEL_TRIPLES])
def test_mel_features(eng, T, nbins, nf):
    worst = 0.0
    for fam, kind, out_kind, nc, dc, en in mel_launches(T, nbins, nf):
        p, b, want, bars = mel_reference(T, nbins, nf, fam, kind, nc)
        feat, energy = run_mel(eng, p, b, out_kind, nc, dc, en)
        assert feat.shape == (T, nc if out_kind == MFCC else nf)
        v = R.mel_judge(feat, energy, p, b, out_kind, nc, dc, want, bars)
        assert v["ok"] and v["left_out"] == 0, "%s: %r" % (v["why"], (fam, kind, out_kind, nc, dc, en))
        worst = max(worst, v["ratio"])
        zero_rows = ~p.any(axis=1)
        if zero_rows.any():                              # a zero frame: eps, log eps and c0 = log eps
            if out_kind == MFE:
                assert (feat[zero_rows].view(np.int32) == R.EPS32.view(np.int32)).all()
            elif out_kind == LMFE or (dc and nc >= 1):
                col = feat[zero_rows] if out_kind == LMFE else feat[zero_rows][:, :1]
                assert (np.abs(col.astype(np.float64) - np.float64(R.LOG_EPS32)) <= np.spacing(np.abs(R.LOG_EPS32))).all()
            if en:
                assert (energy[zero_rows].view(np.int32) == R.EPS32.view(np.int32)).all()
    print("ULPS mel %s T=%d nbins=%d nf=%d worst error / bar %.3f" % ("mfma" if nf <= 256 else "wide", T, nbins, nf, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("nf,nbins,T", [(40, 257, 130), (256, 129, 65), (257, 129, 33), (1024, 65, 17)])
def test_a_mel_frame_alone_equals_itself_in_the_batch(eng, nf, nbins, T):
    p, b = mel_power(T, nbins, "speech"), mel_bank("dense", nf, nbins)
    for out_kind, nc, dc in ((MFE, 1, True), (MFCC, min(13, nf), True), (MFCC, nf, False)):
        feat, energy = run_mel(eng, p, b, out_kind, nc, dc, True)
        for i in sorted({0, 15, 16, T // 2, T - 1}):
            f1, e1 = run_mel(eng, p[i:i + 1], b, out_kind, nc, dc, True)
            assert same(f1, feat[i:i + 1]) and same(e1, energy[i:i + 1]), (out_kind, nc, i)


@pytest.mark.gpu
def test_mel_kernels_agree_across_the_256_filter_threshold(eng):
    """The same (power, bank) through mel_features_mfma_kernel (nf = 256) and, with a zero 257th filter appended,
    through mel_features_kernel (nf = 257): both within the bars of the one reference, so within their sum of each other;
    the appended filter gives eps exactly."""
    T, nbins = 33, 129
    p = mel_power(T, nbins, "hi")
    b256 = mel_bank("dense", 256, nbins)
    b257 = np.concatenate([b256, np.zeros((1, nbins), dtype=np.float32)])
    want = R.mel(p, b256, 13)
    bars = R.mel_bars(p, b256, want)
    for out_kind, key in ((MFE, "mel"), (LMFE, "logmel")):
        a, ea = run_mel(eng, p, b256, out_kind, 1, True, True)
        w, ew = run_mel(eng, p, b257, out_kind, 1, True, True)
        assert R.mel_judge(a, ea, p, b256, out_kind, 1, True, want, bars)["ok"]
        assert R.mel_judge(w[:, :256], ew, p, b256, out_kind, 1, True, want, bars)["ok"]
        assert (np.abs(a.astype(np.float64) - w[:, :256]) <= 2.0 * bars[key]).all()
        assert (np.abs(ea.astype(np.float64) - ew) <= 2.0 * bars["energy"]).all()
        if out_kind == MFE:
            assert (w[:, 256].view(np.int32) == R.EPS32.view(np.int32)).all()
        else:
            assert (np.abs(w[:, 256].astype(np.float64) - np.float64(R.LOG_EPS32)) <= np.spacing(np.abs(R.LOG_EPS32))).all()
